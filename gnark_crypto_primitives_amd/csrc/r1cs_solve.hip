// Batched witness solve of a gnark-shaped R1CS (zkmi_r1cs_solver_load / zkmi_r1cs_solve_batch /
// zkmi_prove_r1cs_submit): the caller holds a gnark ccs -- coefficient table, three term lists per
// constraint, instruction order, hints -- and no witness program of this repository's frontend.
// Stands in for cs.Solve (gnark constraint/bn254 solver.go [UPSTREAM-RECALL]) called once per
// witness on the caller's CPUs.
//
// Such a system has next to no parallelism between instructions (Arbo-160: 40 361 constraints in
// 31 648 dependency levels) and all of it inside them (29 terms per constraint on average, up to
// 323).  So the kernel walks the instructions in gnark's order, S sub-lanes of a wavefront share the
// terms of one proof's instruction, their partial sums are added across the sub-lanes in registers,
// and every sub-lane then solves for the one unknown wire.  The plan it runs -- records with the
// unknowns resolved, terms padded to rows of S -- is built and checked on the host: r1cs_plan.h.
//
// Values stay in gnark's 2^256 image throughout (coefficients are 2^261 images, so a product on the
// 29-bit chain lands in the 2^256 image again): the wire matrix is what
// zkmi_prove_witness_submit leaves for stage 2 of the prover, which runs unchanged.
// There is no CPU fallback in this file.
#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "zkmi_internal.h"
#include "solve_common.h"
#include "r1cs_plan.h"

using namespace zk;

struct zkmi_r1cs_solver {
  uint32_t n_wires = 0, n_constraints = 0, n_inputs = 0, n_instr = 0, S = 1;
  uint32_t n_records = 0;             // what the kernel walks: n_instr, or more with lookup hints
  bool ext = false;                   // the plan holds a record kind of ZKMI_HINTS_STD
  bool emul = false;                  // the plan holds emulated-product records (ZKMI_HINTS_EMULATED)
  std::vector<R1csCommit> commits;    // host: the commitment hints, the launches' boundaries
  uint32_t longest = 0, n_inversions = 0;
  uint64_t n_terms = 0;
  // device: the plan (r1cs_plan.h)
  uint4* records = nullptr;
  uint2* terms = nullptr;
  Fr* coeffs = nullptr;
  uint32_t* outs = nullptr;
};

namespace zk {

// sum over the S sub-lanes of a proof (lanes p, p + 64 / S, ...): every sub-lane ends with the total
template <int S>
__device__ __forceinline__ Fr sum_sublanes(Fr v) {
#pragma unroll
  for (int m = 64 / S; m < 64; m <<= 1) {
    Fr o;
#pragma unroll
    for (int i = 0; i < 8; i++) o.v[i] = __shfl_xor(v.v[i], m, 64);
    v = add(v, o);
  }
  return v;
}

// One wavefront = 64 / S proofs x S sub-lanes, lane l = (sub-lane l / (64 / S), proof l % (64 / S)),
// as in solve_vliw_kernel.  Records are wave-uniform (scalar loads); a row of terms is one 8-byte
// load per lane, the same address in the lanes of a sub-lane; wire values are coalesced row segments.
// A wire stored by one instruction is loaded by later ones of the same wavefront only, and a
// wavefront's vector memory instructions reach the L1 / L2 in issue order (solve.hip relies on the
// same): the wavefront-scope fence pins the compiler's order and costs no instruction.
// The next instruction's record is fetched before this one's stores are issued; terms, wire values
// and coefficients are fetched three and two rows ahead of the row in work, across instruction
// ends.  A wire value fetched ahead of the store that writes it is replaced in registers (the bits
// of an NBits hint: fetched again), so no instruction waits for its predecessor's store.
// A launch runs the records [begin, end): records and terms are contiguous and end in the slack the
// plan appends, so the fetches start at records[begin] and run ahead of `end` like anywhere else.
// EXT = 1: the plan holds record kinds of ZKMI_HINTS_STD (limbs, byte operations, lookup
// multiplicities); plans without one run the EXT = 0 instance, which holds none of their code.
// EXT = 2: the plan also holds emulated-product records (ZKMI_HINTS_EMULATED); the other two
// instances hold none of that code either.  The steps of such a hint leave every sub-lane of a
// proof the field images of all operand limbs (L below, live from the first step to the closing
// record); the closing record is r1cs_emul_finish (r1cs_plan.h), run by every sub-lane alike, with
// the output stores split over the sub-lanes.
// A lookup hint counts with an atomic add on the low word of the counter's wire slot and reads back
// with the same scope, as the CLS_HIST branch of solve_vliw_kernel (solve.hip) does: the sub-lanes of
// a proof share the counters.
// All counts and indices come from a plan that r1cs_plan_build has checked.
template <int S, int EXT>
__global__ __launch_bounds__(64) void r1cs_solve_kernel(const uint4* __restrict__ recs,
                                                        const uint2* __restrict__ terms,
                                                        const Fr* __restrict__ coeffs,
                                                        const uint32_t* __restrict__ outs, Fr* w,
                                                        Fr* __restrict__ a, Fr* __restrict__ b,
                                                        Fr* __restrict__ c,
                                                        int32_t* __restrict__ status, size_t Bp,
                                                        uint32_t begin, uint32_t end) {
  constexpr int PPW = 64 / S;
  const uint32_t sl = threadIdx.x / PPW;
  const size_t p = (size_t)blockIdx.x * PPW + (threadIdx.x % PPW);
  int32_t st = 0;
  uint4 r0 = recs[2 * (size_t)begin], r1 = recs[2 * (size_t)begin + 1];
  // Rows of terms follow each other without gaps from one instruction to the next, so the fetches
  // run ahead of the row in work regardless of where an instruction ends: the term of row r + 3,
  // the wire value and the coefficient of row r + 2.  t0 / x0 / k0 belong to the row in work.
  const uint2* tp = terms + __builtin_amdgcn_readfirstlane(r1.x) + sl;
  uint2 t0 = tp[0], t1 = tp[S], t2 = tp[2 * S];
  Fr x0 = bi_ld(w, t0.x & R1CS_IDX_MASK, p, Bp), x1 = bi_ld(w, t1.x & R1CS_IDX_MASK, p, Bp);
  Fr k0 = coeffs[t0.y & R1CS_IDX_MASK], k1 = coeffs[t1.y & R1CS_IDX_MASK];
  Fr L[8];   // EXT = 2: the operand limbs of the emulated product in work
  if constexpr (EXT == 2) {
#pragma unroll
    for (int q = 0; q < 8; q++) L[q] = Fr::zero();
  }
  for (uint32_t i = begin; i < end; i++) {
    const uint32_t kind = __builtin_amdgcn_readfirstlane(r0.x);
    const uint32_t target = __builtin_amdgcn_readfirstlane(r0.y);
    const uint32_t mul_rows = __builtin_amdgcn_readfirstlane(r1.y);
    const uint32_t unit_rows = __builtin_amdgcn_readfirstlane(r1.z);
    const uint32_t k = __builtin_amdgcn_readfirstlane(r1.w);
    const Fr kinv = coeffs[__builtin_amdgcn_readfirstlane(r0.w)];
    // RK_EMUL_END: where the modulus sits (kinv is the modulus itself, its limbs' images follow)
    const uint32_t mod_at = EXT == 2 ? (uint32_t)__builtin_amdgcn_readfirstlane(r0.w) : 0u;
    const uint32_t par = EXT ? __builtin_amdgcn_readfirstlane(r0.z) : 0u;   // width, operation, size
    Fr sa = Fr::zero(), sb = Fr::zero(), sc = Fr::zero();
    // v joins the sum its tag names; a padding term joins none
    auto accumulate = [&](uint32_t tag, const Fr& v) {
      const Fr s = add(tag == RT_L ? sa : tag == RT_R ? sb : sc, v);
      if (tag == RT_L) sa = s;
      if (tag == RT_R) sb = s;
      if (tag == RT_O) sc = s;
    };
    for (uint32_t row = 0; row < mul_rows + unit_rows; row++) {
      const uint2 t3 = tp[3 * S];
      const Fr x2 = bi_ld(w, t2.x & R1CS_IDX_MASK, p, Bp);
      const Fr k2 = coeffs[t2.y & R1CS_IDX_MASK];
      if (row < mul_rows)   // wave-uniform
        accumulate(t0.x >> 30, fmulp(x0, k0));
      else
        accumulate(t0.x >> 30, (t0.y >> 30) == 2 ? neg(x0) : x0);
      tp += S;
      t0 = t1, t1 = t2, t2 = t3;
      x0 = x1, x1 = x2;
      k0 = k1, k1 = k2;
    }
    // the next instruction's record, before this one's stores
    r0 = recs[2 * (size_t)(i + 1)];
    r1 = recs[2 * (size_t)(i + 1) + 1];
    // a query is its sub-lane's own sum, and so is an operand limb of an emulated product
    if (S > 1 && !(EXT && kind == RK_COUNT_Q) && !(EXT == 2 && kind == RK_EMUL_STEP)) {
      sa = sum_sublanes<S>(sa);
      sb = sum_sublanes<S>(sb);
      sc = sum_sublanes<S>(sc);
    }
    if (EXT == 2 && kind >= RK_EMUL_STEP) {
      if constexpr (EXT == 2) {
        if (kind == RK_EMUL_STEP) {
          // limbs target .. target + k - 1, one per sub-lane: every sub-lane fetches them all from
          // their owners in the same proof
#pragma unroll
          for (int q = 0; q < 8; q++)
            if ((uint32_t)q >= target && (uint32_t)q < target + k) {
              const int owner = (int)((uint32_t)q - target) * PPW + (int)(threadIdx.x % PPW);
#pragma unroll
              for (int t = 0; t < 8; t++) L[q].v[t] = __shfl(sa.v[t], owner, 64);
            }
        } else {
          r1cs_emul_finish(L, kinv, coeffs + mod_at + 1, par,
                           [&](uint32_t o, const Fr& v) {
                             if ((o & (S - 1)) == sl) bi_st(w, outs[target + o], p, Bp, v);
                           });
          // the wire values fetched ahead may be among the wires stored: fetch them again behind the stores
          __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
          x0 = bi_ld(w, t0.x & R1CS_IDX_MASK, p, Bp);
          x1 = bi_ld(w, t1.x & R1CS_IDX_MASK, p, Bp);
        }
      }
    } else if (EXT && kind >= RK_LIMBS) {
      if (kind == RK_BYTEOP) {
        const uint32_t u = from_mont(sa).v[0], v = from_mont(sb).v[0];
        const Fr xs = r1cs_small(par == 1 ? u ^ v : u & v);
        if (sl == 0) bi_st(w, target, p, Bp, xs);
        if ((t0.x & R1CS_IDX_MASK) == target) x0 = xs;
        if ((t1.x & R1CS_IDX_MASK) == target) x1 = xs;
      } else if (kind == RK_COUNT_Q) {
        // k queries, one per sub-lane; a query outside the table (coef = its size) counts nowhere
        const Fr v = from_mont(sa);
        if (sl < k && (v.v[1] | v.v[2] | v.v[3] | v.v[4] | v.v[5] | v.v[6] | v.v[7]) == 0 &&
            v.v[0] < par)
          __hip_atomic_fetch_add(lookup_counter(w, outs[target + v.v[0]], p, Bp), 1u, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
      } else if (kind != RK_COMMIT) {   // (a launch ends in front of a commitment)
        if (kind == RK_LIMBS) {
          // the sub-lanes split the k output wires
          const Fr v = from_mont(sa);
          for (uint32_t j = sl; j < k; j += S)
            bi_st(w, outs[target + j], p, Bp, r1cs_small(r1cs_limb(v, j * par, par)));
        } else if (kind == RK_COUNT_BEGIN) {
          // the sub-lanes zero the k counters; the stores are complete before the first count
          for (uint32_t j = sl; j < k; j += S) bi_st(w, outs[target + j], p, Bp, Fr::zero());
          stores_complete();
        } else {   // RK_COUNT_END: the counts are complete; integers into field images, in place
          stores_complete();
          for (uint32_t j = sl; j < k; j += S) {
            const uint32_t wire = outs[target + j];
            bi_st(w, wire, p, Bp,
                  r1cs_small(__hip_atomic_load(lookup_counter(w, wire, p, Bp), __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT)));
          }
        }
        // the wire values fetched ahead may be among the wires stored: fetch them again behind the stores
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        x0 = bi_ld(w, t0.x & R1CS_IDX_MASK, p, Bp);
        x1 = bi_ld(w, t1.x & R1CS_IDX_MASK, p, Bp);
      }
    } else if (kind == RK_NBITS) {
      // the sub-lanes split the k output wires
      const Fr v = from_mont(sa);
      for (uint32_t j = sl; j < k; j += S) {
        const uint32_t bit = j < 256 ? (v.v[j >> 5] >> (j & 31)) & 1u : 0u;
        bi_st(w, outs[target + j], p, Bp, bit ? Fr::one() : Fr::zero());
      }
      // the wire values fetched ahead may be among the bits: fetch them again behind the stores
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      x0 = bi_ld(w, t0.x & R1CS_IDX_MASK, p, Bp);
      x1 = bi_ld(w, t1.x & R1CS_IDX_MASK, p, Bp);
    } else {
      Fr xs = Fr::zero();
      if (kind == RK_ASSERT || kind == RK_SOLVE_O) {
        const Fr ab = mul(sa, sb);
        if (kind == RK_ASSERT) {
          if (ab != sc) st = ZKMI_ERR_UNSATISFIED;
        } else {   // k x + c = a b; the completed c is a b
          xs = fmulp(sub(ab, sc), kinv);
          sc = ab;
        }
      } else {
        // (a + k x) b = c divides by b, a (b + k x) = c and the InvZero hint by a
        const Fr den = kind == RK_SOLVE_L ? sb : sa;
        const Fr inv = inverse(den);
        if (kind == RK_INVZERO) {
          xs = inv;
        } else {
          if (den.is_zero()) st = ZKMI_ERR_UNSATISFIED;
          const Fr q = mul(sc, inv);   // the completed factor
          xs = fmulp(sub(q, kind == RK_SOLVE_L ? sa : sb), kinv);
          if (kind == RK_SOLVE_L)
            sa = q;
          else
            sb = q;
        }
      }
      // one sub-lane per store; the wire values fetched ahead of the store get the new value here
      if (kind != RK_ASSERT) {
        if (sl == 0) bi_st(w, target, p, Bp, xs);
        if ((t0.x & R1CS_IDX_MASK) == target) x0 = xs;
        if ((t1.x & R1CS_IDX_MASK) == target) x1 = xs;
      }
      if (kind != RK_INVZERO) {
        if (sl == (1 & (S - 1))) bi_st_nt(a, k, p, Bp, sa);
        if (sl == (2 & (S - 1))) bi_st_nt(b, k, p, Bp, sb);
        if (sl == (3 & (S - 1))) bi_st_nt(c, k, p, Bp, sc);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  }
  // every sub-lane of a proof holds the same sums, hence the same verdict
  if (st && sl == 0) status[p] = st;
}

// ONE wire and a clean status
__global__ void r1cs_solve_init_kernel(Fr* w, int32_t* status, size_t Bp) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < Bp) {
    bi_st(w, 0, i, Bp, Fr::one());
    status[i] = 0;
  }
}

template <int S>
static void launch_r1cs_solve(zkmi_ctx* ctx, const zkmi_r1cs_solver* s, Fr* w, Fr* a, Fr* b, Fr* c,
                              int32_t* status, size_t Bp, uint32_t begin, uint32_t end) {
  const auto kernel = s->emul ? r1cs_solve_kernel<S, 2> : s->ext ? r1cs_solve_kernel<S, 1> : r1cs_solve_kernel<S, 0>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(Bp * S / 64)), dim3(64), 0, ctx->stream, s->records,
                     s->terms, s->coeffs, s->outs, w, a, b, c, status, Bp, begin, end);
}

// ONE and a clean status into w [n_wires][Bp] / status[Bp], in front of the first r1cs_solve_range
static int r1cs_solve_init(zkmi_ctx* ctx, Fr* w, int32_t* status, size_t Bp) {
  hipLaunchKernelGGL(r1cs_solve_init_kernel, dim3((unsigned)(Bp / 64)), dim3(64), 0, ctx->stream, w,
                     status, Bp);
  ZK_HIP(hipGetLastError());
  return ZKMI_OK;
}

// the records [begin, end) of the plan, begin <= end <= n_records
static int r1cs_solve_range(zkmi_ctx* ctx, const zkmi_r1cs_solver* s, Fr* w, Fr* a, Fr* b, Fr* c,
                            int32_t* status, size_t Bp, uint32_t begin, uint32_t end) {
  if (begin > end || end > s->n_records) {
    ctx->err = "r1cs solver: record range outside the plan";
    return ZKMI_ERR_ARG;
  }
  if (begin == end) return ZKMI_OK;
  if (!with_lanes(s->S, [&](auto S) { launch_r1cs_solve<S>(ctx, s, w, a, b, c, status, Bp, begin, end); })) {
    ctx->err = "r1cs solver: lanes_per_proof must be a power of two, 1 .. 64";
    return ZKMI_ERR_ARG;
  }
  ZK_HIP(hipGetLastError());
  return ZKMI_OK;
}

// w [n_wires][Bp] with rows 1 .. n_inputs filled: writes every other wire row, a / b / c rows
// [0, n_constraints) and status[Bp], all in gnark's image
static int r1cs_solve_bi(zkmi_ctx* ctx, const zkmi_r1cs_solver* s, Fr* w, Fr* a, Fr* b, Fr* c,
                         int32_t* status, size_t Bp) {
  int rc = r1cs_solve_init(ctx, w, status, Bp);
  return rc ? rc : r1cs_solve_range(ctx, s, w, a, b, c, status, Bp, 0, s->n_records);
}

static int solver_load(zkmi_ctx* ctx, const zkmi_r1cs* m, const zkmi_r1cs_solver_desc* d,
                       zkmi_r1cs_solver** out) {
  // the loaded system and the description, on the host
  std::vector<Fr> coeffs;
  std::vector<uint32_t> ptr[3];
  std::vector<R1csTerm> terms[3];
  static_assert(sizeof(R1csTerm) == sizeof(uint2) && sizeof(R1csTerm) == sizeof(zkmi_term), "term layouts");
  bool ok = fetch(coeffs, m->coeffs, m->n_coeffs);
  for (int s = 0; ok && s < 3; s++)
    ok = fetch(ptr[s], m->ptr[s], (size_t)m->n_constraints + 1) && fetch(terms[s], m->terms[s], m->nnz[s]);
  if (!ok) {
    ctx->err = "r1cs solver: cannot read the loaded system back";
    return ZKMI_ERR_HIP;
  }
  std::vector<uint32_t> instr, hkind, in_ptr, lc_ptr, out_ptr, houts;
  std::vector<zkmi_term> hterms;
  ok = fetch(instr, d->instr, (size_t)d->n_instr * 2);
  if (ok && d->n_hints) {
    ok = fetch(hkind, d->hint_kind, d->n_hints) && fetch(in_ptr, d->hint_in_ptr, (size_t)d->n_hints + 1) &&
         fetch(out_ptr, d->hint_out_ptr, (size_t)d->n_hints + 1);
    // the next sizes are the caller's own numbers: an array no larger than the system's wires and
    // terms allow, or the builder's message about the offsets
    const size_t cap = (size_t)m->n_wires + m->nnz[0] + m->nnz[1] + m->nnz[2] + 2 * (size_t)d->n_instr;
    if (ok && in_ptr[d->n_hints] <= cap && out_ptr[d->n_hints] <= cap) {
      ok = fetch(lc_ptr, d->hint_lc_ptr, (size_t)in_ptr[d->n_hints] + 1) &&
           fetch(houts, d->hint_out, out_ptr[d->n_hints]);
      if (ok && lc_ptr[in_ptr[d->n_hints]] <= cap) ok = fetch(hterms, d->hint_terms, lc_ptr[in_ptr[d->n_hints]]);
    }
  }
  if (!ok) {
    ctx->err = "r1cs solver: cannot read the instruction list or the hint table";
    return ZKMI_ERR_ARG;
  }
  zkmi_r1cs_solver_desc hd = *d;
  hd.instr = instr.data();
  hd.hint_kind = hkind.data();
  hd.hint_in_ptr = in_ptr.data();
  hd.hint_lc_ptr = lc_ptr.empty() ? nullptr : lc_ptr.data();
  hd.hint_terms = hterms.data();
  hd.hint_out_ptr = out_ptr.data();
  hd.hint_out = houts.data();
  if (d->n_hints && (lc_ptr.empty() || hterms.size() != lc_ptr.back() || houts.size() != out_ptr.back())) {
    ctx->err = "r1cs solver: hint table: offsets are not monotone from 0, or larger than the system";
    return ZKMI_ERR_ARG;
  }
  R1csPlanIn in;
  in.n_wires = m->n_wires;
  in.n_constraints = m->n_constraints;
  in.n_coeffs = m->n_coeffs;
  in.coeffs = coeffs.data();
  for (int s = 0; s < 3; s++) {
    in.ptr[s] = ptr[s].data();
    in.terms[s] = terms[s].data();
  }
  in.desc = &hd;
  R1csPlan plan;
  const std::string err = r1cs_plan_build(in, &plan);
  if (!err.empty()) {
    ctx->err = err;
    return ZKMI_ERR_ARG;
  }
  auto* s = new zkmi_r1cs_solver();
  s->n_wires = m->n_wires;
  s->n_constraints = m->n_constraints;
  s->n_inputs = d->n_public - 1 + d->n_secret;
  s->n_instr = plan.n_instr;
  s->n_records = (uint32_t)plan.records.size() - 1;
  s->ext = plan.ext;
  s->emul = plan.emul;
  s->commits = std::move(plan.commits);
  s->S = plan.S;
  s->longest = plan.longest;
  s->n_inversions = plan.n_inversions;
  s->n_terms = plan.n_terms;
  static_assert(sizeof(R1csRecord) == 2 * sizeof(uint4), "record = two quads");
  if (!upload(&s->records, plan.records.data(), plan.records.size() * 2) ||
      !upload(&s->terms, plan.terms.data(), plan.terms.size()) ||
      !upload(&s->coeffs, plan.coeffs.data(), plan.coeffs.size()) ||
      !upload(&s->outs, plan.outs.data(), plan.outs.size())) {
    ctx->err = "r1cs solver: device upload failed";
    zkmi_r1cs_solver_free(ctx, s);
    return ZKMI_ERR_HIP;
  }
  *out = s;
  return ZKMI_OK;
}

}  // namespace zk

extern "C" {

void zkmi_r1cs_solver_free(zkmi_ctx* ctx, zkmi_r1cs_solver* s) {
  if (!s) return;
  if (ctx) {
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    sync_side_streams(ctx);
  }
  if (s->records) hipFree(s->records);
  if (s->terms) hipFree(s->terms);
  if (s->coeffs) hipFree(s->coeffs);
  if (s->outs) hipFree(s->outs);
  delete s;
}

int zkmi_r1cs_solver_load(zkmi_ctx* ctx, const zkmi_r1cs* r1cs, const zkmi_r1cs_solver_desc* desc,
                          zkmi_r1cs_solver** out) {
  ZK_HIP(hipSetDevice(ctx->device));
  if (!r1cs || !desc || !out) {
    ctx->err = "r1cs solver: null argument";
    return ZKMI_ERR_ARG;
  }
  *out = nullptr;
  try {
    return solver_load(ctx, r1cs, desc, out);
  } catch (const std::bad_alloc&) {
    ctx->err = "r1cs solver: out of host memory while building the plan";
    return ZKMI_ERR_OOM;
  }
}

int zkmi_r1cs_solver_info(const zkmi_r1cs_solver* s, uint64_t* info) {
  if (!s || !info) return ZKMI_ERR_ARG;
  info[0] = s->n_instr;
  info[1] = s->S;
  info[2] = s->n_terms;
  info[3] = s->longest;
  info[4] = s->n_inversions;
  info[5] = s->n_wires;
  info[6] = s->n_constraints;
  info[7] = s->n_inputs;
  return ZKMI_OK;
}

int zkmi_r1cs_solve_batch(zkmi_ctx* ctx, const zkmi_r1cs_solver* s, const void* inputs, size_t batch,
                          void* wires_out, void* abc_out, int32_t* status_out) {
  ZK_HIP(hipSetDevice(ctx->device));
  int rc;
  if ((rc = require_idle(ctx))) return rc;
  if (batch == 0) return ZKMI_OK;
  if (!s || !status_out || (s->n_inputs && !inputs)) {
    ctx->err = "r1cs_solve_batch: null argument";
    return ZKMI_ERR_ARG;
  }
  if (!s->commits.empty()) {
    ctx->err = "r1cs_solve_batch: this solver holds commitment hints, whose values need a proving key: "
               "use zkmi_prove_r1cs_submit";
    return ZKMI_ERR_ARG;
  }
  const size_t Bp = round_up(batch, 64), nc = s->n_constraints;
  Staged si(ctx), sw(ctx), sabc(ctx), sst(ctx);
  if ((rc = si.in(inputs, batch * (size_t)s->n_inputs * 32))) return rc;
  if (wires_out && (rc = sw.out(wires_out, batch * (size_t)s->n_wires * 32))) return rc;
  if (abc_out && (rc = sabc.out(abc_out, 3 * batch * nc * 32))) return rc;
  if ((rc = sst.out(status_out, batch * 4))) return rc;
  void *w, *a, *b, *c, *st;
  zkmi_ctx::ProveSet& S = ctx->sets[0];
  if ((rc = ensure_scratch(ctx, S.slots, (size_t)s->n_wires * Bp * 32, &w)) ||
      (rc = ensure_scratch(ctx, S.a, nc * Bp * 32, &a)) || (rc = ensure_scratch(ctx, S.b, nc * Bp * 32, &b)) ||
      (rc = ensure_scratch(ctx, S.c, nc * Bp * 32, &c)) || (rc = ensure_scratch(ctx, S.misc, Bp * 4, &st)))
    return rc;
  if ((rc = transpose_in(ctx, si.dev, (Fr*)w + Bp, s->n_inputs, batch, Bp, 32))) return rc;
  if ((rc = r1cs_solve_bi(ctx, s, (Fr*)w, (Fr*)a, (Fr*)b, (Fr*)c, (int32_t*)st, Bp))) return rc;
  if (wires_out && (rc = transpose_out(ctx, w, sw.dev, s->n_wires, batch, Bp, 32))) return rc;
  if (abc_out) {
    const size_t stride = batch * nc * 32;
    if ((rc = transpose_out(ctx, a, sabc.dev, nc, batch, Bp, 32)) ||
        (rc = transpose_out(ctx, b, (char*)sabc.dev + stride, nc, batch, Bp, 32)) ||
        (rc = transpose_out(ctx, c, (char*)sabc.dev + 2 * stride, nc, batch, Bp, 32)))
      return rc;
  }
  ZK_HIP(hipMemcpyAsync(sst.dev, st, batch * 4, hipMemcpyDeviceToDevice, ctx->stream));
  if ((rc = sw.finish()) || (rc = sabc.finish()) || (rc = sst.finish())) return rc;
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  return ZKMI_OK;
}

// Stage 1 of a prove from inputs: like zkmi_prove_submit, with the value file = the wire matrix in
// gnark's image, as zkmi_prove_witness_submit(r1cs != NULL) leaves it for the collect.
int zkmi_prove_r1cs_submit(zkmi_ctx* ctx, const zkmi_pk* pk, const zkmi_r1cs_solver* s,
                           const void* inputs, size_t batch, const void* rs) {
  ZK_HIP(hipSetDevice(ctx->device));
  if (!pk || !s || !rs || batch == 0 || (s->n_inputs && !inputs)) {
    ctx->err = "prove_r1cs_submit: null argument or empty batch";
    return ZKMI_ERR_ARG;
  }
  // checked before anything is queued: a refused call leaves no batch in flight
  if (!pk->commits.empty() && s->commits.empty()) {
    ctx->err = "prove_r1cs_submit: this key has commitments; the solver holds no commitment hint: load "
               "it with ZKMI_HINTS_STD, or solve with gnark and use zkmi_prove_witness_submit";
    return ZKMI_ERR_ARG;
  }
  if (s->commits.size() != pk->commits.size()) {
    ctx->err = "prove_r1cs_submit: the solver holds " + std::to_string(s->commits.size()) +
               " commitment hints, the proving key " + std::to_string(pk->commits.size()) + " commitments";
    return ZKMI_ERR_ARG;
  }
  for (size_t i = 0; i < s->commits.size(); i++) {
    const R1csCommit& sc = s->commits[i];
    const zkmi_commit_key& ck = pk->commits[i];
    const char* what = sc.wire != ck.wire ? "lands on different wires" :
                       sc.hashed != ck.hashed ? "hashes different wires" :
                       sc.priv != ck.priv ? "commits to different private wires" : nullptr;
    if (what) {
      ctx->err = "prove_r1cs_submit: commitment " + std::to_string(i) + " (instruction " +
                 std::to_string(sc.instr) + ") " + what + " in the solver and in the proving key";
      return ZKMI_ERR_ARG;
    }
  }
  if (pk->n_wires != s->n_wires) {
    ctx->err = "prove_r1cs_submit: proving key and solver disagree on the number of wires";
    return ZKMI_ERR_ARG;
  }
  if (s->n_constraints > ((size_t)1 << pk->log_n)) {
    ctx->err = "prove_r1cs_submit: domain smaller than the number of constraints";
    return ZKMI_ERR_ARG;
  }
  if (pk->folded && s->n_constraints != pk->fold_n_constraints) {
    ctx->err = "prove_r1cs_submit: the key was folded (zkmi_pk_desc.fold_r1cs) with a system of " +
               std::to_string(pk->fold_n_constraints) + " constraints, this one has " +
               std::to_string(s->n_constraints);
    return ZKMI_ERR_ARG;
  }
  hipStream_t main;
  char* stage;
  int rc = prove_set_begin(ctx, pk, s->n_wires, s->n_inputs, batch, rs, &main, &stage);
  if (rc) return rc;
  zkmi_ctx::ProveSet& S = ctx->sets[ctx->next_submit];
  const size_t Bp = S.Bp;
  S.cs = nullptr;
  S.n_constraints = s->n_constraints;
  S.f_domain = false;
  Fr* w = (Fr*)S.slots.p;
  const void* in_dev;
  rc = device_view(ctx, inputs, batch * (size_t)s->n_inputs * 32, stage, &in_dev);
  if (!rc) rc = transpose_in(ctx, in_dev, w + Bp, s->n_inputs, batch, Bp, 32);
  // as zkmi_prove_submit: the solve stops at every commitment hint; the commitment is an MSM over
  // the wires solved so far, its hash becomes the commitment wire's value (commit.hip)
  Fr *a = (Fr*)S.a.p, *b = (Fr*)S.b.p, *c = (Fr*)S.c.p;
  int32_t* st = (int32_t*)S.st;
  if (!rc) rc = r1cs_solve_init(ctx, w, st, Bp);
  uint32_t begin = 0;
  for (size_t i = 0; !rc && i < s->commits.size(); i++) {
    rc = r1cs_solve_range(ctx, s, w, a, b, c, st, Bp, begin, s->commits[i].record);
    if (!rc) rc = commit_phase(ctx, S, (uint32_t)i, true);
    begin = s->commits[i].record + 1;
  }
  if (!rc) rc = r1cs_solve_range(ctx, s, w, a, b, c, st, Bp, begin, s->n_records);
  if (!rc && !s->commits.empty()) rc = commit_finish_submit(ctx, S);
  return prove_set_end(ctx, main, rc);
}

}  // extern "C"
