// Batched witness solve of a gnark-shaped sparse constraint system (zkmi_scs_solver_load /
// zkmi_scs_solve_batch / zkmi_plonk_prove_scs): the caller holds gnark's SparseR1CS -- three wire
// columns, five selectors, instruction order, hints -- and a plonk.ProvingKey, and no witness program
// of this repository's frontend.  Stands in for spr.Solve called once per witness on the caller's
// CPUs.
//
// A sparse gate touches at most three wires, so there is nothing to share inside an instruction (the
// R1CS solver, r1cs_solve.hip, splits the up to 322 terms of one); the parallelism is the one gnark's
// own solver uses, the independent gates of one dependency level.  The plan -- records with the
// unknowns resolved, packed into steps of S records of one level and one class -- is built and
// checked on the host: scs_plan.h.
//
// Values stay in gnark's 2^256 image throughout: the wire matrix is what stage_rows leaves in the
// key's first work buffer for scs_gate_kernel (plonk.hip), which gathers the columns and checks every
// gate afterwards, so the wire-form path of round 1 runs unchanged behind the solve.
// There is no CPU fallback in this file.
#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "zkmi_internal.h"
#include "solve_common.h"
#include "scs_plan.h"

using namespace zk;

struct zkmi_scs_solver {
  zkmi_scs* sys = nullptr;   // the solver's own copy of the system (the caller may free theirs)
  uint32_t n_inputs = 0, n_instr = 0, S = 1, n_records = 0, n_steps = 0, n_levels = 0, n_inversions = 0;
  // device: the plan (scs_plan.h)
  uint4* records = nullptr;
  Fr* coefs = nullptr;       // rows of six: qL qR qO qM as 2^261 images, qC and K in gnark's image
  uint32_t* outs = nullptr;
  uint32_t* input_wire = nullptr;
  // ZKMI_HINTS_STD.  The EXT = 1 instance of scs_solve_kernel runs a plan with a record of the std
  // classes, which only it can, and also every plan with commitment hints: such a plan is loaded under
  // the std set and runs in pieces between its commitments, and those pieces have always run on the
  // kernel with the step range.  EXT = 0 is thereby only ever launched over a whole plan.
  bool ext = false;
  // the commitment hints, with the solver's device copy of their wire lists
  std::vector<ScsPlan::Commit> commits;
  std::vector<uint32_t*> commit_wires;
};

namespace zk {

// Steps [begin, end) of the plan, so that the caller can stop at a commitment's boundary, form the
// commitment and go on.
// One wavefront = 64 / S proofs x S sub-lanes, lane l = (sub-lane l / (64 / S), proof l % (64 / S)),
// as in solve_vliw_kernel and r1cs_solve_kernel.  Steps are a wave-uniform loop; sub-lane s runs
// record s of the step, one 32-byte load that the lanes of a sub-lane share; the step's class is the
// same in all its records (read through readfirstlane), so the only divergence is between the marks
// of the records and the padding.  Wire values are coalesced row segments of the batch-inner matrix,
// in gnark's 2^256 image; products are fmulp against 2^261 images.
// A wire stored in one step is loaded in later steps by lanes of the same wavefront only, and a
// wavefront's vector memory instructions reach the L1 / L2 in issue order (the argument at the top of
// the VLIW solver in solve.hip): the wavefront-scope fence pins the compiler's order and costs no
// instruction; there is no vmcnt(0) per step.  The plan guarantees that no record reads a wire its
// own step writes.  The next step's record is fetched before this step's work; the records are
// contiguous and end in a step of padding, so the fetch ahead of `end` stays inside the array.
// EXT = 1: the plan may hold records of the classes SK_LIMBS .. SK_COUNT_END (ZKMI_HINTS_STD), named
// in a record's fourth control word; plans without one run the EXT = 0 instance, which holds none of
// their code and does not read that word.  The lookup counters are those of solve_common.h, as in
// r1cs_solve.hip; zeroing, counting and reading back are three levels of the plan, so three
// different steps.
// Bits and limbs under a per-lane index come out of chains of selects, never an indexed register array.
// All counts and indices come from a plan that scs_plan_build has checked: a wire index is below
// n_wires, outs[target + j] exists for every j a record names, and a query counts only below its
// table's size.
template <int S, bool EXT>
__global__ __launch_bounds__(64) void scs_solve_kernel(const uint4* __restrict__ recs,
                                                       const Fr* __restrict__ coefs,
                                                       const uint32_t* __restrict__ outs, Fr* w,
                                                       int32_t* __restrict__ status, size_t Bp,
                                                       uint32_t begin, uint32_t end) {
  constexpr int PPW = 64 / S;
  const uint32_t sl = threadIdx.x / PPW;
  const size_t p = (size_t)blockIdx.x * PPW + (threadIdx.x % PPW);
  int32_t st = 0;
  const uint4* rp = recs + 2 * ((size_t)begin * S + sl);
  uint4 r0 = rp[0], r1 = rp[1];
  for (uint32_t t = begin; t < end; t++) {
    const uint4 q0 = r0, q1 = r1;
    rp += 2 * S;
    r0 = rp[0];
    r1 = rp[1];
    const uint32_t ctl = q1.x;
    const uint32_t xcls = EXT ? __builtin_amdgcn_readfirstlane(q1.w) : 0u;
    const uint32_t cls = xcls ? xcls : __builtin_amdgcn_readfirstlane(ctl >> SCS_CTL_CLASS) & 3;
    const Fr* q = coefs + (size_t)q1.y * SCS_COEF_ROW;
    const bool store = ctl & SCS_CTL_STORE;
    Fr va = Fr::zero(), vb = Fr::zero(), vc = Fr::zero();
    if (ctl >> SCS_CTL_READ & 1) va = bi_ld(w, q0.x, p, Bp);
    if (ctl >> (SCS_CTL_READ + 1) & 1) vb = bi_ld(w, q0.y, p, Bp);
    if (ctl >> (SCS_CTL_READ + 2) & 1) vc = bi_ld(w, q0.z, p, Bp);
    const Fr ta = sel_term(ctl & 3, va, q), tb = sel_term((ctl >> 2) & 3, vb, q + 1);
    // the known part of the gate (a hint: its input), in gnark's image: 256 + 261 - 261
    Fr rest = add(add(ta, tb), sel_term((ctl >> 4) & 3, vc, q + 2));
    const bool has_c = ((ctl >> 8) & 3) != SCS_MARK_ZERO;
    if (has_c) rest = add(rest, q[4]);
    const uint32_t mm = (ctl >> 6) & 3, mk = (ctl >> SCS_CTL_MARK_K) & 3;
    if (cls == SK_NBITS) {
      const Fr v = from_mont(rest);
      const uint32_t j0 = q1.z & 0xffffu, cnt = q1.z >> 16;
      for (uint32_t j = 0; j < cnt; j++) {
        // the word by a chain of selects: `at` differs between the sub-lanes, and a register array
        // under a per-lane index leaves the registers
        const uint32_t at = j0 + j;
        uint32_t word = at < 256 ? v.v[0] : 0u;
#pragma unroll
        for (int i = 1; i < 8; i++) word = (at >> 5) == (uint32_t)i ? v.v[i] : word;
        const uint32_t bit = (word >> (at & 31)) & 1u;
        bi_st(w, outs[q0.w + j], p, Bp, bit ? Fr::one() : Fr::zero());
      }
    } else if (EXT && cls == SK_LIMBS) {
      const Fr v = from_mont(rest);
      const uint32_t j0 = q1.z & 0xffffu, cnt = store ? (q1.z >> 16) & 0xffu : 0u, width = q1.z >> 24;
      for (uint32_t j = 0; j < cnt; j++)
        bi_st(w, outs[q0.w + j], p, Bp, r1cs_small(std_limb(v, (j0 + j) * width, width)));
    } else if (EXT && cls == SK_BYTEOP) {
      // the two terms on their own: a constant one sits in qC (a) or K (b)
      const uint32_t u = from_mont(has_c ? add(ta, q[4]) : ta).v[0];
      const uint32_t v = from_mont(mk != SCS_MARK_ZERO ? add(tb, q[5]) : tb).v[0];
      if (store) bi_st(w, q0.w, p, Bp, r1cs_small(q1.z == 1 ? u ^ v : u & v));
    } else if (EXT && cls == SK_COUNT_ZERO) {
      const uint32_t cnt = store ? q1.z >> 16 : 0u;
      for (uint32_t j = 0; j < cnt; j++) bi_st(w, outs[q0.w + j], p, Bp, Fr::zero());
      stores_complete();   // the zeroes, before the first count
    } else if (EXT && cls == SK_COUNT_Q) {
      // a query outside the table counts nowhere
      const Fr v = from_mont(rest);
      if (store && (v.v[1] | v.v[2] | v.v[3] | v.v[4] | v.v[5] | v.v[6] | v.v[7]) == 0 && v.v[0] < q1.z)
        __hip_atomic_fetch_add(lookup_counter(w, outs[q0.w + v.v[0]], p, Bp), 1u, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    } else if (EXT && cls == SK_COUNT_END) {
      // the counts are complete; integers into field images, in place
      stores_complete();
      const uint32_t cnt = store ? q1.z >> 16 : 0u;
      for (uint32_t j = 0; j < cnt; j++) {
        const uint32_t wire = outs[q0.w + j];
        bi_st(w, wire, p, Bp,
              r1cs_small(__hip_atomic_load(lookup_counter(w, wire, p, Bp), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT)));
      }
    } else {
      Fr x;
      if (cls == SK_LIN) {
        // x = K rest, K = -1 / k
        if (mm != SCS_MARK_ZERO) rest = add(rest, sel_term(mm, fmulp(va, lift<5>(vb)), q + 3));
        x = mk == SCS_MARK_ONE ? rest : mk == SCS_MARK_MINUS_ONE ? neg(rest) : fmulp(rest, lift<5>(q[5]));
      } else {
        // DIV: x = -rest / (k + qM other); INVZERO: x = 1 / rest, 0 for 0 (the inverse of 0 is 0)
        Fr den = rest;
        if (cls == SK_DIV) {
          den = sel_term(mm, ctl & SCS_CTL_OTHER_A ? va : vb, q + 3);
          if (mk != SCS_MARK_ZERO) den = add(den, q[5]);
          if (store && den.is_zero()) st = ZKMI_ERR_UNSATISFIED;
        }
        const Fr inv = inverse(den);
        x = cls == SK_DIV ? neg(fmulp(rest, lift<5>(inv))) : inv;
      }
      if (store) bi_st(w, q0.w, p, Bp, x);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  }
  if (st) status[p] = st;
}

// the staged input rows [n_inputs][Bp] to their wires
__global__ void scs_solve_init_kernel(const Fr* __restrict__ in, const uint32_t* __restrict__ input_wire,
                                      Fr* __restrict__ w, uint32_t n_inputs, size_t Bp) {
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (uint32_t i = blockIdx.y; i < n_inputs; i += gridDim.y) {
    const uint32_t wire = input_wire[i];
    if (wire != SCS_NONE) bi_st(w, wire, lane, Bp, bi_ld(in, i, lane, Bp));
  }
}

template <int S>
static void launch_scs_solve(zkmi_ctx* ctx, const zkmi_scs_solver* s, Fr* w, int32_t* status, size_t Bp,
                             uint32_t begin, uint32_t end) {
  const auto kernel = s->ext ? scs_solve_kernel<S, true> : scs_solve_kernel<S, false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(Bp * S / 64)), dim3(64), 0, ctx->stream, s->records, s->coefs,
                     s->outs, w, status, Bp, begin, end);
}

const zkmi_scs* scs_solver_system(const zkmi_scs_solver* s) { return s->sys; }
uint32_t scs_solver_inputs(const zkmi_scs_solver* s) { return s->n_inputs; }
uint32_t scs_solver_steps(const zkmi_scs_solver* s) { return s->n_steps; }
size_t scs_solver_commits(const zkmi_scs_solver* s) { return s->commits.size(); }
ScsSolverCommit scs_solver_commit(const zkmi_scs_solver* s, size_t i) {
  const ScsPlan::Commit& c = s->commits[i];
  return ScsSolverCommit{c.step, c.wire, (uint32_t)c.wires.size(), c.wires.data(), s->commit_wires[i]};
}

int scs_solver_stage(zkmi_ctx* ctx, const zkmi_scs_solver* s, const void* inputs, size_t batch, size_t Bp,
                     Fr* staged, Fr* w) {
  int rc;
  if (s->n_inputs) {
    if ((rc = stage_rows(ctx, inputs, s->n_inputs, batch, Bp, staged))) return rc;
    hipLaunchKernelGGL(scs_solve_init_kernel, dim3((unsigned)(Bp / 64), std::min<uint32_t>(s->n_inputs, 4096)),
                       dim3(64), 0, ctx->stream, (const Fr*)staged, s->input_wire, w, s->n_inputs, Bp);
    ZK_HIP(hipGetLastError());
  }
  return ZKMI_OK;
}
// steps [begin, end) of the plan: all of it, or the piece between two boundaries of its commitments
int scs_solver_run_steps(zkmi_ctx* ctx, const zkmi_scs_solver* s, Fr* w, int32_t* status, size_t Bp,
                         uint32_t begin, uint32_t end) {
  if (begin > end || end > s->n_steps || !with_lanes(s->S, [&](auto S) {
        if (begin < end) launch_scs_solve<S>(ctx, s, w, status, Bp, begin, end);
      })) {
    ctx->err = "scs solver: a step range outside the plan, or lanes_per_proof is no power of two, 1 .. 64";
    return ZKMI_ERR_ARG;
  }
  ZK_HIP(hipGetLastError());
  return ZKMI_OK;
}

int scs_solver_run(zkmi_ctx* ctx, const zkmi_scs_solver* s, const void* inputs, size_t batch, size_t Bp,
                   Fr* staged, Fr* w, int32_t* status) {
  const int rc = scs_solver_stage(ctx, s, inputs, batch, Bp, staged, w);
  return rc ? rc : scs_solver_run_steps(ctx, s, w, status, Bp, 0, s->n_steps);
}

static int solver_load(zkmi_ctx* ctx, const zkmi_scs* m, const zkmi_scs_solver_desc* d, zkmi_scs_solver** out) {
  const size_t ng = m->n_gates;
  // the loaded system on the host: its selectors come back as the 2^261 images of zkmi_scs_load;
  // 2^251 is the Montgomery image of 2^-5, which takes them to gnark's image again
  std::vector<Fr> sel;
  if (!fetch(sel, m->sel, 5 * ng)) {
    ctx->err = "scs solver: cannot read the loaded system back";
    return ZKMI_ERR_HIP;
  }
  Fr down5 = Fr::zero();
  down5.v[7] = 1u << 27;
  for (size_t i = 0; i < 4 * ng; i++) sel[i] = mul(sel[i], down5);
  // the description, on the host; every size below is the caller's own number, bounded by the
  // system's before it sizes a copy
  std::vector<uint32_t> input_wire, instr, hkind, in_ptr, in_wire, out_ptr, houts;
  std::vector<Fr> in_coef;
  const size_t cap = (size_t)m->n_wires + 2 * (size_t)d->n_instr;
  bool ok = d->n_inputs <= m->n_wires + (size_t)m->n_gates && d->n_instr <= 2 * ((size_t)m->n_wires + ng) &&
            d->n_hints <= d->n_instr;
  ok = ok && fetch(input_wire, d->input_wire, d->n_inputs) && fetch(instr, d->instr, (size_t)d->n_instr * 2);
  if (ok && d->n_hints) {
    ok = fetch(hkind, d->hint_kind, d->n_hints) && fetch(in_ptr, d->hint_in_ptr, (size_t)d->n_hints + 1) &&
         fetch(out_ptr, d->hint_out_ptr, (size_t)d->n_hints + 1);
    ok = ok && in_ptr[d->n_hints] <= cap && out_ptr[d->n_hints] <= cap &&
         fetch(in_wire, d->hint_in_wire, in_ptr[d->n_hints]) && fetch(in_coef, d->hint_in_coef, in_ptr[d->n_hints]) &&
         fetch(houts, d->hint_out, out_ptr[d->n_hints]);
  }
  if (!ok) {
    ctx->err = "scs solver: cannot read the instruction list or the hint table (null, or larger than the system allows)";
    return ZKMI_ERR_ARG;
  }
  zkmi_scs_solver_desc hd = *d;
  hd.input_wire = input_wire.data();
  hd.instr = instr.data();
  hd.hint_kind = hkind.data();
  hd.hint_in_ptr = in_ptr.data();
  hd.hint_in_wire = in_wire.data();
  hd.hint_in_coef = in_coef.data();
  hd.hint_out_ptr = out_ptr.data();
  hd.hint_out = houts.data();
  ScsPlanIn in;
  in.n_wires = m->n_wires;
  in.n_gates = m->n_gates;
  in.n_public = m->n_public;
  for (int c = 0; c < 3; c++) in.x[c] = m->hx[c].data();
  in.sel = sel.data();
  in.desc = &hd;
  ScsPlan plan;
  const std::string err = scs_plan_build(in, &plan, ZKMI_HINTS_STD);
  if (!err.empty()) {
    ctx->err = err;
    return ZKMI_ERR_ARG;
  }
  // qL qR qO qM of every row as 2^261 images, for the 29-bit products
  for (size_t r = 0; r < plan.coefs.size(); r += SCS_COEF_ROW)
    for (int q = 0; q < 4; q++)
      for (int t = 0; t < 5; t++) plan.coefs[r + q] = add(plan.coefs[r + q], plan.coefs[r + q]);
  auto* s = new zkmi_scs_solver();
  s->n_inputs = d->n_inputs;
  s->n_instr = plan.n_instr;
  s->S = plan.S;
  s->n_records = plan.n_records;
  s->n_steps = plan.n_steps;
  s->n_levels = plan.n_levels;
  s->n_inversions = plan.n_inversions;
  s->sys = new zkmi_scs();
  s->sys->n_wires = m->n_wires;
  s->sys->n_gates = m->n_gates;
  s->sys->n_public = m->n_public;
  static_assert(sizeof(ScsRecord) == 2 * sizeof(uint4), "record = two quads");
  ok = upload(&s->records, plan.records.data(), plan.records.size() * 2) &&
       upload(&s->coefs, plan.coefs.data(), plan.coefs.size()) &&
       upload(&s->outs, plan.outs.data(), plan.outs.size()) &&
       upload(&s->input_wire, plan.input_wire.data(), plan.input_wire.size()) &&
       upload(&s->sys->marks, m->marks, ng) && upload(&s->sys->sel, m->sel, 5 * ng);
  for (int c = 0; ok && c < 3; c++) {
    s->sys->hx[c] = m->hx[c];
    ok = upload(&s->sys->x[c], m->x[c], ng);
  }
  s->commits = plan.commits;
  s->ext = plan.std_records || !s->commits.empty();
  for (size_t i = 0; ok && i < s->commits.size(); i++) {
    s->commit_wires.push_back(nullptr);
    ok = upload(&s->commit_wires.back(), s->commits[i].wires.data(), s->commits[i].wires.size());
  }
  if (!ok) {
    ctx->err = "scs solver: device upload failed";
    zkmi_scs_solver_free(ctx, s);
    return ZKMI_ERR_HIP;
  }
  *out = s;
  return ZKMI_OK;
}

}  // namespace zk

extern "C" {

void zkmi_scs_solver_free(zkmi_ctx* ctx, zkmi_scs_solver* s) {
  if (!s) return;
  if (ctx) {
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    sync_side_streams(ctx);
  }
  if (s->records) hipFree(s->records);
  if (s->coefs) hipFree(s->coefs);
  if (s->outs) hipFree(s->outs);
  if (s->input_wire) hipFree(s->input_wire);
  for (uint32_t* p : s->commit_wires)
    if (p) hipFree(p);
  zkmi_scs_free(ctx, s->sys);
  delete s;
}

int zkmi_scs_solver_load(zkmi_ctx* ctx, const zkmi_scs* scs, const zkmi_scs_solver_desc* desc,
                         zkmi_scs_solver** out) {
  if (!ctx) return ZKMI_ERR_ARG;
  ZK_HIP(hipSetDevice(ctx->device));
  if (!scs || !desc || !out) {
    ctx->err = "scs solver: null argument";
    return ZKMI_ERR_ARG;
  }
  *out = nullptr;
  try {
    return solver_load(ctx, scs, desc, out);
  } catch (const std::bad_alloc&) {
    ctx->err = "scs solver: out of host memory while building the plan";
    return ZKMI_ERR_OOM;
  }
}

int zkmi_scs_solver_info(const zkmi_scs_solver* s, uint64_t* info) {
  if (!s || !info) return ZKMI_ERR_ARG;
  info[0] = s->n_instr;
  info[1] = s->S;
  info[2] = s->n_records;
  info[3] = s->n_steps;
  info[4] = s->n_inversions;
  info[5] = s->sys->n_wires;
  info[6] = s->sys->n_gates;
  info[7] = s->n_inputs;
  return ZKMI_OK;
}

}  // extern "C"
