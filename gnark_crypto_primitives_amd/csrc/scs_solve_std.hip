// The gnark-shaped PLONK solve under ZKMI_HINTS_STD: scs_std_kernel<S> runs a plan (scs_plan.h) that
// holds records of the classes SK_LIMBS .. SK_COUNT_END beside the four of scs_solve_kernel<S>
// (scs_solve.hip), over a range of steps, so that the caller can stop at a commitment's boundary,
// form the commitment and go on.  A plan without such records keeps running scs_solve_kernel.
//
// Same model as scs_solve_kernel: one wavefront = 64 / S proofs x S sub-lanes, a wave-uniform step
// loop, the class read through readfirstlane, the record fetched one step ahead (the records are
// contiguous and end in a step of padding, so the fetch ahead of `end` stays inside the array), the
// wire matrix batch-inner in gnark's 2^256 image, products on the 29-bit chain against 2^261 images,
// visibility between steps by a wavefront-scope fence.
//
// The lookup counters are the low words of the output wires' rows, as in r1cs_solve.hip: zeroed by
// plain stores that are complete (vmcnt(0), agent-scope fence) before the step ends, counted by
// __hip_atomic_fetch_add at agent scope from every counting sub-lane -- the queries of one step may
// meet on one counter --, read back by __hip_atomic_load at the same scope behind another fence.  The
// three phases are three levels of the plan, so three different steps.
// Bits and limbs under a per-lane index come out of chains of selects, never an indexed register array.
// There is no CPU fallback in this file.
#include "zkmi_internal.h"
#include "ff29.h"
#include "ff29_asm.h"
#include "scs_plan.h"

using namespace zk;

namespace zk {

// a b 2^-261 on the asm chain of ff29_asm.h (scs_fmulp of scs_solve.hip)
__device__ __forceinline__ Fr std_fmulp(const Fr& a, const Fr& b) {
  Fr r;
  pack_canonical<Fr29Params>(r.v, mul_asm(unpack29<Fr29Params>(a.v), unpack29<Fr29Params>(b.v)));
  return r;
}
// x 2^5: a 2^256 image as the 2^261 operand of std_fmulp
__device__ __forceinline__ Fr std_lift5(Fr x) {
#pragma unroll
  for (int i = 0; i < 5; i++) x = add(x, x);
  return x;
}
// selector times value by the selector's mark (scs_check.h); q is a 2^261 image
__device__ __forceinline__ Fr std_sel_term(uint32_t mark, const Fr& x, const Fr* q) {
  if (mark == SCS_MARK_ZERO) return Fr::zero();
  if (mark == SCS_MARK_ONE) return x;
  if (mark == SCS_MARK_MINUS_ONE) return neg(x);
  return std_fmulp(x, *q);
}
// r1cs_limb (r1cs_plan.h) with the three words it reads chosen by selects: pos differs between the
// sub-lanes.  Bits from 256 on are 0: no word is selected.
__device__ __forceinline__ uint64_t std_limb(const Fr& v, uint32_t pos, uint32_t wd) {
  const uint32_t i = pos >> 5, sh = pos & 31;
  uint32_t w0 = 0, w1 = 0, w2 = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    w0 = i == (uint32_t)k ? v.v[k] : w0;
    w1 = i + 1 == (uint32_t)k ? v.v[k] : w1;
    w2 = i + 2 == (uint32_t)k ? v.v[k] : w2;
  }
  uint64_t r = ((uint64_t)w1 << 32 | w0) >> sh;
  if (sh) r |= (uint64_t)w2 << (64 - sh);
  return wd >= 64 ? r : r & (((uint64_t)1 << wd) - 1);
}
// the counter of a lookup: the low word of lane p of the wire's row
__device__ __forceinline__ uint32_t* std_counter(Fr* w, uint32_t wire, size_t p, size_t Bp) {
  return reinterpret_cast<uint32_t*>(reinterpret_cast<uint4*>(w) + (size_t)wire * 2 * Bp + p);
}

// Steps [begin, end) of the plan.  All counts and indices come from a plan that scs_plan_build has
// checked: a wire index is below n_wires, outs[target + j] exists for every j a record names, and a
// query counts only below its table's size.
template <int S>
__global__ __launch_bounds__(64) void scs_std_kernel(const uint4* __restrict__ recs,
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
    const uint32_t xcls = __builtin_amdgcn_readfirstlane(q1.w);
    const uint32_t cls = xcls ? xcls : __builtin_amdgcn_readfirstlane(ctl >> SCS_CTL_CLASS) & 3;
    const Fr* q = coefs + (size_t)q1.y * SCS_COEF_ROW;
    const bool store = ctl & SCS_CTL_STORE;
    Fr va = Fr::zero(), vb = Fr::zero(), vc = Fr::zero();
    if (ctl >> SCS_CTL_READ & 1) va = bi_ld(w, q0.x, p, Bp);
    if (ctl >> (SCS_CTL_READ + 1) & 1) vb = bi_ld(w, q0.y, p, Bp);
    if (ctl >> (SCS_CTL_READ + 2) & 1) vc = bi_ld(w, q0.z, p, Bp);
    const Fr ta = std_sel_term(ctl & 3, va, q), tb = std_sel_term((ctl >> 2) & 3, vb, q + 1);
    // the known part of the gate (a hint: its input), in gnark's image: 256 + 261 - 261
    Fr rest = add(add(ta, tb), std_sel_term((ctl >> 4) & 3, vc, q + 2));
    const bool has_c = ((ctl >> 8) & 3) != SCS_MARK_ZERO;
    if (has_c) rest = add(rest, q[4]);
    const uint32_t mm = (ctl >> 6) & 3, mk = (ctl >> SCS_CTL_MARK_K) & 3;
    if (cls == SK_NBITS) {
      const Fr v = from_mont(rest);
      const uint32_t j0 = q1.z & 0xffffu, cnt = q1.z >> 16;
      for (uint32_t j = 0; j < cnt; j++) {
        const uint32_t at = j0 + j;
        uint32_t word = at < 256 ? v.v[0] : 0u;
#pragma unroll
        for (int i = 1; i < 8; i++) word = (at >> 5) == (uint32_t)i ? v.v[i] : word;
        const uint32_t bit = (word >> (at & 31)) & 1u;
        bi_st(w, outs[q0.w + j], p, Bp, bit ? Fr::one() : Fr::zero());
      }
    } else if (cls == SK_LIMBS) {
      const Fr v = from_mont(rest);
      const uint32_t j0 = q1.z & 0xffffu, cnt = store ? (q1.z >> 16) & 0xffu : 0u, width = q1.z >> 24;
      for (uint32_t j = 0; j < cnt; j++)
        bi_st(w, outs[q0.w + j], p, Bp, r1cs_small(std_limb(v, (j0 + j) * width, width)));
    } else if (cls == SK_BYTEOP) {
      // the two terms on their own: a constant one sits in qC (a) or K (b)
      const uint32_t u = from_mont(has_c ? add(ta, q[4]) : ta).v[0];
      const uint32_t v = from_mont(mk != SCS_MARK_ZERO ? add(tb, q[5]) : tb).v[0];
      if (store) bi_st(w, q0.w, p, Bp, r1cs_small(q1.z == 1 ? u ^ v : u & v));
    } else if (cls == SK_COUNT_ZERO) {
      const uint32_t cnt = store ? q1.z >> 16 : 0u;
      for (uint32_t j = 0; j < cnt; j++) bi_st(w, outs[q0.w + j], p, Bp, Fr::zero());
      // the zeroes are complete before the first count
      __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
    } else if (cls == SK_COUNT_Q) {
      // a query outside the table counts nowhere
      const Fr v = from_mont(rest);
      if (store && (v.v[1] | v.v[2] | v.v[3] | v.v[4] | v.v[5] | v.v[6] | v.v[7]) == 0 && v.v[0] < q1.z)
        __hip_atomic_fetch_add(std_counter(w, outs[q0.w + v.v[0]], p, Bp), 1u, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    } else if (cls == SK_COUNT_END) {
      // the counts are complete; integers into field images, in place
      __builtin_amdgcn_s_waitcnt(0x0F70);
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
      const uint32_t cnt = store ? q1.z >> 16 : 0u;
      for (uint32_t j = 0; j < cnt; j++) {
        const uint32_t wire = outs[q0.w + j];
        bi_st(w, wire, p, Bp,
              r1cs_small(__hip_atomic_load(std_counter(w, wire, p, Bp), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
      }
    } else {
      Fr x;
      if (cls == SK_LIN) {
        // x = K rest, K = -1 / k
        if (mm != SCS_MARK_ZERO) rest = add(rest, std_sel_term(mm, std_fmulp(va, std_lift5(vb)), q + 3));
        x = mk == SCS_MARK_ONE ? rest : mk == SCS_MARK_MINUS_ONE ? neg(rest) : std_fmulp(rest, std_lift5(q[5]));
      } else {
        // DIV: x = -rest / (k + qM other); INVZERO: x = 1 / rest, 0 for 0 (the inverse of 0 is 0)
        Fr den = rest;
        if (cls == SK_DIV) {
          den = std_sel_term(mm, ctl & SCS_CTL_OTHER_A ? va : vb, q + 3);
          if (mk != SCS_MARK_ZERO) den = add(den, q[5]);
          if (store && den.is_zero()) st = ZKMI_ERR_UNSATISFIED;
        }
        const Fr inv = inverse(den);
        x = cls == SK_DIV ? neg(std_fmulp(rest, std_lift5(inv))) : inv;
      }
      if (store) bi_st(w, q0.w, p, Bp, x);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  }
  if (st) status[p] = st;
}

template <int S>
static void launch_scs_std(hipStream_t stream, const uint4* recs, const Fr* coefs, const uint32_t* outs, Fr* w,
                           int32_t* status, size_t Bp, uint32_t begin, uint32_t end) {
  hipLaunchKernelGGL(scs_std_kernel<S>, dim3((unsigned)(Bp * S / 64)), dim3(64), 0, stream, recs, coefs, outs, w,
                     status, Bp, begin, end);
}

// steps [begin, end) of a plan with S lanes per proof on `stream`; false: S is no lane count
bool scs_std_launch(hipStream_t stream, uint32_t S, const uint4* recs, const Fr* coefs, const uint32_t* outs, Fr* w,
                    int32_t* status, size_t Bp, uint32_t begin, uint32_t end) {
  decltype(&launch_scs_std<1>) launch;
  switch (S) {
    case 1: launch = launch_scs_std<1>; break;
    case 2: launch = launch_scs_std<2>; break;
    case 4: launch = launch_scs_std<4>; break;
    case 8: launch = launch_scs_std<8>; break;
    case 16: launch = launch_scs_std<16>; break;
    case 32: launch = launch_scs_std<32>; break;
    case 64: launch = launch_scs_std<64>; break;
    default: return false;
  }
  if (begin < end) launch(stream, recs, coefs, outs, w, status, Bp, begin, end);
  return true;
}

}  // namespace zk
