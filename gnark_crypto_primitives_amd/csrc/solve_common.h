// Device helpers shared by the kernels that work in gnark's image on the 29-bit products: the PLONK
// rounds and the gate check (plonk.hip), the R1CS row evaluation (witness.hip) and the two
// gnark-shaped solvers (r1cs_solve.hip, scs_solve.hip).  One definition each; all are inlined.
#pragma once
#include "ff29.h"
#include "ff29_asm.h"
#include "scs_check.h"   // the selector marks

namespace zk {

// a b 2^-261 on the 9 x 29-bit form (the single-accumulator asm chain of ff29_asm.h: ~365
// instructions with unpack and canonical pack, ~540 for ff.h's mul).  ff.h's mul computes
// a b 2^-256, so exponents are tracked instead of converting data: write im_e(x) = x 2^e mod r
// (gnark's image is e = 256); then
//     fmulp(im_e1(x), im_e2(y)) = im_(e1 + e2 - 261)(x y),
// sums need equal exponents, and every key-side operand is stored (coefficients and selectors as
// 2^261 images: zkmi_r1cs_load, zkmi_scs_load, plonk_pk_load) or every per-proof scalar converted
// once (fmulp by the constant 2^(e' - e + 261)) with the exponent that makes the result come out at
// 256 again.  Each kernel's comments carry the exponents.
__device__ __forceinline__ Fr fmulp(const Fr& a, const Fr& b) {
  Fr r;
  pack_canonical<Fr29Params>(r.v, mul_asm(unpack29<Fr29Params>(a.v), unpack29<Fr29Params>(b.v)));
  return r;
}
// x 2^k by doublings: im_e(x) -> im_(e + k)(x); lift(x, 5) makes a value in gnark's image the 2^261
// operand of fmulp
__host__ __device__ static inline Fr lift(Fr x, int k) {
  for (int i = 0; i < k; i++) x = add(x, x);
  return x;
}
// lift(x, K) with the doublings unrolled: the compiler leaves lift(x, 5) a loop, which is what the gate
// check of plonk.hip runs; the step loop of scs_solve_kernel has them in line
template <int K>
__device__ __forceinline__ Fr lift(Fr x) {
#pragma unroll
  for (int i = 0; i < K; i++) x = add(x, x);
  return x;
}
// selector times value by the selector's mark (scs_check.h); q is a 2^261 image
__device__ __forceinline__ Fr sel_term(uint32_t mark, const Fr& x, const Fr* q) {
  if (mark == SCS_MARK_ZERO) return Fr::zero();
  if (mark == SCS_MARK_ONE) return x;
  if (mark == SCS_MARK_MINUS_ONE) return neg(x);
  return fmulp(x, *q);
}
// r1cs_limb (r1cs_plan.h) with the three words it reads chosen by selects, for a pos that differs
// between the lanes of a wavefront: a register array under a per-lane index leaves the registers.
// Bits from 256 on are 0: no word is selected.
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

// The counters of a lookup hint are the low words of its output wires' slots in the batch-inner wire
// matrix w [n_wires][Bp]: zeroed by plain stores, counted by __hip_atomic_fetch_add at agent scope --
// the sub-lanes of a proof, or the queries of one step, may meet on one counter --, read back by
// __hip_atomic_load at the same scope, with stores_complete() between the phases.
__device__ __forceinline__ uint32_t* lookup_counter(Fr* w, uint32_t wire, size_t p, size_t Bp) {
  return reinterpret_cast<uint32_t*>(reinterpret_cast<uint4*>(w) + (size_t)wire * 2 * Bp + p);
}
// every store and atomic this wavefront has issued is complete, and visible at agent scope
__device__ __forceinline__ void stores_complete() {
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
}

}  // namespace zk
