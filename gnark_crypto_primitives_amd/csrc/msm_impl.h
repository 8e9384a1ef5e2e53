// Templates of the batched MSM (msm.hip has the overview): the kernels, the table builds and one
// launch routine per table layout, all over the coordinate field F = Fq (G1) or Fq2 (G2).
// Included by msm.hip, which instantiates the G1 side, and by msm_g2.hip, which holds the G2
// instantiations of the table-build and launch routines: each is several minutes of hipcc, and the
// two objects compile in parallel.
#pragma once
#include "zkmi_internal.h"
#include "ec29.h"
#include "comb_sign.h"
#include "bit_transpose.h"
#include "msm_part_layout.h"

namespace zk {

ZK_HD Fq to_r261_domain(const Fq& x) {
  Fq k;
#pragma unroll
  for (int i = 0; i < 8; i++) k.v[i] = Fq29Params::k261(i);
  return mul(x, k);
}
ZK_HD Fq2 to_r261_domain(const Fq2& x) { return Fq2{to_r261_domain(x.c0), to_r261_domain(x.c1)}; }

// ---- table construction ------------------------------------------------------------------------
// Table entries are produced in XYZZ and made affine in segments of at most 512 entries with one
// Montgomery batch inversion per segment: push() stores entry d of the segment with its zz, zzz
// and the running product of the zzz before it, finish() inverts the product once and walks
// back.  The scratch (3 * seg_len elements per thread) is interleaved across the T threads of the
// launch so that lanes touch adjacent addresses.  Entries are stored as x*2^261, y*2^261
// (canonical): the accumulate kernels work in the 2^261 domain of ff29.h and only unpack limbs.
template <class F>
struct SegInv {
  F *szz, *szzz, *spre;
  size_t T;
  F pref = F::one();
  __device__ SegInv(F* scratch, uint32_t t, uint32_t T_, uint32_t seg_len)
      : szz(scratch + t), szzz(scratch + (size_t)seg_len * T_ + t),
        spre(scratch + (size_t)2 * seg_len * T_ + t), T(T_) {}
  __device__ void push(Affine<F>* seg, uint32_t d, const F& x, const F& y, const F& zz,
                       const F& zzz) {
    seg[d].x = x;
    seg[d].y = y;
    szz[d * T] = zz;
    szzz[d * T] = zzz;
    spre[d * T] = pref;
    pref = mul(pref, zzz);
  }
  __device__ void finish(Affine<F>* seg, uint32_t len) {
    F inv = inverse(pref);
    for (uint32_t d = len; d-- > 0;) {
      const F zzz = szzz[d * T];
      const F izzz = mul(inv, spre[d * T]);
      inv = mul(inv, zzz);
      const F izz = sqr(mul(izzz, szz[d * T]));
      seg[d].x = to_r261_domain(mul(seg[d].x, izz));
      seg[d].y = to_r261_domain(mul(seg[d].y, izzz));
    }
    pref = F::one();
  }
};

// One thread per table row: (base) for a shared table, (base, window) for per-window tables, whose
// first entry Q = 2^(shift_j) P is reached by shift_j doublings.  A row is a running sum
// d * Q, d = 1..D.
template <class F>
__global__ __launch_bounds__(64) void msm_build_table(const Affine<F>* __restrict__ bases,
                                                      uint64_t r0, uint64_t n_rows, WinPlan plan,
                                                      Affine<F>* __restrict__ table,
                                                      F* __restrict__ scratch, uint32_t T,
                                                      uint32_t seg_len) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t r = r0 + t;
  if (t >= T || r >= n_rows) return;
  uint32_t D;
  Affine<F>* row;
  Affine<F> Q;
  if (plan.shared) {
    D = plan.per_base;
    row = table + (size_t)r * plan.per_base;
    Q = bases[r];
  } else {
    const uint32_t i = (uint32_t)(r / (uint32_t)plan.W), j = (uint32_t)(r % (uint32_t)plan.W);
    D = 1u << (plan.bits[j] - 1);
    row = table + (size_t)i * plan.per_base + plan.off[j];
    Q = bases[i];
    if (!Q.is_inf() && j) {
      uint32_t shift = 0;
      for (uint32_t k = 0; k < j; k++) shift += plan.bits[k];
      XYZZ<F> a = XYZZ<F>::from_affine(Q);
      for (uint32_t k = 0; k < shift; k++) a = dbl(a);
      Q = to_affine(a);
    }
  }
  if (Q.is_inf()) {
    for (uint32_t d = 0; d < D; d++) row[d] = Affine<F>::inf();
    return;
  }
  SegInv<F> inv(scratch, t, T, seg_len);
  XYZZ<F> acc = XYZZ<F>::inf();
  for (uint32_t s0 = 0; s0 < D; s0 += seg_len) {
    Affine<F>* seg = row + s0;
    const uint32_t len = D - s0 < seg_len ? D - s0 : seg_len;
    for (uint32_t d = 0; d < len; d++) {
      madd(acc, Q);
      inv.push(seg, d, acc.x, acc.y, acc.zz, acc.zzz);
    }
    inv.finish(seg, len);
  }
}

// ---- accumulation --------------------------------------------------------------------------------
// grid: x over proofs (Bp / blockDim.x), y over chunks of bases.  c, W wave-uniform.
// The accumulator lives in the 9 x 29-bit lazy representation (ff29.h / ec29.h): every field
// product is a carry-free v_mad_i64_i32 chain; G2 shares one Montgomery reduction per Fq2 component.
template <class F> struct Acc29;
template <> struct Acc29<Fq> {
  typedef G1Acc29 type;
  static __device__ __forceinline__ void add(G1Acc29& acc, const G1Affine& e, bool negd) {
    madd29(acc, unpack29<Fq29Params>(e.x.v), cneg(unpack29<Fq29Params>(e.y.v), negd));
  }
};
template <> struct Acc29<Fq2> {
  typedef G2Acc29 type;
  static __device__ __forceinline__ void add(G2Acc29& acc, const G2Affine& e, bool negd) {
    madd29(acc, unpack2_29(e.x), cneg(unpack2_29(e.y), negd));
  }
};

// Accumulator of the comb kernels.  G1: registers (36 + 18 for the entry: 128 VGPRs, no spills).
// G2 at two waves per SIMD has 256 VGPRs for a 72-limb accumulator, a 36-limb entry and ~90 limbs of
// temporaries: the compiler spilled ~100 registers to scratch (27.9 GB of scratch writes per launch in
// the round-2 PMC pass).  zz and zzz are only touched at the two ends of a mixed addition, so they
// live in LDS instead (36 words x 256 lanes = 36 KB per workgroup, [limb][lane]: conflict-free) and
// are re-read where the addition needs them the second time.
template <class F> struct CombAcc;
template <> struct CombAcc<Fq> {
  static constexpr int LDS_ROWS = 1;   // unused
  typedef G1Acc29 type;
  static __device__ __forceinline__ type init(int32_t (*)[256], uint32_t) { return G1Acc29::infinity(); }
  static __device__ __forceinline__ void add(type& acc, const G1Affine& e, bool negd,
                                             int32_t (*)[256], uint32_t) {
    Acc29<Fq>::add(acc, e, negd);
  }
  static __device__ __forceinline__ Part29<Fq> result(const type& acc, int32_t (*)[256], uint32_t) {
    return pack_part(acc);
  }
};
struct G2AccL {
  Fq2_29 x, y;
  bool inf;
};
static __device__ __forceinline__ Fq2_29 lds_ld2(int32_t (*z)[256], int row0, uint32_t t) {
  Fq2_29 r;
#pragma unroll
  for (int l = 0; l < 9; l++) {
    r.c0.v[l] = z[row0 + l][t];
    r.c1.v[l] = z[row0 + 9 + l][t];
  }
  return r;
}
static __device__ __forceinline__ void lds_st2(int32_t (*z)[256], int row0, uint32_t t,
                                               const Fq2_29& a) {
#pragma unroll
  for (int l = 0; l < 9; l++) {
    z[row0 + l][t] = a.c0.v[l];
    z[row0 + 9 + l][t] = a.c1.v[l];
  }
}
template <> struct CombAcc<Fq2> {
  static constexpr int LDS_ROWS = 36;  // zz: rows 0..17, zzz: rows 18..35
  typedef G2AccL type;
  static __device__ __forceinline__ type init(int32_t (*)[256], uint32_t) {
    G2AccL a;
    a.x = a.y = Fq2_29::zero();
    a.inf = true;
    return a;
  }
  // ec29.h madd29(G2Acc29&, ...) with zz / zzz in LDS
  static __device__ __forceinline__ void add(type& acc, const G2Affine& e, bool negd,
                                             int32_t (*z)[256], uint32_t t) {
    const Fq2_29 qx = unpack2_29(e.x), qy = cneg(unpack2_29(e.y), negd);
    if (acc.inf) {
      acc.x = qx;
      acc.y = norm(qy);
      lds_st2(z, 0, t, Fq2_29::one());
      lds_st2(z, 18, t, Fq2_29::one());
      acc.inf = false;
      return;
    }
    const Fq2_29 u2 = mmul(qx, lds_ld2(z, 0, t));
    const Fq2_29 s2 = mmul(qy, lds_ld2(z, 18, t));
    const Fq2_29 p = sub(u2, acc.x);
    const Fq2_29 r = sub(s2, acc.y);
    const Fq2_29 pp = msqr(p);
    const Fq2_29 rr = msqr(r);
    if (is_zero_mulout(pp)) {
      if (is_zero_mulout(rr)) {
        G2Acc29 d;
        d.inf = false;
        mdbl29(d, qx, qy);
        acc.x = d.x;
        acc.y = d.y;
        lds_st2(z, 0, t, d.zz);
        lds_st2(z, 18, t, d.zzz);
      } else {
        acc.inf = true;
      }
      return;
    }
    const Fq2_29 ppp = mmul(p, pp);
    const Fq2_29 q = mmul(acc.x, pp);
    const Fq2_29 x3 = wred(sub(sub(rr, ppp), zk::add(q, q)));
    const Fq2_29 y3 = wred(sub(mmul(r, sub(q, x3)), mmul(acc.y, ppp)));
    uint32_t t2 = t;                     // opaque copy of the lane index: the second read of zz / zzz
    asm volatile("" : "+v"(t2));         // must be a new LDS read, not the first one kept in registers
    lds_st2(z, 0, t2, mmul(lds_ld2(z, 0, t2), pp));
    lds_st2(z, 18, t2, mmul(lds_ld2(z, 18, t2), ppp));
    acc.x = x3;
    acc.y = y3;
  }
  static __device__ __forceinline__ Part29<Fq2> result(const type& acc, int32_t (*z)[256], uint32_t t) {
    G2Acc29 a = G2Acc29::infinity();
    if (!acc.inf) {
      a.x = acc.x;
      a.y = acc.y;
      a.zz = lds_ld2(z, 0, t);
      a.zzz = lds_ld2(z, 18, t);
      a.inf = false;
    }
    return pack_part(a);
  }
};

// ONE_BASE only changes the symbol name: the one-base launches (delta multiples in the assembly,
// zkmi_fixed_base_mul) then show up separately from the proving-key MSMs in rocprofv3 statistics.
template <class F, bool ONE_BASE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void msm_accumulate(const Affine<F>* __restrict__ table,
                                                      const Fr* __restrict__ scalars,
                                                      const uint32_t* __restrict__ row_idx,
                                                      size_t Bp, uint32_t n, uint32_t per_chunk,
                                                      WinPlan plan, Part29<F>* __restrict__ partial,
                                                      Fr kmul, const uint8_t* __restrict__ inf) {
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t chunk = blockIdx.y;
  const uint32_t i0 = chunk * per_chunk;
  uint32_t i1 = i0 + per_chunk;
  if (i1 > n) i1 = n;
  const int W = plan.W;
  typename Acc29<F>::type acc = Acc29<F>::type::infinity();
  for (uint32_t i = i0; i < i1; i++) {
    if (inf[i]) continue;   // wave-uniform: the point at infinity contributes nothing
    const uint32_t row = row_idx ? row_idx[i] : i;
    // Montgomery image -> integer: product by the plain constant 1 (gnark's x*2^256) or by
    // 2^-5 (the solver's x*2^261)
    Fr s = mul(bi_ld(scalars, row, b, Bp), kmul);
    if (s.is_zero()) continue;
    const Affine<F>* trow = table + (size_t)i * plan.per_base;
    uint32_t carry = 0;
    for (int j = 0; j < W; j++) {
      const int c = plan.bits[j];                 // wave-uniform
      const uint32_t mask = (1u << c) - 1u;
      const uint32_t half = 1u << (c - 1);
      uint32_t d = (s.v[0] & mask) + carry;
#pragma unroll
      for (int l = 0; l < 7; l++) s.v[l] = (s.v[l] >> c) | (s.v[l + 1] << (32 - c));
      s.v[7] >>= c;
      const bool negd = d > half;
      carry = negd ? 1u : 0u;
      const uint32_t mag = negd ? (mask + 1u - d) : d;
      if (mag) {
        const Affine<F> e = trow[plan.off[j] + (mag - 1)];
        Acc29<F>::add(acc, e, negd);
      }
    }
  }
  partial[(size_t)chunk * Bp + b] = pack_part(acc);
}

// ---- shared-table path: one table per base, one accumulator per (window, chunk) -------------------
// The per-window tables above spend HBM on 2^(c_j) multiples of 2^(shift_j) P for EVERY window.
// With a single table of d * P the same HBM holds windows ~5 bits wider (c = 15 instead of ~10 for
// the Arbo-160 key: 17 mixed additions per (base, proof) instead of 25); the price is that the
// windows can no longer share an accumulator.  Lane = proof makes that free: the window index is a
// third grid dimension, every (window, chunk) block keeps its own register accumulator, and the W
// window sums of a proof are combined once per MSM with Horner's rule (255 doublings per proof,
// not per base).
//
// Signed digits without a carry chain: with K = sum_j 2^(pos_j + c_j - 1) and s' = s + K, digit j
// is ((s' >> pos_j) & (2^c_j - 1)) - 2^(c_j - 1), each in [-2^(c_j-1), 2^(c_j-1)).  One pass
// converts the Montgomery scalars to integers and stores the digits as int16, [window][base][proof].
static __global__ __launch_bounds__(256) void msm_digits_kernel(const Fr* __restrict__ scalars,
                                                         const uint32_t* __restrict__ row_idx,
                                                         size_t Bp, uint32_t n, WinPlan plan,
                                                         int32_t kmul32, Fr koff,
                                                         const uint8_t* __restrict__ inf,
                                                         int16_t* __restrict__ digits) {
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (uint32_t i = blockIdx.y; i < n; i += gridDim.y) {
    if (inf[i]) {   // wave-uniform: the point at infinity contributes nothing
      for (int j = 0; j < plan.W; j++) digits[((size_t)j * n + i) * Bp + b] = 0;
      continue;
    }
    const uint32_t row = row_idx ? row_idx[i] : i;
    // Montgomery image -> integer on the 29-bit form: x*2^256 * 32 / 2^261 (gnark's image) or
    // x*2^261 * 1 / 2^261 (the solver's)
    Fr29 k = Fr29::zero();
    k.v[0] = kmul32;
    const Fr raw = bi_ld(scalars, row, b, Bp);
    Fr s;
    pack_canonical<Fr29Params>(s.v, mul(unpack29<Fr29Params>(raw.v), k));
    uint64_t cy = 0;
#pragma unroll
    for (int l = 0; l < 8; l++) {
      cy += (uint64_t)s.v[l] + koff.v[l];
      s.v[l] = (uint32_t)cy;
      cy >>= 32;
    }
    uint32_t pos = 0;
    for (int j = 0; j < plan.W; j++) {
      const uint32_t c = plan.bits[j];              // wave-uniform
      const uint32_t w = pos >> 5, sh = pos & 31u;
      uint32_t v = s.v[w] >> sh;
      if (sh && w + 1 < 8) v |= s.v[w + 1] << (32u - sh);
      const int32_t d = (int32_t)(v & ((1u << c) - 1u)) - (int32_t)(1u << (c - 1));
      digits[((size_t)j * n + i) * Bp + b] = (int16_t)d;
      pos += c;
    }
  }
}

// grid: x over proofs, y over windows, z over chunks of bases (all windows of a chunk are dispatched
// together, so the blocks that walk the same tables run at the same time)
template <class F>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void
msm_accumulate_shared(const Affine<F>* __restrict__ table, const int16_t* __restrict__ digits,
                      size_t Bp, uint32_t n, uint32_t per_chunk, uint32_t per_base,
                      Part29<F>* __restrict__ partial) {
  // (an XCD-aware deal of the chunks -- all blocks of a chunk on one L2 -- measured no better)
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t chunk = blockIdx.z, j = blockIdx.y;
  const uint32_t i0 = chunk * per_chunk;
  uint32_t i1 = i0 + per_chunk;
  if (i1 > n) i1 = n;
  const int16_t* dj = digits + (size_t)j * n * Bp + b;
  typename Acc29<F>::type acc = Acc29<F>::type::infinity();
  for (uint32_t i = i0; i < i1; i++) {
    const int32_t d = dj[(size_t)i * Bp];
    if (d) {
      const bool negd = d < 0;
      const uint32_t mag = (uint32_t)(negd ? -d : d);
      const Affine<F> e = table[(size_t)i * per_base + (mag - 1)];
      Acc29<F>::add(acc, e, negd);
    }
  }
  partial[((size_t)j * gridDim.z + chunk) * Bp + b] = pack_part(acc);
}

// out[b] = sum_j 2^(pos_j) * wsum[j][b]; blockIdx.y selects one of up to four independent sums
template <class F>
struct HornerArgs {
  const XYZZ<F>* wsum[4];
  XYZZ<F>* out[4];
};
template <class F>
__global__ __launch_bounds__(64) void msm_horner(HornerArgs<F> args, size_t Bp, WinPlan plan) {
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= Bp) return;
  const XYZZ<F>* __restrict__ wsum = args.wsum[blockIdx.y];
  XYZZ<F>* __restrict__ out = args.out[blockIdx.y];
  XYZZ<F> acc = wsum[(size_t)(plan.W - 1) * Bp + b];
  for (int j = plan.W - 2; j >= 0; j--) {
    const int c = plan.bits[j];
    for (int k = 0; k < c; k++)
      if (!acc.is_inf()) acc = dbl(acc);
    const XYZZ<F> p = wsum[(size_t)j * Bp + b];
    padd(acc, p);
  }
  out[b] = acc;
}

// ---- comb tables: one mixed addition per (group of k bases, bit, proof) ------------------------------
// A table over single bases spends 2^(c-1) entries per base to consume c scalar bits per addition.
// A JOINT table over k bases with one-bit digits, T[g][m] = sum_{i in m} P_{gk+i} for every non-empty
// subset m, spends 2^k / k entries per base and consumes k scalar bits per addition: k = 18 fits
// the HBM that gave c = 15 (14.1 instead of 17 additions per base and proof), and the G2 table
// affords k = 19.  Digits are plain bits -- no signs, no recoding: the index of (group, bit j) is
// bit j of the group's k scalars, 0 = nothing to add.  The 254 window sums go through the same
// chunk reduction and a Horner pass of one doubling per window.
// D[g][t] = P_t - (P_0 + ... + P_{t-1}): entry(m + 1) = entry(m) + D[number of trailing ones of m]
// (signed tables: every step is twice that, so 2 D is stored); gsum[g] = sum of the group's bases
template <class F>
__global__ void comb_prep(const Affine<F>* __restrict__ bases, uint32_t n, uint32_t k,
                          uint32_t n_groups, Affine<F>* __restrict__ dpts,
                          Affine<F>* __restrict__ gsum, int twice) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_groups) return;
  XYZZ<F> s = XYZZ<F>::inf();
  for (uint32_t t = 0; t < k; t++) {
    const size_t i = (size_t)g * k + t;
    const Affine<F> P = i < n ? bases[i] : Affine<F>::inf();
    XYZZ<F> d = s;
    d.y = neg(d.y);
    madd(d, P);
    if (twice) d = dbl(d);
    dpts[i] = to_affine(d);
    madd(s, P);
  }
  gsum[g] = to_affine(s);
}
// sum of the per-group sums (one thread: a few thousand mixed additions, once per key)
template <class F>
__global__ void comb_total(const Affine<F>* __restrict__ gsum, uint32_t n_groups,
                           Affine<F>* __restrict__ out) {
  XYZZ<F> s = XYZZ<F>::inf();
  for (uint32_t g = 0; g < n_groups; g++) madd(s, gsum[g]);
  *out = to_affine(s);
}

// out[i] = c * bases[i], c a plain integer below r (wave-uniform): the bases of a sign-pattern table
// native to a scalar image (build_comb), double-and-add from c's top bit, once per key
template <class F>
__global__ __launch_bounds__(64) void comb_scale_bases(const Affine<F>* __restrict__ bases,
                                                       uint32_t n, Fr c,
                                                       Affine<F>* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = to_affine(scalar_mul(bases[i], c.v));
}

// one thread per (group, segment of seg_len consecutive table indices).
// Unsigned tables: entry m = sum of the bases whose bit is set in m (2^k entries, entry 0 unused).
// SIGNED tables: entry e (k - 1 bits) = P_(k-1) + sum_{i < k-1} (e_i ? +P_i : -P_i): every k-bit
// sign pattern or its complement has its top bit set, and sigma(~M) = -sigma(M), so 2^(k-1) entries
// serve all 2^k patterns -- one more base per group in the same HBM.
template <class F, bool SIGNED>
__global__ __launch_bounds__(64) void comb_build(const Affine<F>* __restrict__ bases,
                                                 const Affine<F>* __restrict__ dpts, uint32_t n,
                                                 uint32_t k, uint64_t r0, uint64_t n_rows,
                                                 Affine<F>* __restrict__ table,
                                                 F* __restrict__ scratch, uint32_t T,
                                                 uint32_t seg_len, int* __restrict__ any_inf) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t r = r0 + t;
  if (t >= T || r >= n_rows) return;
  const uint32_t idx_bits = SIGNED ? k - 1 : k;
  const uint32_t per_group = 1u << idx_bits, segs = per_group / seg_len;
  const uint32_t g = (uint32_t)(r / segs), m0 = (uint32_t)(r % segs) * seg_len;
  Affine<F>* seg = table + (size_t)g * per_group + m0;
  // entry of the first index of the segment; `live` = bases that exist and are finite (the
  // unsigned digit pass never sets the bit of any other base, so masks outside `live` are never
  // gathered; the signed digit pass gathers every pattern, also in a group with no finite base)
  XYZZ<F> acc = XYZZ<F>::inf();
  uint32_t live = 0;
  for (uint32_t i = 0; i < k; i++) {
    const size_t bi = (size_t)g * k + i;
    if (bi >= n) continue;
    const Affine<F> P = bases[bi];
    if (!P.is_inf()) live |= 1u << i;
    if (SIGNED) {
      if (i == k - 1 || ((m0 >> i) & 1u))
        madd(acc, P);
      else
        madd(acc, neg(P));
    } else if ((m0 >> i) & 1u) {
      madd(acc, P);
    }
  }
  SegInv<F> inv(scratch, t, T, seg_len);
  bool inf_seen = false;
  for (uint32_t d = 0; d < seg_len; d++) {
    const bool is_inf = acc.is_inf();
    const uint32_t m = m0 + d;
    inf_seen = inf_seen || (is_inf && (SIGNED || (m != 0 && (m & ~live) == 0)));
    // an identity entry is stored as (0, 0) (0 stays 0 through the inversion and the domain change)
    if (is_inf)
      inv.push(seg, d, F::zero(), F::zero(), F::one(), F::one());
    else
      inv.push(seg, d, acc.x, acc.y, acc.zz, acc.zzz);
    const uint32_t tz = (uint32_t)__builtin_ctz(m + 1);   // trailing ones of the index
    if (tz < idx_bits) madd(acc, dpts[(size_t)g * k + tz]);
  }
  inv.finish(seg, seg_len);
  if (inf_seen) atomicOr(any_inf, 1);
}

// Sign-pattern tables: every scalar is a sum of 254 signed powers of two.  With t the canonical
// image of the scalar that the table is native to (bases->image; the bases were scaled by
// (2 * 2^256)^-1 or (2 * 2^261)^-1 at the build, so that s P = 2 t P''):
//   e = 1 if t is even;  t' = t + e (odd, <= r);  C = (t' + 2^254 - 1) / 2 < 2^254
//   => t' = sum_j (2 C_j - 1) 2^j, and  s P = 2 (t' P'' - e P'').
// Bit j of C is base i's sign in window j; the parities e are the sign pattern of one extra window
// (index 254) whose sum is subtracted once at the end together with the sum of all scaled bases:
//   sum_i s_i P_i = 2 H - W_254 - S,  H = sum_j 2^j W_j  (msm_horner_comb).
// C and e are t's own bits (comb_sign.h): the digit pass reads the scalar rows as they are.
//
// What is left of a scalar pass, same planar layout (row i of the output = base i):
//   * subset-sum tables: the Montgomery image -> the plain integer (kk = 32 or 1 in limb 0: small
//     values stay small); the rows of bases at infinity are zeroed, their bits must stay clear;
//   * sign-pattern tables whose scalars arrive in the other image: image -> native image
//     (kk = 2^266 mod r for gnark's image on an F-native table, 2^256 mod r the other way round).
static __global__ __launch_bounds__(256) void comb_scalars_kernel(const Fr* __restrict__ scalars,
                                                                  const uint32_t* __restrict__ row_idx,
                                                                  size_t Bp, uint32_t n, Fr29 kk,
                                                                  const uint8_t* __restrict__ inf,
                                                                  Fr* __restrict__ out) {
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (uint32_t i = blockIdx.y; i < n; i += gridDim.y) {
    Fr s = Fr::zero();
    if (!inf[i]) {   // wave-uniform
      const uint32_t row = row_idx ? row_idx[i] : i;
      const Fr raw = bi_ld(scalars, row, b, Bp);
      pack_canonical<Fr29Params>(s.v, mul(unpack29<Fr29Params>(raw.v), kk));
    }
    bi_st(out, i, b, Bp, s);
  }
}

// flags[i] = 1 when row (row_idx ? row_idx[i] : i) of `scalars` differs from its lane 0 within the
// first `batch` lanes, else 0; padding lanes do not take part.  The raw words are compared: equal
// words have equal digits in whatever image they are read, so a comb group whose rows are all
// flagged 0 has the same digits in every proof of the batch (comb_split_kernel).  One wave per
// row, which stops at the first 64 lanes that differ; one plain store per wave, every flag written.
static __global__ __launch_bounds__(256) void rows_vary_kernel(const Fr* __restrict__ scalars,
                                                               const uint32_t* __restrict__ row_idx,
                                                               uint32_t n_rows, size_t Bp,
                                                               size_t batch,
                                                               uint8_t* __restrict__ flags) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);   // wave-uniform
  if (i >= n_rows) return;
  const uint32_t row = row_idx ? row_idx[i] : i;
  const Fr raw0 = bi_ld(scalars, row, 0, Bp);   // wave-uniform
  bool var = false;
  for (size_t b0 = 0; b0 < batch && !var; b0 += 64) {
    const size_t b = b0 + lane;   // < Bp: batch <= Bp, a multiple of 64
    const Fr raw = bi_ld(scalars, row, b, Bp);
    uint32_t diff = 0;
#pragma unroll
    for (int l = 0; l < 8; l++) diff |= raw.v[l] ^ raw0.v[l];
    var = __ballot(b < batch && diff != 0) != 0;
  }
  if (lane == 0) flags[i] = var ? 1 : 0;
}

// Splits the groups: a group varies when `dense` is set or a flag of one of its bases is
// (flags[flag_idx ? flag_idx[i] : i] for base i: rows_vary_kernel's output per scalar row, or per
// base).  vlist / ulist = the varying / uniform groups in increasing order,
// vpos[g] = position of g in vlist (~0u: uniform), counts = {|vlist|, |ulist|}.  One workgroup of
// 1024 threads walks the groups in tiles; the counts stay on the device (the accumulate and
// common-sum grids are sized from n_groups and read them there).
static __global__ __launch_bounds__(1024) void comb_split_kernel(const uint8_t* __restrict__ flags,
                                                                 const uint32_t* __restrict__ flag_idx,
                                                                 uint32_t n, uint32_t k, int dense,
                                                                 uint32_t n_groups,
                                                                 uint32_t* __restrict__ vlist,
                                                                 uint32_t* __restrict__ ulist,
                                                                 uint32_t* __restrict__ vpos,
                                                                 uint32_t* __restrict__ counts) {
  __shared__ uint32_t wave_nv[16];
  const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
  uint32_t nv = 0, nu = 0;
  for (uint32_t g0 = 0; g0 < n_groups; g0 += 1024) {
    const uint32_t g = g0 + t;
    const bool live = g < n_groups;
    bool var = live && dense;
    if (live && !dense) {
      uint32_t any = 0;   // no early exit: the k lookups are independent loads
#pragma unroll 8
      for (uint32_t q = 0; q < k; q++) {
        const size_t i = (size_t)g * k + q;
        if (i < n) any |= flags[flag_idx ? flag_idx[i] : i];
      }
      var = any != 0;
    }
    const unsigned long long vm = __ballot(var);
    if (lane == 0) wave_nv[w] = (uint32_t)__popcll(vm);
    __syncthreads();
    uint32_t before = 0, tile_nv = 0;
    for (uint32_t q = 0; q < 16; q++) {
      before += q < w ? wave_nv[q] : 0u;
      tile_nv += wave_nv[q];
    }
    // varying groups of this tile below g; every group of the tile below g exists
    const uint32_t vb = before + (uint32_t)__popcll(vm & ((1ull << lane) - 1ull));
    if (var) {
      vlist[nv + vb] = g;
      vpos[g] = nv + vb;
    } else if (live) {
      ulist[nu + t - vb] = g;
      vpos[g] = ~0u;
    }
    const uint32_t tile = n_groups - g0 < 1024u ? n_groups - g0 : 1024u;
    nv += tile_nv;
    nu += tile - tile_nv;
    __syncthreads();   // wave_nv is rewritten by the next tile
  }
  if (t == 0) {
    counts[0] = nv;
    counts[1] = nu;
  }
}

// A lane's 32-bit byte offset, opaque to the compiler at the place of use: an access at
// scalar base + lane_offset_here(off) is selected as one global_load / global_store with the base
// in scalar registers and the offset in one VGPR.  Without it the compiler widens the offset to 64
// bits once, outside the loop, and every access adds base and offset in two vector registers.
__device__ __forceinline__ uint32_t lane_offset_here(uint32_t off) {
  asm volatile("" : "+v"(off));
  return off;
}

// digits[j][p][b] = sum_i bit_j(s[gk+i][b]) << i for the varying group g = vlist[p].  SIGNED: k-bit
// sign pattern M -> (index, negate): top bit set: entry M & (2^(k-1) - 1); clear: entry
// ~M & (2^(k-1) - 1), negated (bit 31 of the digit).  SIGNED reads the table's native image t as
// it is (base i's row is row_idx[i] of `sint`: the value file itself, or the converted rows):
// comb_sign_window names the window of every bit of t, the bits of window 253 are all ones, and
// rows past n read as zero.  The row of a base at infinity is read like any other: its bits select
// between entries that are equal (or both the identity), whatever they are.
// A uniform group has lane 0's digits in every proof: only lane 0 of the grid transposes it and
// writes d0[j][g] (comb_common_sums).
// The transposes and the sign-pattern digit are bit_transpose.h's.  SIGNED feeds the group's top
// row, k - 1, as row 31 (k is a run-time value, the slot is not), so that a pattern's top bit is
// the sign bit of its window word; the rows below it keep their places 0 .. k - 2.
// Addresses: window, group position and n_groups are wave-uniform, so every load and store is a
// scalar base plus the lane's fixed 32-bit byte offset (b * 16 into a scalar row, b * 4 into a
// window: Bp < 2^28 is the launch routine's check), and the window base advances by one scalar
// stride per digit.  No vector address arithmetic is left in the loops.
// At least three waves per SIMD (at most 168 VGPRs; the 21 x 4 loaded words and the 32 transposed
// ones take 106 and leave room for four): the pass is bound by issue, and at two waves it measured
// 1.4 x slower.  No scratch (profiles/r20_digits_kernel_resources.csv).
template <int KMAX, bool SIGNED>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void comb_digits_kernel(const Fr* __restrict__ sint,
                                                          const uint32_t* __restrict__ row_idx,
                                                          size_t Bp, uint32_t n, uint32_t k,
                                                          uint32_t n_groups,
                                                          const uint32_t* __restrict__ vpos,
                                                          uint32_t* __restrict__ digits,
                                                          uint32_t* __restrict__ d0) {
  constexpr int NLOW = SIGNED ? KMAX - 1 : KMAX;   // row slots below the top one
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t boff16 = b * 16u, boff4 = b * 4u;   // the lane's part of every address
  const char* base = reinterpret_cast<const char*>(sint);
  const size_t row_bytes = Bp * 16;                  // half a scalar row: four words per proof
  const uint32_t low = (1u << (k - 1)) - 1u;
  for (uint32_t g = blockIdx.y; g < n_groups; g += gridDim.y) {
    const uint32_t p = vpos[g];
    const bool uni = p == ~0u;
    if (uni && b != 0) continue;
    // window j of this group: wbase + j * wstride (+ boff4; lane 0 alone is here when uni)
    char* const wbase = uni ? reinterpret_cast<char*>(d0 + g)
                            : reinterpret_cast<char*>(digits + (size_t)p * Bp);
    const size_t wstride = (uni ? (size_t)n_groups : (size_t)n_groups * Bp) * sizeof(uint32_t);
    if (SIGNED)   // window 253: every sign is +, the entry of the all-ones pattern
      *reinterpret_cast<uint32_t*>(wbase + (size_t)COMB_SIGN_ONES * wstride +
                                   lane_offset_here(boff4)) = low;
    // slot i < NLOW holds row i of the group, SIGNED: below the top row k - 1, which has the last
    // slot; ~0: nothing to read (past k, or past n in a short last group)
    size_t rows[KMAX];   // wave-uniform
#pragma unroll
    for (int i = 0; i < KMAX; i++) {
      const uint32_t r = SIGNED && i == NLOW ? k - 1 : (uint32_t)i;
      const bool in_group = SIGNED ? (i == NLOW || (uint32_t)i + 1 < k) : (uint32_t)i < k;
      const size_t bi = (size_t)g * k + r;
      rows[i] = (in_group && bi < n) ? (row_idx ? (size_t)row_idx[bi] : bi) : ~(size_t)0;
    }
    char* wnext = wbase;   // windows come in increasing order but for the parity window: jn is
    int jn = 0;            // the window wnext stands at, a constant once the loops are unrolled
#pragma unroll
    for (int h = 0; h < 2; h++) {
      uint4 wv[KMAX];
#pragma unroll
      for (int i = 0; i < KMAX; i++)
        wv[i] = rows[i] != ~(size_t)0
                    ? *reinterpret_cast<const uint4*>(base + (rows[i] * 2 + h) * row_bytes +
                                                      lane_offset_here(boff16))
                    : make_uint4(0, 0, 0, 0);
#pragma unroll
      for (int c = 0; c < 4; c++) {
        uint32_t m[32];
#pragma unroll
        for (int i = 0; i < 32; i++) {
          const int s = i < NLOW ? i : (SIGNED && i == 31) ? NLOW : -1;
          m[i] = s < 0 ? 0u : c == 0 ? wv[s].x : c == 1 ? wv[s].y : c == 2 ? wv[s].z : wv[s].w;
        }
        bit_transpose32<NLOW, SIGNED>(m);
        const uint32_t woff = lane_offset_here(boff4);
#pragma unroll
        for (int bit = 0; bit < 32; bit++) {
          int j = (h * 4 + c) * 32 + bit;
          bool comp = false;
          if (SIGNED) {
            j = comb_sign_window(h * 4 + c, bit, &comp);
            if (j < 0) continue;        // t < 2^254
          } else if (j >= COMB_W) {
            break;
          }
          const uint32_t x = comp ? ~m[bit] : m[bit];
          char* dst = wbase + (size_t)j * wstride;
          if (j == jn) {
            dst = wnext;
            wnext += wstride;
            jn++;
          }
          *reinterpret_cast<uint32_t*>(dst + woff) = SIGNED ? comb_sign_digit(x, low) : x;
        }
      }
    }
  }
}

// Chunks in use when nv groups vary: a chunk costs the reduction about 1.25 additions of two
// accumulators plus the packing, ~2.2 mixed additions, so a chunk has to be worth
// COMB_MIN_GROUPS_PER_CHUNK of them.  The accumulate kernel and the reduction both derive the
// count from counts[0] on the device; the grid (grid_chunks) is sized from all groups on the host.
__host__ __device__ inline uint32_t comb_eff_chunks(uint32_t nv, uint32_t grid_chunks) {
  const uint32_t want = (nv + COMB_MIN_GROUPS_PER_CHUNK - 1) / COMB_MIN_GROUPS_PER_CHUNK;
  return want < 1 ? 1 : want > grid_chunks ? grid_chunks : want;
}

// grid: x over proofs, y over the windows (254, or 255 for signed tables), z over chunks of the
// varying groups: the grid is sized from n_groups, the first comb_eff_chunks blocks of z share
// counts[0] groups (an empty chunk leaves the identity: chunk 0 when nothing varies), the others
// leave at once and write nothing
template <class F, bool CHECK_INF, bool SIGNED>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void
msm_accumulate_comb(const Affine<F>* __restrict__ table, const uint32_t* __restrict__ digits,
                    size_t Bp, uint32_t n_groups, const uint32_t* __restrict__ vlist,
                    const uint32_t* __restrict__ counts, uint32_t per_group,
                    Part29<F>* __restrict__ partial) {
  const uint32_t chunk = blockIdx.z, j = blockIdx.y;
  const uint32_t nv = counts[0];
  const uint32_t eff = comb_eff_chunks(nv, gridDim.z);
  if (chunk >= eff) return;
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t per_chunk = (nv + eff - 1) / eff;
  const uint32_t p0 = chunk * per_chunk;
  uint32_t p1 = p0 + per_chunk;
  if (p1 > nv) p1 = nv;
  const uint32_t* dj = digits + (size_t)j * n_groups * Bp + b;
  __shared__ int32_t zl[CombAcc<F>::LDS_ROWS][256];
  const uint32_t t = threadIdx.x;
  typename CombAcc<F>::type acc = CombAcc<F>::init(zl, t);
  for (uint32_t p = p0; p < p1; p++) {
    const uint32_t m = dj[(size_t)p * Bp];
    const Affine<F>* tg = table + (size_t)vlist[p] * per_group;
    if (SIGNED) {   // a sign pattern is never "nothing to add"
      const Affine<F> e = tg[m & 0x7fffffffu];
      if (CHECK_INF && e.is_inf()) continue;
      CombAcc<F>::add(acc, e, (m >> 31) != 0, zl, t);
    } else if (m) {
      const Affine<F> e = tg[m];
      if (CHECK_INF && e.is_inf()) continue;
      CombAcc<F>::add(acc, e, false, zl, t);
    }
  }
  partial[((size_t)j * gridDim.z + chunk) * Bp + b] = CombAcc<F>::result(acc, zl, t);
}

// all 32-bit words of a lane's value from lane (lane ^ mask)
template <class T>
static __device__ __forceinline__ T shfl_xor_words(const T& x, int mask) {
  static_assert(sizeof(T) % 4 == 0, "word-sized value");
  T r;
  const uint32_t* s = reinterpret_cast<const uint32_t*>(&x);
  uint32_t* d = reinterpret_cast<uint32_t*>(&r);
#pragma unroll
  for (int i = 0; i < (int)(sizeof(T) / 4); i++) d[i] = (uint32_t)__shfl_xor((int)s[i], mask);
  return r;
}

// usum[j] = sum over the uniform groups g = ulist[c] of T[g][d0[j][g]]: the part of window sum j
// that every proof of the batch shares, added once per lane by the last msm_reduce pass (stored
// packed, as the partials are).  One
// block of 256 lanes per window; each lane sums a strided share of the groups, then a butterfly
// over the wave and the four wave sums through LDS.  Same entries as msm_accumulate_comb would
// gather, so the window sums are unchanged (a group sum does not depend on the order).
template <class F, bool CHECK_INF, bool SIGNED>
__global__ __launch_bounds__(256) void comb_common_sums(const Affine<F>* __restrict__ table,
                                                        const uint32_t* __restrict__ d0,
                                                        uint32_t n_groups,
                                                        const uint32_t* __restrict__ ulist,
                                                        const uint32_t* __restrict__ counts,
                                                        uint32_t per_group,
                                                        Part29<F>* __restrict__ usum) {
  const uint32_t j = blockIdx.x, t = threadIdx.x;
  const uint32_t nu = counts[1];
  const uint32_t* dj = d0 + (size_t)j * n_groups;
  typename Acc29<F>::type acc = Acc29<F>::type::infinity();
  for (uint32_t c = t; c < nu; c += blockDim.x) {
    const uint32_t g = ulist[c];
    const uint32_t m = dj[g];
    if (!SIGNED && !m) continue;
    const Affine<F> e = table[(size_t)g * per_group + (SIGNED ? (m & 0x7fffffffu) : m)];
    if (CHECK_INF && e.is_inf()) continue;
    Acc29<F>::add(acc, e, SIGNED && (m >> 31) != 0);
  }
  XYZZ<F> s = to_std(acc);
#pragma unroll 1
  for (int off = 32; off > 0; off >>= 1) {
    const XYZZ<F> o = shfl_xor_words(s, off);
    padd(s, o);
  }
  constexpr int NW = (int)(sizeof(XYZZ<F>) / 4);
  __shared__ uint32_t wave_sum[4][NW];
  if ((t & 63u) == 0) {
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(&s);
    for (int i = 0; i < NW; i++) wave_sum[t >> 6][i] = sw[i];
  }
  __syncthreads();
  if (t == 0) {
    for (uint32_t q = 1; q < blockDim.x / 64; q++) {
      XYZZ<F> o;
      uint32_t* ow = reinterpret_cast<uint32_t*>(&o);
      for (int i = 0; i < NW; i++) ow[i] = wave_sum[q][i];
      padd(s, o);
    }
    usum[j] = pack_part(from_std(s));
  }
}

// out[b] = sum_j 2^j * wsum[j][b], j < W, in two levels so that the dependent chain is short:
// comb_fold8 replaces wsum[8q] by sum_{i<8} 2^i wsum[8q+i] (one lane per (proof, q), 7 doublings +
// 7 additions), msm_horner_comb then runs Horner over the folded sums (8 doublings + 1 addition per
// step): 256 doublings + 32 additions on the critical path instead of 254 + 254.
template <class F>
struct HornerArgsRW {
  XYZZ<F>* wsum[4];
  XYZZ<F>* out[4];
  Affine<F> stotal[4];   // signed tables: sum of all bases of the MSM (standard Montgomery image)
};
template <class F>
__global__ __launch_bounds__(64) void comb_fold8(HornerArgsRW<F> args, size_t Bp, int W) {
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= Bp) return;
  XYZZ<F>* __restrict__ wsum = args.wsum[blockIdx.y];
  const int j0 = 8 * (int)blockIdx.z;
  int top = j0 + 7;
  if (top > W - 1) top = W - 1;
  XYZZ<F> acc = wsum[(size_t)top * Bp + b];
  for (int j = top - 1; j >= j0; j--) {
    acc = dbl(acc);
    const XYZZ<F> p = wsum[(size_t)j * Bp + b];
    padd(acc, p);
  }
  wsum[(size_t)j0 * Bp + b] = acc;
}
// W = number of power-of-two windows (254).  signed_tail: out = 2 H - wsum[W] - stotal.
template <class F>
__global__ __launch_bounds__(64) void msm_horner_comb(HornerArgsRW<F> args, size_t Bp, int W,
                                                      int signed_tail) {
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= Bp) return;
  const XYZZ<F>* __restrict__ wsum = args.wsum[blockIdx.y];
  const int Q = (W + 7) / 8;
  XYZZ<F> acc = wsum[(size_t)(8 * (Q - 1)) * Bp + b];
  for (int q = Q - 2; q >= 0; q--) {
#pragma unroll 1
    for (int i = 0; i < 8; i++) acc = dbl(acc);
    const XYZZ<F> p = wsum[(size_t)(8 * q) * Bp + b];
    padd(acc, p);
  }
  if (signed_tail) {
    acc = dbl(acc);
    XYZZ<F> corr = wsum[(size_t)W * Bp + b];
    corr.y = neg(corr.y);
    padd(acc, corr);
    madd(acc, neg(args.stotal[blockIdx.y]));
  }
  args.out[blockIdx.y][b] = acc;
}
template <class F>
static void launch_comb_horner(hipStream_t stream, const HornerArgsRW<F>& ha, int count, size_t Bp,
                               const WinPlan& plan) {
  const int W = COMB_W;   // plan.W = 254, or 255 with the correction window of signed tables
  hipLaunchKernelGGL((comb_fold8<F>),
                     dim3((unsigned)(Bp / 64), (unsigned)count, (unsigned)((W + 7) / 8)), dim3(64), 0,
                     stream, ha, Bp, W);
  hipLaunchKernelGGL((msm_horner_comb<F>), dim3((unsigned)(Bp / 64), (unsigned)count), dim3(64), 0,
                     stream, ha, Bp, W, (int)plan.comb_signed);
}

// sums groups of `group` consecutive chunk partials: out[g][b] = sum_{k < group} in[g*group + k][b]
// (blockIdx.z selects an independent set: partial += z * in_zstride, out += z * out_zstride);
// addend (may be null): addend[z] is added to every sum of set z (comb_common_sums).
// Partials, group sums and the addend are packed accumulators (ec29.h); the LAST pass writes the
// final sums as XYZZ<F> for what follows.
// counts (comb tables; null: all `chunks` inputs are summed): only the first
// comb_eff_chunks(counts[0], grid_chunks) chunk partials were written by this batch's accumulate
// launch, the other slots hold an earlier batch's.  This pass sums the first ceil(eff / div)
// inputs: div = 1 over the chunk partials, div = the first level's group size over its group
// sums; a group that starts beyond them is skipped and its output never read.
template <class F, bool LAST>
__global__ __launch_bounds__(64) void msm_reduce(
    const Part29<F>* __restrict__ partial, size_t Bp, uint32_t chunks, uint32_t group,
    typename std::conditional<LAST, XYZZ<F>, Part29<F>>::type* __restrict__ out, size_t in_zstride,
    size_t out_zstride, const Part29<F>* __restrict__ addend, const uint32_t* __restrict__ counts,
    uint32_t grid_chunks, uint32_t div) {
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= Bp) return;
  if (counts) chunks = (comb_eff_chunks(counts[0], grid_chunks) + div - 1) / div;
  partial += (size_t)blockIdx.z * in_zstride;
  out += (size_t)blockIdx.z * out_zstride;
  const uint32_t k0 = blockIdx.y * group;
  if (k0 >= chunks) return;
  uint32_t k1 = k0 + group;
  if (k1 > chunks) k1 = chunks;
  typename Acc29<F>::type acc = unpack_part(partial[(size_t)k0 * Bp + b]);
  for (uint32_t k = k0 + 1; k < k1; k++) padd29(acc, unpack_part(partial[(size_t)k * Bp + b]));
  if (addend) padd29(acc, unpack_part(addend[blockIdx.z]));
  if constexpr (LAST)
    out[(size_t)blockIdx.y * Bp + b] = to_std(acc);
  else
    out[(size_t)blockIdx.y * Bp + b] = pack_part(acc);
}

template <class F>
__global__ __launch_bounds__(64) void xyzz_to_affine_kernel(const XYZZ<F>* __restrict__ in,
                                                            Affine<F>* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = to_affine(in[i]);
}

// inf[i] = 1 when base i is the point at infinity: its table rows are zeros and must never reach a
// mixed addition (the digit pass / the accumulate loop skip the base)
template <class F>
__global__ void msm_inf_flags(const Affine<F>* __restrict__ bases, uint32_t n,
                              uint8_t* __restrict__ inf) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) inf[i] = bases[i].is_inf() ? 1 : 0;
}

template <class F>
__global__ void fill_inf(XYZZ<F>* out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = XYZZ<F>::inf();
}

// ---- host side: table builds -----------------------------------------------------------------------
// Threads of one table-build launch (a slab of rows) and the bytes of their inversion scratch:
// as many threads as keep the scratch under ~2 GB, a multiple of 64, at most 262144.
struct BuildSlab {
  size_t T, bytes;
};
template <class F>
static BuildSlab build_slab(uint32_t seg_len, uint64_t n_rows) {
  const size_t per_thread = (size_t)3 * seg_len * sizeof(F);
  size_t T = (size_t)2e9 / per_thread;
  if (T > n_rows) T = (size_t)n_rows;
  T = round_up(T, 64);
  if (T > 262144) T = 262144;
  return {T, per_thread * T};
}

// signed comb tables: sum of all bases of the key
template <class B> static auto& stotal_of(B* b, Fq) { return b->stotal1; }
template <class B> static auto& stotal_of(B* b, Fq2) { return b->stotal2; }

// (2 * 2^256)^-1 or (2 * 2^261)^-1 mod r as a plain integer: the factor on the bases of a
// sign-pattern table native to gnark's image / the F image (comb_scalars_kernel's comment)
static inline Fr comb_base_scale(int image) {
  Fr x = Fr::one();   // 2^0 in Montgomery form
  const int e = image == MSM_IMAGE_F ? 262 : 257;
  for (int i = 0; i < e; i++) x = dbl(x);
  return from_mont(inverse(x));
}

// Sign-pattern tables are built over the bases scaled by comb_base_scale(image), so stotal comes
// out scaled as well; subset-sum tables over the bases as they are.
template <class F>
int build_comb(zkmi_ctx* ctx, const Affine<F>* bases_dev, size_t n, const WinPlan& plan, int image,
               Affine<F>* table, int* any_inf_host, Affine<F>* stotal_host) {
  const uint32_t k = plan.comb;
  const bool sg = plan.comb_signed != 0;
  const size_t n_groups = (n + k - 1) / k;
  const uint32_t per_group = 1u << (sg ? k - 1 : k);
  const uint32_t seg_len = per_group < 512u ? per_group : 512u;
  const uint64_t n_rows = (uint64_t)n_groups * (per_group / seg_len);
  const BuildSlab slab = build_slab<F>(seg_len, n_rows);
  const size_t T = slab.T;
  void* scratch;
  const size_t dp_bytes = round_up(n_groups * k * sizeof(Affine<F>), 256);
  const size_t gs_bytes = round_up((n_groups + 1) * sizeof(Affine<F>), 256);
  const size_t sc_bytes = sg ? round_up(n * sizeof(Affine<F>), 256) : 0;
  int rc = ensure_scratch(ctx, ctx->build_tmp, dp_bytes + gs_bytes + 256 + slab.bytes + sc_bytes,
                          &scratch);
  if (rc) return rc;
  Affine<F>* dpts = (Affine<F>*)scratch;
  Affine<F>* gsum = (Affine<F>*)((char*)scratch + dp_bytes);
  int* any_inf = (int*)((char*)scratch + dp_bytes + gs_bytes);
  F* inv_scratch = (F*)((char*)scratch + dp_bytes + gs_bytes + 256);
  if (sg) {
    Affine<F>* scaled = (Affine<F>*)((char*)inv_scratch + slab.bytes);
    hipLaunchKernelGGL((comb_scale_bases<F>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0,
                       ctx->stream, bases_dev, (uint32_t)n, comb_base_scale(image), scaled);
    bases_dev = scaled;
  }
  ZK_HIP(hipMemsetAsync(any_inf, 0, sizeof(int), ctx->stream));
  hipLaunchKernelGGL((comb_prep<F>), dim3((unsigned)((n_groups + 63) / 64)), dim3(64), 0,
                     ctx->stream, bases_dev, (uint32_t)n, k, (uint32_t)n_groups, dpts, gsum,
                     sg ? 1 : 0);
  hipLaunchKernelGGL((comb_total<F>), dim3(1), dim3(1), 0, ctx->stream, (const Affine<F>*)gsum,
                     (uint32_t)n_groups, gsum + n_groups);
  const auto build = sg ? comb_build<F, true> : comb_build<F, false>;
  for (uint64_t r0 = 0; r0 < n_rows; r0 += T)
    hipLaunchKernelGGL(build, dim3((unsigned)(T / 64)), dim3(64), 0, ctx->stream, bases_dev,
                       (const Affine<F>*)dpts, (uint32_t)n, k, r0, n_rows, table, inv_scratch,
                       (uint32_t)T, seg_len, any_inf);
  ZK_HIP(hipGetLastError());
  ZK_HIP(hipMemcpyAsync(any_inf_host, any_inf, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(hipMemcpyAsync(stotal_host, gsum + n_groups, sizeof(Affine<F>), hipMemcpyDeviceToHost,
                        ctx->stream));
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  return ZKMI_OK;
}

template <class F>
int build_impl(zkmi_ctx* ctx, const Affine<F>* bases_dev, size_t n, const WinPlan& plan,
               Affine<F>* table) {
  const uint32_t Dmax = plan.shared ? plan.per_base : 1u << (plan.bits[0] - 1);
  const uint32_t seg_len = Dmax < 512u ? Dmax : 512u;
  const uint64_t n_rows = plan.shared ? (uint64_t)n : (uint64_t)n * (uint64_t)plan.W;
  const BuildSlab slab = build_slab<F>(seg_len, n_rows);
  const size_t T = slab.T;
  void* scratch;
  int rc = ensure_scratch(ctx, ctx->build_tmp, slab.bytes, &scratch);
  if (rc) return rc;
  for (uint64_t r0 = 0; r0 < n_rows; r0 += T)
    hipLaunchKernelGGL((msm_build_table<F>), dim3((unsigned)(T / 64)), dim3(64), 0, ctx->stream,
                       bases_dev, r0, n_rows, plan, table, (F*)scratch, (uint32_t)T, seg_len);
  ZK_HIP(hipGetLastError());
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  return ZKMI_OK;
}

// ---- host side: plumbing shared by the three launch routines -----------------------------------------
// Split of `items` (bases, or groups of a comb table) into at most `want` chunks of per_chunk items,
// one row of accumulate blocks each, and of the chunks into about sqrt(chunks) groups for the
// two-level sum of their partials (reduce_partials), which keeps the tail parallel.
struct ChunkSplit {
  size_t chunks;
  uint32_t per_chunk, group, ngroups;
};
static inline ChunkSplit split_chunks(size_t items, size_t want) {
  size_t chunks = want;
  if (chunks < 1) chunks = 1;
  if (chunks > items) chunks = items;
  const uint32_t per_chunk = (uint32_t)((items + chunks - 1) / chunks);
  chunks = (items + per_chunk - 1) / per_chunk;
  uint32_t group = 1;
  while ((size_t)group * group < chunks) group++;
  return {chunks, per_chunk, group, (uint32_t)((chunks + group - 1) / group)};
}

// out[w][b] = sum of the chunk partials partial[w][chunk][b] for each of W independent sets, through
// the group sums mid[w][group][b] when there is more than one group.  addend (may be null):
// addend[w] joins every sum of set w in the last pass.  counts (may be null): see msm_reduce.
template <class F>
static void reduce_partials(hipStream_t stream, const XYZZ<F>* partial, XYZZ<F>* mid, XYZZ<F>* out,
                            size_t Bp, const ChunkSplit& cs, int W, const XYZZ<F>* addend,
                            const uint32_t* counts) {
  const Part29<F>* in = (const Part29<F>*)partial;
  uint32_t count = (uint32_t)cs.chunks, div = 1;
  if (cs.ngroups > 1) {
    hipLaunchKernelGGL((msm_reduce<F, false>), dim3((unsigned)(Bp / 64), cs.ngroups, (unsigned)W),
                       dim3(64), 0, stream, in, Bp, count, cs.group, (Part29<F>*)mid,
                       (size_t)count * Bp, (size_t)cs.ngroups * Bp, (const Part29<F>*)nullptr, counts,
                       (uint32_t)cs.chunks, div);
    in = (const Part29<F>*)mid;
    count = cs.ngroups;
    div = cs.group;
  }
  hipLaunchKernelGGL((msm_reduce<F, true>), dim3((unsigned)(Bp / 64), 1, (unsigned)W), dim3(64), 0,
                     stream, in, Bp, count, count, out, (size_t)count * Bp, Bp,
                     (const Part29<F>*)addend, counts, (uint32_t)cs.chunks, div);
}

// msm_part[pb] of the comb and shared-table routines (msm_part_layout.h has the regions and their
// order): the chunk partials [W][chunks][Bp], the group sums [W][ngroups][Bp], the window sums
// [W][Bp] (unused when the caller takes them), and for comb tables everything else the tail of the
// MSM reads: the W common sums of the uniform groups, the two counts of comb_split_kernel, lane 0's
// digits of the uniform groups d0 [W][G] and the list of those groups ulist [G].  Only wsum holds
// XYZZ<F> values: the other sums are packed accumulators of the same size (Part29<F>, ec29.h).
// The tail (comb_common_sums, msm_reduce) may run on the finish stream while the main stream
// already splits the next MSM's groups and writes its digits, hence the invariant: nothing the
// tail stream reads is written by the main stream between wait_partials_free(pb) and the next
// part_ev[pb].  vlist, vpos and the per-lane digits are read on the main stream only and live in
// msm_digits.
template <class F>
struct PartView {
  XYZZ<F> *partial, *mid, *wsum, *usum;
  uint32_t *counts, *d0, *ulist;
  static MsmPartLayout layout(const ChunkSplit& cs, int W, size_t Bp, size_t G, bool common_sums) {
    return msm_part_layout(sizeof(XYZZ<F>), cs.chunks, cs.ngroups, (size_t)W, Bp, G, common_sums);
  }
  static size_t bytes(const ChunkSplit& cs, int W, size_t Bp, size_t G, bool common_sums) {
    return layout(cs, W, Bp, G, common_sums).bytes();
  }
  PartView(void* base, const ChunkSplit& cs, int W, size_t Bp, size_t G, bool common_sums) {
    static_assert(sizeof(XYZZ<F>) == sizeof(Part29<F>), "packed accumulators share the regions");
    const MsmPartLayout l = layout(cs, W, Bp, G, common_sums);
    char* m = (char*)base;
    partial = (XYZZ<F>*)(m + l.off[MSM_PART_PARTIAL]);
    mid = (XYZZ<F>*)(m + l.off[MSM_PART_MID]);
    wsum = (XYZZ<F>*)(m + l.off[MSM_PART_WSUM]);
    usum = (XYZZ<F>*)(m + l.off[MSM_PART_USUM]);
    counts = (uint32_t*)(m + l.off[MSM_PART_COUNTS]);
    d0 = (uint32_t*)(m + l.off[MSM_PART_D0]);
    ulist = (uint32_t*)(m + l.off[MSM_PART_ULIST]);
  }
};

// The deferred tail of an earlier MSM (run_comb) may still be reading msm_part[pb] on its finish
// stream: the main stream waits for that reduction before the buffer is written again.
static inline int wait_partials_free(zkmi_ctx* ctx, int pb) {
  if (ctx->part_ev_valid[pb]) {
    ZK_HIP(hipStreamWaitEvent(ctx->stream, ctx->part_ev[pb], 0));
    ctx->part_ev_valid[pb] = false;
  }
  return ZKMI_OK;
}

// Event pair around the mixed additions of one proving-key MSM (zkmi_last_timings [6], [7]):
// claims a slot of the set being timed and records its first event; null when nothing is being
// timed or the slots are used up.  acc_timer_end records the second.
static inline hipEvent_t acc_timer_begin(zkmi_ctx* ctx, const zkmi_msm_bases* bases) {
  if (ctx->msm_ev_set < 0) return nullptr;
  zkmi_ctx::ProveSet& es = ctx->sets[ctx->msm_ev_set];
  if (es.msm_ev_used >= 8) return nullptr;
  const int ev = es.msm_ev_used++;
  es.msm_ev_group[ev] = bases->group;
  hipEventRecord(es.msm_ev[ev][0], ctx->stream);
  return es.msm_ev[ev][1];
}
static inline void acc_timer_end(zkmi_ctx* ctx, hipEvent_t end) {
  if (end) hipEventRecord(end, ctx->stream);
}

// ---- host side: one launch routine per table layout --------------------------------------------------
// Arguments as msm_run (zkmi_internal.h); n > 0.
template <class F>
int run_comb(zkmi_ctx* ctx, const zkmi_msm_bases* bases, const Fr* scalars, const uint32_t* row_idx,
             size_t Bp, size_t batch, XYZZ<F>* out, bool scalars_f, XYZZ<F>* wsum_out,
             hipStream_t finish_stream, const uint8_t* row_varies, bool dense) {
  const size_t n = bases->n;
  const uint32_t k = bases->plan.comb;
  const bool sg = bases->plan.comb_signed != 0;
  const size_t G = bases->n_groups;
  const int W = bases->plan.W;   // 254, + the correction window of signed tables
  if (Bp >> 28) return ZKMI_ERR_ARG;   // comb_digits_kernel: a lane's byte offsets are 32-bit
  // measured at 4 / 8 / 12 / 16 / 24: 277 / 275 / 273.5 / 272 / 273.6 ms per Arbo-160 batch
  const size_t comb_factor = bases->chunk_factor ? bases->chunk_factor : 16;
  const ChunkSplit cs = split_chunks(G, comb_factor * 262144 / Bp / (size_t)W);
  void *part, *digits, *sint;
  // deferred tail: the reductions run on finish_stream while the next MSM's accumulate already
  // writes the other partial buffer
  const bool defer = wsum_out && finish_stream && finish_stream != ctx->stream;
  const int pb = defer ? (int)(ctx->part_next++ & 1u) : 0;
  // (everything the tail reads, possibly on finish_stream, is in this buffer, under part_ev)
  int rc = ensure_scratch(ctx, ctx->msm_part[pb], PartView<F>::bytes(cs, W, Bp, G, true), &part);
  if (rc) return rc;
  if ((rc = wait_partials_free(ctx, pb))) return rc;
  // (Measured and dropped: the digit pass one MSM ahead on a fourth stream through two digit
  // buffers -- correct, no gain: the pass is ALU work like the accumulate kernel it would hide
  // under, which slowed down by exactly the pass's 7 ms.)
  // digits [W][G][Bp] (the first |vlist| rows of every window are used), then what else only the
  // main stream reads: vlist, vpos [G], and the flags of the bases [n] when the caller brings none
  if ((rc = ensure_scratch(ctx, ctx->msm_digits,
                           ((size_t)W * G * Bp + (size_t)2 * G) * sizeof(uint32_t) + n, &digits)))
    return rc;
  uint32_t* vlist = (uint32_t*)digits + (size_t)W * G * Bp;
  uint32_t* vpos = vlist + G;
  const PartView<F> pv(part, cs, W, Bp, G, true);
  uint32_t *counts = pv.counts, *d0 = pv.d0, *ulist = pv.ulist;
  XYZZ<F>* wsum = wsum_out ? wsum_out : pv.wsum;
  const unsigned bx = (Bp % 256 == 0) ? 256 : 64;
  const dim3 dgrid((unsigned)(Bp / bx), (unsigned)(G < 8192 ? G : 8192));
  // which groups vary: from the caller's flags per scalar row, or from the scalars as they arrive
  const uint8_t* flags = row_varies;
  const uint32_t* flag_idx = row_idx;
  if (!flags && !dense) {
    uint8_t* own = (uint8_t*)(vpos + G);
    hipLaunchKernelGGL(rows_vary_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, ctx->stream,
                       scalars, row_idx, (uint32_t)n, Bp, batch, own);
    flags = own;
    flag_idx = nullptr;
  }
  hipLaunchKernelGGL(comb_split_kernel, dim3(1), dim3(1024), 0, ctx->stream, flags, flag_idx,
                     (uint32_t)n, k, dense ? 1 : 0, (uint32_t)G, vlist, ulist, vpos, counts);
  // what the digit pass reads: the scalar rows themselves when a sign-pattern table is native to
  // their image, else one pass writes the plain integers (subset sums) or the native image
  const Fr* dsrc = scalars;
  const uint32_t* didx = row_idx;
  if (!(sg && scalars_f == (bases->image == MSM_IMAGE_F))) {
    if ((rc = ensure_scratch(ctx, ctx->msm_sint, n * Bp * sizeof(Fr), &sint))) return rc;
    Fr29 kk = Fr29::zero();
    if (!sg)
      kk.v[0] = scalars_f ? 1 : 32;
    else
      for (int i = 0; i < 9; i++) kk.v[i] = scalars_f ? Fr29Params::c256(i) : Fr29Params::c266(i);
    const dim3 sgrid((unsigned)(Bp / bx), (unsigned)(n < 16384 ? n : 16384));
    hipLaunchKernelGGL(comb_scalars_kernel, sgrid, dim3(bx), 0, ctx->stream, scalars, row_idx, Bp,
                       (uint32_t)n, kk, (const uint8_t*)bases->inf, (Fr*)sint);
    dsrc = (const Fr*)sint;
    didx = nullptr;
  }
  hipLaunchKernelGGL((sg ? comb_digits_kernel<21, true> : comb_digits_kernel<20, false>), dgrid,
                     dim3(bx), 0, ctx->stream, dsrc, didx, Bp, (uint32_t)n, k, (uint32_t)G,
                     (const uint32_t*)vpos, (uint32_t*)digits, d0);
  const dim3 grid((unsigned)(Bp / bx), (unsigned)W, (unsigned)cs.chunks);
  const uint32_t per_group = 1u << (sg ? k - 1 : k);
  const bool ci = bases->entries_may_be_inf != 0;
  const auto sums = ci ? (sg ? comb_common_sums<F, true, true> : comb_common_sums<F, true, false>)
                       : (sg ? comb_common_sums<F, false, true> : comb_common_sums<F, false, false>);
  const auto accumulate =
      ci ? (sg ? msm_accumulate_comb<F, true, true> : msm_accumulate_comb<F, true, false>)
         : (sg ? msm_accumulate_comb<F, false, true> : msm_accumulate_comb<F, false, false>);
  // The tail: the common sums of the uniform groups, then the sums over the chunk partials.  Only
  // the last reduction pass reads the common sums, so with a deferred tail they run on the finish
  // stream beside the accumulate launch (255 workgroups: one wave per SIMD on a quarter of the
  // chip), ordered after the split and the digit pass by dig_ev.  A dense MSM has no uniform group:
  // no launch, no addend.
  hipStream_t rq = defer ? finish_stream : ctx->stream;
  const XYZZ<F>* addend = nullptr;
  if (!dense) {
    if (defer) {
      ZK_HIP(hipEventRecord(ctx->dig_ev[pb], ctx->stream));
      ZK_HIP(hipStreamWaitEvent(rq, ctx->dig_ev[pb], 0));
    }
    hipLaunchKernelGGL(sums, dim3((unsigned)W), dim3(256), 0, rq, (const Affine<F>*)bases->table,
                       (const uint32_t*)d0, (uint32_t)G, (const uint32_t*)ulist,
                       (const uint32_t*)counts, per_group, (Part29<F>*)pv.usum);
    addend = pv.usum;
  }
  const hipEvent_t timed = acc_timer_begin(ctx, bases);   // the accumulate launch alone
  hipLaunchKernelGGL(accumulate, grid, dim3(bx), 0, ctx->stream, (const Affine<F>*)bases->table,
                     (const uint32_t*)digits, Bp, (uint32_t)G, (const uint32_t*)vlist,
                     (const uint32_t*)counts, per_group, (Part29<F>*)pv.partial);
  acc_timer_end(ctx, timed);
  if (defer) {
    ZK_HIP(hipEventRecord(ctx->acc_ev[pb], ctx->stream));
    ZK_HIP(hipStreamWaitEvent(rq, ctx->acc_ev[pb], 0));
  }
  reduce_partials<F>(rq, pv.partial, pv.mid, wsum, Bp, cs, W, addend, counts);
  if (defer) {
    ZK_HIP(hipEventRecord(ctx->part_ev[pb], finish_stream));
    ctx->part_ev_valid[pb] = true;
  }
  if (!wsum_out) {
    HornerArgsRW<F> ha{};
    ha.wsum[0] = wsum;
    ha.out[0] = out;
    ha.stotal[0] = stotal_of(bases, F{});
    launch_comb_horner<F>(ctx->stream, ha, 1, Bp, bases->plan);
  }
  ZK_HIP(hipGetLastError());
  return ZKMI_OK;
}

template <class F>
int run_shared(zkmi_ctx* ctx, const zkmi_msm_bases* bases, const Fr* scalars,
               const uint32_t* row_idx, size_t Bp, XYZZ<F>* out, bool scalars_f,
               XYZZ<F>* wsum_out) {
  const size_t n = bases->n;
  const WinPlan& plan = bases->plan;
  const int W = plan.W;
  Fr koff = Fr::zero();   // K = sum_j 2^(pos_j + c_j - 1)
  {
    uint32_t pos = 0;
    for (int j = 0; j < W; j++) {
      const uint32_t bit = pos + plan.bits[j] - 1;
      koff.v[bit >> 5] |= 1u << (bit & 31);
      pos += plan.bits[j];
    }
  }
  // (window, chunk) blocks: 8 x the wave slots of the chip, as for the per-window tables
  const size_t shared_factor = bases->chunk_factor ? bases->chunk_factor : 8;
  const ChunkSplit cs = split_chunks(n, shared_factor * 262144 / Bp / (size_t)W);
  void *part, *digits;
  int rc = ensure_scratch(ctx, ctx->msm_part[0], PartView<F>::bytes(cs, W, Bp, 0, false), &part);
  if (rc) return rc;
  if ((rc = wait_partials_free(ctx, 0))) return rc;
  if ((rc = ensure_scratch(ctx, ctx->msm_digits, (size_t)W * n * Bp * sizeof(int16_t), &digits)))
    return rc;
  const PartView<F> pv(part, cs, W, Bp, 0, false);
  // window sums: into the caller's buffer when the Horner step is deferred (msm_horner_run)
  XYZZ<F>* wsum = wsum_out ? wsum_out : pv.wsum;
  const unsigned bx = (Bp % 256 == 0) ? 256 : 64;
  hipLaunchKernelGGL(msm_digits_kernel,
                     dim3((unsigned)(Bp / bx), (unsigned)(n < 16384 ? n : 16384)), dim3(bx), 0,
                     ctx->stream, scalars, row_idx, Bp, (uint32_t)n, plan,
                     (int32_t)(scalars_f ? 1 : 32), koff, (const uint8_t*)bases->inf,
                     (int16_t*)digits);
  const hipEvent_t timed = acc_timer_begin(ctx, bases);   // the accumulate launch alone
  hipLaunchKernelGGL((msm_accumulate_shared<F>),
                     dim3((unsigned)(Bp / bx), (unsigned)W, (unsigned)cs.chunks), dim3(bx), 0,
                     ctx->stream, (const Affine<F>*)bases->table, (const int16_t*)digits, Bp,
                     (uint32_t)n, cs.per_chunk, plan.per_base, (Part29<F>*)pv.partial);
  acc_timer_end(ctx, timed);
  reduce_partials<F>(ctx->stream, pv.partial, pv.mid, wsum, Bp, cs, W, nullptr, nullptr);
  if (!wsum_out) {
    HornerArgs<F> ha{};
    ha.wsum[0] = wsum;
    ha.out[0] = out;
    hipLaunchKernelGGL((msm_horner<F>), dim3((unsigned)(Bp / 64), 1), dim3(64), 0, ctx->stream,
                       ha, Bp, plan);
  }
  ZK_HIP(hipGetLastError());
  return ZKMI_OK;
}

// Per-window tables: every window of a base into one accumulator, so the sum of the chunk partials
// is the result (no window sums, no Horner step).  Also the one-base multiples (n = 1) and the side
// bases, which run beside an MSM of the main stream and are not timed.
template <class F>
int run_windows(zkmi_ctx* ctx, const zkmi_msm_bases* bases, const Fr* scalars,
                const uint32_t* row_idx, size_t Bp, XYZZ<F>* out, bool scalars_f) {
  const size_t n = bases->n;
  Fr kmul = Fr::zero();
  kmul.v[0] = 1;  // plain 1: from_mont
  if (scalars_f) {  // plain 2^-5 mod r
    Fr t = Fr::zero();
    t.v[0] = 32;
    kmul = from_mont(inverse(to_mont(t)));
  }
  // 8 x as many chunks as it takes to put 4 waves on every SIMD: all blocks of the coarse grid
  // run for the whole kernel, so a few occupied wave slots (the overlapped solve of the next
  // batch) or uneven clocks cost a full extra round; measured per 1024-proof batch, G1 launches:
  // x1 325 ms, x2 315, x4 299, x8 292 (best end to end), x16 289 + dearer reduction.
  const size_t chunk_factor = bases->chunk_factor ? bases->chunk_factor : 8;
  const ChunkSplit cs = split_chunks(n, chunk_factor * (size_t)262144 / Bp);
  void* part;
  // partials + room for the intermediate level of the reduction; side bases have their own
  DevBuf& buf = bases->side == 2 ? ctx->side_part3 : bases->side ? ctx->side_part2 : ctx->msm_part[0];
  int rc = ensure_scratch(ctx, buf, (cs.chunks + 256) * Bp * sizeof(XYZZ<F>), &part);
  if (rc) return rc;
  if (!bases->side && (rc = wait_partials_free(ctx, 0))) return rc;
  XYZZ<F>* partial = (XYZZ<F>*)part;
  const unsigned bx = (Bp % 256 == 0) ? 256 : 64;
  const dim3 grid((unsigned)(Bp / bx), (unsigned)cs.chunks);
  const hipEvent_t timed = (bases->side || n == 1) ? nullptr : acc_timer_begin(ctx, bases);
  hipLaunchKernelGGL((n == 1 ? msm_accumulate<F, true> : msm_accumulate<F, false>), grid, dim3(bx), 0,
                     ctx->stream, (const Affine<F>*)bases->table, scalars, row_idx, Bp, (uint32_t)n,
                     cs.per_chunk, bases->plan, (Part29<F>*)partial, kmul,
                     (const uint8_t*)bases->inf);
  acc_timer_end(ctx, timed);
  reduce_partials<F>(ctx->stream, partial, partial + cs.chunks * Bp, out, Bp, cs, 1, nullptr,
                     nullptr);
  ZK_HIP(hipGetLastError());
  return ZKMI_OK;
}

template <class F>
int run_impl(zkmi_ctx* ctx, const zkmi_msm_bases* bases, const Fr* scalars,
             const uint32_t* row_idx, size_t Bp, size_t batch, XYZZ<F>* out, bool scalars_f,
             XYZZ<F>* wsum_out, hipStream_t finish_stream, const uint8_t* row_varies, bool dense) {
  if (bases->plan.comb)
    return run_comb<F>(ctx, bases, scalars, row_idx, Bp, batch, out, scalars_f, wsum_out,
                       finish_stream, row_varies, dense);
  if (bases->plan.shared)
    return run_shared<F>(ctx, bases, scalars, row_idx, Bp, out, scalars_f, wsum_out);
  if (wsum_out) {
    ctx->err = "msm: deferred window sums need a shared-table plan";
    return ZKMI_ERR_ARG;
  }
  return run_windows<F>(ctx, bases, scalars, row_idx, Bp, out, scalars_f);
}

}  // namespace zk
