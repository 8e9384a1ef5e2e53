// PLONK prover rounds for a batch of independent witnesses (BASELINE config 5 names the PLONK
// backend).  Stands in for plonk.Prove in gnark backend/plonk/bn254/prove.go [UPSTREAM-RECALL,
// SURVEY.md §3.2, §8 a-2 / f-4]: KZG commitments (G1 MSMs over the SRS: the same fixed-base comb
// tables as the Groth16 key), wire polynomials blinded with multiples of Z_H, grand-product
// permutation argument, quotient on the coset 5<w_4n> split in three, linearisation and two
// openings.  The Fiat-Shamir hashing stays on the host between rounds, as in gnark (the five
// zkmi_plonk_round* calls); everything else runs here.  Protocol: DESIGN.md §PLONK; the reference
// holds no PLONK vector: parity unpinned, pinned instead to oracle/plonk_ref.py and to the pairing
// check of the openings.
//
// Layout: as everywhere, batch-inner.  A polynomial of a batch is a matrix [coefficient][proof]
// with the proof index fastest: lane = proof, so the sequential recurrences of the protocol
// (grand product, Horner evaluation, division by X - zeta) are plain per-lane loops that run for
// the whole batch at once, and every key-side quantity (selectors, sigma, coset points) is
// wave-uniform.  Field elements are in gnark's image (x * 2^256, ff.h) throughout.
#include <algorithm>

#include "zkmi_internal.h"
#include "scs_check.h"
#include "plonk_commit_check.h"
#include "sha256.h"
#include <atomic>
#include <cstring>
#include "solve_common.h"

using namespace zk;

struct zkmi_plonk_pk {
  uint32_t log_n = 0, n_public = 0, max_batch = 0;
  Fr *coef = nullptr, *coset = nullptr, *sigma = nullptr, *omega = nullptr, *coset_x = nullptr,
     *l1 = nullptr, *zh_inv = nullptr;
  zkmi_msm_bases* srs = nullptr;
  zkmi_msm_bases* lag[3] = {nullptr, nullptr, nullptr};   // Lagrange points of a, b, c (optional)
  uint32_t* lag_rows[3] = {nullptr, nullptr, nullptr};    // their scalar rows (device)
  uint32_t* chunk_idx = nullptr;   // 3 x (n + 6): scalar rows of t_lo / t_mid / t_hi in the 4n buffer
  // a key loaded from its trace form keeps its permutation (3n positions, host) for the wiring check
  // of the witness entry; `serial` names the key in the systems already checked against it
  std::vector<uint32_t> perm;
  uint64_t serial = 0;
  // state of the batch in flight
  size_t batch = 0, Bp = 0;
  int round = 0;
  DevBuf cf[4];      // coefficient forms of a, b, c, z: (n + 8) rows
  DevBuf big[6];     // 4n-row work buffers
  DevBuf small[4];   // challenges / per-proof scalars, MSM outputs
  // ---- commitments (api.Commit under PLONK, zkmi_plonk_pk_set_commitments; empty for a plain key)
  struct Commit {
    uint32_t n_rows = 0, row = 0;
    std::vector<uint32_t> slots;        // host: value-file slots of the operands (may be empty)
    std::vector<uint32_t> rows;         // host: C_i (the solver entry compares its hints' wires with them)
    uint32_t* rows_dev = nullptr;       // n_rows + 2: C_i, then the blinding rows r_i and n - 1
    uint32_t* slots_dev = nullptr;      // n_rows, or null
    zkmi_msm_bases* lag = nullptr;      // subset-sum tables of the n_rows + 2 Lagrange points
    size_t scal_row = 0;                // first row of this commitment's scalars in cm_scal
  };
  std::vector<Commit> commits;
  Fr *qcp_coef = nullptr, *qcp_coset = nullptr;   // n_c x n (256 image), n_c x 4n (261 image)
  uint8_t* cm_skip = nullptr;   // n bytes: 1 on committed and commitment rows (satisfied by construction)
  bool proved = false;          // a prove has started on this key
  DevBuf cm_scal;    // per commitment n_rows + 2 rows: the scalars of [pi2_i] (gnark's image)
  DevBuf cm_blind;   // 2 n_c rows: the caller's blinding scalars
  DevBuf cm_h;       // n_c rows: H_i
  DevBuf cm_pi2;     // n_c x n rows: coefficient forms of pi2_i, from round 3 to round 5
  std::vector<G1Affine> cm_pts;   // host: [pi2_i] of the batch in flight, proof-major (batch x n_c)
  std::vector<Fr> cm_H;           // host: H_i, proof-major, Montgomery
};

namespace zk {

#define LANE const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x

// Products of the element-wise kernels are fmulp on the 9 x 29-bit form; the exponent calculus the
// kernels' comments use (im_e, lift) is written out with it in solve_common.h.
__global__ void plonk_lift_kernel(Fr* x, size_t count, int k) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) x[i] = lift(x[i], k);
}
// 2^e mod r as a canonical integer, e >= 256: Fr::one() doubled e - 256 times (host)
static Fr pow2_image(int e) {
  Fr x = Fr::one();
  for (int i = 256; i < e; i++) x = add(x, x);
  return x;
}

// cf[j] -= b_j, cf[n + j] += b_j: adds (b_(nb-1) X^(nb-1) + ... + b_0)(X^n - 1); the blinding rows
// of `blind` are ordered highest power first (b1 X + b2 -> rows r0, r0 + 1)
__global__ void plonk_blind(Fr* cf, size_t n, const Fr* blind, int r0, int nb, size_t Bp) {
  LANE;
  for (int j = 0; j < nb; j++) {
    const Fr bj = bi_ld(blind, r0 + nb - 1 - j, lane, Bp);
    bi_st(cf, j, lane, Bp, sub(bi_ld(cf, j, lane, Bp), bj));
    bi_st(cf, n + j, lane, Bp, add(bi_ld(cf, n + j, lane, Bp), bj));
  }
}

__global__ void plonk_zero_rows(Fr* p, size_t r0, size_t r1, size_t Bp) {
  LANE;
  for (size_t r = r0 + blockIdx.y; r < r1; r += gridDim.y) bi_st(p, r, lane, Bp, Fr::zero());
}

// PI Lagrange values: row j = -x_j for the public inputs (rows 0 .. n_pub-1 of `inputs`), else 0
__global__ void plonk_pi(const Fr* inputs, Fr* pi, size_t n_pub, size_t n, size_t Bp) {
  LANE;
  for (size_t r = blockIdx.y; r < n; r += gridDim.y)
    bi_st(pi, r, lane, Bp, r < n_pub ? neg(bi_ld(inputs, r, lane, Bp)) : Fr::zero());
}

// F[i] = prod_c (w_c,i + beta k_c w^i + gamma), G[i] = prod_c (w_c,i + beta sigma_c,i + gamma)
__global__ __launch_bounds__(64) void plonk_fg(const Fr* a, const Fr* b, const Fr* c,
                                               const Fr* sigma, const Fr* omega, const Fr* ch,
                                               Fr* F, Fr* G, size_t n, size_t Bp, Fr k1, Fr k2) {
  LANE;
  const Fr beta = bi_ld(ch, 0, lane, Bp), gamma = bi_ld(ch, 1, lane, Bp);
  for (size_t i = blockIdx.y; i < n; i += gridDim.y) {
    const Fr bx = mul(beta, omega[i]);
    const Fr wa = add(bi_ld(a, i, lane, Bp), gamma), wb = add(bi_ld(b, i, lane, Bp), gamma),
             wc = add(bi_ld(c, i, lane, Bp), gamma);
    const Fr f = mul(mul(add(wa, bx), add(wb, mul(bx, k1))), add(wc, mul(bx, k2)));
    const Fr g = mul(mul(add(wa, mul(beta, sigma[i])), add(wb, mul(beta, sigma[n + i]))),
                     add(wc, mul(beta, sigma[2 * n + i])));
    bi_st(F, i, lane, Bp, f);
    bi_st(G, i, lane, Bp, g);
  }
}

// per (lane, chunk): ratio[i] = F[i] / G[i] with one inversion per chunk (Montgomery's trick; P is
// prefix scratch), then the chunk's product into cp[chunk]
__global__ __launch_bounds__(64) void plonk_ratio(Fr* F, const Fr* G, Fr* P, Fr* cp, size_t n,
                                                  size_t chunk, size_t Bp) {
  LANE;
  const size_t i0 = (size_t)blockIdx.y * chunk, i1 = i0 + chunk < n ? i0 + chunk : n;
  Fr acc = Fr::one();
  for (size_t i = i0; i < i1; i++) {
    bi_st(P, i, lane, Bp, acc);
    acc = mul(acc, bi_ld(G, i, lane, Bp));
  }
  Fr inv = inverse(acc);
  for (size_t i = i1; i-- > i0;) {
    const Fr gi = mul(inv, bi_ld(P, i, lane, Bp));
    inv = mul(inv, bi_ld(G, i, lane, Bp));
    bi_st(F, i, lane, Bp, mul(bi_ld(F, i, lane, Bp), gi));
  }
  acc = Fr::one();
  for (size_t i = i0; i < i1; i++) acc = mul(acc, bi_ld(F, i, lane, Bp));
  bi_st(cp, blockIdx.y, lane, Bp, acc);
}
// exclusive prefix product of the chunk products, per lane
__global__ void plonk_chunk_scan(Fr* cp, size_t n_chunks, size_t Bp) {
  LANE;
  Fr acc = Fr::one();
  for (size_t k = 0; k < n_chunks; k++) {
    const Fr v = bi_ld(cp, k, lane, Bp);
    bi_st(cp, k, lane, Bp, acc);
    acc = mul(acc, v);
  }
}
// z[i0] = carry-in, z[i + 1] = z[i] * ratio[i]
__global__ __launch_bounds__(64) void plonk_z_fill(const Fr* ratio, const Fr* cp, Fr* z, size_t n,
                                                   size_t chunk, size_t Bp) {
  LANE;
  const size_t i0 = (size_t)blockIdx.y * chunk, i1 = i0 + chunk < n ? i0 + chunk : n;
  Fr acc = bi_ld(cp, blockIdx.y, lane, Bp);
  for (size_t i = i0; i < i1; i++) {
    bi_st(z, i, lane, Bp, acc);
    acc = mul(acc, bi_ld(ratio, i, lane, Bp));
  }
}

// quotient on the coset: T[j] = (gate + alpha (p1 - p2) + alpha^2 (z - 1) L1) / Z_H
// key-side arrays (`ks`: qL, qR, qO, qM, qC, S1, S2, S3 on the coset, 4n each) are wave-uniform
__global__ __launch_bounds__(64, 2) void plonk_quotient(const Fr* ea, const Fr* eb, const Fr* ec,
                                                     const Fr* ez, const Fr* epi, const Fr* ks,
                                                     const Fr* xs, const Fr* l1, const Fr* zh_inv,
                                                     const Fr* ch, Fr* T, size_t m, size_t Bp,
                                                     Fr k1, Fr k2, int n_pub_direct, Fr c271,
                                                     Fr c281) {
  // exponents (fmulp above): per-proof data a, b, c, z, pub, beta, gamma, alpha: 256.  Key side as
  // stored by zkmi_plonk_pk_load: qL qR qO S1 S2 S3 (ks rows 0 1 2 5 6 7), xs, l1, zh_inv, k1 = 5,
  // k2 = 25: 261; qM (ks row 3): 266; qC (row 4): 256.
  LANE;
  const Fr beta = bi_ld(ch, 0, lane, Bp), gamma = bi_ld(ch, 1, lane, Bp),
           alpha = bi_ld(ch, 2, lane, Bp);
  const Fr al2 = fmulp(fmulp(alpha, alpha), c271);   // alpha^2: 251 -> 261
  const Fr al_x = fmulp(alpha, c281);                 // alpha: 276, for the 241 of p1 - p2
  // n_pub_direct >= 0: `epi` holds the public inputs x_t themselves (rows 0 .. n_pub - 1) and PI on
  // the coset is evaluated in closed form: L_t(x) = L_0(x / w^t) and x_j / w^t = x_(j - 4t) on the
  // coset 5 <w_4n>, so PI(x_j) = - sum_t x_t L1[j - 4t] -- no transform for a handful of inputs
  Fr pub[8];
  for (int t = 0; t < 8; t++) pub[t] = t < n_pub_direct ? bi_ld(epi, t, lane, Bp) : Fr::zero();
  for (size_t j = blockIdx.y; j < m; j += gridDim.y) {
    const Fr a = bi_ld(ea, j, lane, Bp), b = bi_ld(eb, j, lane, Bp), c = bi_ld(ec, j, lane, Bp),
             z = bi_ld(ez, j, lane, Bp), zw = bi_ld(ez, (j + 4) & (m - 1), lane, Bp);
    Fr gate = add(add(fmulp(ks[j], a), fmulp(ks[m + j], b)), fmulp(ks[2 * m + j], c));   // 256
    Fr pi;
    if (n_pub_direct >= 0) {
      pi = Fr::zero();
      for (int t = 0; t < n_pub_direct; t++)
        pi = sub(pi, fmulp(pub[t], l1[(j - 4 * (size_t)t) & (m - 1)]));                 // 256
    } else {
      pi = bi_ld(epi, j, lane, Bp);
    }
    gate = add(add(gate, fmulp(ks[3 * m + j], fmulp(a, b))), add(ks[4 * m + j], pi));  // 266 + 251 -> 256
    const Fr bx = fmulp(beta, xs[j]);                                                     // 256
    const Fr ag = add(a, gamma), bg = add(b, gamma), cg = add(c, gamma);
    // three 256 factors and z: 251, 246, 241
    const Fr p1 = fmulp(fmulp(fmulp(add(ag, bx), add(bg, fmulp(bx, k1))), add(cg, fmulp(bx, k2))), z);
    const Fr p2 = fmulp(fmulp(fmulp(add(ag, fmulp(beta, ks[5 * m + j])),
                                    add(bg, fmulp(beta, ks[6 * m + j]))),
                              add(cg, fmulp(beta, ks[7 * m + j]))),
                        zw);
    const Fr t3 = fmulp(fmulp(al2, sub(z, Fr::one())), l1[j]);                           // 261, 256 -> 256
    const Fr num = add(add(gate, fmulp(al_x, sub(p1, p2))), t3);                          // 276 + 241 -> 256
    bi_st(T, j, lane, Bp, fmulp(num, zh_inv[j & 3]));
  }
}

// Evaluation of up to six polynomials at per-lane points, in two levels so that no lane walks a
// whole polynomial alone: plonk_chunk_horner evaluates every chunk of CH coefficients at x
// (blockIdx.y = chunk, blockIdx.z = polynomial), plonk_eval_combine folds the chunk values with
// x^CH.  shared != 0: the polynomial is key-side (one coefficient array for all proofs).
constexpr uint32_t CH = 512;
struct EvalArgs {
  const Fr* poly[6];
  uint32_t len[6];
  uint8_t shared[6];
  uint8_t point_row[6];   // row of `pts` holding the evaluation point
};
__global__ __launch_bounds__(64) void plonk_chunk_horner(EvalArgs args, const Fr* pts, Fr* part,
                                                         uint32_t n_chunks, size_t Bp) {
  LANE;
  const int k = blockIdx.z;
  const uint32_t c = blockIdx.y, len = args.len[k];
  const uint32_t i0 = c * CH, i1 = i0 + CH < len ? i0 + CH : len;
  const Fr x = bi_ld(pts, args.point_row[k], lane, Bp);
  const Fr* p = args.poly[k];
  Fr acc = Fr::zero();
  if (args.shared[k]) {
    for (uint32_t i = i1; i-- > i0;) acc = add(mul(acc, x), p[i]);
  } else {
    for (uint32_t i = i1; i-- > i0;) acc = add(mul(acc, x), bi_ld(p, i, lane, Bp));
  }
  bi_st(part, (size_t)k * n_chunks + c, lane, Bp, acc);   // 0 for chunks past the end
}
__global__ __launch_bounds__(64) void plonk_eval_combine(EvalArgs args, const Fr* pts,
                                                         const Fr* part, Fr* out,
                                                         uint32_t n_chunks, size_t Bp) {
  LANE;
  const int k = blockIdx.y;
  Fr xl = bi_ld(pts, args.point_row[k], lane, Bp);
  for (uint32_t t = 1; t < CH; t <<= 1) xl = sqr(xl);   // x^CH
  Fr acc = Fr::zero();
  for (uint32_t c = n_chunks; c-- > 0;)
    acc = add(mul(acc, xl), bi_ld(part, (size_t)k * n_chunks + c, lane, Bp));
  bi_st(out, k, lane, Bp, acc);
}

// numerators of the two openings.  sc rows: 0 qm, 1 ql, 2 qr, 3 qo, 4 s3, 5 z, 6 tlo, 7 tmid, 8 thi,
// 9 c0 (constant term: r0 - sum_i v^i e_i), 10 v, 11 zeta, 12 zeta*w, 13 z(zeta w)
// CM (key with n_c commitments): sc rows 14 + i = Qcp_i(zeta); the numerator at zeta gains
// Qcp_i(zeta) pi2_i(X) (pi2: n_c x n rows, per proof) + v^(6+i) Qcp_i(X) (qcp: n_c x n, key side)
template <bool CM>
__global__ __launch_bounds__(64, 2) void plonk_lin(const Fr* ca, const Fr* cb, const Fr* cc,
                                                const Fr* cz, const Fr* t, const Fr* kc,
                                                const Fr* sc, Fr* N, Fr* NZ, size_t n, size_t Bp,
                                                Fr c266, uint32_t n_c, const Fr* pi2,
                                                const Fr* qcp) {
  // every product is (per-proof scalar) x (coefficient at 256): the scalars are lifted to 261 once
  // per lane (fmulp by 2^266: 256 + 266 - 261), the products then land at 256 (see fmulp)
  LANE;
  const Fr v = bi_ld(sc, 10, lane, Bp);
  const Fr vF = fmulp(v, c266);
  const Fr v2 = fmulp(vF, v), v3 = fmulp(vF, v2), v4 = fmulp(vF, v3), v5 = fmulp(vF, v4);   // 256
  const Fr v2F = fmulp(v2, c266), v3F = fmulp(v3, c266), v4F = fmulp(v4, c266), v5F = fmulp(v5, c266);
#define SCF(row) fmulp(bi_ld(sc, (row), lane, Bp), c266)
  const Fr sqm = SCF(0), sql = SCF(1), sqr_ = SCF(2), sqo = SCF(3), ss3 = SCF(4), sz = SCF(5),
           stl = SCF(6), stm = SCF(7), sth = SCF(8);
#undef SCF
  const size_t L = n + 3;
  for (size_t i = blockIdx.y; i < L; i += gridDim.y) {
    Fr r = Fr::zero();
    if (i < n) {   // key polynomials: qL qR qO qM qC S1 S2 S3 coefficient forms, n each
      r = add(add(fmulp(sql, kc[i]), fmulp(sqr_, kc[n + i])),
              add(fmulp(sqo, kc[2 * n + i]), fmulp(sqm, kc[3 * n + i])));
      r = add(r, add(kc[4 * n + i], fmulp(ss3, kc[7 * n + i])));
      r = add(r, add(fmulp(v4F, kc[5 * n + i]), fmulp(v5F, kc[6 * n + i])));
      if (CM) {   // scalars lifted to 261 as above, coefficients at 256
        Fr vp = v5;
        for (uint32_t k = 0; k < n_c; k++) {
          vp = fmulp(vF, vp);   // v^(6+k): 261 + 256 - 261
          r = add(r, add(fmulp(fmulp(bi_ld(sc, 14 + k, lane, Bp), c266), bi_ld(pi2, k * n + i, lane, Bp)),
                         fmulp(fmulp(vp, c266), qcp[k * n + i])));
        }
      }
    }
    const Fr zi = bi_ld(cz, i, lane, Bp);
    r = add(r, fmulp(sz, zi));
    if (i < n + 2) {
      r = add(r, add(fmulp(stl, bi_ld(t, i, lane, Bp)),
                     add(fmulp(stm, bi_ld(t, n + 2 + i, lane, Bp)),
                         fmulp(sth, bi_ld(t, 2 * n + 4 + i, lane, Bp)))));
      r = add(r, add(fmulp(vF, bi_ld(ca, i, lane, Bp)),
                     add(fmulp(v2F, bi_ld(cb, i, lane, Bp)), fmulp(v3F, bi_ld(cc, i, lane, Bp)))));
    }
    if (i == 0) r = add(r, bi_ld(sc, 9, lane, Bp));
    bi_st(N, i, lane, Bp, r);
    bi_st(NZ, i, lane, Bp, i == 0 ? sub(zi, bi_ld(sc, 13, lane, Bp)) : zi);
  }
}

// q = p / (X - x), exact: q[k-1] = p[k] + x q[k], in chunks of CH coefficients: the carry into
// chunk c is the suffix value S_c = sum_{k >= (c+1) CH} p[k] x^(k - (c+1) CH), a scan over the chunk
// values of plonk_chunk_horner (plonk_div_suffix), then every chunk runs its own recurrence
// (plonk_div_local).  `which` = blockIdx.z: 0 = (N, zeta), 1 = (NZ, zeta w).
__global__ __launch_bounds__(64) void plonk_div_suffix(const Fr* pts, Fr* part, uint32_t n_chunks,
                                                       size_t Bp) {
  LANE;
  const int k = blockIdx.y;
  Fr xl = bi_ld(pts, k, lane, Bp);
  for (uint32_t t = 1; t < CH; t <<= 1) xl = sqr(xl);
  Fr s = Fr::zero();   // S for the last chunk
  for (uint32_t c = n_chunks; c-- > 0;) {
    const Fr h = bi_ld(part, (size_t)k * n_chunks + c, lane, Bp);
    bi_st(part, (size_t)k * n_chunks + c, lane, Bp, s);
    s = add(h, mul(xl, s));
  }
}
__global__ __launch_bounds__(64) void plonk_div_local(const Fr* N, const Fr* NZ, const Fr* pts,
                                                      const Fr* part, Fr* W, Fr* WZ, uint32_t len,
                                                      uint32_t n_chunks, size_t Bp) {
  LANE;
  const int k = blockIdx.z;
  const uint32_t c = blockIdx.y;
  const Fr* p = k ? NZ : N;
  Fr* q = k ? WZ : W;
  const Fr x = bi_ld(pts, k, lane, Bp);
  const uint32_t i0 = c * CH, i1 = i0 + CH < len ? i0 + CH : len;
  Fr carry = bi_ld(part, (size_t)k * n_chunks + c, lane, Bp);   // q at index i1 - 1
  for (uint32_t i = i1; i-- > i0;) {
    if (i + 1 < len) bi_st(q, i, lane, Bp, carry);
    else bi_st(q, i, lane, Bp, Fr::zero());
    carry = add(bi_ld(p, i, lane, Bp), mul(x, carry));
  }
}

// ---- key from the trace form (zkmi_plonk_pk_load_trace): what the transforms do not compute -------
// out[i] = first base^i, square and multiply over the bits of i: w^i, and 5 w_4n^j
__global__ void plonk_powers_kernel(Fr* out, size_t count, Fr base, Fr first) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  Fr acc = first, b = base;
  for (size_t e = i; e; e >>= 1) {
    if (e & 1) acc = mul(acc, b);
    b = sqr(b);
  }
  out[i] = acc;
}
// sigma[p] = k_c' w^r' for perm[p] = c' n + r', k = 1, 5, 25; the loader has checked perm[p] < 3n
__global__ void plonk_sigma_kernel(const uint32_t* perm, const Fr* omega, Fr* sigma, uint32_t log_n,
                                   Fr k1, Fr k2) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= ((size_t)3 << log_n)) return;
  const uint32_t q = perm[p], c = q >> log_n;
  const Fr v = omega[q & (((uint32_t)1 << log_n) - 1)];
  sigma[p] = c == 0 ? v : mul(v, c == 1 ? k1 : k2);
}
// L_1(x) = (x^n - 1) / (n (x - 1)) at the coset points: x^n - 1 has period 4 there, zh_n[k] is its
// value over n; one inversion per point (ff.h's inverse: the divsteps of modinv30.h)
struct Fr4 {
  Fr v[4];
};
__global__ __launch_bounds__(256) void plonk_l1_kernel(const Fr* xs, Fr* l1, size_t m, Fr4 zh_n) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  l1[j] = mul(zh_n.v[j & 3], inverse(sub(xs[j], Fr::one())));
}

// ---- round 1 from solved wires (zkmi_plonk_round1_witness) ------------------------------------------
// One gate row per wavefront, 64 proofs per wavefront: the three wire indices, the marks and the
// selectors of the row are wave-uniform (scalar loads), the wires three coalesced row reads of the
// transposed wire matrix, the columns three row writes.  Gate value
//     qL a + qR b + qO c + qM a b + qC + PI_g,   PI_g = -a_g for g < n_public
// in gnark's image: qL qR qO qM are 2^261 images (fmulp: 256 + 261 - 261), a b = fmulp(a, 2^5 b)
// likewise; a selector marked 0 / +1 / -1 (scs_check.h) takes no product.  Rows below n_public also
// leave their a in `pub`, the public inputs round 3 and the transcript read.
// For a key with commitments (CM), committed rows and commitment rows are satisfied by construction,
// as the public rows are: their term of the gate equation, Qcp_i pi2_i resp. + H_i, is made from the
// columns afterwards (plonk_commit_check compares H_i).  The mark is the key's: bit 0 of skip[g]
// (the system's mark words are shared between keys).
struct ScsDev {
  const uint32_t* x[3];
  const uint32_t* marks;
  const Fr* sel;
  uint32_t n_gates, n_public;
  const uint8_t* skip;
};
// COLS = false (zkmi_scs_solve_batch): the check alone, no column and no public-input stores.
template <bool CM, bool COLS>
__device__ __forceinline__ void scs_gate_rows(const ScsDev& s, const Fr* __restrict__ w,
                                              Fr* __restrict__ a, Fr* __restrict__ b,
                                              Fr* __restrict__ c, Fr* __restrict__ pub,
                                              int32_t* __restrict__ st, size_t Bp) {
  const size_t p = (size_t)blockIdx.x * 64 + (threadIdx.x & 63);
  const size_t ng = s.n_gates;
  for (uint32_t g = __builtin_amdgcn_readfirstlane(blockIdx.y * 4 + (threadIdx.x >> 6)); g < s.n_gates;
       g += gridDim.y * 4) {
    const uint32_t mk = s.marks[g];
    const Fr va = bi_ld(w, s.x[0][g], p, Bp), vb = bi_ld(w, s.x[1][g], p, Bp),
             vc = bi_ld(w, s.x[2][g], p, Bp);
    if (COLS) {
      bi_st(a, g, p, Bp, va);
      bi_st(b, g, p, Bp, vb);
      bi_st(c, g, p, Bp, vc);
    }
    Fr sum = add(add(sel_term(mk & 3, va, s.sel + g), sel_term((mk >> 2) & 3, vb, s.sel + ng + g)),
                 sel_term((mk >> 4) & 3, vc, s.sel + 2 * ng + g));
    const uint32_t mm = (mk >> 6) & 3;
    if (mm != SCS_MARK_ZERO) sum = add(sum, sel_term(mm, fmulp(va, lift(vb, 5)), s.sel + 3 * ng + g));
    if (((mk >> 8) & 3) != SCS_MARK_ZERO) sum = add(sum, s.sel[4 * ng + g]);
    if (g < s.n_public) {
      sum = sub(sum, va);
      if (COLS) bi_st(pub, g, p, Bp, va);
    }
    if (CM && s.skip[g]) continue;
    if (!sum.is_zero()) st[p] = ZKMI_ERR_UNSATISFIED;
  }
}
template <bool CM>
__global__ __launch_bounds__(256) void scs_gate_kernel(ScsDev s, const Fr* __restrict__ w,
                                                       Fr* __restrict__ a, Fr* __restrict__ b,
                                                       Fr* __restrict__ c, Fr* __restrict__ pub,
                                                       int32_t* __restrict__ st, size_t Bp) {
  scs_gate_rows<CM, true>(s, w, a, b, c, pub, st, Bp);
}
__global__ __launch_bounds__(256) void scs_gate_check_kernel(ScsDev s, const Fr* __restrict__ w,
                                                             int32_t* __restrict__ st, size_t Bp) {
  scs_gate_rows<false, false>(s, w, nullptr, nullptr, nullptr, nullptr, st, Bp);
}

// ---- commitments (api.Commit) -------------------------------------------------------------------------
// dst row j = src row idx[j]: the committed values of one commitment, out of the value file or out of
// column a, as the rows of the matrix its MSM reads
__global__ void plonk_commit_gather(const Fr* __restrict__ src, const uint32_t* __restrict__ idx,
                                    Fr* __restrict__ dst, uint32_t count, size_t Bp) {
  LANE;
  for (uint32_t j = blockIdx.y; j < count; j += gridDim.y)
    bi_st(dst, j, lane, Bp, bi_ld(src, idx[j], lane, Bp));
}
// col row idx[j] = src row j, j in [j0, j1): pi2_i as a column of the domain (every other row was zeroed)
__global__ void plonk_commit_scatter(const Fr* __restrict__ src, const uint32_t* __restrict__ idx,
                                     Fr* __restrict__ col, uint32_t j0, uint32_t j1, size_t Bp) {
  LANE;
  for (uint32_t j = j0 + blockIdx.y; j < j1; j += gridDim.y)
    bi_st(col, idx[j], lane, Bp, bi_ld(src, j, lane, Bp));
}
// the solved columns against the commitments: a[r_i] must be H_i (one row of `h` per commitment)
struct CommitRows {
  uint32_t row[PLONK_MAX_COMMITMENTS];
};
__global__ void plonk_commit_check(const Fr* __restrict__ a, const Fr* __restrict__ h, CommitRows rows,
                                   uint32_t n_c, int32_t* __restrict__ st, size_t Bp) {
  LANE;
  for (uint32_t i = 0; i < n_c; i++)
    if (!(bi_ld(a, rows.row[i], lane, Bp) == bi_ld(h, i, lane, Bp))) st[lane] = ZKMI_ERR_UNSATISFIED;
}
// PI' beyond the public rows: + H_i at row r_i of the PI Lagrange column
__global__ void plonk_pi_commit(Fr* __restrict__ pi, const Fr* __restrict__ h, CommitRows rows,
                                uint32_t n_c, size_t Bp) {
  LANE;
  for (uint32_t i = 0; i < n_c; i++)
    bi_st(pi, rows.row[i], lane, Bp, add(bi_ld(pi, rows.row[i], lane, Bp), bi_ld(h, i, lane, Bp)));
}
// epi += Qcp_i pi2_i on the coset.  Exponents (fmulp): pi2 256 (per-proof data), the wave-uniform
// Qcp_i coset values 261 as stored by zkmi_plonk_pk_set_commitments: 256 + 261 - 261 = 256, as epi
__global__ __launch_bounds__(64) void plonk_qcp_fold(const Fr* __restrict__ e, const Fr* __restrict__ q,
                                                     Fr* __restrict__ epi, size_t m, size_t Bp) {
  LANE;
  for (size_t j = blockIdx.y; j < m; j += gridDim.y)
    bi_st(epi, j, lane, Bp, add(bi_ld(epi, j, lane, Bp), fmulp(bi_ld(e, j, lane, Bp), q[j])));
}

static int buf(zkmi_ctx* ctx, DevBuf& b, size_t bytes) {
  if (b.bytes >= bytes) return ZKMI_OK;
  if (b.p) {
    hipStreamSynchronize(ctx->stream);
    hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
  }
  if (hipMalloc(&b.p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    ctx->err = "plonk: hipMalloc(" + std::to_string(bytes) + " B) failed";
    return ZKMI_ERR_OOM;
  }
  b.bytes = bytes;
  return ZKMI_OK;
}

static Fr fr_small(uint32_t v) {
  Fr x = Fr::zero();
  x.v[0] = v;
  return to_mont(x);
}

// commitment of `count` polynomials whose coefficient rows start at scal[k] (row_idx[k] maps SRS
// power i to a row, or null): MSM over the SRS, affine, copied to out (proof-major, 64 B each)
static int commit(zkmi_ctx* ctx, zkmi_plonk_pk* pk, int count, const Fr* const* scal,
                  const uint32_t* const* row_idx, void* out_host_or_dev, size_t batch) {
  const size_t Bp = pk->Bp;
  int rc;
  if ((rc = buf(ctx, pk->small[2], Bp * 128)) || (rc = buf(ctx, pk->small[3], Bp * 64))) return rc;
  for (int k = 0; k < count; k++) {
    if ((rc = msm_run(ctx, pk->srs, scal[k], row_idx ? row_idx[k] : nullptr, Bp, batch,
                      pk->small[2].p)))
      return rc;
    if ((rc = xyzz_to_affine(ctx, 1, pk->small[2].p, pk->small[3].p, Bp))) return rc;
    // [lane] affine -> out[(lane * count + k)]
    ZK_HIP(hipMemcpy2DAsync((char*)out_host_or_dev + (size_t)k * 64, (size_t)count * 64,
                            pk->small[3].p, 64, 64, batch, hipMemcpyDefault, ctx->stream));
  }
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  return ZKMI_OK;
}

// staging buffer of one round call: freed on every exit path, after the stream has drained
struct RoundTmp {
  zkmi_ctx* ctx;
  void* p = nullptr;
  explicit RoundTmp(zkmi_ctx* c) : ctx(c) {}
  int alloc(size_t bytes) {
    if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) {
      (void)hipGetLastError();
      p = nullptr;
      ctx->err = "plonk: hipMalloc(" + std::to_string(bytes) + " B) failed";
      return ZKMI_ERR_OOM;
    }
    return ZKMI_OK;
  }
  ~RoundTmp() {
    if (p) {
      hipStreamSynchronize(ctx->stream);
      hipFree(p);
    }
  }
};

// ---- the commitment step (shared by the solver path, the witness path and the hint entry) ----------
// rows of commitment i's scalars in cm_scal; the buffers of a batch of Bp lanes
static int commit_buffers(zkmi_ctx* ctx, zkmi_plonk_pk* pk, size_t Bp) {
  size_t rows = 0;
  for (auto& c : pk->commits) {
    c.scal_row = rows;
    rows += c.n_rows + 2;
  }
  const size_t n_c = pk->commits.size();
  int rc;
  if ((rc = buf(ctx, pk->cm_scal, rows * Bp * 32)) || (rc = buf(ctx, pk->cm_blind, 2 * n_c * Bp * 32)) ||
      (rc = buf(ctx, pk->cm_h, n_c * Bp * 32)) || (rc = buf(ctx, pk->small[2], Bp * 128)) ||
      (rc = buf(ctx, pk->small[3], Bp * 64)))
    return rc;
  return ZKMI_OK;
}
static CommitRows commit_rows_of(const zkmi_plonk_pk* pk) {
  CommitRows r{};
  for (size_t i = 0; i < pk->commits.size(); i++) r.row[i] = pk->commits[i].row;
  return r;
}
// With the n_rows committed values of commitment i in its rows of cm_scal (gnark's image) and its two
// blinding scalars in `blind2` (two device rows): [pi2_i] = MSM over the n_rows + 2 Lagrange points
// -> affine -> host; H_i = hash_to_field(marshal, "BSB22-Plonk") on the host -> row i of cm_h.
// pts / hs: the host results of proof p at pts[p * stride], hs[p * stride].
static int commit_step(zkmi_ctx* ctx, zkmi_plonk_pk* pk, uint32_t i, const Fr* blind2, size_t Bp,
                       size_t batch, G1Affine* pts, Fr* hs, size_t stride) {
  const zkmi_plonk_pk::Commit& c = pk->commits[i];
  const size_t n = (size_t)1 << pk->log_n;
  Fr* scal = (Fr*)pk->cm_scal.p + c.scal_row * Bp;
  ZK_HIP(hipMemcpyAsync(scal + (size_t)c.n_rows * Bp, blind2, 2 * Bp * sizeof(Fr),
                        hipMemcpyDeviceToDevice, ctx->stream));
  if (c.row == n - 1)   // both blinding rows coincide: the second write wins
    ZK_HIP(hipMemsetAsync(scal + (size_t)c.n_rows * Bp, 0, Bp * sizeof(Fr), ctx->stream));
  int rc;
  if ((rc = msm_run(ctx, c.lag, scal, nullptr, Bp, batch, pk->small[2].p)) ||
      (rc = xyzz_to_affine(ctx, 1, pk->small[2].p, pk->small[3].p, Bp)))
    return rc;
  std::vector<G1Affine> hp(batch);
  ZK_HIP(hipMemcpyAsync(hp.data(), pk->small[3].p, batch * 64, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  std::vector<uint4> row(2 * Bp, make_uint4(0, 0, 0, 0));
  uint8_t msg[64];
  for (size_t p = 0; p < batch; p++) {
    g1_marshal(msg, hp[p]);
    const Fr h = hash_to_fr_dst(msg, 64, "BSB22-Plonk");
    pts[p * stride] = hp[p];
    hs[p * stride] = h;
    row[p] = make_uint4(h.v[0], h.v[1], h.v[2], h.v[3]);
    row[Bp + p] = make_uint4(h.v[4], h.v[5], h.v[6], h.v[7]);
  }
  ZK_HIP(hipMemcpyAsync((Fr*)pk->cm_h.p + (size_t)i * Bp, row.data(), 2 * Bp * 16, hipMemcpyHostToDevice,
                        ctx->stream));
  ZK_HIP(hipStreamSynchronize(ctx->stream));   // `row` is a local
  return ZKMI_OK;
}
static inline unsigned grid_rows(size_t rows) { return (unsigned)std::min<size_t>(std::max<size_t>(rows, 1), 4096); }
// the blinding scalars of the commitments: batch x 2 n_c fr -> rows of cm_blind; host result buffers
static int commit_begin(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const void* blind_commit, size_t batch,
                        size_t Bp) {
  const size_t n_c = pk->commits.size();
  int rc;
  if ((rc = commit_buffers(ctx, pk, Bp))) return rc;
  RoundTmp t(ctx);
  if ((rc = t.alloc(batch * 2 * n_c * 32))) return rc;
  ZK_HIP(hipMemcpyAsync(t.p, blind_commit, batch * 2 * n_c * 32, hipMemcpyDefault, ctx->stream));
  if ((rc = transpose_in(ctx, t.p, pk->cm_blind.p, 2 * n_c, batch, Bp, 32))) return rc;
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  pk->cm_pts.assign(batch * n_c, G1Affine{});
  pk->cm_H.assign(batch * n_c, Fr::zero());
  return ZKMI_OK;
}
// commitment i from rows idx[0 .. n_rows) of `src` (column a, or the value file in the F domain)
static int commit_from_rows(zkmi_ctx* ctx, zkmi_plonk_pk* pk, uint32_t i, const Fr* src,
                            const uint32_t* idx, bool f_domain, size_t Bp, size_t batch) {
  const zkmi_plonk_pk::Commit& c = pk->commits[i];
  const size_t n_c = pk->commits.size();
  Fr* scal = (Fr*)pk->cm_scal.p + c.scal_row * Bp;
  hipLaunchKernelGGL(plonk_commit_gather, dim3((unsigned)(Bp / 64), grid_rows(c.n_rows)), dim3(64), 0,
                     ctx->stream, src, idx, scal, c.n_rows, Bp);
  ZK_HIP(hipGetLastError());
  int rc;
  if (f_domain && (rc = rows_to_std_domain(ctx, scal, c.n_rows, Bp))) return rc;
  return commit_step(ctx, pk, i, (const Fr*)pk->cm_blind.p + (size_t)2 * i * Bp, Bp, batch,
                     pk->cm_pts.data() + i, pk->cm_H.data() + i, n_c);
}

}  // namespace zk

extern "C" {

void zkmi_plonk_pk_free(zkmi_ctx* ctx, zkmi_plonk_pk* pk) {
  if (!pk) return;
  if (ctx) {
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
  }
  for (Fr* p : {pk->coef, pk->coset, pk->sigma, pk->omega, pk->coset_x, pk->l1, pk->zh_inv})
    if (p) hipFree(p);
  if (pk->chunk_idx) hipFree(pk->chunk_idx);
  zkmi_msm_bases_free(ctx, pk->srs);
  for (int c = 0; c < 3; c++) {
    zkmi_msm_bases_free(ctx, pk->lag[c]);
    if (pk->lag_rows[c]) hipFree(pk->lag_rows[c]);
  }
  for (auto& b : pk->cf)
    if (b.p) hipFree(b.p);
  for (auto& b : pk->big)
    if (b.p) hipFree(b.p);
  for (auto& b : pk->small)
    if (b.p) hipFree(b.p);
  for (auto& c : pk->commits) {
    zkmi_msm_bases_free(ctx, c.lag);
    if (c.rows_dev) hipFree(c.rows_dev);
    if (c.slots_dev) hipFree(c.slots_dev);
  }
  for (void* p : {(void*)pk->qcp_coef, (void*)pk->qcp_coset, (void*)pk->cm_skip, pk->cm_scal.p,
                  pk->cm_blind.p, pk->cm_h.p, pk->cm_pi2.p})
    if (p) hipFree(p);
  delete pk;
}

// What both loaders share.  pk_new: the checks on the domain and the empty key; pk_finish, once the
// seven arrays of the key are on the device in gnark's image: the exponents the kernels expect, the
// rows of the quotient chunks, the SRS tables, the Lagrange tables.  On failure the caller frees pk.
struct PkCommon {
  const void* srs_g1;
  uint32_t window_bits;
  const void* const* lag_g1;
  const uint32_t* const* lag_rows;
  uint32_t lag_k;
};
static int pk_new(zkmi_ctx* ctx, uint32_t log_n, uint32_t n_public, uint32_t max_batch,
                  zkmi_plonk_pk** out) {
  if (log_n < 4 || log_n > 24) {
    ctx->err = "plonk pk: log_n out of range [4,24]";
    return ZKMI_ERR_ARG;
  }
  if (n_public >= (size_t)1 << log_n) {
    ctx->err = "plonk pk: more public inputs than gates";
    return ZKMI_ERR_ARG;
  }
  static std::atomic<uint64_t> serial{0};
  auto* pk = new zkmi_plonk_pk();
  pk->log_n = log_n;
  pk->n_public = n_public;
  pk->max_batch = max_batch ? max_batch : 64;
  pk->serial = ++serial;
  *out = pk;
  return ZKMI_OK;
}
static int pk_finish(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const PkCommon& k) {
  const size_t n = (size_t)1 << pk->log_n, m = 4 * n;
  // exponents the quotient kernel expects (plonk_quotient): 2^261 images of qL qR qO S1 S2 S3 on the
  // coset, of the coset points, L_1 and 1 / Z_H; 2^266 of qM; qC as uploaded
  {
    struct { Fr* p; size_t count; int k; } lifts[7] = {
        {pk->coset, 3 * m, 5},   {pk->coset + 3 * m, m, 10}, {pk->coset + 5 * m, 3 * m, 5},
        {pk->coset_x, m, 5},     {pk->l1, m, 5},             {pk->zh_inv, 4, 5},
        {nullptr, 0, 0}};
    for (auto& l : lifts)
      if (l.count)
        hipLaunchKernelGGL(plonk_lift_kernel, dim3((unsigned)((l.count + 255) / 256)), dim3(256), 0,
                           ctx->stream, l.p, l.count, l.k);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) {
      ctx->err = "plonk pk: key scaling failed";
      return ZKMI_ERR_HIP;
    }
  }
  // scalar-row maps of the three quotient chunks: power i of chunk c -> row c (n + 2) + i of the
  // 4n-row coefficient buffer; powers n+2 .. n+5 -> its last row (zero: deg t < 3n + 6)
  {
    std::vector<uint32_t> idx(3 * (n + 6));
    for (size_t c = 0; c < 3; c++)
      for (size_t i = 0; i < n + 6; i++)
        idx[c * (n + 6) + i] = (uint32_t)(i < n + 2 ? c * (n + 2) + i : m - 1);
    if (hipMalloc((void**)&pk->chunk_idx, idx.size() * 4) != hipSuccess ||
        hipMemcpy(pk->chunk_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
      return ZKMI_ERR_HIP;
  }
  int rc = zkmi_msm_bases_load(ctx, 1, k.srs_g1, n + 6, (int)k.window_bits, &pk->srs);
  if (rc) return rc;
  if (k.lag_k) {   // after the SRS tables: these are small (2^k / k entries per point)
    if (k.lag_k < 4 || k.lag_k > 16) {
      ctx->err = "plonk pk: lag_k must be 0 or in [4,16]";
      return ZKMI_ERR_ARG;
    }
    for (int c = 0; c < 3; c++) {
      if (!k.lag_g1[c] || !k.lag_rows[c]) {
        ctx->err = "plonk pk: lag_k set without lag_g1 / lag_rows";
        return ZKMI_ERR_ARG;
      }
      std::vector<uint32_t> rows(n + 2);
      if (hipMemcpy(rows.data(), k.lag_rows[c], (n + 2) * 4, hipMemcpyDefault) != hipSuccess)
        return ZKMI_ERR_HIP;
      for (uint32_t r : rows)
        if (r >= n + 2) {
          ctx->err = "plonk pk: lag_rows entry out of range";
          return ZKMI_ERR_ARG;
        }
      if (hipMalloc((void**)&pk->lag_rows[c], (n + 2) * 4) != hipSuccess ||
          hipMemcpy(pk->lag_rows[c], rows.data(), (n + 2) * 4, hipMemcpyHostToDevice) != hipSuccess)
        return ZKMI_ERR_HIP;
      // 200 + k: subset-sum comb tables over groups of k points (zero digits are skipped)
      if ((rc = zkmi_msm_bases_load(ctx, 1, k.lag_g1[c], n + 2, 200 + (int)k.lag_k, &pk->lag[c])))
        return rc;
    }
  }
  return ZKMI_OK;
}

int zkmi_plonk_pk_load(zkmi_ctx* ctx, const zkmi_plonk_pk_desc* d, zkmi_plonk_pk** out) {
  ZK_HIP(hipSetDevice(ctx->device));
  if (!d || !out) return ZKMI_ERR_ARG;
  zkmi_plonk_pk* pk;
  int rc = pk_new(ctx, d->log_n, d->n_public, d->max_batch, &pk);
  if (rc) return rc;
  const size_t n = (size_t)1 << d->log_n, m = 4 * n;
  struct { Fr** dst; const void* src; size_t count; } up[7] = {
      {&pk->coef, d->coef, 8 * n},   {&pk->coset, d->coset, 8 * m},   {&pk->sigma, d->sigma, 3 * n},
      {&pk->omega, d->omega, n},     {&pk->coset_x, d->coset_x, m},   {&pk->l1, d->l1_coset, m},
      {&pk->zh_inv, d->zh_inv, 4}};
  for (auto& u : up) {
    if (!u.src || hipMalloc((void**)u.dst, u.count * 32) != hipSuccess ||
        hipMemcpy(*u.dst, u.src, u.count * 32, hipMemcpyDefault) != hipSuccess) {
      ctx->err = "plonk pk: upload failed";
      zkmi_plonk_pk_free(ctx, pk);
      return ZKMI_ERR_HIP;
    }
  }
  if ((rc = pk_finish(ctx, pk, PkCommon{d->srs_g1, d->window_bits, d->lag_g1, d->lag_rows, d->lag_k}))) {
    zkmi_plonk_pk_free(ctx, pk);
    return rc;
  }
  *out = pk;
  return ZKMI_OK;
}

// Round 1 is shared by its two entries (zkmi_plonk_round1: the solver; zkmi_plonk_round1_witness:
// solved wires) apart from how the columns come to be.  round1_begin: the batch's buffers;
// round1_tail, with the Lagrange values of a, b, c in rows [0, nc) of big[1..3]: inverse transforms,
// blinding (rows of small[0]), commitments in coefficient form or in the Lagrange basis.
static int round1_begin(zkmi_ctx* ctx, zkmi_plonk_pk* pk, size_t batch) {
  const size_t n = (size_t)1 << pk->log_n, m = 4 * n, Bp = round_up(batch, 64);
  int rc;
  pk->batch = batch;
  pk->Bp = Bp;
  pk->round = 0;
  pk->proved = true;
  for (auto& b : pk->cf)
    if ((rc = buf(ctx, b, (n + 8) * Bp * 32))) return rc;
  for (auto& b : pk->big)
    if ((rc = buf(ctx, b, m * Bp * 32))) return rc;
  // small[0]: the 9 blinding rows, then the evaluations, then the 14 (+ n_c) scalars of round 5
  const size_t rows0 = pk->commits.empty() ? 16 : 24;
  if ((rc = buf(ctx, pk->small[0], rows0 * Bp * 32)) || (rc = buf(ctx, pk->small[1], 16 * Bp * 32)))
    return rc;
  if (!pk->commits.empty() && (rc = buf(ctx, pk->cm_pi2, pk->commits.size() * n * Bp * 32))) return rc;
  return ZKMI_OK;
}
static const char* const kNoCommitments =
    "plonk: this key carries commitments: prove it with zkmi_plonk_prove_ex / "
    "zkmi_plonk_prove_witness_ex (the plain and the round-by-round entries do not carry them)";
static int round1_tail(zkmi_ctx* ctx, zkmi_plonk_pk* pk, size_t nc, void* commits_out) {
  const size_t n = (size_t)1 << pk->log_n, Bp = pk->Bp, batch = pk->batch;
  Fr *A = (Fr*)pk->big[1].p, *B = (Fr*)pk->big[2].p, *C = (Fr*)pk->big[3].p;
  int rc;
  Fr* cols[3] = {A, B, C};
  // rows no gate writes (padding gates) must read as zero in round 2
  if (nc < n)
    for (Fr* col : cols)
      hipLaunchKernelGGL(plonk_zero_rows, dim3((unsigned)(Bp / 64), 64), dim3(64), 0, ctx->stream,
                         col, nc, n, Bp);
  NttPlan* plan;
  if ((rc = get_plan(ctx, (int)pk->log_n, &plan))) return rc;
  const dim3 gl((unsigned)(Bp / 64));
  // columns (rows >= nc read as zero) -> coefficients -> blinded
  for (int k = 0; k < 3; k++) {
    Fr* cf = (Fr*)pk->cf[k].p;
    if ((rc = ntt_bi(ctx, plan, cols[k], cf, Bp, true, false, nc))) return rc;
    hipLaunchKernelGGL(plonk_zero_rows, dim3((unsigned)(Bp / 64), 8), dim3(64), 0, ctx->stream, cf, n,
                       n + 8, Bp);
    hipLaunchKernelGGL(plonk_blind, gl, dim3(64), 0, ctx->stream, cf, n, (const Fr*)pk->small[0].p,
                       2 * k, 2, Bp);
  }
  ZK_HIP(hipGetLastError());
  if (pk->lag[0]) {
    // Lagrange basis: the columns' values are the scalars; rows n, n + 1 of a column buffer take
    // its blinding scalars b1, b2 (points [tau^(n+1) - tau], [tau^n - 1])
    if ((rc = buf(ctx, pk->small[2], Bp * 128)) || (rc = buf(ctx, pk->small[3], Bp * 64))) return rc;
    for (int k = 0; k < 3; k++) {
      ZK_HIP(hipMemcpyAsync(cols[k] + n * Bp, (const Fr*)pk->small[0].p + (size_t)(2 * k) * Bp,
                            2 * Bp * sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream));
      if ((rc = msm_run(ctx, pk->lag[k], cols[k], pk->lag_rows[k], Bp, batch, pk->small[2].p)))
        return rc;
      if ((rc = xyzz_to_affine(ctx, 1, pk->small[2].p, pk->small[3].p, Bp))) return rc;
      ZK_HIP(hipMemcpy2DAsync((char*)commits_out + (size_t)k * 64, (size_t)3 * 64, pk->small[3].p, 64,
                              64, batch, hipMemcpyDefault, ctx->stream));
    }
    ZK_HIP(hipStreamSynchronize(ctx->stream));
  } else {
    const Fr* sc[3] = {(Fr*)pk->cf[0].p, (Fr*)pk->cf[1].p, (Fr*)pk->cf[2].p};
    if ((rc = commit(ctx, pk, 3, sc, nullptr, commits_out, batch))) return rc;
  }
  pk->round = 1;
  return ZKMI_OK;
}

// Round 1: witness solve (the constraint system's rows are the gate columns a, b, c), blinding,
// commitments [a], [b], [c].
static int round1_solve(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const zkmi_cs* cs, const void* inputs,
                        size_t batch, const void* blind, const void* blind_commit, void* commits_out,
                        int32_t* status_out);
int zkmi_plonk_round1(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const zkmi_cs* cs, const void* inputs,
                      size_t batch, const void* blind, void* commits_out, int32_t* status_out) {
  if (!pk->commits.empty()) {
    ctx->err = kNoCommitments;
    return ZKMI_ERR_ARG;
  }
  return round1_solve(ctx, pk, cs, inputs, batch, blind, nullptr, commits_out, status_out);
}
// blind_commit: the blinding scalars of the key's commitments (null for a key without)
static int round1_solve(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const zkmi_cs* cs, const void* inputs,
                        size_t batch, const void* blind, const void* blind_commit, void* commits_out,
                        int32_t* status_out) {
  ZK_HIP(hipSetDevice(ctx->device));
  int rc;
  if ((rc = require_idle(ctx))) return rc;
  if (batch == 0 || batch > pk->max_batch) {
    ctx->err = "plonk: batch must be in [1, max_batch]";
    return ZKMI_ERR_ARG;
  }
  const size_t n = (size_t)1 << pk->log_n, m = 4 * n, Bp = round_up(batch, 64);
  if (cs->n_constraints > n || cs->n_public - 1 != pk->n_public) {
    ctx->err = "plonk: constraint system does not match the key";
    return ZKMI_ERR_ARG;
  }
  // the program's COMMIT rows are the key's commitments, in order, and every operand slot is a wire
  const size_t n_c = pk->commits.size();
  if (cs->commit_rows.size() != n_c) {
    ctx->err = "plonk: the constraint system has " + std::to_string(cs->commit_rows.size()) +
               " COMMIT rows, the key " + std::to_string(n_c) + " commitments";
    return ZKMI_ERR_ARG;
  }
  for (size_t i = 0; i < n_c; i++) {
    const auto& c = pk->commits[i];
    bool ok = !c.slots.empty();
    for (uint32_t sl : c.slots) ok = ok && sl < cs->n_wires;
    if (!ok) {
      ctx->err = "plonk: commitment " + std::to_string(i) +
                 " has no operand slots, or one that is not a wire of the constraint system";
      return ZKMI_ERR_ARG;
    }
  }
  if ((rc = round1_begin(ctx, pk, batch))) return rc;
  if (n_c && (rc = commit_begin(ctx, pk, blind_commit, batch, Bp))) return rc;
  const size_t n_in = cs->n_public - 1 + cs->n_secret, nc = cs->n_constraints;
  // stage inputs + blinding scalars (host or device, proof-major)
  // value file and gate columns: big[0] = slots (reused later), big[1..3] = a, b, c; every size is
  // checked before anything is staged
  if ((size_t)cs->n_slots > m || n_in > m) {
    ctx->err = "plonk: value file or input vector larger than the 4n work buffer";
    return ZKMI_ERR_ARG;
  }
  RoundTmp tin(ctx), tbl(ctx);
  if ((rc = tin.alloc(batch * n_in * 32)) || (rc = tbl.alloc(batch * 9 * 32))) return rc;
  void *in_dev = tin.p, *bl_dev = tbl.p;
  ZK_HIP(hipMemcpyAsync(in_dev, inputs, batch * n_in * 32, hipMemcpyDefault, ctx->stream));
  ZK_HIP(hipMemcpyAsync(bl_dev, blind, batch * 9 * 32, hipMemcpyDefault, ctx->stream));
  Fr* slots = (Fr*)pk->big[0].p;
  Fr *A = (Fr*)pk->big[1].p, *B = (Fr*)pk->big[2].p, *C = (Fr*)pk->big[3].p;
  void* st;
  if ((rc = ensure_scratch(ctx, ctx->sets[0].misc, Bp * 4, &st))) return rc;
  rc = transpose_in(ctx, in_dev, slots + Bp, n_in, batch, Bp, 32);
  // the inputs in gnark's image, for PI(X) in round 3: big[5] rows 0 .. n_pub - 1 are the public ones
  if (!rc) rc = transpose_in(ctx, in_dev, pk->big[5].p, n_in, batch, Bp, 32);
  if (!rc) rc = rows_to_f_domain(ctx, slots + Bp, n_in, Bp);
  if (!rc) rc = transpose_in(ctx, bl_dev, pk->small[0].p, 9, batch, Bp, 32);
  if (!rc && n_c == 0) {
    rc = solve_bi(ctx, cs, slots, A, B, C, (int32_t*)st, Bp);
  } else if (!rc) {
    // the program stops at every COMMIT row: the commitment step on the operands' slots of the value
    // file (F domain), H_i into the challenge wire's slot, and on
    rc = solve_init(ctx, slots, (int32_t*)st, Bp);
    uint32_t begin = 0;
    for (size_t i = 0; !rc && i < n_c; i++) {
      rc = solve_rows(ctx, cs, slots, A, B, C, (int32_t*)st, Bp, begin, cs->commit_rows[i].first);
      if (!rc) rc = commit_from_rows(ctx, pk, (uint32_t)i, slots, pk->commits[i].slots_dev, true, Bp, batch);
      Fr* wire = slots + (size_t)cs->commit_rows[i].second * Bp;
      if (!rc && hipMemcpyAsync(wire, (const Fr*)pk->cm_h.p + i * Bp, Bp * sizeof(Fr),
                                hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)
        rc = ZKMI_ERR_HIP;
      if (!rc) rc = rows_to_f_domain(ctx, wire, 1, Bp);
      begin = cs->commit_rows[i].first + 1;
    }
    if (!rc) rc = solve_rows(ctx, cs, slots, A, B, C, (int32_t*)st, Bp, begin, cs->n_rows);
  }
  if (!rc) rc = rows_to_std_domain(ctx, A, nc, Bp);
  if (!rc) rc = rows_to_std_domain(ctx, B, nc, Bp);
  if (!rc) rc = rows_to_std_domain(ctx, C, nc, Bp);
  hipStreamSynchronize(ctx->stream);
  if (rc) return rc;
  ZK_HIP(hipMemcpy(status_out, st, batch * 4, hipMemcpyDefault));
  return round1_tail(ctx, pk, nc, commits_out);
}

// Round 2: beta, gamma (batch x 2 fr) -> grand product z, blinded, commitment [z].
// The gate columns are still in big[1..3] (Lagrange values).
int zkmi_plonk_round2(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const void* beta_gamma, void* commit_z_out) {
  ZK_HIP(hipSetDevice(ctx->device));
  if (pk->round != 1) {
    ctx->err = "plonk: round 2 out of order";
    return ZKMI_ERR_ARG;
  }
  const size_t n = (size_t)1 << pk->log_n, Bp = pk->Bp, batch = pk->batch;
  int rc;
  RoundTmp t2(ctx);
  if ((rc = t2.alloc(batch * 64))) return rc;
  void* tmp = t2.p;
  ZK_HIP(hipMemcpyAsync(tmp, beta_gamma, batch * 64, hipMemcpyDefault, ctx->stream));
  Fr* ch = (Fr*)pk->small[1].p;   // rows: 0 beta, 1 gamma, 2 alpha, 3 zeta ...
  rc = transpose_in(ctx, tmp, ch, 2, batch, Bp, 32);
  if (rc) return rc;
  // the solver leaves rows >= n_constraints of the columns untouched: they must read as zero here
  Fr *A = (Fr*)pk->big[1].p, *B = (Fr*)pk->big[2].p, *C = (Fr*)pk->big[3].p;
  Fr *F = (Fr*)pk->big[0].p, *G = F + n * Bp, *P = G + n * Bp, *cp = P + n * Bp;   // 4n rows in all
  const size_t chunk = 256, n_chunks = (n + chunk - 1) / chunk;
  const unsigned gy = (unsigned)(n < 4096 ? n : 4096);
  hipLaunchKernelGGL(plonk_fg, dim3((unsigned)(Bp / 64), gy), dim3(64), 0, ctx->stream, A, B, C,
                     pk->sigma, pk->omega, ch, F, G, n, Bp, fr_small(5), fr_small(25));
  hipLaunchKernelGGL(plonk_ratio, dim3((unsigned)(Bp / 64), (unsigned)n_chunks), dim3(64), 0,
                     ctx->stream, F, G, P, cp, n, chunk, Bp);
  hipLaunchKernelGGL(plonk_chunk_scan, dim3((unsigned)(Bp / 64)), dim3(64), 0, ctx->stream, cp,
                     n_chunks, Bp);
  Fr* Z = (Fr*)pk->big[4].p;
  hipLaunchKernelGGL(plonk_z_fill, dim3((unsigned)(Bp / 64), (unsigned)n_chunks), dim3(64), 0,
                     ctx->stream, F, cp, Z, n, chunk, Bp);
  ZK_HIP(hipGetLastError());
  NttPlan* plan;
  if ((rc = get_plan(ctx, (int)pk->log_n, &plan))) return rc;
  Fr* cz = (Fr*)pk->cf[3].p;
  if ((rc = ntt_bi(ctx, plan, Z, cz, Bp, true, false, n))) return rc;
  hipLaunchKernelGGL(plonk_zero_rows, dim3((unsigned)(Bp / 64), 8), dim3(64), 0, ctx->stream, cz, n,
                     n + 8, Bp);
  hipLaunchKernelGGL(plonk_blind, dim3((unsigned)(Bp / 64)), dim3(64), 0, ctx->stream, cz, n,
                     (const Fr*)pk->small[0].p, 6, 3, Bp);
  ZK_HIP(hipGetLastError());
  const Fr* sc[1] = {cz};
  if ((rc = commit(ctx, pk, 1, sc, nullptr, commit_z_out, batch))) return rc;
  pk->round = 2;
  return ZKMI_OK;
}

// Round 3: alpha (batch fr) -> quotient, commitments [t_lo], [t_mid], [t_hi].
int zkmi_plonk_round3(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const void* alpha, void* commits_t_out) {
  ZK_HIP(hipSetDevice(ctx->device));
  if (pk->round != 2) {
    ctx->err = "plonk: round 3 out of order";
    return ZKMI_ERR_ARG;
  }
  const size_t n = (size_t)1 << pk->log_n, m = 4 * n, Bp = pk->Bp, batch = pk->batch;
  int rc;
  RoundTmp t3(ctx);
  if ((rc = t3.alloc(batch * 32))) return rc;
  void* tmp = t3.p;
  ZK_HIP(hipMemcpyAsync(tmp, alpha, batch * 32, hipMemcpyDefault, ctx->stream));
  Fr* ch = (Fr*)pk->small[1].p;
  rc = transpose_in(ctx, tmp, ch + 2 * Bp, 1, batch, Bp, 32);   // row 2
  if (rc) return rc;
  NttPlan *plan_n, *plan_m;
  if ((rc = get_plan(ctx, (int)pk->log_n, &plan_n)) ||
      (rc = get_plan(ctx, (int)pk->log_n + 2, &plan_m)))
    return rc;
  // PI(X): Lagrange values (-x_j) from the public-input rows saved in big[5] -> coefficients
  // (big[0]) -> coset evaluations (big[5])
  // (circuits with more than eight public inputs; otherwise plonk_quotient evaluates PI itself)
  // (a key with commitments always takes the buffer: it then holds PI' + sum_i Qcp_i pi2_i)
  const size_t n_c = pk->commits.size();
  const int n_pub_direct = pk->n_public <= 8 && n_c == 0 ? (int)pk->n_public : -1;
  Fr *EA = (Fr*)pk->big[1].p, *EB = (Fr*)pk->big[2].p, *EC = (Fr*)pk->big[3].p,
     *EZ = (Fr*)pk->big[4].p, *EPI = (Fr*)pk->big[5].p;
  if (n_pub_direct < 0) {
    Fr* pil = (Fr*)pk->big[0].p;
    hipLaunchKernelGGL(plonk_pi, dim3((unsigned)(Bp / 64), (unsigned)(n < 4096 ? n : 4096)),
                       dim3(64), 0, ctx->stream, (const Fr*)pk->big[5].p, pil, (size_t)pk->n_public, n,
                       Bp);
    if (n_c)
      hipLaunchKernelGGL(plonk_pi_commit, dim3((unsigned)(Bp / 64)), dim3(64), 0, ctx->stream, pil,
                         (const Fr*)pk->cm_h.p, commit_rows_of(pk), (uint32_t)n_c, Bp);
    ZK_HIP(hipGetLastError());
    Fr* pic = pil + n * Bp;
    if ((rc = ntt_bi(ctx, plan_n, pil, pic, Bp, true, false, n)) ||
        (rc = ntt_bi(ctx, plan_m, pic, EPI, Bp, false, true, n)))
      return rc;
  }
  // Commitments.  PI' also holds + H_i at row r_i (added to the Lagrange column above, before its
  // transforms: see the launch order below).  Then per commitment: pi2_i as a column of the domain
  // (big[0] rows [0, n): zeroed, its n_rows + 2 scalars scattered; the blinding row n - 1 last, so
  // that it wins where both blinding rows coincide) -> coefficient form, kept in cm_pi2 for round 5
  // -> coset evaluations in big[4], which is free here (Z's Lagrange values are no longer needed and
  // its coset evaluations are made below) -> epi += Qcp_i pi2_i.  No further 4n buffer.
  for (size_t i = 0; i < n_c; i++) {
    const zkmi_plonk_pk::Commit& c = pk->commits[i];
    Fr* col = (Fr*)pk->big[0].p;
    Fr* cf = (Fr*)pk->cm_pi2.p + i * n * Bp;
    Fr* E = (Fr*)pk->big[4].p;
    const Fr* scal = (const Fr*)pk->cm_scal.p + c.scal_row * Bp;
    ZK_HIP(hipMemsetAsync(col, 0, n * Bp * sizeof(Fr), ctx->stream));
    hipLaunchKernelGGL(plonk_commit_scatter, dim3((unsigned)(Bp / 64), grid_rows(c.n_rows + 1)), dim3(64),
                       0, ctx->stream, scal, (const uint32_t*)c.rows_dev, col, 0u, c.n_rows + 1, Bp);
    hipLaunchKernelGGL(plonk_commit_scatter, dim3((unsigned)(Bp / 64), 1), dim3(64), 0, ctx->stream, scal,
                       (const uint32_t*)c.rows_dev, col, c.n_rows + 1, c.n_rows + 2, Bp);
    ZK_HIP(hipGetLastError());
    if ((rc = ntt_bi(ctx, plan_n, col, cf, Bp, true, false, n)) ||
        (rc = ntt_bi(ctx, plan_m, cf, E, Bp, false, true, n)))
      return rc;
    hipLaunchKernelGGL(plonk_qcp_fold, dim3((unsigned)(Bp / 64), (unsigned)(m < 8192 ? m : 8192)), dim3(64),
                       0, ctx->stream, (const Fr*)E, (const Fr*)(pk->qcp_coset + i * m), EPI, m, Bp);
    ZK_HIP(hipGetLastError());
  }
  if ((rc = ntt_bi(ctx, plan_m, (Fr*)pk->cf[0].p, EA, Bp, false, true, n + 2)) ||
      (rc = ntt_bi(ctx, plan_m, (Fr*)pk->cf[1].p, EB, Bp, false, true, n + 2)) ||
      (rc = ntt_bi(ctx, plan_m, (Fr*)pk->cf[2].p, EC, Bp, false, true, n + 2)) ||
      (rc = ntt_bi(ctx, plan_m, (Fr*)pk->cf[3].p, EZ, Bp, false, true, n + 3)))
    return rc;
  Fr* T = (Fr*)pk->big[0].p;
  hipLaunchKernelGGL(plonk_quotient, dim3((unsigned)(Bp / 64), (unsigned)(m < 8192 ? m : 8192)),
                     dim3(64), 0, ctx->stream, EA, EB, EC, EZ, EPI, pk->coset, pk->coset_x, pk->l1,
                     pk->zh_inv, ch, T, m, Bp, lift(fr_small(5), 5),
                     lift(fr_small(25), 5), n_pub_direct, pow2_image(271), pow2_image(281));
  ZK_HIP(hipGetLastError());
  // coset interpolation: t coefficients in big[1]
  Fr* ct = (Fr*)pk->big[1].p;
  if ((rc = ntt_bi(ctx, plan_m, T, ct, Bp, true, true, m))) return rc;
  const Fr* sc[3] = {ct, ct, ct};
  const uint32_t* ri[3] = {pk->chunk_idx, pk->chunk_idx + (n + 6), pk->chunk_idx + 2 * (n + 6)};
  if ((rc = commit(ctx, pk, 3, sc, ri, commits_t_out, batch))) return rc;
  pk->round = 3;
  return ZKMI_OK;
}

// Round 4: zeta (batch fr) -> a(zeta), b(zeta), c(zeta), S1(zeta), S2(zeta), z(zeta w)
static int round4_run(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const void* zeta_zetaw, void* evals_out,
                      void* qcp_out);
int zkmi_plonk_round4(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const void* zeta_zetaw, void* evals_out) {
  return round4_run(ctx, pk, zeta_zetaw, evals_out, nullptr);
}
// qcp_out (keys with commitments): batch x n_c fr, Qcp_i(zeta)
static int round4_run(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const void* zeta_zetaw, void* evals_out,
                      void* qcp_out) {
  ZK_HIP(hipSetDevice(ctx->device));
  if (pk->round != 3) {
    ctx->err = "plonk: round 4 out of order";
    return ZKMI_ERR_ARG;
  }
  const size_t n = (size_t)1 << pk->log_n, Bp = pk->Bp, batch = pk->batch;
  int rc;
  RoundTmp t4(ctx), t4o(ctx);
  if ((rc = t4.alloc(batch * 64)) || (rc = t4o.alloc(batch * 6 * 32))) return rc;
  void* tmp = t4.p;
  ZK_HIP(hipMemcpyAsync(tmp, zeta_zetaw, batch * 64, hipMemcpyDefault, ctx->stream));
  Fr* pts = (Fr*)pk->small[1].p + 4 * Bp;   // rows 4, 5 of the challenge block: zeta, zeta w
  rc = transpose_in(ctx, tmp, pts, 2, batch, Bp, 32);
  if (rc) return rc;
  EvalArgs ea{};
  const Fr* polys[6] = {(Fr*)pk->cf[0].p, (Fr*)pk->cf[1].p, (Fr*)pk->cf[2].p, pk->coef + 5 * n,
                        pk->coef + 6 * n, (Fr*)pk->cf[3].p};
  const uint32_t lens[6] = {(uint32_t)n + 2, (uint32_t)n + 2, (uint32_t)n + 2, (uint32_t)n,
                            (uint32_t)n, (uint32_t)n + 3};
  for (int k = 0; k < 6; k++) {
    ea.poly[k] = polys[k];
    ea.len[k] = lens[k];
    ea.shared[k] = (k == 3 || k == 4) ? 1 : 0;
    ea.point_row[k] = k == 5 ? 1 : 0;
  }
  Fr* ev = (Fr*)pk->small[0].p;   // rows 0 .. 5 (the blinding rows are no longer needed)
  const uint32_t n_chunks = (uint32_t)((n + 3 + CH - 1) / CH);
  Fr* part = (Fr*)pk->big[2].p;   // 6 * n_chunks rows
  hipLaunchKernelGGL(plonk_chunk_horner, dim3((unsigned)(Bp / 64), n_chunks, 6), dim3(64), 0,
                     ctx->stream, ea, (const Fr*)pts, part, n_chunks, Bp);
  hipLaunchKernelGGL(plonk_eval_combine, dim3((unsigned)(Bp / 64), 6), dim3(64), 0, ctx->stream, ea,
                     (const Fr*)pts, (const Fr*)part, ev, n_chunks, Bp);
  ZK_HIP(hipGetLastError());
  // Qcp_i(zeta): the same two kernels over the key-side coefficient forms, six slots per launch,
  // into rows 6 .. 6 + n_c - 1 of ev; their chunk values behind the first launch's
  const size_t n_c = pk->commits.size();
  RoundTmp t4q(ctx);
  if (n_c) {
    if (!qcp_out) {
      ctx->err = kNoCommitments;
      return ZKMI_ERR_ARG;
    }
    if ((rc = t4q.alloc(batch * n_c * 32))) return rc;
    for (size_t i0 = 0; i0 < n_c; i0 += 6) {
      const unsigned cnt = (unsigned)std::min<size_t>(6, n_c - i0);
      EvalArgs eq{};
      for (unsigned k = 0; k < cnt; k++) {
        eq.poly[k] = pk->qcp_coef + (i0 + k) * n;
        eq.len[k] = (uint32_t)n;
        eq.shared[k] = 1;
        eq.point_row[k] = 0;
      }
      Fr* part_q = part + (size_t)(6 + i0) * n_chunks * Bp;
      hipLaunchKernelGGL(plonk_chunk_horner, dim3((unsigned)(Bp / 64), n_chunks, cnt), dim3(64), 0,
                         ctx->stream, eq, (const Fr*)pts, part_q, n_chunks, Bp);
      hipLaunchKernelGGL(plonk_eval_combine, dim3((unsigned)(Bp / 64), cnt), dim3(64), 0, ctx->stream, eq,
                         (const Fr*)pts, (const Fr*)part_q, ev + (6 + i0) * Bp, n_chunks, Bp);
    }
    ZK_HIP(hipGetLastError());
    rc = transpose_out(ctx, ev + 6 * Bp, t4q.p, n_c, batch, Bp, 32);
    if (!rc && hipMemcpyAsync(qcp_out, t4q.p, batch * n_c * 32, hipMemcpyDefault, ctx->stream) !=
                   hipSuccess)
      rc = ZKMI_ERR_HIP;
    if (rc) return rc;
  }
  void* out_dev = t4o.p;
  rc = transpose_out(ctx, ev, out_dev, 6, batch, Bp, 32);
  if (!rc && hipMemcpyAsync(evals_out, out_dev, batch * 6 * 32, hipMemcpyDefault, ctx->stream) !=
                 hipSuccess)
    rc = ZKMI_ERR_HIP;
  hipStreamSynchronize(ctx->stream);
  if (rc) return rc;
  pk->round = 4;
  return ZKMI_OK;
}

// Round 5: per-proof scalars of the linearisation polynomial and of the openings (batch x 14 fr,
// see plonk_lin) -> commitments [W_zeta], [W_zeta_w]
static int round5_run(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const void* scalars, size_t n_sc,
                      void* commits_w_out);
int zkmi_plonk_round5(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const void* scalars, void* commits_w_out) {
  if (!pk->commits.empty()) {
    ctx->err = kNoCommitments;
    return ZKMI_ERR_ARG;
  }
  return round5_run(ctx, pk, scalars, 14, commits_w_out);
}
// n_sc = 14 + n_c scalars per proof: the 14 above, then Qcp_i(zeta)
static int round5_run(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const void* scalars, size_t n_sc,
                      void* commits_w_out) {
  ZK_HIP(hipSetDevice(ctx->device));
  if (pk->round != 4) {
    ctx->err = "plonk: round 5 out of order";
    return ZKMI_ERR_ARG;
  }
  const size_t n = (size_t)1 << pk->log_n, Bp = pk->Bp, batch = pk->batch;
  int rc;
  RoundTmp t5(ctx);
  if ((rc = t5.alloc(batch * n_sc * 32))) return rc;
  void* tmp = t5.p;
  ZK_HIP(hipMemcpyAsync(tmp, scalars, batch * n_sc * 32, hipMemcpyDefault, ctx->stream));
  Fr* sc = (Fr*)pk->small[0].p;
  rc = transpose_in(ctx, tmp, sc, n_sc, batch, Bp, 32);
  if (rc) return rc;
  const size_t L = n + 3;
  // numerators in big[2], quotients in big[3]: 2 (n + 8) rows each (log_n >= 4)
  Fr* N = (Fr*)pk->big[2].p;
  Fr* NZ = N + (n + 8) * Bp;
  Fr* W = (Fr*)pk->big[3].p;
  Fr* WZ = W + (n + 8) * Bp;
  const auto lin = pk->commits.empty() ? plonk_lin<false> : plonk_lin<true>;
  hipLaunchKernelGGL(lin, dim3((unsigned)(Bp / 64), (unsigned)(L < 4096 ? L : 4096)),
                     dim3(64), 0, ctx->stream, (const Fr*)pk->cf[0].p, (const Fr*)pk->cf[1].p,
                     (const Fr*)pk->cf[2].p, (const Fr*)pk->cf[3].p, (const Fr*)pk->big[1].p,
                     (const Fr*)pk->coef, (const Fr*)sc, N, NZ, n, Bp, pow2_image(266),
                     (uint32_t)pk->commits.size(), (const Fr*)pk->cm_pi2.p, (const Fr*)pk->qcp_coef);
  hipLaunchKernelGGL(plonk_zero_rows, dim3((unsigned)(Bp / 64), 8), dim3(64), 0, ctx->stream, W, L - 1,
                     n + 8, Bp);
  hipLaunchKernelGGL(plonk_zero_rows, dim3((unsigned)(Bp / 64), 8), dim3(64), 0, ctx->stream, WZ,
                     L - 1, n + 8, Bp);
  {
    // chunk values of N at zeta and of NZ at zeta w (rows 11, 12 of sc), suffix scan, local division
    const uint32_t n_chunks = (uint32_t)((L + CH - 1) / CH);
    Fr* part = (Fr*)pk->big[4].p;
    const Fr* pts = sc + 11 * Bp;
    EvalArgs ea{};
    ea.poly[0] = N;
    ea.poly[1] = NZ;
    ea.len[0] = ea.len[1] = (uint32_t)L;
    ea.point_row[0] = 0;
    ea.point_row[1] = 1;
    hipLaunchKernelGGL(plonk_chunk_horner, dim3((unsigned)(Bp / 64), n_chunks, 2), dim3(64), 0,
                       ctx->stream, ea, pts, part, n_chunks, Bp);
    hipLaunchKernelGGL(plonk_div_suffix, dim3((unsigned)(Bp / 64), 2), dim3(64), 0, ctx->stream, pts,
                       part, n_chunks, Bp);
    hipLaunchKernelGGL(plonk_div_local, dim3((unsigned)(Bp / 64), n_chunks, 2), dim3(64), 0,
                       ctx->stream, (const Fr*)N, (const Fr*)NZ, pts, (const Fr*)part, W, WZ,
                       (uint32_t)L, n_chunks, Bp);
  }
  ZK_HIP(hipGetLastError());
  const Fr* scs[2] = {W, WZ};
  if ((rc = commit(ctx, pk, 2, scs, nullptr, commits_w_out, batch))) return rc;
  pk->round = 0;
  return ZKMI_OK;
}

}  // extern "C"

// ---- plonk.Prove in one call: the five rounds with the Fiat-Shamir transcript on the host in C++ --------
// Transcript (the Python twin is plonk.py::challenge / lin_scalars): SHA-256(label ||
// parts) mod r, integers as 32 big-endian bytes, G1 points as x || y big-endian (infinity: 64 zero
// bytes).  gamma = H("gamma", vk digest, public inputs, [a], [b], [c]); beta = H("beta", gamma);
// alpha = H("alpha", beta, [z]); zeta = H("zeta", alpha, [t_lo], [t_mid], [t_hi]);
// v = H("v", zeta, six evaluations).
namespace {
void fr_be(uint8_t out[32], const Fr& plain) {
  for (int i = 0; i < 8; i++) {
    const uint32_t x = plain.v[7 - i];
    out[4 * i] = (uint8_t)(x >> 24);
    out[4 * i + 1] = (uint8_t)(x >> 16);
    out[4 * i + 2] = (uint8_t)(x >> 8);
    out[4 * i + 3] = (uint8_t)x;
  }
}
struct Transcript {
  Sha256 h;
  explicit Transcript(const char* label) { h.update((const uint8_t*)label, strlen(label)); }
  void fr_mont(const Fr& m) {   // a field element given in Montgomery form
    uint8_t b[32];
    fr_be(b, from_mont(m));
    h.update(b, 32);
  }
  void point(const G1Affine& p) {
    uint8_t b[64] = {0};
    if (!(p.x.is_zero() && p.y.is_zero())) {
      const Fq x = from_mont(p.x), y = from_mont(p.y);
      for (int i = 0; i < 8; i++)
        for (int k = 0; k < 4; k++) {
          b[4 * i + k] = (uint8_t)(x.v[7 - i] >> (24 - 8 * k));
          b[32 + 4 * i + k] = (uint8_t)(y.v[7 - i] >> (24 - 8 * k));
        }
    }
    h.update(b, 64);
  }
  Fr challenge() {   // digest as a big-endian integer, reduced mod r, in Montgomery form
    uint8_t d[32];
    h.final(d);
    Fr x = Fr::zero();
    for (int i = 0; i < 32; i++) x.v[7 - i / 4] |= (uint32_t)d[i] << (24 - 8 * (i % 4));
    for (;;) {
      bool ge = true;
      for (int j = 7; j >= 0; j--)
        if (x.v[j] != FrParams::p(j)) {
          ge = x.v[j] > FrParams::p(j);
          break;
        }
      if (!ge) break;
      int64_t br = 0;
      for (int j = 0; j < 8; j++) {
        const int64_t t = (int64_t)x.v[j] - (int64_t)FrParams::p(j) + br;
        x.v[j] = (uint32_t)t;
        br = t >> 32;
      }
    }
    return to_mont(x);
  }
};
Fr fr_pow_u64(Fr base, uint64_t e) {
  Fr r = Fr::one();
  while (e) {
    if (e & 1) r = mul(r, base);
    base = sqr(base);
    e >>= 1;
  }
  return r;
}
Fr fr_u64(uint64_t v) {
  Fr x = Fr::zero();
  x.v[0] = (uint32_t)v;
  x.v[1] = (uint32_t)(v >> 32);
  return to_mont(x);
}
}  // namespace

extern "C" {

// Rounds 2 .. 5 with the transcript between them, after either round 1: pubs = batch x n_public public
// inputs (gnark's image, host), abc = the commitments of round 1; assembles the records
// For a key with n_c commitments (pk->cm_pts, pk->cm_H: what round 1 left): [pi2_i] enter alpha, the
// Qcp_i(zeta) enter v after the six evaluations, PI(zeta) gains H_i L_(r_i)(zeta), the scalars of
// round 5 gain the Qcp_i(zeta), and commit_out takes batch x n_c x 96 bytes.
static int prove_after_round1(zkmi_ctx* ctx, zkmi_plonk_pk* pk, size_t batch, const std::vector<Fr>& pubs,
                              const std::vector<G1Affine>& abc, const uint8_t* vk_digest,
                              void* proofs_out, void* commit_out = nullptr) {
  const size_t n = (size_t)1 << pk->log_n, n_pub = pk->n_public, n_c = pk->commits.size();
  const size_t n_sc = 14 + n_c;
  std::vector<G1Affine> cz(batch), ct(batch * 3), cw(batch * 2);
  std::vector<Fr> bg(batch * 2), al(batch), zz(batch * 2), ev(batch * 6), sc(batch * n_sc),
      eq(batch * n_c);
  int rc;
  for (size_t p = 0; p < batch; p++) {
    Transcript t("gamma");
    t.h.update(vk_digest, 32);
    for (size_t j = 0; j < n_pub; j++) t.fr_mont(pubs[p * n_pub + j]);
    for (int k = 0; k < 3; k++) t.point(abc[p * 3 + k]);
    const Fr gamma = t.challenge();
    Transcript tb("beta");
    tb.fr_mont(gamma);
    bg[2 * p] = tb.challenge();
    bg[2 * p + 1] = gamma;
  }
  if ((rc = zkmi_plonk_round2(ctx, pk, bg.data(), cz.data()))) return rc;
  for (size_t p = 0; p < batch; p++) {
    Transcript t("alpha");
    t.fr_mont(bg[2 * p]);
    for (size_t i = 0; i < n_c; i++) t.point(pk->cm_pts[p * n_c + i]);
    t.point(cz[p]);
    al[p] = t.challenge();
  }
  if ((rc = zkmi_plonk_round3(ctx, pk, al.data(), ct.data()))) return rc;
  // w = 5^((r - 1) / n): root of unity of the domain, from the key's omega table
  Fr w;
  if (hipMemcpy(&w, pk->omega + 1, 32, hipMemcpyDefault) != hipSuccess) return ZKMI_ERR_HIP;
  for (size_t p = 0; p < batch; p++) {
    Transcript t("zeta");
    t.fr_mont(al[p]);
    for (int k = 0; k < 3; k++) t.point(ct[p * 3 + k]);
    zz[2 * p] = t.challenge();
    zz[2 * p + 1] = mul(zz[2 * p], w);
  }
  if ((rc = round4_run(ctx, pk, zz.data(), ev.data(), n_c ? eq.data() : nullptr))) return rc;
  const Fr ninv = inverse(fr_u64(n)), five = fr_u64(5), tf = fr_u64(25);
  // 1 / (zeta - w^j), j = 0 .. max(n_pub, 1) - 1 (j = 0 also serves L_1), for every proof: one
  // inversion in all (Montgomery's trick); zeta = w^j has probability 2^-250
  const size_t nd = n_pub ? n_pub : 1;
  std::vector<Fr> den(batch * nd), pre(batch * nd);
  {
    Fr acc = Fr::one();
    for (size_t p = 0; p < batch; p++) {
      Fr wj = Fr::one();
      for (size_t j = 0; j < nd; j++) {
        den[p * nd + j] = sub(zz[2 * p], wj);
        pre[p * nd + j] = acc;
        if (!den[p * nd + j].is_zero()) acc = mul(acc, den[p * nd + j]);
        wj = mul(wj, w);
      }
    }
    Fr inv = inverse(acc);
    for (size_t i = batch * nd; i-- > 0;) {
      if (den[i].is_zero()) continue;
      const Fr t = mul(inv, pre[i]);
      inv = mul(inv, den[i]);
      den[i] = t;
    }
  }
  for (size_t p = 0; p < batch; p++) {
    const Fr beta = bg[2 * p], gamma = bg[2 * p + 1], alpha = al[p], zeta = zz[2 * p];
    const Fr* e = ev.data() + 6 * p;   // a, b, c, s1, s2, z(zeta w)
    Transcript t("v");
    t.fr_mont(zeta);
    for (int k = 0; k < 6; k++) t.fr_mont(e[k]);
    for (size_t i = 0; i < n_c; i++) t.fr_mont(eq[p * n_c + i]);
    const Fr v = t.challenge();
    // scalars of the linearisation polynomial (plonk.py::lin_scalars)
    const Fr zh = sub(fr_pow_u64(zeta, n), Fr::one());
    const Fr l1 = mul(mul(zh, ninv), den[p * nd]);
    Fr pi = Fr::zero(), wj = Fr::one();
    for (size_t j = 0; j < n_pub; j++) {   // PI(zeta) = sum_j -x_j L_j(zeta)
      const Fr lj = mul(mul(mul(zh, wj), ninv), den[p * nd + j]);
      pi = sub(pi, mul(pubs[p * n_pub + j], lj));
      wj = mul(wj, w);
    }
    for (size_t i = 0; i < n_c; i++) {   // + H_i L_(r_i)(zeta)
      const Fr wr = fr_pow_u64(w, pk->commits[i].row);
      const Fr lr = mul(mul(mul(zh, wr), ninv), inverse(sub(zeta, wr)));
      pi = add(pi, mul(pk->cm_H[p * n_c + i], lr));
    }
    const Fr bz = mul(beta, zeta);
    const Fr a1 = mul(mul(add(add(e[0], bz), gamma), add(add(e[1], mul(five, bz)), gamma)),
                      add(add(e[2], mul(tf, bz)), gamma));
    const Fr a2 = mul(add(add(e[0], mul(beta, e[3])), gamma), add(add(e[1], mul(beta, e[4])), gamma));
    const Fr zn2 = fr_pow_u64(zeta, n + 2), al2 = mul(alpha, alpha);
    Fr* s = sc.data() + n_sc * p;
    s[0] = mul(e[0], e[1]);                                        // qm
    s[1] = e[0];                                                   // ql
    s[2] = e[1];                                                   // qr
    s[3] = e[2];                                                   // qo
    s[4] = neg(mul(mul(mul(alpha, a2), beta), e[5]));              // s3
    s[5] = add(mul(alpha, a1), mul(al2, l1));                      // z
    s[6] = neg(zh);                                                // t_lo
    s[7] = neg(mul(zh, zn2));                                      // t_mid
    s[8] = neg(mul(mul(zh, zn2), zn2));                            // t_hi
    Fr c0 = sub(sub(pi, mul(al2, l1)), mul(mul(mul(alpha, a2), add(e[2], gamma)), e[5]));   // r0
    Fr vp = Fr::one();
    for (int k = 0; k < 5; k++) {
      vp = mul(vp, v);
      c0 = sub(c0, mul(vp, e[k]));
    }
    for (size_t i = 0; i < n_c; i++) {   // v^(6+i) Qcp_i(zeta)
      vp = mul(vp, v);
      c0 = sub(c0, mul(vp, eq[p * n_c + i]));
      s[14 + i] = eq[p * n_c + i];
    }
    s[9] = c0;
    s[10] = v;
    s[11] = zeta;
    s[12] = zz[2 * p + 1];
    s[13] = e[5];
  }
  if ((rc = round5_run(ctx, pk, sc.data(), n_sc, cw.data()))) return rc;
  // assemble the records on the host, one copy out (host or device destination)
  std::vector<uint8_t> rec(batch * 768);
  for (size_t p = 0; p < batch; p++) {
    uint8_t* r = rec.data() + p * 768;
    memcpy(r, &abc[p * 3], 192);
    memcpy(r + 192, &cz[p], 64);
    memcpy(r + 256, &ct[p * 3], 192);
    memcpy(r + 448, &cw[p * 2], 128);
    memcpy(r + 576, &ev[p * 6], 192);
  }
  ZK_HIP(hipMemcpy(proofs_out, rec.data(), rec.size(), hipMemcpyDefault));
  if (n_c) {
    std::vector<uint8_t> cm(batch * n_c * 96);
    for (size_t k = 0; k < batch * n_c; k++) {
      memcpy(cm.data() + k * 96, &pk->cm_pts[k], 64);
      memcpy(cm.data() + k * 96 + 64, &eq[k], 32);
    }
    ZK_HIP(hipMemcpy(commit_out, cm.data(), cm.size(), hipMemcpyDefault));
  }
  return ZKMI_OK;
}

/* proofs_out: batch x 96 words of 8 bytes = 9 G1 affine points ([a] [b] [c] [z] [t_lo] [t_mid] [t_hi]
 * [W_zeta] [W_zeta_w], Montgomery) then 6 fr (a, b, c, S1, S2 at zeta, z at zeta w; Montgomery). */
// the extras of a key with commitments are both given, those of a key without both null
static int commit_args_check(zkmi_ctx* ctx, const zkmi_plonk_pk* pk, const void* blind_commit,
                             const void* commit_out) {
  const bool has = !pk->commits.empty();
  if (has ? (!blind_commit || !commit_out) : (blind_commit || commit_out)) {
    ctx->err = has ? "plonk: a key with commitments needs blind_commit and commit_out"
                   : "plonk: blind_commit / commit_out given for a key without commitments";
    return ZKMI_ERR_ARG;
  }
  return ZKMI_OK;
}
int zkmi_plonk_prove(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const zkmi_cs* cs, const void* inputs,
                     size_t batch, const void* blind, const uint8_t* vk_digest /* 32 bytes */,
                     void* proofs_out, int32_t* status_out) {
  if (ctx && pk && !pk->commits.empty()) {
    ctx->err = kNoCommitments;
    return ZKMI_ERR_ARG;
  }
  return zkmi_plonk_prove_ex(ctx, pk, cs, inputs, batch, blind, nullptr, vk_digest, proofs_out, nullptr,
                             status_out);
}
int zkmi_plonk_prove_ex(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const zkmi_cs* cs, const void* inputs,
                        size_t batch, const void* blind, const void* blind_commit,
                        const uint8_t* vk_digest, void* proofs_out, void* commit_out,
                        int32_t* status_out) {
  if (!ctx || !pk || !cs || !inputs || !blind || !vk_digest || !proofs_out || !status_out || batch == 0)
    return ZKMI_ERR_ARG;
  if (int bad = commit_args_check(ctx, pk, blind_commit, commit_out)) return bad;
  const size_t n_pub = pk->n_public;
  const size_t n_in = cs->n_public - 1 + cs->n_secret;
  // public inputs on the host (gnark's image)
  std::vector<Fr> pubs(batch * (n_pub ? n_pub : 1));
  for (size_t p = 0; p < batch && n_pub; p++)
    if (hipMemcpy(pubs.data() + p * n_pub, (const char*)inputs + p * n_in * 32, n_pub * 32,
                  hipMemcpyDefault) != hipSuccess) {
      ctx->err = "plonk_prove: cannot read the public inputs";
      return ZKMI_ERR_HIP;
    }
  std::vector<G1Affine> abc(batch * 3);
  int rc = round1_solve(ctx, pk, cs, inputs, batch, blind, blind_commit, abc.data(), status_out);
  if (rc) return rc;
  return prove_after_round1(ctx, pk, batch, pubs, abc, vk_digest, proofs_out, commit_out);
}

// ---- the gnark drop-in entry: key from the trace form, round 1 from solved witnesses ----------------
// The seven arrays zkmi_plonk_pk_load takes as data, computed here in gnark's image: the powers and
// the sigma lookup by the kernels above; the eight polynomials (five selectors, three sigma columns)
// as eight lanes of one batch-inner matrix of 64: inverse transform on the domain, then the coset
// transform on 5 <w_4n> that round 3 runs for the wire polynomials, each transposed back out to the
// poly-major arrays the kernels read wave-uniformly.
static int pk_from_trace(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const zkmi_plonk_trace_desc* d) {
  const size_t n = (size_t)1 << pk->log_n, m = 4 * n, Bp = 64;
  if (!d->selectors || !d->perm) {
    ctx->err = "plonk trace: selectors and perm must not be null";
    return ZKMI_ERR_ARG;
  }
  pk->perm.resize(3 * n);
  ZK_HIP(hipMemcpy(pk->perm.data(), d->perm, 3 * n * 4, hipMemcpyDefault));
  const std::string bad = scs_perm_validate(pk->perm.data(), n);
  if (!bad.empty()) {
    ctx->err = bad;
    return ZKMI_ERR_ARG;
  }
  int rc;
  NttPlan *plan_n, *plan_m;
  if ((rc = get_plan(ctx, (int)pk->log_n, &plan_n)) ||
      (rc = get_plan(ctx, (int)pk->log_n + 2, &plan_m)))
    return rc;
  struct { Fr** dst; size_t count; } arr[7] = {{&pk->coef, 8 * n}, {&pk->coset, 8 * m},
                                               {&pk->sigma, 3 * n}, {&pk->omega, n},
                                               {&pk->coset_x, m},   {&pk->l1, m},
                                               {&pk->zh_inv, 4}};
  for (auto& a : arr)
    if (hipMalloc((void**)a.dst, a.count * 32) != hipSuccess) {
      (void)hipGetLastError();
      ctx->err = "plonk trace: hipMalloc(" + std::to_string(a.count * 32) + " B) failed";
      return ZKMI_ERR_OOM;
    }
  // temporaries: the permutation, the eight Lagrange columns poly-major, and the two matrices the
  // transforms alternate between (n rows; 4n rows, which first holds the n rows going in)
  RoundTmp perm_dev(ctx), lag(ctx), mat_n(ctx), mat_m(ctx);
  if ((rc = perm_dev.alloc(3 * n * 4)) || (rc = lag.alloc(8 * n * 32)) ||
      (rc = mat_n.alloc(n * Bp * 32)) || (rc = mat_m.alloc(m * Bp * 32)))
    return rc;
  // generators of the two domains, from the plans' twiddle tables (w^i, i < n / 2; n >= 16)
  Fr w, w4;
  ZK_HIP(hipMemcpy(&w, plan_n->tw_fwd + 1, 32, hipMemcpyDeviceToHost));
  ZK_HIP(hipMemcpy(&w4, plan_m->tw_fwd + 1, 32, hipMemcpyDeviceToHost));
  const auto grid = [](size_t count) { return dim3((unsigned)((count + 255) / 256)); };
  hipLaunchKernelGGL(plonk_powers_kernel, grid(n), dim3(256), 0, ctx->stream, pk->omega, n, w,
                     Fr::one());
  hipLaunchKernelGGL(plonk_powers_kernel, grid(m), dim3(256), 0, ctx->stream, pk->coset_x, m, w4,
                     fr_small(5));
  ZK_HIP(hipMemcpyAsync(perm_dev.p, pk->perm.data(), 3 * n * 4, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(plonk_sigma_kernel, grid(3 * n), dim3(256), 0, ctx->stream,
                     (const uint32_t*)perm_dev.p, (const Fr*)pk->omega, pk->sigma, pk->log_n,
                     fr_small(5), fr_small(25));
  ZK_HIP(hipGetLastError());
  Fr* lg = (Fr*)lag.p;
  ZK_HIP(hipMemcpyAsync(lg, d->selectors, 5 * n * 32, hipMemcpyDefault, ctx->stream));
  ZK_HIP(hipMemcpyAsync(lg + 5 * n, pk->sigma, 3 * n * 32, hipMemcpyDeviceToDevice, ctx->stream));
  Fr *Mn = (Fr*)mat_n.p, *Mm = (Fr*)mat_m.p;
  if ((rc = transpose_in(ctx, lg, Mm, n, 8, Bp, 32)) ||
      (rc = ntt_bi(ctx, plan_n, Mm, Mn, Bp, true, false, n)) ||
      (rc = transpose_out(ctx, Mn, pk->coef, n, 8, Bp, 32)) ||
      (rc = ntt_bi(ctx, plan_m, Mn, Mm, Bp, false, true, n)) ||
      (rc = transpose_out(ctx, Mm, pk->coset, m, 8, Bp, 32)))
    return rc;
  // Z_H on the coset: x_j^n - 1 = 5^n i^j - 1 with i = w_4n^n, period 4; L_1 from it
  const Fr ninv = inverse(fr_u64(n)), i4 = fr_pow_u64(w4, n);
  Fr4 zh_n;
  Fr zh_inv[4], t = fr_pow_u64(fr_small(5), n);
  for (int k = 0; k < 4; k++) {
    const Fr zh = sub(t, Fr::one());
    zh_inv[k] = inverse(zh);
    zh_n.v[k] = mul(zh, ninv);
    t = mul(t, i4);
  }
  ZK_HIP(hipMemcpyAsync(pk->zh_inv, zh_inv, sizeof zh_inv, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(plonk_l1_kernel, grid(m), dim3(256), 0, ctx->stream, (const Fr*)pk->coset_x,
                     pk->l1, m, zh_n);
  ZK_HIP(hipGetLastError());
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  return ZKMI_OK;
}

int zkmi_plonk_pk_load_trace(zkmi_ctx* ctx, const zkmi_plonk_trace_desc* d, zkmi_plonk_pk** out) {
  ZK_HIP(hipSetDevice(ctx->device));
  if (!d || !out) return ZKMI_ERR_ARG;
  zkmi_plonk_pk* pk;
  int rc = pk_new(ctx, d->log_n, d->n_public, d->max_batch, &pk);
  if (rc) return rc;
  if ((rc = require_idle(ctx)) || (rc = pk_from_trace(ctx, pk, d)) ||
      (rc = pk_finish(ctx, pk, PkCommon{d->srs_g1, d->window_bits, d->lag_g1, d->lag_rows, d->lag_k}))) {
    zkmi_plonk_pk_free(ctx, pk);
    return rc;
  }
  *out = pk;
  return ZKMI_OK;
}

void zkmi_scs_free(zkmi_ctx* ctx, zkmi_scs* scs) {
  if (!scs) return;
  if (ctx) {
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
  }
  for (uint32_t* p : scs->x)
    if (p) hipFree(p);
  if (scs->marks) hipFree(scs->marks);
  if (scs->sel) hipFree(scs->sel);
  delete scs;
}

int zkmi_scs_load(zkmi_ctx* ctx, const zkmi_scs_desc* d, zkmi_scs** out) {
  ZK_HIP(hipSetDevice(ctx->device));
  if (!d || !out) return ZKMI_ERR_ARG;
  *out = nullptr;
  const ScsShape shape{d->n_wires, d->n_gates, d->n_public};
  // the counts and the pointers before anything is sized or read by them
  std::string bad = !d->xa || !d->xb || !d->xc || !d->selectors
                        ? std::string("scs: xa, xb, xc and selectors must not be null")
                        : scs_shape_check(shape);
  if (!bad.empty()) {
    ctx->err = bad;
    return ZKMI_ERR_ARG;
  }
  const size_t ng = d->n_gates;
  auto* s = new zkmi_scs();
  s->n_wires = d->n_wires;
  s->n_gates = d->n_gates;
  s->n_public = d->n_public;
  const uint32_t* src[3] = {d->xa, d->xb, d->xc};
  std::vector<Fr> sel(5 * ng);
  std::vector<uint32_t> marks(ng);
  bool ok = hipMemcpy(sel.data(), d->selectors, 5 * ng * 32, hipMemcpyDefault) == hipSuccess;
  for (int c = 0; ok && c < 3; c++) {
    s->hx[c].resize(ng);
    ok = hipMemcpy(s->hx[c].data(), src[c], ng * 4, hipMemcpyDefault) == hipSuccess;
  }
  if (!ok) {
    (void)hipGetLastError();
    ctx->err = "scs: cannot read the system";
    zkmi_scs_free(ctx, s);
    return ZKMI_ERR_HIP;
  }
  // every wire index is range-checked here, before a kernel can use it as an address
  bad = scs_validate(shape, s->hx[0].data(), s->hx[1].data(), s->hx[2].data(), sel.data(),
                     marks.data());
  if (!bad.empty()) {
    ctx->err = bad;
    zkmi_scs_free(ctx, s);
    return ZKMI_ERR_ARG;
  }
  for (size_t i = 0; i < 4 * ng; i++) sel[i] = lift(sel[i], 5);   // qL qR qO qM: 2^261 images
  for (int c = 0; ok && c < 3; c++)
    ok = hipMalloc((void**)&s->x[c], ng * 4) == hipSuccess &&
         hipMemcpy(s->x[c], s->hx[c].data(), ng * 4, hipMemcpyHostToDevice) == hipSuccess;
  ok = ok && hipMalloc((void**)&s->marks, ng * 4) == hipSuccess &&
       hipMemcpy(s->marks, marks.data(), ng * 4, hipMemcpyHostToDevice) == hipSuccess &&
       hipMalloc((void**)&s->sel, 5 * ng * 32) == hipSuccess &&
       hipMemcpy(s->sel, sel.data(), 5 * ng * 32, hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    ctx->err = "scs: device upload failed";
    zkmi_scs_free(ctx, s);
    return ZKMI_ERR_HIP;
  }
  *out = s;
  return ZKMI_OK;
}

// solver != NULL (zkmi_plonk_round1_scs / zkmi_plonk_prove_scs): scs is the solver's system and the
// wires are solved on the device from `wires`, which then holds the batch's inputs
static int round1_witness(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const zkmi_scs* scs, const void* wires,
                          const void* a, const void* b, const void* c, size_t n_gates, size_t batch,
                          const void* blind, const void* blind_commit, void* commits_out,
                          int32_t* status_out, const zkmi_scs_solver* solver = nullptr);
int zkmi_plonk_round1_witness(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const zkmi_scs* scs,
                              const void* wires, const void* a, const void* b, const void* c,
                              size_t n_gates, size_t batch, const void* blind, void* commits_out,
                              int32_t* status_out) {
  if (pk && !pk->commits.empty()) {
    ctx->err = kNoCommitments;
    return ZKMI_ERR_ARG;
  }
  return round1_witness(ctx, pk, scs, wires, a, b, c, n_gates, batch, blind, nullptr, commits_out,
                        status_out);
}
static int round1_witness(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const zkmi_scs* scs, const void* wires,
                          const void* a, const void* b, const void* c, size_t n_gates, size_t batch,
                          const void* blind, const void* blind_commit, void* commits_out,
                          int32_t* status_out, const zkmi_scs_solver* solver) {
  ZK_HIP(hipSetDevice(ctx->device));
  int rc;
  if ((rc = require_idle(ctx))) return rc;
  if (!pk || !blind || !commits_out || !status_out) {
    ctx->err = "plonk witness: null argument";
    return ZKMI_ERR_ARG;
  }
  if (batch == 0 || batch > pk->max_batch) {
    ctx->err = "plonk: batch must be in [1, max_batch]";
    return ZKMI_ERR_ARG;
  }
  const bool wire_form = scs && (wires || (solver && !scs_solver_inputs(solver))) && !a && !b && !c;
  const bool column_form = !scs && !wires && a && b && c;
  if (!wire_form && !column_form) {
    ctx->err = "plonk witness: give either a system and its wires (a = b = c = NULL) or the three "
               "columns a, b, c (scs = wires = NULL)";
    return ZKMI_ERR_ARG;
  }
  const size_t n = (size_t)1 << pk->log_n, m = 4 * n, n_pub = pk->n_public;
  if (scs) {
    if (n_gates && n_gates != scs->n_gates) {
      ctx->err = "plonk witness: n_gates differs from the loaded system's";
      return ZKMI_ERR_ARG;
    }
    n_gates = scs->n_gates;
  }
  if (n_gates == 0 || n_gates > n) {
    ctx->err = "plonk witness: n_gates must be in [1, 2^log_n], the key's domain";
    return ZKMI_ERR_ARG;
  }
  if (scs ? scs->n_public != n_pub : n_gates < n_pub) {
    ctx->err = scs ? "plonk witness: the system has " + std::to_string(scs->n_public) +
                         " public inputs, the key " + std::to_string(n_pub)
                   : std::string("plonk witness: fewer gate rows than the key has public inputs");
    return ZKMI_ERR_ARG;
  }
  if (scs && scs->n_wires > m) {
    ctx->err = "plonk witness: wire vector larger than the 4n work buffer";
    return ZKMI_ERR_ARG;
  }
  if (solver && scs_solver_inputs(solver) > m) {
    ctx->err = "plonk solver: more inputs than the 4n work buffer holds";
    return ZKMI_ERR_ARG;
  }
  // first prove of this (trace-loaded key, system) pair: the wiring against the key's permutation
  if (scs && !pk->perm.empty() && scs->checked_key != pk->serial) {
    const std::string bad =
        scs_wiring_check(ScsShape{scs->n_wires, scs->n_gates, scs->n_public}, scs->hx[0].data(),
                         scs->hx[1].data(), scs->hx[2].data(), pk->perm.data(), n);
    if (!bad.empty()) {
      ctx->err = bad;
      return ZKMI_ERR_ARG;
    }
    scs->checked_key = pk->serial;
  }
  const size_t n_c = pk->commits.size();
  // a solver behind a key with commitments (zkmi_plonk_prove_scs_ex): its commitment hints are the
  // key's commitments, one by one
  if (solver && (n_c || scs_solver_commits(solver))) {
    if (scs_solver_commits(solver) != n_c) {
      ctx->err = "plonk solver: the key carries " + std::to_string(n_c) + " commitments, the solver's plan holds " +
                 std::to_string(scs_solver_commits(solver)) + " commitment hints";
      return ZKMI_ERR_ARG;
    }
    for (size_t i = 0; i < n_c; i++) {
      const ScsSolverCommit h = scs_solver_commit(solver, i);
      const zkmi_plonk_pk::Commit& c = pk->commits[i];
      bool same = h.n_wires == c.n_rows && c.row < scs->n_gates && h.wire == scs->hx[0][c.row];
      for (uint32_t j = 0; same && j < c.n_rows; j++)
        same = c.rows[j] < scs->n_gates && h.wires[j] == scs->hx[0][c.rows[j]];
      if (!same) {
        ctx->err = "plonk solver: commitment hint " + std::to_string(i) + " of the plan is not commitment " +
                   std::to_string(i) + " of the key: its committed wires must be xa[rows[j]] in order and its "
                   "output xa[row]";
        return ZKMI_ERR_ARG;
      }
    }
  }
  if ((rc = round1_begin(ctx, pk, batch))) return rc;
  const size_t Bp = pk->Bp;
  if (n_c && (rc = commit_begin(ctx, pk, blind_commit, batch, Bp))) return rc;
  RoundTmp tbl(ctx);
  if ((rc = tbl.alloc(batch * 9 * 32))) return rc;
  ZK_HIP(hipMemcpyAsync(tbl.p, blind, batch * 9 * 32, hipMemcpyDefault, ctx->stream));
  void* st;
  if ((rc = ensure_scratch(ctx, ctx->sets[0].misc, Bp * 4, &st))) return rc;
  ZK_HIP(hipMemsetAsync(st, 0, Bp * 4, ctx->stream));
  Fr *W = (Fr*)pk->big[0].p, *A = (Fr*)pk->big[1].p, *B = (Fr*)pk->big[2].p, *C = (Fr*)pk->big[3].p;
  Fr* pub = (Fr*)pk->big[5].p;   // rows 0 .. n_pub - 1: the public inputs, for PI(X) in round 3
  rc = transpose_in(ctx, tbl.p, pk->small[0].p, 9, batch, Bp, 32);
  if (!rc && scs) {
    // the solver stages its inputs through A, which the gather below overwrites
    if (solver && n_c) {
      // per commitment: the steps up to its boundary, the commitment step on the committed wires
      // straight from the wire matrix (gnark's image), H_i into the commitment wire's row
      rc = scs_solver_stage(ctx, solver, wires, batch, Bp, A, W);
      uint32_t at = 0;
      for (size_t i = 0; !rc && i < n_c; i++) {
        const ScsSolverCommit h = scs_solver_commit(solver, i);
        rc = scs_solver_run_steps(ctx, solver, W, (int32_t*)st, Bp, at, h.step);
        at = h.step;
        if (!rc) rc = commit_from_rows(ctx, pk, (uint32_t)i, W, h.wires_dev, false, Bp, batch);
        if (!rc && hipMemcpyAsync(W + (size_t)h.wire * Bp, (const Fr*)pk->cm_h.p + i * Bp, Bp * sizeof(Fr),
                                  hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)
          rc = ZKMI_ERR_HIP;
      }
      if (!rc) rc = scs_solver_run_steps(ctx, solver, W, (int32_t*)st, Bp, at, scs_solver_steps(solver));
    } else {
      rc = solver ? scs_solver_run(ctx, solver, wires, batch, Bp, A, W, (int32_t*)st)
                  : stage_rows(ctx, wires, scs->n_wires, batch, Bp, W);
    }
    if (!rc) {
      const ScsDev dev{{scs->x[0], scs->x[1], scs->x[2]}, scs->marks, scs->sel, scs->n_gates,
                       scs->n_public, pk->cm_skip};
      hipLaunchKernelGGL(n_c ? scs_gate_kernel<true> : scs_gate_kernel<false>,
                         dim3((unsigned)(Bp / 64), (unsigned)std::min<size_t>((n_gates + 3) / 4, 32768)),
                         dim3(256), 0, ctx->stream, dev, (const Fr*)W, A, B, C, pub, (int32_t*)st, Bp);
      if (hipGetLastError() != hipSuccess) rc = ZKMI_ERR_HIP;
    }
  } else if (!rc) {
    rc = stage_rows(ctx, a, n_gates, batch, Bp, A);
    if (!rc) rc = stage_rows(ctx, b, n_gates, batch, Bp, B);
    if (!rc) rc = stage_rows(ctx, c, n_gates, batch, Bp, C);
    if (!rc && n_pub &&
        hipMemcpyAsync(pub, A, n_pub * Bp * 32, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)
      rc = ZKMI_ERR_HIP;
  }
  // commitments: the step for every i from column a (rows >= n_gates of the domain read as zero, as
  // round 2 reads them), then a[r_i] against H_i
  if (!rc && n_c) {
    if (n_gates < n)
      hipLaunchKernelGGL(plonk_zero_rows, dim3((unsigned)(Bp / 64), 64), dim3(64), 0, ctx->stream, A,
                         n_gates, n, Bp);
    // (behind the solver the step has run already, on the same values: cm_pts / cm_H / cm_h hold it)
    for (size_t i = 0; !rc && !solver && i < n_c; i++)
      rc = commit_from_rows(ctx, pk, (uint32_t)i, A, pk->commits[i].rows_dev, false, Bp, batch);
    if (!rc) {
      hipLaunchKernelGGL(plonk_commit_check, dim3((unsigned)(Bp / 64)), dim3(64), 0, ctx->stream,
                         (const Fr*)A, (const Fr*)pk->cm_h.p, commit_rows_of(pk), (uint32_t)n_c,
                         (int32_t*)st, Bp);
      if (hipGetLastError() != hipSuccess) rc = ZKMI_ERR_HIP;
    }
  }
  // the caller's arrays have been consumed once the stream has passed the copies
  if (hipStreamSynchronize(ctx->stream) != hipSuccess && !rc) rc = ZKMI_ERR_HIP;
  if (rc) {
    if (rc == ZKMI_ERR_HIP && ctx->err.empty()) ctx->err = "plonk witness: HIP error while staging";
    return rc;
  }
  ZK_HIP(hipMemcpy(status_out, st, batch * 4, hipMemcpyDefault));
  return round1_tail(ctx, pk, n_gates, commits_out);
}

int zkmi_plonk_prove_witness(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const zkmi_scs* scs,
                             const void* wires, const void* a, const void* b, const void* c,
                             size_t n_gates, size_t batch, const void* blind,
                             const uint8_t* vk_digest, void* proofs_out, int32_t* status_out) {
  if (ctx && pk && !pk->commits.empty()) {
    ctx->err = kNoCommitments;
    return ZKMI_ERR_ARG;
  }
  return zkmi_plonk_prove_witness_ex(ctx, pk, scs, wires, a, b, c, n_gates, batch, blind, nullptr,
                                     vk_digest, proofs_out, nullptr, status_out);
}
static int prove_after_round1_witness(zkmi_ctx* ctx, zkmi_plonk_pk* pk, size_t batch,
                                      const std::vector<G1Affine>& abc, const uint8_t* vk_digest,
                                      void* proofs_out, void* commit_out);
int zkmi_plonk_prove_witness_ex(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const zkmi_scs* scs,
                                const void* wires, const void* a, const void* b, const void* c,
                                size_t n_gates, size_t batch, const void* blind,
                                const void* blind_commit, const uint8_t* vk_digest, void* proofs_out,
                                void* commit_out, int32_t* status_out) {
  if (!ctx) return ZKMI_ERR_ARG;
  if (!pk || !blind || !vk_digest || !proofs_out || !status_out || batch == 0) {
    ctx->err = "plonk_prove_witness: null argument or empty batch";
    return ZKMI_ERR_ARG;
  }
  if (int bad = commit_args_check(ctx, pk, blind_commit, commit_out)) return bad;
  std::vector<G1Affine> abc(batch * 3);
  int rc = round1_witness(ctx, pk, scs, wires, a, b, c, n_gates, batch, blind, blind_commit, abc.data(),
                          status_out);
  if (rc) return rc;
  return prove_after_round1_witness(ctx, pk, batch, abc, vk_digest, proofs_out, commit_out);
}
// rounds 2 .. 5 behind round1_witness
static int prove_after_round1_witness(zkmi_ctx* ctx, zkmi_plonk_pk* pk, size_t batch,
                                      const std::vector<G1Affine>& abc, const uint8_t* vk_digest,
                                      void* proofs_out, void* commit_out) {
  int rc;
  // public inputs: column a of rows 0 .. n_public - 1, which round 1 left in big[5]
  const size_t n_pub = pk->n_public;
  std::vector<Fr> pubs(batch * (n_pub ? n_pub : 1));
  if (n_pub) {
    RoundTmp t(ctx);
    if ((rc = t.alloc(batch * n_pub * 32)) ||
        (rc = transpose_out(ctx, pk->big[5].p, t.p, n_pub, batch, pk->Bp, 32)))
      return rc;
    ZK_HIP(hipMemcpyAsync(pubs.data(), t.p, batch * n_pub * 32, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
  }
  return prove_after_round1(ctx, pk, batch, pubs, abc, vk_digest, proofs_out, commit_out);
}

// ---- the gnark-shaped solve (scs_solve.hip) in front of the wire-form path ----------------------------
static const char* const kNoCommitmentsScs =
    "plonk: this key carries commitments: the solver entries (zkmi_plonk_round1_scs / "
    "zkmi_plonk_prove_scs) do not carry them; solve with gnark and use zkmi_plonk_prove_witness_ex";
static const char* const kCommitHintsScs =
    "scs solver: the plan holds commitment hints: their values need a proving key; use "
    "zkmi_plonk_prove_scs_ex with the key that carries the commitments";
int zkmi_scs_solve_batch(zkmi_ctx* ctx, const zkmi_scs_solver* solver, const void* inputs, size_t batch,
                         void* wires_out, int32_t* status_out) {
  if (!ctx) return ZKMI_ERR_ARG;
  ZK_HIP(hipSetDevice(ctx->device));
  int rc;
  if ((rc = require_idle(ctx))) return rc;
  if (batch == 0) return ZKMI_OK;
  if (!solver || !status_out || (scs_solver_inputs(solver) && !inputs)) {
    ctx->err = "scs_solve_batch: null argument";
    return ZKMI_ERR_ARG;
  }
  if (scs_solver_commits(solver)) {
    ctx->err = kCommitHintsScs;
    return ZKMI_ERR_ARG;
  }
  const zkmi_scs* scs = scs_solver_system(solver);
  const size_t Bp = round_up(batch, 64), n_in = scs_solver_inputs(solver);
  Staged sw(ctx), sst(ctx);
  if (wires_out && (rc = sw.out(wires_out, batch * (size_t)scs->n_wires * 32))) return rc;
  if ((rc = sst.out(status_out, batch * 4))) return rc;
  void *w, *staged, *st;
  zkmi_ctx::ProveSet& S = ctx->sets[0];
  if ((rc = ensure_scratch(ctx, S.slots, (size_t)scs->n_wires * Bp * 32, &w)) ||
      (rc = ensure_scratch(ctx, S.a, std::max<size_t>(n_in, 1) * Bp * 32, &staged)) ||
      (rc = ensure_scratch(ctx, S.misc, Bp * 4, &st)))
    return rc;
  ZK_HIP(hipMemsetAsync(st, 0, Bp * 4, ctx->stream));
  if ((rc = scs_solver_run(ctx, solver, inputs, batch, Bp, (Fr*)staged, (Fr*)w, (int32_t*)st))) return rc;
  const ScsDev dev{{scs->x[0], scs->x[1], scs->x[2]}, scs->marks, scs->sel, scs->n_gates, scs->n_public, nullptr};
  hipLaunchKernelGGL(scs_gate_check_kernel,
                     dim3((unsigned)(Bp / 64), (unsigned)std::min<size_t>((scs->n_gates + 3) / 4, 32768)),
                     dim3(256), 0, ctx->stream, dev, (const Fr*)w, (int32_t*)st, Bp);
  ZK_HIP(hipGetLastError());
  if (wires_out && (rc = transpose_out(ctx, w, sw.dev, scs->n_wires, batch, Bp, 32))) return rc;
  ZK_HIP(hipMemcpyAsync(sst.dev, st, batch * 4, hipMemcpyDeviceToDevice, ctx->stream));
  if ((rc = sw.finish()) || (rc = sst.finish())) return rc;
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  return ZKMI_OK;
}
int zkmi_plonk_round1_scs(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const zkmi_scs_solver* solver,
                          const void* inputs, size_t batch, const void* blind, void* commits_out,
                          int32_t* status_out) {
  if (!ctx) return ZKMI_ERR_ARG;
  if (!pk || !solver || (scs_solver_inputs(solver) && !inputs)) {
    ctx->err = "plonk solver: null argument";
    return ZKMI_ERR_ARG;
  }
  if (!pk->commits.empty()) {
    ctx->err = kNoCommitmentsScs;
    return ZKMI_ERR_ARG;
  }
  if (scs_solver_commits(solver)) {
    ctx->err = kCommitHintsScs;
    return ZKMI_ERR_ARG;
  }
  return round1_witness(ctx, pk, scs_solver_system(solver), inputs, nullptr, nullptr, nullptr, 0, batch, blind,
                        nullptr, commits_out, status_out, solver);
}
int zkmi_plonk_prove_scs(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const zkmi_scs_solver* solver,
                         const void* inputs, size_t batch, const void* blind, const uint8_t* vk_digest,
                         void* proofs_out, int32_t* status_out) {
  if (!ctx) return ZKMI_ERR_ARG;
  if (!pk || !solver || !blind || !vk_digest || !proofs_out || !status_out || batch == 0) {
    ctx->err = "plonk_prove_scs: null argument or empty batch";
    return ZKMI_ERR_ARG;
  }
  std::vector<G1Affine> abc(batch * 3);
  int rc = zkmi_plonk_round1_scs(ctx, pk, solver, inputs, batch, blind, abc.data(), status_out);
  if (rc) return rc;
  return prove_after_round1_witness(ctx, pk, batch, abc, vk_digest, proofs_out, nullptr);
}
int zkmi_plonk_prove_scs_ex(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const zkmi_scs_solver* solver,
                            const void* inputs, size_t batch, const void* blind, const void* blind_commit,
                            const uint8_t* vk_digest, void* proofs_out, void* commit_out,
                            int32_t* status_out) {
  if (!ctx) return ZKMI_ERR_ARG;
  if (!pk || !solver || !blind || !vk_digest || !proofs_out || !status_out || batch == 0 ||
      (scs_solver_inputs(solver) && !inputs)) {
    ctx->err = "plonk_prove_scs: null argument or empty batch";
    return ZKMI_ERR_ARG;
  }
  if (int bad = commit_args_check(ctx, pk, blind_commit, commit_out)) return bad;
  std::vector<G1Affine> abc(batch * 3);
  int rc = round1_witness(ctx, pk, scs_solver_system(solver), inputs, nullptr, nullptr, nullptr, 0, batch, blind,
                          blind_commit, abc.data(), status_out, solver);
  if (rc) return rc;
  return prove_after_round1_witness(ctx, pk, batch, abc, vk_digest, proofs_out, commit_out);
}

// ---- commitments of a key (api.Commit under PLONK; parity with gnark unpinned) ----------------------
// Qcp_i: indicator column of C_i -> coefficient form -> coset evaluations in the 2^261 image the other
// selectors have, by the prover's own transforms, the commitments being the lanes of one batch-inner
// matrix of 64 (as pk_from_trace computes the eight key polynomials).
int zkmi_plonk_pk_set_commitments(zkmi_ctx* ctx, zkmi_plonk_pk* pk,
                                  const zkmi_plonk_commit_desc* descs, uint32_t n_c) {
  if (!ctx) return ZKMI_ERR_ARG;
  if (!pk) {
    ctx->err = "plonk commitments: no key";
    return ZKMI_ERR_ARG;
  }
  ZK_HIP(hipSetDevice(ctx->device));
  int rc;
  if ((rc = require_idle(ctx))) return rc;
  const size_t n = (size_t)1 << pk->log_n, m = 4 * n, Bp = 64;
  // host copies of the rows, then every check before anything is built
  const uint32_t cnt = descs ? std::min<uint32_t>(n_c, PLONK_MAX_COMMITMENTS + 1) : 0;
  std::vector<std::vector<uint32_t>> rows(cnt);
  std::vector<PlonkCommitShape> shapes(cnt);
  for (uint32_t i = 0; i < cnt; i++) {
    const zkmi_plonk_commit_desc& d = descs[i];
    if (d.rows && d.n_rows && d.n_rows <= n) {
      rows[i].resize(d.n_rows);
      ZK_HIP(hipMemcpy(rows[i].data(), d.rows, (size_t)d.n_rows * 4, hipMemcpyDefault));
    }
    shapes[i] = PlonkCommitShape{d.n_rows, rows[i].empty() ? nullptr : rows[i].data(), d.row,
                                 d.lag_g1 != nullptr, d.lag_k};
    if (d.n_rows > n) shapes[i].rows = &d.row;   // refused by its count before a row is read
  }
  const std::string bad = plonk_commit_validate(
      shapes.data(), n_c > PLONK_MAX_COMMITMENTS ? n_c : cnt,
      PlonkCommitKeyState{n, !pk->commits.empty(), pk->proved});
  if (!bad.empty()) {
    ctx->err = bad;
    return ZKMI_ERR_ARG;
  }
  // built aside; the key takes them only when all of it has succeeded
  std::vector<zkmi_plonk_pk::Commit> cm(n_c);
  Fr *qcoef = nullptr, *qcoset = nullptr;
  uint8_t* skip = nullptr;
  auto undo = [&](int code) {
    hipStreamSynchronize(ctx->stream);
    for (auto& c : cm) {
      zkmi_msm_bases_free(ctx, c.lag);
      if (c.rows_dev) hipFree(c.rows_dev);
      if (c.slots_dev) hipFree(c.slots_dev);
    }
    for (void* p : {(void*)qcoef, (void*)qcoset, (void*)skip})
      if (p) hipFree(p);
    (void)hipGetLastError();
    if (code == ZKMI_ERR_HIP && ctx->err.empty()) ctx->err = "plonk commitments: HIP error while building";
    return code;
  };
  std::vector<Fr> ind((size_t)n_c * n, Fr::zero());
  std::vector<uint8_t> hskip(n, 0);
  for (uint32_t i = 0; i < n_c; i++) {
    const zkmi_plonk_commit_desc& d = descs[i];
    zkmi_plonk_pk::Commit& c = cm[i];
    c.n_rows = d.n_rows;
    c.row = d.row;
    c.rows = rows[i];
    std::vector<uint32_t> all(rows[i]);
    all.push_back(d.row);
    all.push_back((uint32_t)(n - 1));
    for (uint32_t r : rows[i]) {
      ind[(size_t)i * n + r] = Fr::one();
      hskip[r] = 1;
    }
    hskip[d.row] = 1;
    bool ok = hipMalloc((void**)&c.rows_dev, all.size() * 4) == hipSuccess &&
              hipMemcpy(c.rows_dev, all.data(), all.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
    if (ok && d.slots) {
      c.slots.resize(d.n_rows);
      ok = hipMemcpy(c.slots.data(), d.slots, (size_t)d.n_rows * 4, hipMemcpyDefault) == hipSuccess &&
           hipMalloc((void**)&c.slots_dev, (size_t)d.n_rows * 4) == hipSuccess &&
           hipMemcpy(c.slots_dev, c.slots.data(), (size_t)d.n_rows * 4, hipMemcpyHostToDevice) ==
               hipSuccess;
    }
    if (!ok) return undo(ZKMI_ERR_HIP);
    // 200 + k: subset-sum comb tables (zero digits are skipped: the scalars are mostly nibbles and bytes)
    const uint32_t k = d.lag_k ? d.lag_k : plonk_commit_auto_k(d.n_rows + 2);
    if ((rc = zkmi_msm_bases_load(ctx, 1, d.lag_g1, (size_t)d.n_rows + 2, 200 + (int)k, &c.lag)))
      return undo(rc);
  }
  NttPlan *plan_n, *plan_m;
  if ((rc = get_plan(ctx, (int)pk->log_n, &plan_n)) || (rc = get_plan(ctx, (int)pk->log_n + 2, &plan_m)))
    return undo(rc);
  {
    RoundTmp lag(ctx), mat_n(ctx), mat_m(ctx);
    if ((rc = lag.alloc((size_t)n_c * n * 32)) || (rc = mat_n.alloc(n * Bp * 32)) ||
        (rc = mat_m.alloc(m * Bp * 32)))
      return undo(rc);
    if (hipMalloc((void**)&qcoef, (size_t)n_c * n * 32) != hipSuccess ||
        hipMalloc((void**)&qcoset, (size_t)n_c * m * 32) != hipSuccess ||
        hipMalloc((void**)&skip, n) != hipSuccess ||
        hipMemcpy(skip, hskip.data(), n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(lag.p, ind.data(), (size_t)n_c * n * 32, hipMemcpyHostToDevice) != hipSuccess)
      return undo(ZKMI_ERR_HIP);
    Fr *Mn = (Fr*)mat_n.p, *Mm = (Fr*)mat_m.p;
    // lanes n_c .. 63 of the matrices carry nothing that is read back
    if (hipMemsetAsync(Mm, 0, n * Bp * 32, ctx->stream) != hipSuccess) return undo(ZKMI_ERR_HIP);
    if ((rc = transpose_in(ctx, lag.p, Mm, n, n_c, Bp, 32)) ||
        (rc = ntt_bi(ctx, plan_n, Mm, Mn, Bp, true, false, n)) ||
        (rc = transpose_out(ctx, Mn, qcoef, n, n_c, Bp, 32)) ||
        (rc = ntt_bi(ctx, plan_m, Mn, Mm, Bp, false, true, n)) ||
        (rc = transpose_out(ctx, Mm, qcoset, m, n_c, Bp, 32)))
      return undo(rc);
    hipLaunchKernelGGL(plonk_lift_kernel, dim3((unsigned)(((size_t)n_c * m + 255) / 256)), dim3(256), 0,
                       ctx->stream, qcoset, (size_t)n_c * m, 5);   // 2^261 image (plonk_qcp_fold)
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
      return undo(ZKMI_ERR_HIP);
  }
  pk->commits = std::move(cm);
  pk->qcp_coef = qcoef;
  pk->qcp_coset = qcoset;
  pk->cm_skip = skip;
  return ZKMI_OK;
}

int zkmi_plonk_commit_hint(zkmi_ctx* ctx, zkmi_plonk_pk* pk, uint32_t index, const void* values,
                           const void* blind2, size_t batch, void* commit_out, void* h_out) {
  if (!ctx) return ZKMI_ERR_ARG;
  if (!pk || !values || !blind2 || !commit_out || !h_out) {
    ctx->err = "plonk commit hint: null argument";
    return ZKMI_ERR_ARG;
  }
  ZK_HIP(hipSetDevice(ctx->device));
  int rc;
  if ((rc = require_idle(ctx))) return rc;
  if (index >= pk->commits.size()) {
    ctx->err = "plonk commit hint: the key has " + std::to_string(pk->commits.size()) +
               " commitments, index " + std::to_string(index);
    return ZKMI_ERR_ARG;
  }
  if (batch == 0 || batch > pk->max_batch) {
    ctx->err = "plonk: batch must be in [1, max_batch]";
    return ZKMI_ERR_ARG;
  }
  const size_t Bp = round_up(batch, 64);
  if ((rc = commit_buffers(ctx, pk, Bp))) return rc;
  const zkmi_plonk_pk::Commit& c = pk->commits[index];
  RoundTmp tv(ctx), tb(ctx);
  if ((rc = tv.alloc(batch * c.n_rows * 32)) || (rc = tb.alloc(batch * 64))) return rc;
  ZK_HIP(hipMemcpyAsync(tv.p, values, batch * c.n_rows * 32, hipMemcpyDefault, ctx->stream));
  ZK_HIP(hipMemcpyAsync(tb.p, blind2, batch * 64, hipMemcpyDefault, ctx->stream));
  Fr* scal = (Fr*)pk->cm_scal.p + c.scal_row * Bp;
  Fr* bl = (Fr*)pk->cm_blind.p + (size_t)2 * index * Bp;
  if ((rc = transpose_in(ctx, tv.p, scal, c.n_rows, batch, Bp, 32)) ||
      (rc = transpose_in(ctx, tb.p, bl, 2, batch, Bp, 32)))
    return rc;
  std::vector<G1Affine> pts(batch);
  std::vector<Fr> hs(batch);
  if ((rc = commit_step(ctx, pk, index, bl, Bp, batch, pts.data(), hs.data(), 1))) return rc;
  ZK_HIP(hipMemcpy(commit_out, pts.data(), batch * 64, hipMemcpyDefault));
  ZK_HIP(hipMemcpy(h_out, hs.data(), batch * 32, hipMemcpyDefault));
  return ZKMI_OK;
}

}  // extern "C"
