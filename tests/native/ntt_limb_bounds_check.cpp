// Host run of the schedule of the 29-bit transform chains of csrc/ntt.hip with the limb form between
// the passes: norm at every load, no wred except where the kernels keep one (the chain value that
// multiplies another chain value, ldw29).  One lane is simulated: its n elements go through the first
// pass with the unit products skipped, ntt_mid29 with 1..3 stages, the middle passes, the fused pass,
// the forward passes and the a_c * b_c product (compute_ab_coset_bi), and through ntt_fused29<true>
// and the final inverse transform (compute_h_bi), for log n = 8..12.
// Checked at every product and store: sums and differences fit an int32 limb for limb, the column
// sums of a product fit an int64, |a b| < 64 r^2, a product leaves (-r/2, 3r/2), a value after s
// stages is below (24 + 1.5 (s - 4)) r as the head of ntt.hip states, and the value is what 256-bit
// integer arithmetic mod r (unsigned __int128, independent of ff29.h) gives.
// Inputs (patterns 0..3): all zero, all r - 1, alternating 0 / r - 1, pseudo-random; each also with
// every product replaced by the representative of its class inside (-r/2, 3r/2) that makes the
// butterfly's larger output largest (the worst sign pattern for growth a product's contract allows).
//   g++ -O2 -std=c++17 -I gnark_crypto_primitives_amd/csrc tests/native/ntt_limb_bounds_check.cpp
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ff29.h"

using namespace zk;
typedef unsigned __int128 u128;

static int fails = 0;
#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      if (fails < 20) printf("FAIL line %d: %s\n", __LINE__, #c);    \
      fails++;                                                       \
    }                                                                \
  } while (0)

// ---- 256-bit integers mod r on unsigned __int128 -------------------------------------------------
struct U256 {
  uint64_t w[4];
};
static U256 RMOD, R2, INV261, ONE = {{1, 0, 0, 0}}, ZERO = {{0, 0, 0, 0}};
static uint64_t NINV;
static bool geq(const U256& a, const U256& b) {
  for (int i = 3; i >= 0; i--)
    if (a.w[i] != b.w[i]) return a.w[i] > b.w[i];
  return true;
}
static bool eq(const U256& a, const U256& b) {
  return a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2] && a.w[3] == b.w[3];
}
static U256 sub_raw(const U256& a, const U256& b) {
  U256 r;
  uint64_t br = 0;
  for (int i = 0; i < 4; i++) {
    const u128 t = (u128)a.w[i] - b.w[i] - br;
    r.w[i] = (uint64_t)t;
    br = (uint64_t)(t >> 64) & 1;
  }
  return r;
}
static U256 addmod(const U256& a, const U256& b) {   // a, b < r < 2^254
  U256 r;
  uint64_t c = 0;
  for (int i = 0; i < 4; i++) {
    const u128 t = (u128)a.w[i] + b.w[i] + c;
    r.w[i] = (uint64_t)t;
    c = (uint64_t)(t >> 64);
  }
  return geq(r, RMOD) ? sub_raw(r, RMOD) : r;
}
static U256 submod(const U256& a, const U256& b) {
  return geq(a, b) ? sub_raw(a, b) : sub_raw(RMOD, sub_raw(b, a));
}
static U256 montmul(const U256& a, const U256& b) {   // a b / 2^256 mod r
  uint64_t t[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 4; i++) {
    u128 c = 0;
    for (int j = 0; j < 4; j++) {
      c += (u128)a.w[j] * b.w[i] + t[j];
      t[j] = (uint64_t)c;
      c >>= 64;
    }
    c += t[4];
    t[4] = (uint64_t)c;
    t[5] = (uint64_t)(c >> 64);
    const uint64_t m = t[0] * NINV;
    c = ((u128)m * RMOD.w[0] + t[0]) >> 64;
    for (int j = 1; j < 4; j++) {
      c += (u128)m * RMOD.w[j] + t[j];
      t[j - 1] = (uint64_t)c;
      c >>= 64;
    }
    c += t[4];
    t[3] = (uint64_t)c;
    t[4] = t[5] + (uint64_t)(c >> 64);
  }
  U256 r = {{t[0], t[1], t[2], t[3]}};
  return (t[4] || geq(r, RMOD)) ? sub_raw(r, RMOD) : r;
}
static U256 mulmod(const U256& a, const U256& b) { return montmul(montmul(a, b), R2); }
static U256 powmod(U256 b, const U256& e) {
  U256 r = ONE;
  for (int i = 0; i < 256; i++) {
    if ((e.w[i / 64] >> (i % 64)) & 1) r = mulmod(r, b);
    b = mulmod(b, b);
  }
  return r;
}
static U256 from_limbs29(const int64_t l[9]) {   // limbs in [0, 2^29), value < 2^256
  U256 r = ZERO;
  for (int i = 0; i < 9; i++) {
    const int bit = 29 * i;
    r.w[bit / 64] |= (uint64_t)l[i] << (bit % 64);
    if (bit % 64 > 35 && bit / 64 < 3) r.w[bit / 64 + 1] |= (uint64_t)l[i] >> (64 - bit % 64);
  }
  return r;
}
static void init_mod() {
  int64_t l[9];
  for (int i = 0; i < 9; i++) l[i] = Fr29Params::p(i);
  RMOD = from_limbs29(l);
  uint64_t x = 1;
  for (int i = 0; i < 7; i++) x *= 2 - RMOD.w[0] * x;
  NINV = (uint64_t)0 - x;
  R2 = ONE;
  for (int i = 0; i < 512; i++) R2 = addmod(R2, R2);
  INV261 = ONE;
  for (int i = 0; i < 261; i++) {   // halve
    U256 h = INV261;
    uint64_t top = 0;
    if (h.w[0] & 1) {
      uint64_t c = 0;
      for (int j = 0; j < 4; j++) {
        const u128 t = (u128)h.w[j] + RMOD.w[j] + c;
        h.w[j] = (uint64_t)t;
        c = (uint64_t)(t >> 64);
      }
      top = c;
    }
    for (int j = 0; j < 4; j++) h.w[j] = (h.w[j] >> 1) | ((j < 3 ? h.w[j + 1] : top) << 63);
    INV261 = h;
  }
}

// ---- what is known about an F29 value ------------------------------------------------------------
static long double RLD;
static long double val(const Fr29& a) {   // the integer, to 64 bits
  long double v = 0;
  for (int i = 8; i >= 0; i--) v = v * 536870912.0L + (long double)a.v[i];
  return v;
}
static long double in_r(const Fr29& a) { return fabsl(val(a)) / RLD; }
// the value mod r, for |value| < 2^7 r and any int32 limbs
static U256 residue(const Fr29& a) {
  int64_t l[10];
  for (int i = 0; i < 9; i++) l[i] = (int64_t)a.v[i] + 128 * (int64_t)Fr29Params::p(i);
  int64_t c = 0;
  for (int i = 0; i < 8; i++) {
    const int64_t t = l[i] + c;
    l[i] = t & Fr29::MASK;
    c = t >> 29;
  }
  l[8] += c;
  CHECK(l[8] >= 0 && l[8] < ((int64_t)1 << 31));   // 0 <= value + 128 r < 256 r < 2^263
  // 263 bits: reduce the part above 2^232 first, then pack
  static U256 p232 = ZERO;
  if (eq(p232, ZERO)) {
    p232 = ONE;
    for (int i = 0; i < 232; i++) p232 = addmod(p232, p232);
  }
  const U256 hi = {{(uint64_t)l[8], 0, 0, 0}};
  l[8] = 0;
  return addmod(from_limbs29(l), mulmod(hi, p232));   // from_limbs29 < 2^232 < r
}
static bool normalised(const Fr29& a) {
  for (int i = 0; i < 8; i++)
    if (a.v[i] < 0 || a.v[i] > Fr29::MASK) return false;
  return true;
}

// an element of the simulated lane: the limbs the kernels would hold and the residue they stand for
struct El {
  Fr29 x;
  U256 ref;
};
static bool adversarial = false;

static El cadd(const El& a, const El& b, bool minus) {
  for (int i = 0; i < 9; i++) {
    const int64_t t = minus ? (int64_t)a.x.v[i] - b.x.v[i] : (int64_t)a.x.v[i] + b.x.v[i];
    CHECK(t >= INT32_MIN && t <= INT32_MAX);
  }
  return {minus ? sub(a.x, b.x) : add(a.x, b.x), minus ? submod(a.ref, b.ref) : addmod(a.ref, b.ref)};
}
static El cnorm(const El& a) {
  int64_t c = 0;
  for (int i = 0; i < 9; i++) {
    const int64_t t = (int64_t)a.x.v[i] + c;
    CHECK(t >= INT32_MIN && t <= INT32_MAX);
    c = t >> 29;
  }
  const El r = {norm(a.x), a.ref};
  CHECK(normalised(r.x) && fabsl(val(r.x) - val(a.x)) <= 0x1p-60L * RLD);
  return r;
}
// mul under its contract: column sums inside an int64, |a b| < 64 r^2; result normalised, in
// (-r/2, 3r/2), and a b / 2^261 mod r
static El cmul(const El& a, const El& b) {
  for (int k = 0; k < 17; k++) {
    u128 col = 0;
    for (int i = 0; i < 9; i++)
      if (k - i >= 0 && k - i < 9)
        col += (u128)(uint64_t)llabs((long long)a.x.v[i]) * (uint64_t)llabs((long long)b.x.v[k - i]) +
               ((u128)1 << 58);   // and m_i p_j
    CHECK(col + ((u128)1 << 35) < ((u128)1 << 63));   // plus the carry from the column before
  }
  CHECK(in_r(a.x) * in_r(b.x) < 64.0L);
  El r = {mul(a.x, b.x), mulmod(mulmod(a.ref, b.ref), INV261)};
  const long double v = val(r.x) / RLD;
  CHECK(normalised(r.x) && v > -0.5L && v < 1.5L);
  CHECK(eq(residue(r.x), r.ref));
  return r;
}
static El cwred(const El& a) {
  CHECK(in_r(a.x) < 128.0L);
  const El r = {wred(a.x), a.ref};
  CHECK(normalised(r.x) && in_r(r.x) < 0.6L && eq(residue(r.x), r.ref));
  return r;
}
// the representative of t's class in (-r/2, 3r/2) that makes max(|u + t|, |u - t|) largest
static El worst_rep(const El& t, const El& u) {
  Fr29 p;
  for (int i = 0; i < 9; i++) p.v[i] = Fr29Params::p(i);
  El best = t;
  long double bv = fabsl(val(u.x)) + fabsl(val(t.x));
  for (int s = -1; s <= 1; s += 2) {
    const Fr29 c = norm(s > 0 ? add(t.x, p) : sub(t.x, p));
    const long double v = val(c) / RLD;
    if (v > -0.5L && v < 1.5L && fabsl(val(u.x)) + fabsl(val(c)) > bv) {
      best.x = c;
      bv = fabsl(val(u.x)) + fabsl(val(c));
    }
  }
  return best;
}
static El canon(const U256& v) {   // a canonical memory image read by ld29 / ldc29
  uint32_t w[8];
  for (int i = 0; i < 8; i++) w[i] = (uint32_t)(v.w[i / 2] >> (32 * (i % 2)));
  return {unpack29<Fr29Params>(w), v};
}
static void check_canonical_store(const El& a) {   // pack_canonical of a product's output
  uint32_t w[8];
  pack_canonical<Fr29Params>(w, a.x);
  for (int i = 0; i < 8; i++) CHECK(w[i] == (uint32_t)(a.ref.w[i / 2] >> (32 * (i % 2))));
}

// ---- the schedule of ntt.hip ---------------------------------------------------------------------
struct Domain {
  int lg;
  std::vector<El> tw_fwd, tw_inv, cosetn;   // w^i, w^-i (i < n/2), g^i / n (i < n): F-domain tables
};
static uint32_t bitrev(uint32_t x, int bits) {
  uint32_t r = 0;
  for (int i = 0; i < bits; i++) r |= ((x >> i) & 1u) << (bits - 1 - i);
  return r;
}
static uint32_t pass_row(uint32_t hi, uint32_t q, uint32_t lo, int s0, int K) {
  return (hi << (s0 + K)) | (q << s0) | lo;
}
// butterflies<J0, NJ, LQ, FROM0> on the m values x[0..m)
static void butterflies(int J0, int NJ, int LQ, bool from0, El* x, int m, uint32_t qb, int log_n,
                        int s0, uint32_t lo, const std::vector<El>& tw) {
  for (int j = J0; j < J0 + NJ; j++) {
    const int s = (from0 ? 0 : s0) + j, jj = j - LQ;
    for (int bf = 0; bf < m / 2; bf++) {
      const int i0 = ((bf >> jj) << (jj + 1)) | (bf & ((1 << jj) - 1));
      const int i1 = i0 | (1 << jj);
      const uint32_t q = qb + ((uint32_t)i0 << LQ);
      const uint32_t qlow = q & ((1u << j) - 1u);
      const uint32_t pos = from0 ? qlow : ((qlow << s0) | lo);
      El t = x[i1];
      if (!(from0 && pos == 0)) {
        t = cmul(x[i1], tw[pos << (log_n - 1 - s)]);
        if (adversarial) t = worst_rep(t, x[i0]);
      }
      const El u = x[i0];
      x[i1] = cadd(u, t, true);
      x[i0] = cadd(u, t, false);
    }
  }
}
// the four stages of a block of 16 (ntt_pass4_lds29, either half of a fused pass): X[q], q < 16
static void block16(El* X, bool from0, int log_n, int s0, uint32_t lo, const std::vector<El>& tw) {
  for (uint32_t w = 0; w < 4; w++) butterflies(0, 2, 0, from0, X + 4 * w, 4, 4 * w, log_n, s0, lo, tw);
  for (int q = 0; q < 16; q++) X[q] = cnorm(X[q]);   // exchange29
  for (uint32_t w = 0; w < 4; w++) {
    El x[4] = {X[w], X[w + 4], X[w + 8], X[w + 12]};
    butterflies(2, 2, 2, from0, x, 4, w, log_n, s0, lo, tw);
    for (int i = 0; i < 4; i++) X[w + 4 * i] = x[i];
  }
}
// a store in limb form after `stages` stages of a transform: the bound of the head of ntt.hip
static long double largest_stored = 0;
static void check_limb_store(const El& a, int stages) {
  if (in_r(a.x) > largest_stored) largest_stored = in_r(a.x);
  CHECK(in_r(a.x) < 24.0L + 1.5L * (stages - 4));
  CHECK(eq(residue(a.x), a.ref));
}
struct Post {
  bool any = false;
  bool factor = true;                       // a product by table[row] or `uniform`
  const std::vector<El>* table = nullptr;   // per row, else `uniform`
  El uniform;
  const std::vector<El>* times = nullptr;   // limb form
};
// stages [s_from, s_to) as ntt29 runs them; src is canonical (first pass) or dst itself
static void ntt29(const Domain& D, const std::vector<El>* src, std::vector<El>& dst,
                  const std::vector<El>& tw, bool in_std, size_t n_valid, const Post& post,
                  int s_from, int s_to) {
  const int lg = D.lg, rem = lg % 4;
  const uint32_t n = 1u << lg;
  for (int s0 = s_from; s0 < s_to;) {
    if (rem && s0 == 4) {   // ntt_mid29<rem>
      const int m = 1 << rem;
      for (uint32_t g = 0; g < (n >> rem); g++) {
        const uint32_t lo = g & 15u, hi = g >> 4;
        El x[8];
        for (int i = 0; i < m; i++) x[i] = cnorm(dst[pass_row(hi, i, lo, s0, rem)]);
        butterflies(0, rem < 2 ? rem : 2, 0, false, x, m, 0, lg, s0, lo, tw);
        if (rem == 3) {
          for (int i = 0; i < m; i++) x[i] = cnorm(x[i]);
          butterflies(2, 1, 0, false, x, m, 0, lg, s0, lo, tw);
        }
        for (int i = 0; i < m; i++) {
          check_limb_store(x[i], s0 + rem);
          dst[pass_row(hi, i, lo, s0, rem)] = x[i];
        }
      }
      s0 += rem;
      continue;
    }
    const bool first = s0 == 0, last = s0 + 4 == lg;
    for (uint32_t g = 0; g < n / 16; g++) {
      const uint32_t lo = g & ((1u << s0) - 1u), hi = g >> s0;
      El X[16];
      for (uint32_t q = 0; q < 16; q++) {
        const uint32_t row = pass_row(hi, q, lo, s0, 4);
        if (first) {   // first_load29
          const uint32_t srow = bitrev(row, lg);
          if (srow >= n_valid) {
            X[q] = {Fr29::zero(), ZERO};
          } else {
            X[q] = (*src)[srow];
            if (in_std) {
              Fr29 c;
              for (int l = 0; l < 9; l++) c.v[l] = Fr29Params::c266(l);
              X[q] = cmul(X[q], {c, residue(c)});
            }
          }
        } else {
          X[q] = cnorm(dst[row]);   // ldl29
        }
      }
      block16(X, first, lg, s0, lo, tw);
      for (uint32_t q = 0; q < 16; q++) {
        const uint32_t row = pass_row(hi, q, lo, s0, 4);
        if (last && post.any) {
          El v = cnorm(X[q]);
          if (post.times) v = cmul(v, cwred((*post.times)[row]));   // ldw29
          if (post.factor) v = cmul(v, post.table ? (*post.table)[row] : post.uniform);
          check_canonical_store(v);
          dst[row] = canon(v.ref);
        } else {
          check_limb_store(X[q], s0 + 4);
          dst[row] = X[q];
        }
      }
    }
    s0 += 4;
  }
}
// ntt_fused29<PRODUCT>: last pass of one transform, a product per row, first pass of the next
static void fused29(const Domain& D, const std::vector<El>& src, std::vector<El>& dst,
                    const std::vector<El>& tw_last, const std::vector<El>& tw_first,
                    const std::vector<El>& factor, bool product) {
  const int lg = D.lg, s0 = lg - 4;
  for (uint32_t lo = 0; lo < (1u << s0); lo++) {
    El X[16], Y[16];
    for (uint32_t q = 0; q < 16; q++) X[q] = cnorm(src[pass_row(0, q, lo, s0, 4)]);
    block16(X, false, lg, s0, lo, tw_last);
    for (uint32_t k = 0; k < 16; k++) {
      const uint32_t row = pass_row(0, k, lo, s0, 4);
      CHECK(in_r(X[k].x) < 24.0L + 1.5L * (lg - 4));
      Y[bitrev(k, 4)] = cmul(cnorm(X[k]), product ? cwred(factor[row]) : factor[row]);
    }
    block16(Y, true, lg, 0, 0, tw_first);
    const uint32_t hi = bitrev(lo, s0);
    for (uint32_t q = 0; q < 16; q++) {
      check_limb_store(Y[q], 4);
      dst[pass_row(hi, q, 0, 0, 4)] = Y[q];
    }
  }
}
static void to_coset29(const Domain& D, std::vector<El>& x, std::vector<El>& t0, size_t n_valid,
                       bool in_std, int s_to, const Post& post) {
  const std::vector<El> in = x;
  ntt29(D, &in, t0, D.tw_inv, in_std, n_valid, Post(), 0, D.lg - 4);
  fused29(D, t0, x, D.tw_inv, D.tw_fwd, D.cosetn, false);
  ntt29(D, nullptr, x, D.tw_fwd, false, (size_t)1 << D.lg, post, 4, s_to);
}

static Domain make_domain(int lg) {
  Domain D;
  D.lg = lg;
  const uint32_t n = 1u << lg;
  U256 e = sub_raw(RMOD, ONE);   // (r - 1) >> lg
  for (int i = 0; i < lg; i++)
    for (int j = 0; j < 4; j++) e.w[j] = (e.w[j] >> 1) | (j < 3 ? e.w[j + 1] << 63 : 0);
  const U256 five = {{5, 0, 0, 0}};
  const U256 w = powmod(five, e), wi = powmod(w, sub_raw(RMOD, {{2, 0, 0, 0}}));
  U256 f261 = ONE;   // 2^261: the F domain's unit
  for (int i = 0; i < 261; i++) f261 = addmod(f261, f261);
  const U256 ninv = powmod({{n, 0, 0, 0}}, sub_raw(RMOD, {{2, 0, 0, 0}}));
  U256 a = f261, b = f261, c = mulmod(f261, ninv);
  for (uint32_t i = 0; i < n; i++) {
    if (i < n / 2) {
      D.tw_fwd.push_back(canon(a));
      D.tw_inv.push_back(canon(b));
      a = mulmod(a, w);
      b = mulmod(b, wi);
    }
    D.cosetn.push_back(canon(c));
    c = mulmod(c, five);
  }
  return D;
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}
static std::vector<El> input(int pattern, uint32_t n, uint32_t shift) {
  std::vector<El> v;
  const U256 top = sub_raw(RMOD, ONE);
  for (uint32_t i = 0; i < n; i++) {
    U256 x = ZERO;
    if (pattern == 1) x = top;
    if (pattern == 2) x = ((i + shift) & 1) ? top : ZERO;
    if (pattern == 3) {
      x = {{rnd(), rnd(), rnd(), rnd() >> 3}};
      while (geq(x, RMOD)) x = sub_raw(x, RMOD);
    }
    v.push_back(canon(x));
  }
  return v;
}

static void run(int lg, int pattern, bool adv) {
  adversarial = adv;
  const Domain D = make_domain(lg);
  const uint32_t n = 1u << lg;
  const size_t n_valid = n - 3;   // rows read as zero, as the prover's domains have
  U256 c256 = ONE;   // the unit of gnark's image
  for (int i = 0; i < 256; i++) c256 = addmod(c256, c256);
  Post unit;
  unit.any = true;
  unit.uniform = canon(c256);
  // compute_ab_coset_bi: a to stage lg in limb form, b's last store times a_c and the unit of
  // gnark's image, or (out_f) times a_c alone
  for (int out_f = 0; out_f < 2; out_f++) {
    std::vector<El> a = input(pattern, n, 0), b = input(pattern, n, 1), t0(n);
    to_coset29(D, a, t0, n_valid, true, lg, Post());
    Post times = unit;
    times.times = &a;
    times.factor = !out_f;
    to_coset29(D, b, t0, n_valid, out_f != 0, lg, times);
  }
  // compute_h_bi: b to stage lg - 4, ntt_fused29<true> against a_c, the inverse transform's last
  // store with a per-row table (any canonical table serves: g^i / n)
  {
    std::vector<El> a = input(pattern, n, 1), b = input(pattern, n, 0), t0(n);
    to_coset29(D, a, t0, n_valid, false, lg, Post());
    to_coset29(D, b, t0, n_valid, true, lg - 4, Post());
    fused29(D, b, t0, D.tw_fwd, D.tw_inv, a, true);
    Post last;
    last.any = true;
    last.table = &D.cosetn;
    ntt29(D, nullptr, t0, D.tw_inv, false, n, last, 4, lg);
  }
  // ntt_bi: one transform, gnark's image in, canonical out
  {
    const std::vector<El> src = input(pattern, n, 0);
    std::vector<El> dst(n);
    ntt29(D, &src, dst, D.tw_fwd, true, n, unit, 0, lg);
  }
}

int main() {
  init_mod();
  Fr29 p;
  for (int i = 0; i < 9; i++) p.v[i] = Fr29Params::p(i);
  RLD = val(p);
  // the arithmetic of this file against itself: 2^261 * 2^-261 = 1, (r - 1)^2 = 1
  U256 f261 = ONE;
  for (int i = 0; i < 261; i++) f261 = addmod(f261, f261);
  CHECK(eq(mulmod(f261, INV261), ONE));
  CHECK(eq(mulmod(sub_raw(RMOD, ONE), sub_raw(RMOD, ONE)), ONE));
  CHECK(eq(residue(Fr29::one()), f261));
  // the largest chain the kernels can run, log n = 28: (24 + 1.5 * 24) r = 60 r, inside 64 r and
  // with a top limb below 2^28
  CHECK(24.0 + 1.5 * (28 - 4) <= 60.0 && 60.0L * (Fr29Params::p(8) + 1) < (long double)(1 << 28));
  for (int lg = 8; lg <= 12; lg++)
    for (int pattern = 0; pattern < 4; pattern++)
      for (int adv = 0; adv < 2; adv++) {
        // every input at 2^8 and 2^9; the larger domains (ntt_mid29<2>, <3>, a middle LDS pass)
        // with the inputs that grow most
        if (lg >= 10 && !(adv && (pattern == 3 || (pattern == 1 && lg < 12)))) continue;
        const int before = fails;
        largest_stored = 0;
        run(lg, pattern, adv != 0);
        printf("log n %2d pattern %d %s: largest stored value %.2Lf r of %.1f r: %s\n", lg, pattern,
               adv ? "worst signs" : "as computed", largest_stored, 24.0 + 1.5 * (lg - 4),
               fails == before ? "ok" : "FAILED");
      }
  printf(fails ? "ntt limb bounds FAILED (%d)\n" : "ntt limb bounds ok\n", fails);
  return fails ? 1 : 0;
}
