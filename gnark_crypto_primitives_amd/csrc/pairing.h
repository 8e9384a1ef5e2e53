// BN254 optimal-ate pairing and the per-proof Groth16 check on the fully reduced Fq / Fq2 of ff.h,
// written for the host and for gfx950 like ff.h and ec.h.  Stands in for bn254.PairingCheck /
// groth16.Verify (gnark backend/groth16/bn254/verify.go [UPSTREAM-RECALL]); the host reference is
// verify.py.  Today only the host side is built and tested (tests/test_native_pairing.py); no
// kernel of libzkmi.so includes this header yet.
//
// Tower: Fq2 = Fq[u]/(u^2 + 1), Fq6 = Fq2[v]/(v^3 - xi), Fq12 = Fq6[w]/(w^2 - v), xi = 9 + u, so
// w^6 = xi and an element is sum_i a_i w^i with a_i in Fq2: (c0.c0, c1.c0, c0.c1, c1.c1, c0.c2, c1.c2).
// G2 is the r-torsion of the D-type twist E': y^2 = x^3 + 3/xi, carried into E(Fq12) by
// (x, y) -> (x w^2, y w^3) (the map verify.py uses).
//
// Code shape.  ZK_HD is __forceinline__, and an Fq12 product is 54 Fq products of ~540 instructions:
// everything from the Fq2 product upwards is therefore a ZK_NI (__noinline__) routine taking
// references, emitted once per object, and every bit loop is rolled (#pragma unroll 1).  Results go
// through an out reference that may alias an input.  This path is bound by latency, not by multiplier
// throughput; private stack use is accepted.
//
// Constants.  The Frobenius coefficients and the twist's b are computed from p and xi by
// pairing_consts_init below (host), the loop counts come from BN_U; BN_U, the ate count 6u + 2, the
// hard-part digits and the generators are checked against Python integers by
// tests/test_native_pairing.py.
#pragma once
#include <string.h>

#include <vector>

#include "ec.h"

#if defined(__HIPCC__)
#define ZK_NI __host__ __device__ __noinline__
#else
#define ZK_NI inline
#endif

namespace zk {

// ---- curve parameter ------------------------------------------------------------------------------
// p = 36u^4 + 36u^3 + 24u^2 + 6u + 1, r = 36u^4 + 36u^3 + 18u^2 + 6u + 1
constexpr uint64_t BN_U = 0x44e992b44a6909f1ull;   // 63 bits
constexpr int BN_U_BITS = 63;
// ate loop count 6u + 2 = 2^64 + ATE_LO (65 bits; the product wraps exactly once)
constexpr uint64_t ATE_LO = BN_U * 6u + 2u;
constexpr int ATE_BITS = 65;
ZK_HD int ate_bit(int i) { return i == 64 ? 1 : (int)((ATE_LO >> i) & 1); }
// lines of one Miller loop: 64 doublings, one addition per set bit below the top, two Frobenius lines
ZK_HD int ate_n_lines() {
  int n = 64 + 2;
  for (int i = 0; i < 64; i++) n += ate_bit(i);
  return n;
}

// ---- Fq2 ------------------------------------------------------------------------------------------
ZK_HD Fq2 conj(const Fq2& a) { return Fq2{a.c0, neg(a.c1)}; }
ZK_HD Fq2 mul_fq(const Fq2& a, const Fq& k) { return Fq2{mul(a.c0, k), mul(a.c1, k)}; }
// (9 + u) a
ZK_HD Fq2 mul_xi(const Fq2& a) {
  Fq2 t = add(dbl(dbl(dbl(a))), a);
  return Fq2{sub(t.c0, a.c1), add(t.c1, a.c0)};
}
ZK_NI void fq2_mul(Fq2& r, const Fq2& a, const Fq2& b) { r = mul(a, b); }
ZK_NI void fq2_sqr(Fq2& r, const Fq2& a) { r = sqr(a); }
ZK_NI void fq2_inv(Fq2& r, const Fq2& a) { r = inverse(a); }
ZK_NI void fq_inv(Fq& r, const Fq& a) { r = inverse(a); }
// value forms of the above, for formulas
ZK_HD Fq2 M(const Fq2& a, const Fq2& b) {
  Fq2 r;
  fq2_mul(r, a, b);
  return r;
}
ZK_HD Fq2 S(const Fq2& a) {
  Fq2 r;
  fq2_sqr(r, a);
  return r;
}

// ---- Fq6 ------------------------------------------------------------------------------------------
struct Fq6 {
  Fq2 c0, c1, c2;
};
struct Fq12 {
  Fq6 c0, c1;
};

ZK_NI void f6_add(Fq6& r, const Fq6& a, const Fq6& b) {
  r.c0 = add(a.c0, b.c0);
  r.c1 = add(a.c1, b.c1);
  r.c2 = add(a.c2, b.c2);
}
ZK_NI void f6_sub(Fq6& r, const Fq6& a, const Fq6& b) {
  r.c0 = sub(a.c0, b.c0);
  r.c1 = sub(a.c1, b.c1);
  r.c2 = sub(a.c2, b.c2);
}
ZK_NI void f6_neg(Fq6& r, const Fq6& a) {
  r.c0 = neg(a.c0);
  r.c1 = neg(a.c1);
  r.c2 = neg(a.c2);
}
// v a = (xi a2, a0, a1)
ZK_NI void f6_mul_v(Fq6& r, const Fq6& a) {
  Fq2 t = mul_xi(a.c2);
  r.c2 = a.c1;
  r.c1 = a.c0;
  r.c0 = t;
}
ZK_NI void f6_mul(Fq6& r, const Fq6& a, const Fq6& b) {
  Fq2 v0 = M(a.c0, b.c0), v1 = M(a.c1, b.c1), v2 = M(a.c2, b.c2);
  Fq2 t0 = sub(sub(M(add(a.c1, a.c2), add(b.c1, b.c2)), v1), v2);
  Fq2 t1 = sub(sub(M(add(a.c0, a.c1), add(b.c0, b.c1)), v0), v1);
  Fq2 t2 = sub(sub(M(add(a.c0, a.c2), add(b.c0, b.c2)), v0), v2);
  r.c0 = add(v0, mul_xi(t0));
  r.c1 = add(t1, mul_xi(v2));
  r.c2 = add(t2, v1);
}
// a (b0 + b1 v)
ZK_NI void f6_mul_01(Fq6& r, const Fq6& a, const Fq2& b0, const Fq2& b1) {
  Fq2 v0 = M(a.c0, b0), v1 = M(a.c1, b1);
  Fq2 t0 = M(a.c2, b1);
  Fq2 t1 = sub(sub(M(add(a.c0, a.c1), add(b0, b1)), v0), v1);
  Fq2 t2 = M(a.c2, b0);
  r.c0 = add(v0, mul_xi(t0));
  r.c1 = t1;
  r.c2 = add(t2, v1);
}
// a k, k in Fq
ZK_NI void f6_mul_fq(Fq6& r, const Fq6& a, const Fq& k) {
  r.c0 = mul_fq(a.c0, k);
  r.c1 = mul_fq(a.c1, k);
  r.c2 = mul_fq(a.c2, k);
}
// 1/a through the norm to Fq2 (then Fq): (t0, t1, t2) / (a0 t0 + xi (a2 t1 + a1 t2))
ZK_NI void f6_inv(Fq6& r, const Fq6& a) {
  Fq2 t0 = sub(S(a.c0), mul_xi(M(a.c1, a.c2)));
  Fq2 t1 = sub(mul_xi(S(a.c2)), M(a.c0, a.c1));
  Fq2 t2 = sub(S(a.c1), M(a.c0, a.c2));
  Fq2 d = add(M(a.c0, t0), mul_xi(add(M(a.c2, t1), M(a.c1, t2))));
  Fq2 di;
  fq2_inv(di, d);
  r.c0 = M(t0, di);
  r.c1 = M(t1, di);
  r.c2 = M(t2, di);
}

// ---- Fq12 -----------------------------------------------------------------------------------------
ZK_HD Fq6 f6_zero() { return Fq6{Fq2::zero(), Fq2::zero(), Fq2::zero()}; }
ZK_HD Fq12 f12_one() { return Fq12{Fq6{Fq2::one(), Fq2::zero(), Fq2::zero()}, f6_zero()}; }
ZK_HD bool f6_eq(const Fq6& a, const Fq6& b) { return a.c0 == b.c0 && a.c1 == b.c1 && a.c2 == b.c2; }
ZK_HD bool f12_eq(const Fq12& a, const Fq12& b) { return f6_eq(a.c0, b.c0) && f6_eq(a.c1, b.c1); }

ZK_NI void f12_mul(Fq12& r, const Fq12& a, const Fq12& b) {
  Fq6 t0, t1, s, sa, sb;
  f6_mul(t0, a.c0, b.c0);
  f6_mul(t1, a.c1, b.c1);
  f6_add(sa, a.c0, a.c1);
  f6_add(sb, b.c0, b.c1);
  f6_mul(s, sa, sb);
  f6_sub(s, s, t0);
  f6_sub(r.c1, s, t1);
  f6_mul_v(t1, t1);
  f6_add(r.c0, t0, t1);
}
// (a0 + a1 w)^2 = (a0 + a1)(a0 + v a1) - t - v t + 2 t w, t = a0 a1
ZK_NI void f12_sqr(Fq12& r, const Fq12& a) {
  Fq6 t, vt, s0, s1;
  f6_mul(t, a.c0, a.c1);
  f6_add(s0, a.c0, a.c1);
  f6_mul_v(s1, a.c1);
  f6_add(s1, s1, a.c0);
  f6_mul(s0, s0, s1);
  f6_mul_v(vt, t);
  f6_sub(s0, s0, t);
  f6_sub(r.c0, s0, vt);
  f6_add(r.c1, t, t);
}
// the p^6 Frobenius, w -> -w; the inverse of an element of the cyclotomic subgroup
ZK_NI void f12_conj(Fq12& r, const Fq12& a) {
  r.c0 = a.c0;
  f6_neg(r.c1, a.c1);
}
// 1/a = (a0 - a1 w) / (a0^2 - v a1^2): one Fq inversion in all
ZK_NI void f12_inv(Fq12& r, const Fq12& a) {
  Fq6 t0, t1;
  f6_mul(t0, a.c0, a.c0);
  f6_mul(t1, a.c1, a.c1);
  f6_mul_v(t1, t1);
  f6_sub(t0, t0, t1);
  f6_inv(t0, t0);
  f6_mul(r.c0, a.c0, t0);
  f6_mul(t1, a.c1, t0);
  f6_neg(r.c1, t1);
}

// Everything about the field tower and the twist that a kernel reads (wave-uniform).
struct PairingConsts {
  // frob[k - 1][i] = xi^(i (p^k - 1) / 6): coefficient of w^i under the p^k Frobenius, k = 1, 2, 3
  // (after conjugating a_i when k is odd)
  Fq2 frob[3][6];
  Fq2 twist_b;   // 3 / xi
};

// coefficient i of sum a_i w^i
ZK_HD Fq2& f12_coef(Fq12& a, int i) {
  Fq6& h = (i & 1) ? a.c1 : a.c0;
  return (i >> 1) == 0 ? h.c0 : (i >> 1) == 1 ? h.c1 : h.c2;
}
// a^(p^k), k = 1, 2, 3
ZK_NI void f12_frob(Fq12& r, const Fq12& a, int k, const PairingConsts& pc) {
  Fq12 t = a;
#pragma unroll 1
  for (int i = 0; i < 6; i++) {
    Fq2& c = f12_coef(t, i);
    if (k & 1) c = conj(c);
    if (i) fq2_mul(c, c, pc.frob[k - 1][i]);
  }
  r = t;
}

// a^e, e < 2^64, square and multiply from the top bit
ZK_NI void f12_pow_u64(Fq12& r, const Fq12& a, uint64_t e) {
  Fq12 acc = f12_one();
#pragma unroll 1
  for (int i = 63; i >= 0; i--) {
    f12_sqr(acc, acc);
    if ((e >> i) & 1) f12_mul(acc, acc, a);
  }
  r = acc;
}

// ---- Miller loop ----------------------------------------------------------------------------------
// The line through T = (xT, yT) on the twist with slope lam, at P = (xP, yP) in G1:
//   yP - lam xP w + (lam xT - yT) w^3      (w^3 = v w)
// up to factors in proper subfields, which the final exponentiation removes.
struct LineCoef {
  Fq2 nlam;   // -lam
  Fq2 mu;     // lam xT - yT
};

// T <- 2T and the tangent at the old T.  T has order r: y != 0.
ZK_NI void g2_dbl_line(G2Affine& T, LineCoef& l) {
  Fq2 x2 = S(T.x);
  Fq2 den;
  fq2_inv(den, dbl(T.y));
  Fq2 lam = M(add(dbl(x2), x2), den);
  l.nlam = neg(lam);
  l.mu = sub(M(lam, T.x), T.y);
  Fq2 x3 = sub(sub(S(lam), T.x), T.x);
  T.y = sub(M(lam, sub(T.x, x3)), T.y);
  T.x = x3;
}
// T <- T + Q and the chord through them.  In the ate loop T = kQ with k != +-1 mod r: x differ.
ZK_NI void g2_add_line(G2Affine& T, const G2Affine& Q, LineCoef& l) {
  Fq2 den;
  fq2_inv(den, sub(Q.x, T.x));
  Fq2 lam = M(sub(Q.y, T.y), den);
  l.nlam = neg(lam);
  l.mu = sub(M(lam, T.x), T.y);
  Fq2 x3 = sub(sub(S(lam), T.x), Q.x);
  T.y = sub(M(lam, sub(T.x, x3)), T.y);
  T.x = x3;
}
// pi(Q) and -pi^2(Q) in twist coordinates
ZK_NI void g2_frob_points(const G2Affine& Q, const PairingConsts& pc, G2Affine& q1, G2Affine& nq2) {
  q1.x = M(conj(Q.x), pc.frob[0][2]);
  q1.y = M(conj(Q.y), pc.frob[0][3]);
  nq2.x = M(Q.x, pc.frob[1][2]);
  nq2.y = neg(M(Q.y, pc.frob[1][3]));
}

// The ate loop as a sequence of steps, shared by the running-point form and the table form:
// step s of ate_n_lines(); sq = f is squared before the line of this step is multiplied in.
struct AteWalk {
  int bit = ATE_BITS - 2;   // next bit to double for; -1 / -2 = first / second Frobenius line
  bool add_pending = false;
  ZK_HD bool done() const { return bit < -2; }
};
// the line of the next step for the running point T of Q; returns whether f is squared first
ZK_HD bool ate_next_line(AteWalk& w, G2Affine& T, const G2Affine& Q, const G2Affine& q1,
                         const G2Affine& nq2, LineCoef& l) {
  if (w.add_pending) {
    g2_add_line(T, Q, l);
    w.add_pending = false;
    w.bit--;
    return false;
  }
  if (w.bit >= 0) {
    g2_dbl_line(T, l);
    if (ate_bit(w.bit))
      w.add_pending = true;
    else
      w.bit--;
    return true;
  }
  g2_add_line(T, w.bit == -1 ? q1 : nq2, l);
  w.bit--;
  return false;
}
// the same walk without a point: whether the next table entry is preceded by a squaring
ZK_HD bool ate_next_sq(AteWalk& w) {
  if (w.add_pending) {
    w.add_pending = false;
    w.bit--;
    return false;
  }
  if (w.bit >= 0) {
    if (ate_bit(w.bit))
      w.add_pending = true;
    else
      w.bit--;
    return true;
  }
  w.bit--;
  return false;
}

// the ate_n_lines() line coefficients of a fixed Q (the key's gamma and delta), in walk order
ZK_NI void g2_line_table(const G2Affine& Q, const PairingConsts& pc, LineCoef* out) {
  G2Affine T = Q, q1, nq2;
  g2_frob_points(Q, pc, q1, nq2);
  AteWalk w;
  int n = 0;
#pragma unroll 1
  while (!w.done()) ate_next_line(w, T, Q, q1, nq2, out[n++]);
}

// f <- f * line(P); a P at infinity contributes 1.
//   f (a + (b + c v) w), a = yP in Fq, b = nlam xP, c = mu
ZK_NI void f12_mul_line(Fq12& f, const LineCoef& l, const G1Affine& P) {
  if (P.is_inf()) return;
  Fq2 b = mul_fq(l.nlam, P.x);
  Fq6 t0, t1, s;
  f6_mul_fq(t0, f.c0, P.y);
  f6_mul_01(t1, f.c1, b, l.mu);
  f6_add(s, f.c0, f.c1);
  f6_mul_01(s, s, Fq2{add(b.c0, P.y), b.c1}, l.mu);
  f6_sub(s, s, t0);
  f6_sub(f.c1, s, t1);
  f6_mul_v(t1, t1);
  f6_add(f.c0, t0, t1);
}

// f = prod of the Miller functions of (P0, Q0) with Q0's running point, (P1, tab1), (P2, tab2):
// one squaring per step serves all three.  Q0 is on the twist, of order r, not infinity.
ZK_NI void miller_loop3(Fq12& f, const G1Affine& P0, const G2Affine& Q0, const G1Affine& P1,
                        const LineCoef* tab1, const G1Affine& P2, const LineCoef* tab2,
                        const PairingConsts& pc) {
  G2Affine T = Q0, q1, nq2;
  g2_frob_points(Q0, pc, q1, nq2);
  Fq12 acc = f12_one();
  AteWalk w;
  int n = 0;
#pragma unroll 1
  while (!w.done()) {
    LineCoef l;
    if (ate_next_line(w, T, Q0, q1, nq2, l)) f12_sqr(acc, acc);
    f12_mul_line(acc, l, P0);
    if (tab1) f12_mul_line(acc, tab1[n], P1);
    if (tab2) f12_mul_line(acc, tab2[n], P2);
    n++;
  }
  f = acc;
}

// ---- final exponentiation -------------------------------------------------------------------------
// f^((p^12 - 1) / r) exactly (the multiple c of the hard part is 1): easy part (p^6 - 1)(p^2 + 1),
// then the hard part h = (p^4 - p^2 + 1) / r in base p,
//   h = L0 + L1 p + L2 p^2 + p^3,  L0 = -(36u^3 + 30u^2 + 18u + 2),  L1 = -(36u^3 + 18u^2 + 12u) + 1,
//   L2 = 6u^2 + 1
// (the identity is checked against Python integers by the host test), with three powers by u and
// small powers of those.  After the easy part the inverse is the conjugate.
constexpr uint32_t HARD_L0[4] = {2, 18, 30, 36};   // -L0 = sum HARD_L0[i] u^i
constexpr uint32_t HARD_L1[4] = {0, 12, 18, 36};   // 1 - L1
constexpr uint32_t HARD_L2[4] = {1, 0, 6, 0};      // L2
ZK_NI void final_exp(Fq12& r, const Fq12& f, const PairingConsts& pc) {
  Fq12 t, x;
  f12_conj(t, f);
  f12_inv(x, f);
  f12_mul(t, t, x);          // f^(p^6 - 1)
  f12_frob(x, t, 2, pc);
  f12_mul(t, x, t);          // ^(p^2 + 1)
  Fq12 fu, fu2, fu3;
  f12_pow_u64(fu, t, BN_U);
  f12_pow_u64(fu2, fu, BN_U);
  f12_pow_u64(fu3, fu2, BN_U);
  Fq12 a, b, y;
  f12_pow_u64(a, fu3, 36);   // shared by L0 and L1
  f12_pow_u64(x, fu2, 30);
  f12_mul(y, a, x);
  f12_pow_u64(x, fu, 18);
  f12_mul(y, y, x);
  f12_sqr(x, t);
  f12_mul(y, y, x);
  f12_conj(y, y);            // t^L0
  f12_pow_u64(x, fu2, 18);
  f12_mul(b, a, x);
  f12_pow_u64(x, fu, 12);
  f12_mul(b, b, x);
  f12_conj(b, b);
  f12_mul(b, b, t);          // t^L1
  f12_frob(b, b, 1, pc);
  f12_mul(y, y, b);
  f12_pow_u64(x, fu2, 6);
  f12_mul(x, x, t);          // t^L2
  f12_frob(x, x, 2, pc);
  f12_mul(y, y, x);
  f12_frob(x, t, 3, pc);
  f12_mul(r, y, x);
}

// ---- points ---------------------------------------------------------------------------------------
ZK_HD Fq fq_small(uint32_t k) {
  Fq r = Fq::zero();
  r.v[0] = k;
  return to_mont(r);
}
ZK_HD G1Affine g1_generator() { return G1Affine{Fq::one(), dbl(Fq::one())}; }
ZK_HD G2Affine g2_generator() {   // Montgomery images; checked by the host test
  constexpr uint32_t g[4][8] = {
      {0x02bc2026u, 0x8e83b5d1u, 0x497b0172u, 0xdceb1935u, 0x97811adfu, 0xfbb82647u, 0xaf96503bu, 0x19573841u},
      {0xa84c6140u, 0xafb4737du, 0x5802d8c4u, 0x6043dd5au, 0x52a02f86u, 0x09e950fcu, 0x3aea7b6bu, 0x14fef083u},
      {0x886be9f6u, 0x619dfa9du, 0xf59e9b78u, 0xfe7fd297u, 0x231b7dfeu, 0xff9e1a62u, 0xae9e4206u, 0x28fd7eebu},
      {0xc71856eeu, 0x64095b56u, 0x327d3cbbu, 0xdc57f922u, 0x33351076u, 0x55f935beu, 0x93fd6482u, 0x0da4a0e6u}};
  G2Affine q;
  for (int i = 0; i < 8; i++) {
    q.x.c0.v[i] = g[0][i];
    q.x.c1.v[i] = g[1][i];
    q.y.c0.v[i] = g[2][i];
    q.y.c1.v[i] = g[3][i];
  }
  return q;
}

// a < m as 256-bit integers (m = the modulus of P): the canonical-encoding check
template <class P>
ZK_HD bool below_modulus(const uint32_t a[8]) {
  int64_t br = 0;
  for (int i = 0; i < 8; i++) {
    int64_t t = (int64_t)a[i] - (int64_t)P::p(i) + br;
    br = t >> 32;
  }
  return br != 0;
}
// y^2 = x^3 + 3; infinity (0, 0) is on the curve
ZK_NI bool g1_on_curve(const G1Affine& a) {
  if (a.is_inf()) return true;
  Fq rhs = add(mul(sqr(a.x), a.x), fq_small(3));
  return sqr(a.y) == rhs;
}
ZK_NI bool g2_on_curve(const G2Affine& a, const PairingConsts& pc) {
  if (a.is_inf()) return true;
  Fq2 rhs = add(M(S(a.x), a.x), pc.twist_b);
  return S(a.y) == rhs;
}
// [r]Q == O with the group law of ec.h (rolled double-and-add over the bits of r)
ZK_NI bool g2_in_subgroup(const G2Affine& q) {
  G2XYZZ acc = G2XYZZ::inf();
#pragma unroll 1
  for (int i = 253; i >= 0; i--) {
    acc = dbl(acc);
    if ((FrParams::p(i >> 5) >> (i & 31)) & 1) madd(acc, q);
  }
  return acc.is_inf();
}

// ---- the Groth16 check, in three stages (one kernel each on a GPU) --------------------------------
struct ProofPoints {
  G1Affine ar, krs;
  G2Affine bs;
};
// Stage 1.  words: the 256-byte proof image Ar | Krs | Bs.  False when a coordinate is not
// canonical, a point is off its curve, Bs is outside the r-subgroup, or Ar / Bs is at infinity (Krs
// may be); `out` then holds the generators, so that the later stages run on valid points.
ZK_NI bool proof_decode(const uint32_t* words, const PairingConsts& pc, ProofPoints& out) {
  bool ok = true;
#pragma unroll 1
  for (int i = 0; i < 8; i++) ok = below_modulus<FqParams>(words + 8 * i) && ok;
  Fq c[8];   // Ar.x Ar.y Krs.x Krs.y Bs.x.a0 Bs.x.a1 Bs.y.a0 Bs.y.a1
#pragma unroll 1
  for (int i = 0; i < 8; i++)
    for (int j = 0; j < 8; j++) c[i].v[j] = words[8 * i + j];
  ProofPoints pp{G1Affine{c[0], c[1]}, G1Affine{c[2], c[3]}, G2Affine{Fq2{c[4], c[5]}, Fq2{c[6], c[7]}}};
  ok = ok && !pp.ar.is_inf() && !pp.bs.is_inf();
  ok = ok && g1_on_curve(pp.ar) && g1_on_curve(pp.krs) && g2_on_curve(pp.bs, pc);
  ok = ok && g2_in_subgroup(pp.bs);
  if (!ok) {
    pp.ar = g1_generator();
    pp.krs = g1_generator();
    pp.bs = g2_generator();
  }
  out = pp;
  return ok;
}
// Stage 2.  vk_x = k0 + msm (both may be the identity, as may their sum), then the shared Miller
// loop over (-Ar, Bs), (vk_x, gamma), (Krs, delta).
ZK_NI void proof_miller(Fq12& f, const ProofPoints& pp, const G1Affine& k0, const G1XYZZ& msm,
                        const LineCoef* gamma_tab, const LineCoef* delta_tab,
                        const PairingConsts& pc) {
  G1XYZZ acc = msm;
  madd(acc, k0);
  G1Affine vkx;
  if (acc.is_inf()) {
    vkx = G1Affine::inf();
  } else {
    Fq izzz;
    fq_inv(izzz, acc.zzz);
    Fq izz = sqr(mul(izzz, acc.zz));
    vkx = G1Affine{mul(acc.x, izz), mul(acc.y, izzz)};
  }
  miller_loop3(f, neg(pp.ar), pp.bs, vkx, gamma_tab, pp.krs, delta_tab, pc);
}
// Stage 3.  e(-Ar, Bs) e(vk_x, gamma) e(Krs, delta) == 1 / e(alpha, beta)
ZK_NI bool proof_finish(const Fq12& f, const Fq12& eab_inv, const PairingConsts& pc) {
  Fq12 g;
  final_exp(g, f, pc);
  return f12_eq(g, eab_inv);
}

// ---- host: constants and key --------------------------------------------------------------------------
// a^e in Fq2, e a 256-bit integer (8 x 32, little-endian)
inline Fq2 fq2_pow(const Fq2& a, const uint32_t e[8]) {
  Fq2 acc = Fq2::one();
  for (int i = 255; i >= 0; i--) {
    acc = S(acc);
    if ((e[i >> 5] >> (i & 31)) & 1) acc = M(acc, a);
  }
  return acc;
}
inline void pairing_consts_init(PairingConsts& pc) {
  // e = (p - 1) / 6 by long division over the limbs of p - 1 (p is odd: p - 1 clears bit 0)
  uint32_t e[8];
  uint64_t rem = 0;
  for (int i = 7; i >= 0; i--) {
    uint64_t cur = (rem << 32) | (FqParams::p(i) - (i == 0 ? 1u : 0u));
    e[i] = (uint32_t)(cur / 6);
    rem = cur % 6;
  }
  const Fq2 xi{fq_small(9), Fq::one()};
  const Fq2 g = fq2_pow(xi, e);   // xi^((p - 1) / 6)
  pc.frob[0][0] = Fq2::one();
  for (int i = 1; i < 6; i++) pc.frob[0][i] = M(pc.frob[0][i - 1], g);
  for (int i = 0; i < 6; i++) {
    // xi^(i (p^2 - 1) / 6) = g_i^(p + 1) = g_i conj(g_i);  xi^(i (p^3 - 1) / 6) = g_i^(p^2 + p + 1)
    pc.frob[1][i] = M(pc.frob[0][i], conj(pc.frob[0][i]));
    pc.frob[2][i] = M(pc.frob[0][i], pc.frob[1][i]);
  }
  Fq2 xi_inv;
  fq2_inv(xi_inv, xi);
  pc.twist_b = mul_fq(xi_inv, fq_small(3));
}

// e(P, Q) for one pair (Q on the twist, of order r; either at infinity gives 1)
inline void pairing(Fq12& r, const G1Affine& P, const G2Affine& Q, const PairingConsts& pc) {
  if (P.is_inf() || Q.is_inf()) {
    r = f12_one();
    return;
  }
  Fq12 f;
  miller_loop3(f, P, Q, G1Affine::inf(), nullptr, G1Affine::inf(), nullptr, pc);
  final_exp(r, f, pc);
}

// What a loaded verifying key holds: checked points, 1 / e(alpha, beta), the line tables.
struct VkHost {
  PairingConsts pc;
  Fq12 eab_inv;   // 1 / e(alpha, beta)
  std::vector<G1Affine> k;
  std::vector<LineCoef> gamma_tab, delta_tab;
};
inline bool g1_image_ok(const void* image, G1Affine& out) {
  const uint32_t* w = (const uint32_t*)image;
  for (int i = 0; i < 2; i++)
    if (!below_modulus<FqParams>(w + 8 * i)) return false;
  memcpy(&out, image, sizeof(out));
  return g1_on_curve(out);
}
inline bool g2_image_ok(const void* image, const PairingConsts& pc, G2Affine& out) {
  const uint32_t* w = (const uint32_t*)image;
  for (int i = 0; i < 4; i++)
    if (!below_modulus<FqParams>(w + 8 * i)) return false;
  memcpy(&out, image, sizeof(out));
  return g2_on_curve(out, pc) && g2_in_subgroup(out);
}
// False when a key point is not canonical, off its curve, (G2) outside the subgroup, or one of
// alpha, beta, gamma, delta is at infinity (no setup produces such a key).
inline bool vk_host_init(VkHost& vk, uint32_t n_public, const void* g1_k, const void* g1_alpha,
                         const void* g2_beta, const void* g2_gamma, const void* g2_delta) {
  if (n_public == 0 || !g1_k || !g1_alpha || !g2_beta || !g2_gamma || !g2_delta) return false;
  pairing_consts_init(vk.pc);
  G1Affine alpha;
  G2Affine beta, gamma, delta;
  if (!g1_image_ok(g1_alpha, alpha) || !g2_image_ok(g2_beta, vk.pc, beta) ||
      !g2_image_ok(g2_gamma, vk.pc, gamma) || !g2_image_ok(g2_delta, vk.pc, delta))
    return false;
  if (alpha.is_inf() || beta.is_inf() || gamma.is_inf() || delta.is_inf()) return false;
  vk.k.resize(n_public);
  for (uint32_t i = 0; i < n_public; i++)
    if (!g1_image_ok((const char*)g1_k + 64 * (size_t)i, vk.k[i])) return false;
  Fq12 eab;
  pairing(eab, alpha, beta, vk.pc);
  f12_conj(vk.eab_inv, eab);
  vk.gamma_tab.resize(ate_n_lines());
  vk.delta_tab.resize(ate_n_lines());
  g2_line_table(gamma, vk.pc, vk.gamma_tab.data());
  g2_line_table(delta, vk.pc, vk.delta_tab.data());
  return true;
}
// The whole per-proof decision on the host: the three stages above around a double-and-add sum for
// vk_x.  publics: n_public - 1 fr images (Montgomery); one that is not below r fails the proof.
inline bool verify_one_host(const VkHost& vk, const void* proof, const void* publics) {
  ProofPoints pp;
  bool ok = proof_decode((const uint32_t*)proof, vk.pc, pp);
  G1XYZZ sum = G1XYZZ::inf();
  for (size_t j = 1; j < vk.k.size(); j++) {
    Fr s;
    memcpy(&s, (const char*)publics + 32 * (j - 1), 32);
    if (!below_modulus<FrParams>(s.v)) {
      ok = false;
      continue;
    }
    s = from_mont(s);
    padd(sum, scalar_mul(vk.k[j], s.v));
  }
  Fq12 f;
  proof_miller(f, pp, vk.k[0], sum, vk.gamma_tab.data(), vk.delta_tab.data(), vk.pc);
  return proof_finish(f, vk.eab_inv, vk.pc) && ok;
}

}  // namespace zk
