// G1 mixed addition on the 9 x 29-bit lazy representation (ff29.h) for the MSM inner loop.
// Same formulas as ec.h (EFD madd-2008-s / mdbl-2008-s-1); the comments track the limb and value
// bounds that ff29.h's mul/sqr contracts need.
#pragma once
#include "ec.h"
#include "ff29.h"
#if defined(__HIP_DEVICE_COMPILE__)
#include "ff29_asm.h"
#endif

namespace zk {

// Field products of the MSM inner loop: on the device the single-accumulator asm chains of
// ff29_asm.h (no v_lshl_add_u64 merges: 2192 -> ~2010 instructions per G1 mixed addition), on the
// host (tests/native/test_ff29.cpp) the C++ forms they restate.
#if defined(__HIP_DEVICE_COMPILE__)
template <class P> ZK_HD F29<P> mmul(const F29<P>& a, const F29<P>& b) { return mul_asm(a, b); }
template <class P> ZK_HD F29<P> msqr(const F29<P>& a) { return sqr_asm(a); }
template <class P>
ZK_HD F29<P> mmul_add2(const F29<P>& a, const F29<P>& b, const F29<P>& c, const F29<P>& d) {
  return mul_add2_asm(a, b, c, d);
}
#else
template <class P> ZK_HD F29<P> mmul(const F29<P>& a, const F29<P>& b) { return mul(a, b); }
template <class P> ZK_HD F29<P> msqr(const F29<P>& a) { return sqr(a); }
template <class P>
ZK_HD F29<P> mmul_add2(const F29<P>& a, const F29<P>& b, const F29<P>& c, const F29<P>& d) {
  return mul_add2(a, b, c, d);
}
#endif

// Invariants between calls: x, y normalised with |x| < 5p, |y| < 2p; zz, zzz mul outputs.
struct G1Acc29 {
  Fq29 x, y, zz, zzz;
  bool inf;
  static ZK_HD G1Acc29 infinity() {
    G1Acc29 a;
    a.x = a.y = a.zz = a.zzz = Fq29::zero();
    a.inf = true;
    return a;
  }
};

// 2 * (qx, qy), affine input with |limbs| < 2^29
ZK_HD void mdbl29(G1Acc29& acc, const Fq29& qx, const Fq29& qy) {
  const Fq29 u = norm(add(qy, qy));
  const Fq29 v = sqr(u);
  const Fq29 w = mul(u, v);
  const Fq29 s = mul(qx, v);
  const Fq29 x2 = sqr(qx);
  const Fq29 m = norm(add(add(x2, x2), x2));
  const Fq29 x3 = norm(sub(sqr(m), add(s, s)));
  const Fq29 y3 = norm(sub(mul(m, sub(s, x3)), mul(w, qy)));
  acc.x = x3;
  acc.y = y3;
  acc.zz = v;
  acc.zzz = w;
  acc.inf = false;
}

// acc += (qx, qy); the addend is a finite point, canonical x in [0,p), y possibly negated
// limb-wise (|limbs| < 2^29).
// The accumulator is loop-carried in the MSM kernels.  LLVM proves at IR level that its masked limbs
// are non-negative and rewrites their sign extensions as zero extensions, but instruction selection
// works per basic block and cannot see that proof: a product of such a limb with a signed limb is
// then expanded into two v_mad_u64_u32 plus two moves instead of one v_mad_i64_i32 (96 extra mads
// and 192 moves per G1 mixed addition).  Passing the limbs through an empty asm hides the range, so
// every product stays a signed 32 x 32 -> 64 multiply-add.
ZK_HD void opaque_limbs(Fq29& a) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
  for (int i = 0; i < 9; i++) asm volatile("" : "+v"(a.v[i]));
#endif
}

ZK_HD void madd29(G1Acc29& acc, const Fq29& qx, const Fq29& qy) {
#if !defined(__HIP_DEVICE_COMPILE__)
  opaque_limbs(acc.x);
  opaque_limbs(acc.y);
  opaque_limbs(acc.zz);
  opaque_limbs(acc.zzz);
#endif
  if (acc.inf) {
    acc.x = qx;
    acc.y = norm(qy);
    acc.zz = acc.zzz = Fq29::one();
    acc.inf = false;
    return;
  }
  const Fq29 u2 = mmul(qx, acc.zz);
  const Fq29 s2 = mmul(qy, acc.zzz);
  const Fq29 p = sub(u2, acc.x);  // |limbs| < 2^29, |value| < 6.5p
  const Fq29 r = sub(s2, acc.y);  // |value| < 3.5p
  const Fq29 pp = msqr(p);
  const Fq29 rr = msqr(r);
  if (is_zero_mulout(pp)) {  // same x: doubling or cancellation (never on honest random data)
    if (is_zero_mulout(rr))
      mdbl29(acc, qx, qy);
    else
      acc.inf = true;
    return;
  }
  const Fq29 ppp = mmul(p, pp);
  const Fq29 q = mmul(acc.x, pp);
  const Fq29 x3 = norm(sub(sub(rr, ppp), add(q, q)));  // (-5p, 3p)
  // y3 = r*(q - x3) - y1*ppp with ONE Montgomery reduction for both products (saves 90 of the
  // 342 mads and the normalisation); |r (q-x3)| + |y1 ppp| < 26 p^2, result in (-p/2, 3p/2)
  const Fq29 y3 = mmul_add2(r, sub(q, x3), neg(acc.y), ppp);
  acc.zz = mmul(acc.zz, pp);
  acc.zzz = mmul(acc.zzz, ppp);
  acc.x = x3;
  acc.y = y3;
}

// ---- G2 (Fq2 components, lazy reduction) -------------------------------------------------------
// ff29.h's Fq2 product and square on the products above
ZK_HD Fq2_29 mmul(const Fq2_29& a, const Fq2_29& b) {
  return {mmul_add2(a.c0, b.c0, neg(a.c1), b.c1), mmul_add2(a.c0, b.c1, a.c1, b.c0)};
}
ZK_HD Fq2_29 msqr(const Fq2_29& a) {
  return {mmul(add(a.c0, a.c1), sub(a.c0, a.c1)), mmul(add(a.c0, a.c0), a.c1)};
}

// Invariants between calls: x, y weakly reduced (|component| < 0.6p); zz, zzz products.
struct G2Acc29 {
  Fq2_29 x, y, zz, zzz;
  bool inf;
  static ZK_HD G2Acc29 infinity() {
    G2Acc29 a;
    a.x = a.y = a.zz = a.zzz = Fq2_29::zero();
    a.inf = true;
    return a;
  }
};

ZK_HD void mdbl29(G2Acc29& acc, const Fq2_29& qx, const Fq2_29& qy) {
  const Fq2_29 u = norm(add(qy, qy));
  const Fq2_29 v = sqr(u);
  const Fq2_29 w = mul(u, v);
  const Fq2_29 s = mul(qx, v);
  const Fq2_29 x2 = sqr(qx);
  const Fq2_29 m = norm(add(add(x2, x2), x2));
  const Fq2_29 x3 = wred(sub(sqr(m), add(s, s)));
  const Fq2_29 y3 = wred(sub(mul(m, sub(s, x3)), mul(w, qy)));
  acc.x = x3;
  acc.y = y3;
  acc.zz = v;
  acc.zzz = w;
  acc.inf = false;
}

// qx canonical components, qy canonical or limb-wise negated
ZK_HD void madd29(G2Acc29& acc, const Fq2_29& qx, const Fq2_29& qy) {
#if !defined(__HIP_DEVICE_COMPILE__)
  opaque_limbs(acc.x.c0);    // see the G1 madd29
  opaque_limbs(acc.x.c1);
  opaque_limbs(acc.y.c0);
  opaque_limbs(acc.y.c1);
  opaque_limbs(acc.zz.c0);
  opaque_limbs(acc.zz.c1);
  opaque_limbs(acc.zzz.c0);
  opaque_limbs(acc.zzz.c1);
#endif
  if (acc.inf) {
    acc.x = qx;
    acc.y = norm(qy);
    acc.zz = acc.zzz = Fq2_29::one();
    acc.inf = false;
    return;
  }
  const Fq2_29 u2 = mmul(qx, acc.zz);
  const Fq2_29 s2 = mmul(qy, acc.zzz);
  const Fq2_29 p = sub(u2, acc.x);  // |component| < 1.7p, |limb| < 2^29
  const Fq2_29 r = sub(s2, acc.y);
  const Fq2_29 pp = msqr(p);
  const Fq2_29 rr = msqr(r);
  if (is_zero_mulout(pp)) {
    if (is_zero_mulout(rr))
      mdbl29(acc, qx, qy);
    else
      acc.inf = true;
    return;
  }
  const Fq2_29 ppp = mmul(p, pp);
  const Fq2_29 q = mmul(acc.x, pp);
  const Fq2_29 x3 = wred(sub(sub(rr, ppp), add(q, q)));
  const Fq2_29 y3 = wred(sub(mmul(r, sub(q, x3)), mmul(acc.y, ppp)));
  acc.zz = mmul(acc.zz, pp);
  acc.zzz = mmul(acc.zzz, ppp);
  acc.x = x3;
  acc.y = y3;
}

ZK_HD G2XYZZ to_std(const G2Acc29& a) {
  if (a.inf) return G2XYZZ::inf();
  return G2XYZZ{to_std(a.x), to_std(a.y), to_std(a.zz), to_std(a.zzz)};
}

ZK_HD G1XYZZ to_std(const G1Acc29& a) {
  if (a.inf) return G1XYZZ::inf();
  return G1XYZZ{to_std(a.x), to_std(a.y), to_std(a.zz), to_std(a.zzz)};
}

// ---- sums of accumulators (the chunk reduction of the MSM) ----------------------------------------
// The accumulate kernels leave their chunk partials in the 2^261 domain: a Part29 holds x, y, zz and
// zzz as lazy memory images (ff29.h pack_lazy: a normalised value with |v| < 2^255 as a signed
// 256-bit integer), so neither side of the hand-over pays a domain change.  The word containers are
// Fq / Fq2 only to have the size and alignment of an XYZZ<F>; a Part29 is never a field element of
// ff.h.  Infinity: every word of zz zero (a finite point has zz != 0 mod p, and the image of a
// non-zero residue is never the integer 0).
// What is packed: x weakly reduced (|v| < 0.6p; canonical table values, 0 <= v < p, pass wred
// unchanged in range), y in (-p, 3p/2), zz and zzz products in (-p/2, 3p/2); all normalised.
template <class F>
struct Part29 {
  F x, y, zz, zzz;
};
static_assert(sizeof(Part29<Fq>) == sizeof(G1XYZZ) && sizeof(Part29<Fq2>) == sizeof(G2XYZZ),
              "a packed partial takes the place of an XYZZ");

ZK_HD void pack_lazy2(Fq2& w, const Fq2_29& a) {
  pack_lazy<Fq29Params>(w.c0.v, a.c0);
  pack_lazy<Fq29Params>(w.c1.v, a.c1);
}
ZK_HD Fq2_29 unpack_lazy2(const Fq2& w) {
  return {unpack_lazy<Fq29Params>(w.c0.v), unpack_lazy<Fq29Params>(w.c1.v)};
}

// G1: madd29 leaves |x| < 5p, which the image cannot hold: x goes through wred (a no-op in value
// for padd29's results, which are weakly reduced already)
ZK_HD Part29<Fq> pack_part(const G1Acc29& a) {
  Part29<Fq> r;
  if (a.inf) {
    r.x = r.y = r.zz = r.zzz = Fq::zero();
    return r;
  }
  pack_lazy<Fq29Params>(r.x.v, wred(a.x));
  pack_lazy<Fq29Params>(r.y.v, a.y);
  pack_lazy<Fq29Params>(r.zz.v, a.zz);
  pack_lazy<Fq29Params>(r.zzz.v, a.zzz);
  return r;
}
ZK_HD G1Acc29 unpack_part(const Part29<Fq>& w) {
  G1Acc29 a;
  a.inf = w.zz.is_zero();
  a.x = unpack_lazy<Fq29Params>(w.x.v);
  a.y = unpack_lazy<Fq29Params>(w.y.v);
  a.zz = unpack_lazy<Fq29Params>(w.zz.v);
  a.zzz = unpack_lazy<Fq29Params>(w.zzz.v);
  return a;
}
// G2: x and y are weakly reduced (or a table entry's components) after every step
ZK_HD Part29<Fq2> pack_part(const G2Acc29& a) {
  Part29<Fq2> r;
  if (a.inf) {
    r.x = r.y = r.zz = r.zzz = Fq2::zero();
    return r;
  }
  pack_lazy2(r.x, a.x);
  pack_lazy2(r.y, a.y);
  pack_lazy2(r.zz, a.zz);
  pack_lazy2(r.zzz, a.zzz);
  return r;
}
ZK_HD G2Acc29 unpack_part(const Part29<Fq2>& w) {
  G2Acc29 a;
  a.inf = w.zz.is_zero();
  a.x = unpack_lazy2(w.x);
  a.y = unpack_lazy2(w.y);
  a.zz = unpack_lazy2(w.zz);
  a.zzz = unpack_lazy2(w.zzz);
  return a;
}

ZK_HD Fq2_29 from_std(const Fq2& x) {
  return {from_std<Fq29Params>(x.c0), from_std<Fq29Params>(x.c1)};
}
// standard XYZZ -> accumulator (the results of from_std are products: within every bound above)
ZK_HD G1Acc29 from_std(const G1XYZZ& p) {
  if (p.is_inf()) return G1Acc29::infinity();
  G1Acc29 a;
  a.x = from_std<Fq29Params>(p.x);
  a.y = from_std<Fq29Params>(p.y);
  a.zz = from_std<Fq29Params>(p.zz);
  a.zzz = from_std<Fq29Params>(p.zzz);
  a.inf = false;
  return a;
}
ZK_HD G2Acc29 from_std(const G2XYZZ& p) {
  if (p.is_inf()) return G2Acc29::infinity();
  G2Acc29 a;
  a.x = from_std(p.x);
  a.y = from_std(p.y);
  a.zz = from_std(p.zz);
  a.zzz = from_std(p.zzz);
  a.inf = false;
  return a;
}

// acc += b, both accumulators (add-2008-s).  Operands as unpack_part or an earlier padd29 leaves
// them: x, y normalised with |x| < p, |y| < 3p/2; zz, zzz products, (-p/2, 3p/2).  The result keeps
// these bounds (x weakly reduced, y a product), so sums chain without limit: chunk sums, then
// group sums, then the common addend.
// Equal x (pp = 0: the same point twice, or a point and its negative) is left to ec.h.
ZK_HD void padd29(G1Acc29& acc, const G1Acc29& b) {
  if (b.inf) return;
  if (acc.inf) {
    acc = b;
    return;
  }
  const Fq29 u1 = mmul(acc.x, b.zz);    // |a b| < 1.5 p^2; every product below is in (-p/2, 3p/2)
  const Fq29 u2 = mmul(b.x, acc.zz);
  const Fq29 s1 = mmul(acc.y, b.zzz);   // < 2.25 p^2
  const Fq29 s2 = mmul(b.y, acc.zzz);
  const Fq29 p = sub(u2, u1);           // |limbs| < 2^29, |value| < 2p
  const Fq29 r = sub(s2, s1);           // the same
  const Fq29 pp = msqr(p);              // < 4 p^2
  if (is_zero_mulout(pp)) {
    G1XYZZ s = to_std(acc);
    padd(s, to_std(b));
    acc = from_std(s);
    return;
  }
  const Fq29 rr = msqr(r);
  const Fq29 ppp = mmul(p, pp);         // < 3 p^2
  const Fq29 q = mmul(u1, pp);          // < 2.25 p^2
  // rr - ppp - 2q in (-5p, 3p), limbs in (-3 * 2^29, 2^29): wred's range; |x3| < 0.6p
  const Fq29 x3 = wred(sub(sub(rr, ppp), add(q, q)));
  // one reduction for both products (madd29): |q - x3| < 2.1p, limbs a difference of normalised
  // values; |r (q - x3)| + |s1 ppp| < 4.2 p^2 + 2.25 p^2
  const Fq29 y3 = mmul_add2(r, sub(q, x3), neg(s1), ppp);
  acc.zz = mmul(mmul(acc.zz, b.zz), pp);
  acc.zzz = mmul(mmul(acc.zzz, b.zzz), ppp);
  acc.x = x3;
  acc.y = y3;
}

// G2: components of x, y normalised with |v| < p; of zz, zzz products.  An Fq2 product takes the
// sum of two component products, each < 64 p^2 / 2.  p and r are normalised before they are
// squared: msqr forms c0 + c1 and c0 - c1, and only one of the two may exceed 2^29 per limb.
ZK_HD void padd29(G2Acc29& acc, const G2Acc29& b) {
  if (b.inf) return;
  if (acc.inf) {
    acc = b;
    return;
  }
  const Fq2_29 u1 = mmul(acc.x, b.zz);    // 2 * 1.5 p^2; components of a product in (-p/2, 3p/2)
  const Fq2_29 u2 = mmul(b.x, acc.zz);
  const Fq2_29 s1 = mmul(acc.y, b.zzz);
  const Fq2_29 s2 = mmul(b.y, acc.zzz);
  const Fq2_29 p = norm(sub(u2, u1));     // |component| < 2p
  const Fq2_29 r = norm(sub(s2, s1));
  const Fq2_29 pp = msqr(p);              // (c0 + c1)(c0 - c1), 2 c0 c1: < 16 p^2
  if (is_zero_mulout(pp)) {
    G2XYZZ s = to_std(acc);
    padd(s, to_std(b));
    acc = from_std(s);
    return;
  }
  const Fq2_29 rr = msqr(r);
  const Fq2_29 ppp = mmul(p, pp);         // 2 * 3 p^2
  const Fq2_29 q = mmul(u1, pp);          // 2 * 2.25 p^2
  // components of rr - ppp - 2q in (-5p, 3p), limbs in (-3 * 2^29, 2^29); |x3| < 0.6p
  const Fq2_29 x3 = wred(sub(sub(rr, ppp), add(q, q)));
  // |q - x3| < 2.1p per component: 2 * 4.2 p^2 and 2 * 2.25 p^2; the difference of the two products
  // has |component| < 2p, |y3| < 0.6p
  const Fq2_29 y3 = wred(sub(mmul(r, sub(q, x3)), mmul(s1, ppp)));
  acc.zz = mmul(mmul(acc.zz, b.zz), pp);
  acc.zzz = mmul(mmul(acc.zzz, b.zzz), ppp);
  acc.x = x3;
  acc.y = y3;
}

}  // namespace zk
