// Host-side test of csrc/ec29.h padd29 and the packed partials (pack_part / unpack_part) against
// csrc/ec.h padd, G1 and G2.  Built with -fsanitize=undefined,address: a signed overflow inside
// the documented bounds ends the program.
//   g++ -O1 -std=c++17 -fsanitize=undefined,address -fno-sanitize-recover=all \
//       -I gnark_crypto_primitives_amd/csrc tests/native/test_ec29_padd.cpp -o /tmp/t && /tmp/t
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "ec29.h"

using namespace zk;

static std::mt19937_64 rng(20261);
static int fails = 0;
#define CHECK(c)                                            \
  do {                                                      \
    if (!(c)) {                                             \
      printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);    \
      fails++;                                              \
    }                                                       \
  } while (0)

static Fq k261() {
  Fq k;
  for (int i = 0; i < 8; i++) k.v[i] = Fq29Params::k261(i);
  return k;
}
// table image of an affine point: canonical coordinates in the 2^261 domain, y negated limb-wise
static void entry(const G1Affine& q, bool negd, Fq29& x, Fq29& y) {
  const Fq kx = mul(q.x, k261()), ky = mul(q.y, k261());
  x = unpack29<Fq29Params>(kx.v);
  y = cneg(unpack29<Fq29Params>(ky.v), negd);
}
static void entry(const G2Affine& q, bool negd, Fq2_29& x, Fq2_29& y) {
  const Fq2 kx{mul(q.x.c0, k261()), mul(q.x.c1, k261())}, ky{mul(q.y.c0, k261()), mul(q.y.c1, k261())};
  x = unpack2_29(kx);
  y = cneg(unpack2_29(ky), negd);
}

template <class F> struct Types;
template <> struct Types<Fq> { typedef G1Acc29 Acc; };
template <> struct Types<Fq2> { typedef G2Acc29 Acc; };

// a partial as an accumulate kernel leaves it and the reference sum of the same additions
template <class F>
struct Sum {
  Part29<F> packed;
  XYZZ<F> ref;
};

template <class F>
static void add_entry(Sum<F>& s, typename Types<F>::Acc& acc, const Affine<F>& q, bool negd) {
  decltype(acc.x) x, y;
  entry(q, negd, x, y);
  madd29(acc, x, y);
  Affine<F> qs = q;
  if (negd) qs.y = neg(q.y);
  madd(s.ref, qs);
}

// sum of `steps` random table entries; flip: every sign reversed (the negative of the same walk)
template <class F>
static Sum<F> walk(const std::vector<Affine<F>>& pts, int steps, uint64_t seed, bool flip = false) {
  std::mt19937_64 r(seed);
  Sum<F> s;
  s.ref = XYZZ<F>::inf();
  typename Types<F>::Acc acc = Types<F>::Acc::infinity();
  for (int i = 0; i < steps; i++) {
    const Affine<F>& q = pts[r() % pts.size()];
    const bool negd = (r() & 1) != 0;
    add_entry(s, acc, q, negd != flip);
  }
  s.packed = pack_part(acc);
  return s;
}

// the packed sum equals the reference: infinity flags, and the affine points
template <class F>
static bool same(const Part29<F>& packed, const XYZZ<F>& ref) {
  const typename Types<F>::Acc a = unpack_part(packed);
  if (a.inf != packed.zz.is_zero()) return false;
  if (a.inf != ref.is_inf()) return false;
  if (a.inf) return true;
  const Affine<F> p1 = to_affine(to_std(a)), p2 = to_affine(ref);
  return p1.x == p2.x && p1.y == p2.y;
}

// a + b through the packed images, as one msm_reduce step does
template <class F>
static Sum<F> sum(const Sum<F>& a, const Sum<F>& b) {
  typename Types<F>::Acc acc = unpack_part(a.packed);
  padd29(acc, unpack_part(b.packed));
  Sum<F> s;
  s.packed = pack_part(acc);
  s.ref = a.ref;
  padd(s.ref, b.ref);
  return s;
}

template <class F>
static void run(const Affine<F>& gen, const char* name) {
  std::vector<Affine<F>> pts;
  {
    XYZZ<F> a = XYZZ<F>::inf();
    for (int i = 0; i < 16; i++) {
      madd(a, gen);
      if (i % 3 == 2) a = dbl(a);
      pts.push_back(to_affine(a));
    }
  }
  Sum<F> inf;
  inf.packed = pack_part(Types<F>::Acc::infinity());
  inf.ref = XYZZ<F>::inf();
  CHECK(inf.packed.zz.is_zero());
  // sums of 1..40 mixed additions on both sides: zz, zzz are not 1 and the limbs are lazy
  for (int n1 = 1; n1 <= 40; n1++)
    for (int n2 = 1; n2 <= 40; n2 += (n1 % 4 == 0 ? 1 : 7)) {
      const Sum<F> a = walk<F>(pts, n1, 1000 * n1 + n2), b = walk<F>(pts, n2, 77000 + 1000 * n2 + n1);
      CHECK(same(a.packed, a.ref) && same(b.packed, b.ref));
      const Sum<F> s = sum(a, b);
      CHECK(same(s.packed, s.ref));
    }
  for (int n = 1; n <= 40; n += 3) {
    const Sum<F> a = walk<F>(pts, n, 5000 + n);
    if (a.ref.is_inf()) continue;
    // P + P: the same image twice, and the same point with zz = 1
    Sum<F> s = sum(a, a);
    CHECK(!s.ref.is_inf() && same(s.packed, s.ref));
    Sum<F> aff;
    aff.ref = XYZZ<F>::inf();
    typename Types<F>::Acc one = Types<F>::Acc::infinity();
    add_entry(aff, one, to_affine(a.ref), false);
    aff.packed = pack_part(one);
    s = sum(a, aff);
    CHECK(!s.ref.is_inf() && same(s.packed, s.ref));
    s = sum(aff, a);
    CHECK(same(s.packed, s.ref));
    // P + (-P): the walk with every sign reversed, and the affine negative
    const Sum<F> m = walk<F>(pts, n, 5000 + n, true);
    s = sum(a, m);
    CHECK(s.ref.is_inf() && same(s.packed, s.ref));
    Sum<F> naff;
    naff.ref = XYZZ<F>::inf();
    one = Types<F>::Acc::infinity();
    add_entry(naff, one, to_affine(a.ref), true);
    naff.packed = pack_part(one);
    s = sum(a, naff);
    CHECK(s.ref.is_inf() && same(s.packed, s.ref));
    // infinity on either side
    s = sum(inf, a);
    CHECK(same(s.packed, a.ref));
    s = sum(a, inf);
    CHECK(same(s.packed, a.ref));
  }
  {
    const Sum<F> s = sum(inf, inf);
    CHECK(s.packed.zz.is_zero() && same(s.packed, s.ref));
  }
  // 64 consecutive sums on packed intermediates (chunk sums, group sums, the common addend), with
  // an infinity, a doubling and a cancellation on the way
  for (int trial = 0; trial < 4; trial++) {
    Sum<F> acc = walk<F>(pts, 1 + trial * 13, 9000 + trial);
    for (int i = 0; i < 64; i++) {
      Sum<F> b = walk<F>(pts, 1 + (int)(rng() % 40), 9100 + 100 * trial + i);
      if (i == 20) b = inf;
      if (i == 30) b = acc;
      if (i == 40 && trial == 1) b = walk<F>(pts, 0, 0);
      acc = sum(acc, b);
      CHECK(same(acc.packed, acc.ref));
    }
    // ... and back to nothing: minus the whole sum, as an affine entry
    if (!acc.ref.is_inf()) {
      Sum<F> neg_all;
      neg_all.ref = XYZZ<F>::inf();
      typename Types<F>::Acc one = Types<F>::Acc::infinity();
      add_entry(neg_all, one, to_affine(acc.ref), true);
      neg_all.packed = pack_part(one);
      acc = sum(acc, neg_all);
      CHECK(acc.ref.is_inf() && same(acc.packed, acc.ref));
    }
  }
  printf("%s: %s\n", name, fails ? "FAILED" : "ok");
}

int main() {
  run<Fq>(G1Affine{Fq::one(), dbl(Fq::one())}, "g1");   // (1, 2)
  // G2 generator (plain integers -> Montgomery)
  const Fq gx0 = to_mont(Fq{{0xd992f6edu, 0x46debd5cu, 0xf75edaddu, 0x674322d4u, 0x5e5c4479u,
                             0x426a0066u, 0x121f1e76u, 0x1800deefu}});
  const Fq gx1 = to_mont(Fq{{0xaef312c2u, 0x97e485b7u, 0x35a9e712u, 0xf1aa4933u, 0x31fb5d25u,
                             0x7260bfb7u, 0x920d483au, 0x198e9393u}});
  const Fq gy0 = to_mont(Fq{{0x66fa7daau, 0x4ce6cc01u, 0x0c43d37bu, 0xe3d1e769u, 0x8dcb408fu,
                             0x4aab7180u, 0xdb8c6debu, 0x12c85ea5u}});
  const Fq gy1 = to_mont(Fq{{0xd122975bu, 0x55acdadcu, 0x70b38ef3u, 0xbc4b3133u, 0x690c3395u,
                             0xec9e99adu, 0x585ff075u, 0x090689d0u}});
  run<Fq2>(G2Affine{Fq2{gx0, gx1}, Fq2{gy0, gy1}}, "g2");
  printf(fails ? "ec29 padd tests FAILED (%d)\n" : "ec29 padd tests ok\n", fails);
  return fails != 0;
}
