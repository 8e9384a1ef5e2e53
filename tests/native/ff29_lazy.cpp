// Host test of the lazy memory image of csrc/ff29.h (pack_lazy / unpack_lazy), the code the NTT
// passes run on the GPU, against plain big-integer arithmetic.  Built with UBSan + ASan by
// tests/test_native_ff29_lazy.py; also
//   g++ -O1 -std=c++17 -fsanitize=undefined,address -I gnark_crypto_primitives_amd/csrc \
//       tests/native/ff29_lazy.cpp -o /tmp/t && /tmp/t
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "ff29.h"

using namespace zk;

static int fails = 0;
#define CHECK(c)                                            \
  do {                                                      \
    if (!(c)) {                                             \
      printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);    \
      fails++;                                              \
    }                                                       \
  } while (0)

// ---- a small signed big integer: 20 x 16-bit digits, two's complement, 320 bits ----------------
struct Big {
  int32_t d[20];   // digits in [0, 2^16) after fix(), the sign is digit 19's bit 15
};
static void fix(Big& x) {
  int64_t c = 0;
  for (int i = 0; i < 20; i++) {
    const int64_t t = (int64_t)x.d[i] + c;
    x.d[i] = (int32_t)(t & 0xffff);
    c = t >> 16;
  }
}
static Big big_zero() {
  Big r;
  for (int i = 0; i < 20; i++) r.d[i] = 0;
  return r;
}
static bool big_eq(const Big& a, const Big& b) {
  for (int i = 0; i < 20; i++)
    if (a.d[i] != b.d[i]) return false;
  return true;
}
static bool big_neg(const Big& a) { return (a.d[19] >> 15) & 1; }
// r += m * 2^sh for a 32-bit signed m
static void big_add_shifted(Big& r, int64_t m, int sh) {
  const int q = sh / 16, s = sh % 16;
  // m * 2^s fits 48 bits signed: spread over digits with a running carry
  int64_t v = m * ((int64_t)1 << s);
  for (int i = q; i < 20; i++) {
    r.d[i] += (int32_t)(v & 0xffff);
    v >>= 16;   // arithmetic: sign-extends to the top
  }
  fix(r);
}
static Big big_from_limbs(const Fr29& a) {   // sum v[i] 2^(29 i), any signed limbs
  Big r = big_zero();
  for (int i = 0; i < 9; i++) big_add_shifted(r, a.v[i], 29 * i);
  return r;
}
static Big big_from_words_signed(const uint32_t w[8]) {   // 256-bit two's complement
  Big r = big_zero();
  for (int i = 0; i < 8; i++) {
    r.d[2 * i] = (int32_t)(w[i] & 0xffff);
    r.d[2 * i + 1] = (int32_t)(w[i] >> 16);
  }
  const int32_t ext = (w[7] >> 31) ? 0xffff : 0;
  for (int i = 16; i < 20; i++) r.d[i] = ext;
  return r;
}
static Big big_r() {
  Fr29 p;
  for (int i = 0; i < 9; i++) p.v[i] = Fr29Params::p(i);
  return big_from_limbs(p);
}
static Big big_sub(const Big& a, const Big& b) {
  Big r;
  for (int i = 0; i < 20; i++) r.d[i] = a.d[i] - b.d[i];
  fix(r);
  return r;
}
static Big big_mul_small(const Big& a, int64_t k) {   // |k| < 2^31
  Big r = big_zero();
  int64_t c = 0;
  for (int i = 0; i < 20; i++) {
    // the digits are a (+ 2^320 if a is negative): mod 2^320 the plain product is right
    const int64_t t = (int64_t)a.d[i] * k + c;
    r.d[i] = (int32_t)(t & 0xffff);
    c = t >> 16;
  }
  return r;
}
// a == b mod r, for |a - b| below 2^9 r
static bool big_congruent(const Big& a, const Big& b) {
  const Big d = big_sub(a, b), r = big_r();
  for (int k = -512; k <= 512; k++)
    if (big_eq(d, big_mul_small(r, k))) return true;
  return false;
}

static bool normalised(const Fr29& a) {
  for (int i = 0; i < 8; i++)
    if (a.v[i] < 0 || a.v[i] > Fr29::MASK) return false;
  return true;
}

// the property: a normalised v with |v| < 2^255 survives the image limb for limb, and the image
// is v as a signed 256-bit integer
static void round_trip(const Fr29& v) {
  CHECK(normalised(v));
  uint32_t w[8];
  pack_lazy<Fr29Params>(w, v);
  const Fr29 u = unpack_lazy<Fr29Params>(w);
  for (int i = 0; i < 9; i++) CHECK(u.v[i] == v.v[i]);
  CHECK(big_eq(big_from_words_signed(w), big_from_limbs(v)));
}

static Fr29 r_times(int k) {   // k * r, normalised
  Fr29 x;
  int64_t c = 0;
  for (int i = 0; i < 8; i++) {
    c += (int64_t)k * Fr29Params::p(i);
    x.v[i] = (int32_t)(c & Fr29::MASK);
    c >>= 29;
  }
  x.v[8] = (int32_t)(c + (int64_t)k * Fr29Params::p(8));
  return x;
}
// the same value with every low limb moved by m * 2^29 (m = +-3: a limb of 2^29 - 1 becomes
// 2^31 - 1, a limb of 0 becomes -(2^31 - 2^29)), the way lazy additions leave them
static Fr29 spread(const Fr29& a, int m) {
  Fr29 x = a;
  for (int i = 0; i < 8; i++) {
    x.v[i] += m * (1 << 29);
    x.v[i + 1] -= m;
  }
  return x;
}

// wred's contract on x (|x| < 2^7 r, |limb| < 2^31), then the image of its output
static void wred_then_round_trip(const Fr29& x) {
  const Fr29 v = wred(x);
  CHECK(big_congruent(big_from_limbs(v), big_from_limbs(x)));
  // |v| < 0.6 r: 5 |v| < 3 r
  const Big r3 = big_mul_small(big_r(), 3), v5 = big_mul_small(big_from_limbs(v), 5);
  CHECK(big_neg(big_sub(v5, r3)));                          // 5 v < 3 r
  CHECK(big_neg(big_sub(big_mul_small(r3, -1), v5)));       // -3 r < 5 v
  round_trip(v);
}

int main() {
  std::mt19937_64 rng(2907);
  const int32_t M = Fr29::MASK;
  // zero, +-1
  {
    Fr29 z = Fr29::zero();
    round_trip(z);
    Fr29 one = z;
    one.v[0] = 1;
    round_trip(one);
    Fr29 m1;   // -1 normalised: low limbs all ones, limb 8 = -1
    for (int i = 0; i < 8; i++) m1.v[i] = M;
    m1.v[8] = -1;
    CHECK(big_eq(big_from_limbs(m1), big_sub(big_zero(), big_from_limbs(one))));
    round_trip(m1);
  }
  // limbs all 2^29 - 1, with every sign carrier wred can leave and the extremes of the image's
  // own range (limb 8 = +-2^22: |v| < 2^255)
  for (int32_t top : {0, 1, -1, 0x1d0a5c, -0x1d0a5c, (1 << 22) - 1, -(1 << 22)}) {
    Fr29 x;
    for (int i = 0; i < 8; i++) x.v[i] = M;
    x.v[8] = top;
    round_trip(x);
    for (int i = 0; i < 8; i++) x.v[i] = 0;
    round_trip(x);
  }
  // the extremes of wred's output range, both signs: the largest and smallest normalised values
  // with |v| < 0.6 r, i.e. +-(3 r / 5) rounded towards zero, and the same next to zero
  {
    // 3 r / 5 by long division on 16-bit digits
    Big r3 = big_mul_small(big_r(), 3), q = big_zero();
    int64_t rem = 0;
    for (int i = 19; i >= 0; i--) {
      const int64_t cur = rem * 65536 + r3.d[i];
      q.d[i] = (int32_t)(cur / 5);
      rem = cur % 5;
    }
    for (int sign = 0; sign < 2; sign++) {
      Big v = sign ? big_sub(big_zero(), q) : q;
      Fr29 x;   // normalised limbs of v: 29 bits at a time, the rest (signed) in limb 8
      for (int i = 0; i < 9; i++) {
        int64_t limb = 0;
        for (int bit = 0; bit < (i < 8 ? 29 : 32); bit++) {
          const int at = 29 * i + bit;
          limb |= (int64_t)((v.d[at / 16] >> (at % 16)) & 1) << bit;
        }
        x.v[i] = (int32_t)(uint32_t)limb;
      }
      CHECK(big_eq(big_from_limbs(x), v));
      round_trip(x);
    }
  }
  // wred on +-(24 r), the most a first pass leaves once unit products are skipped, and on
  // +-(2^7 r - 1), the ends of its contract: normalised and with the limbs spread to both ends
  for (int k : {24, -24, 128, -128, 23, 1, -1, 0}) {
    Fr29 x = r_times(k);
    if (k == 128 || k == -128) {   // +-(2^7 r - 1): the low limb of 2^7 r is 2^7, no borrow
      x.v[0] -= k > 0 ? 1 : -1;
      CHECK(normalised(x));
    }
    for (int m : {0, 3, -3}) {
      const Fr29 y = spread(x, m);
      CHECK(big_eq(big_from_limbs(y), big_from_limbs(x)));
      wred_then_round_trip(y);
    }
  }
  // wred with limbs at +-(2^31 - 1): every low limb at the end of an int32, limb 8 chosen so that
  // the value stays inside +-2^7 r (r's top limb is 0x30644e: |limb 8| <= 2^7 * 0x30644e - 8)
  for (int32_t lowlimb : {INT32_MAX, -INT32_MAX})
    for (int32_t top : {0, 128 * 0x30644e - 8, -(128 * 0x30644e - 8), 24 * 0x30644e, -24 * 0x30644e}) {
      Fr29 x;
      for (int i = 0; i < 8; i++) x.v[i] = lowlimb;
      x.v[8] = top;
      wred_then_round_trip(x);
      for (int i = 0; i < 8; i++) x.v[i] = (i & 1) ? lowlimb : -lowlimb;
      wred_then_round_trip(x);
    }
  // random butterfly-like sums in the contract
  for (int it = 0; it < 20000; it++) {
    Fr29 x;
    for (int i = 0; i < 8; i++) {   // any int32 with |limb| < 2^31
      x.v[i] = (int32_t)(uint32_t)rng();
      if (x.v[i] == INT32_MIN) x.v[i] = -INT32_MAX;
    }
    x.v[8] = (int32_t)(rng() % (2 * 120 * 0x30644e)) - 120 * 0x30644e;
    wred_then_round_trip(x);
  }
  // canonical values read through unpack_lazy are what unpack29 gives: 0, 1, r - 1, random < r
  {
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto same = [&]() {
      const Fr29 a = unpack_lazy<Fr29Params>(w), b = unpack29<Fr29Params>(w);
      for (int i = 0; i < 9; i++) CHECK(a.v[i] == b.v[i]);
      CHECK(normalised(a) && a.v[8] >= 0);
    };
    same();
    w[0] = 1;
    same();
    for (int i = 0; i < 8; i++) w[i] = FrParams::p(i);
    w[0] -= 1;   // r - 1 (the low word of r is 0xf0000001)
    same();
    // and it is the image pack_lazy gives r - 1
    uint32_t w2[8];
    pack_lazy<Fr29Params>(w2, unpack29<Fr29Params>(w));
    for (int i = 0; i < 8; i++) CHECK(w2[i] == w[i]);
    for (int it = 0; it < 2000; it++) {
      for (int i = 0; i < 8; i++) w[i] = (uint32_t)rng();
      w[7] &= 0x2fffffffu;   // < r
      same();
    }
  }
  printf(fails ? "ff29 lazy image tests FAILED (%d)\n" : "ff29 lazy image tests ok\n", fails);
  return fails != 0;
}
