// Host check of csrc/bit_transpose.h: the 32 x 32 bit transpose of the comb digit pass and the
// digit of a sign-pattern window, against a bit-by-bit extraction written here.  For every group
// size k = 1 .. 21 a group of k scalars (eight words each) goes through the transpose the way
// comb_digits_kernel feeds it: unsigned, row i of the group is row i; signed, rows 0 .. k - 2 keep
// their places and row k - 1 is row 31.  Checked per word and bit: the window word, the unsigned
// digit, and the signed digit against the rule restated below (top bit set: entry M & low; clear:
// entry ~M & low with bit 31 set) on the pattern M that comb_sign.h's own comb_sign_bit gathers.
// Complemented windows and skipped bits come from comb_sign_window.  Prints one line per input
// class; any mismatch prints where and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "bit_transpose.h"
#include "comb_sign.h"

using namespace zk;

static constexpr int KSIGNED = 21, KUNSIGNED = 20;   // the kernel's two instantiations

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd32() {   // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}

static long checked = 0;

static void fail(const char* what, int k, int w, int bit, uint32_t got, uint32_t want) {
  std::printf("FAIL %s: k=%d word=%d bit=%d got=%08x want=%08x\n", what, k, w, bit, got, want);
  std::exit(1);
}

// bit q of a 256-bit scalar
static uint32_t sbit(const uint32_t t[8], int q) { return (t[q / 32] >> (q % 32)) & 1u; }

// comb_sign_bit(t, j) through a table of comb_sign_window's answers (comb_sign_bit itself walks
// all 256 bits per call); main() checks that the two agree
static int src_bit[255];
static bool src_comp[255];
static uint32_t sign_bit(const uint32_t t[8], int j) {
  if (j == COMB_SIGN_ONES) return 1u;
  return sbit(t, src_bit[j]) ^ (src_comp[j] ? 1u : 0u);
}

// one group of k scalars s[0 .. k-1]
static void check_group(int k, const uint32_t s[][8]) {
  const uint32_t low = (1u << (k - 1)) - 1u;
  for (int w = 0; w < 8; w++) {
    // ---- unsigned: rows in their order (the subset-sum kernel, k <= 20; 21 through its own size)
    uint32_t m[32];
    for (int i = 0; i < 32; i++) m[i] = i < k ? s[i][w] : (i < (k <= KUNSIGNED ? KUNSIGNED : 21) ? 0u : rnd32());
    if (k <= KUNSIGNED)
      bit_transpose32<KUNSIGNED, false>(m);
    else
      bit_transpose32<21, false>(m);
    for (int bit = 0; bit < 32; bit++) {
      uint32_t want = 0;
      for (int i = 0; i < k; i++) want |= ((s[i][w] >> bit) & 1u) << i;
      if (m[bit] != want) fail("unsigned window word", k, w, bit, m[bit], want);
      const int j = w * 32 + bit;   // the window of an unsigned table is the bit itself
      uint32_t digit = 0;
      for (int i = 0; i < k; i++) digit |= sbit(s[i], j) << i;
      if (m[bit] != digit) fail("unsigned digit", k, w, bit, m[bit], digit);
      checked++;
    }
    // ---- signed: the top row of the group at 31, the others below it; dead rows hold anything
    for (int i = 0; i < 32; i++) m[i] = i < k - 1 ? s[i][w] : (i < KSIGNED - 1 ? 0u : rnd32());
    m[31] = s[k - 1][w];
    bit_transpose32<KSIGNED - 1, true>(m);
    for (int bit = 0; bit < 32; bit++) {
      uint32_t want = 0;
      for (int i = 0; i < k - 1; i++) want |= ((s[i][w] >> bit) & 1u) << i;
      want |= ((s[k - 1][w] >> bit) & 1u) << 31;
      if (m[bit] != want) fail("signed window word", k, w, bit, m[bit], want);
      bool comp;
      const int j = comb_sign_window(w, bit, &comp);
      if (j < 0) continue;
      if (comp != (w == 0 && bit == 0)) fail("complement", k, w, bit, comp, w == 0 && bit == 0);
      const uint32_t got = comb_sign_digit(comp ? ~m[bit] : m[bit], low);
      // the pattern of window j, sign by sign, through comb_sign.h
      uint32_t M = 0;
      for (int i = 0; i < k; i++) M |= sign_bit(s[i], j) << i;
      const uint32_t rule = ((M >> (k - 1)) & 1u) ? (M & low) : ((~M & low) | 0x80000000u);
      if (got != rule) fail("signed digit", k, w, bit, got, rule);
      // and the pass's earlier expression on the word with the top row at bit k - 1
      uint32_t old = 0;
      for (int i = 0; i < k; i++) old |= ((s[i][w] >> bit) & 1u) << i;
      uint32_t idx = comp ? ~old : old;
      idx = ((idx >> (k - 1)) & 1u) ? (idx & low) : ((~idx & low) | 0x80000000u);
      if (got != idx) fail("signed digit (earlier form)", k, w, bit, got, idx);
      checked++;
    }
  }
  // window 253 is written as `low` without a transpose: the all-ones pattern under the rule
  uint32_t M = 0;
  for (int i = 0; i < k; i++) M |= comb_sign_bit(s[i], COMB_SIGN_ONES) << i;
  if (M != ((low << 1) | 1u) || (M & low) != low) fail("window of ones", k, 0, 0, M, low);
}

int main(int argc, char** argv) {
  const int n_random = argc > 1 ? std::atoi(argv[1]) : 150;   // per k
  static uint32_t s[21][8];
  for (int w = 0; w < 8; w++)
    for (int bit = 0; bit < 32; bit++) {
      bool comp;
      const int j = comb_sign_window(w, bit, &comp);
      if (j < 0) continue;
      src_bit[j] = w * 32 + bit;
      src_comp[j] = comp;
    }
  for (int it = 0; it < 16; it++) {
    uint32_t t[8];
    for (int w = 0; w < 8; w++) t[w] = it == 0 ? 0u : it == 1 ? ~0u : rnd32();
    for (int j = 0; j < 255; j++)
      if (sign_bit(t, j) != comb_sign_bit(t, j)) fail("sign table", 0, 0, j, sign_bit(t, j), comb_sign_bit(t, j));
  }
  // a full transpose: no dead row
  for (int it = 0; it < 64; it++) {
    uint32_t in[32], m[32];
    for (int i = 0; i < 32; i++) m[i] = in[i] = it == 0 ? 0u : it == 1 ? ~0u : rnd32();
    bit_transpose32<32, false>(m);
    for (int bit = 0; bit < 32; bit++) {
      uint32_t want = 0;
      for (int i = 0; i < 32; i++) want |= ((in[i] >> bit) & 1u) << i;
      if (m[bit] != want) fail("full transpose", 32, 0, bit, m[bit], want);
    }
  }
  std::printf("ok full\n");
  for (int k = 1; k <= 21; k++) {
    std::memset(s, 0, sizeof s);
    check_group(k, s);
    std::memset(s, 0xff, sizeof s);
    check_group(k, s);
    for (int r = 0; r < k; r++) {   // one-hot rows
      std::memset(s, 0, sizeof s);
      std::memset(s[r], 0xff, sizeof s[r]);
      check_group(k, s);
    }
    const int hot_rows[3] = {0, k / 2, k - 1};   // one-hot bits
    for (int h = 0; h < 3; h++)
      for (int q = 0; q < 256; q++) {
        std::memset(s, 0, sizeof s);
        s[hot_rows[h]][q / 32] = 1u << (q % 32);
        check_group(k, s);
      }
    for (int it = 0; it < n_random; it++) {
      for (int i = 0; i < k; i++)
        for (int w = 0; w < 8; w++) s[i][w] = rnd32();
      check_group(k, s);
    }
  }
  std::printf("ok groups k=1..21: %ld window words and digits\n", checked);
  return 0;
}
