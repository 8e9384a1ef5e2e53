// Sign-pattern comb tables: from the bits of a scalar image to the windows of the digit pass
// (msm_impl.h comb_digits_kernel).  Host and device, so that the mapping is tested without a GPU.
//
// t < r < 2^254 is the canonical image the table was built for (msm_bases_build).  With e = 1 when
// t is even, t' = t + e = t | 1 is odd and C = ((t & ~1) + 2^254) >> 1 = (t' - 1 + 2^254) / 2 gives
//   t' = sum_{j < 254} (2 C_j - 1) 2^j,
// C_j = base's sign in window j.  The sum (t & ~1) + 2^254 has no carry, so C is t shifted down by
// one bit with bit 253 set: nothing is computed, the windows read t's own bits.
#pragma once
#include "ff.h"

namespace zk {

constexpr int COMB_SIGN_ONES = 253;     // window whose pattern is all ones (bit 254 of the sum)
constexpr int COMB_SIGN_PARITY = 254;   // correction window: the pattern of the parities e

// Window that bit `bit` of word `word` of t feeds, or -1 for the bits above t's range.
// *complement: the window takes the complement of the bit (the parity e = !t_0).
ZK_HD int comb_sign_window(int word, int bit, bool* complement) {
  const int q = word * 32 + bit;
  *complement = q == 0;
  if (q == 0) return COMB_SIGN_PARITY;
  if (q <= COMB_SIGN_ONES) return q - 1;   // C_j = t_(j+1), j <= 252
  return -1;                               // t < 2^254
}

// Sign of one scalar in window j < 255, through the mapping above (the host test's view of what
// the digit pass gathers bit by bit)
ZK_HD uint32_t comb_sign_bit(const uint32_t t[8], int j) {
  if (j == COMB_SIGN_ONES) return 1u;
  for (int w = 0; w < 8; w++)
    for (int b = 0; b < 32; b++) {
      bool comp;
      if (comb_sign_window(w, b, &comp) == j) return ((t[w] >> b) & 1u) ^ (comp ? 1u : 0u);
    }
  return 0u;
}

}  // namespace zk
