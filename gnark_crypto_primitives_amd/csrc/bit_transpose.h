// The 32 x 32 bit transpose of the comb digit pass (msm_impl.h comb_digits_kernel) and the digit of
// a sign-pattern window.  Host and device, so that both are tested without a GPU
// (tests/native/bit_transpose_check.cpp); nothing else knows how the window words come about.
//
// Rows are the scalar words of a group's bases, one row per base; afterwards word `bit` holds, in
// bit i, bit `bit` of row i: the pattern of the window that this bit of the scalars feeds.  Five
// butterfly stages of 16 swaps.  A swap of distance d exchanges, between rows a = m[r] and
// b = m[r + d], the bits of a whose position has bit d set with the bits of b whose position has
// it clear (M = the positions with bit d clear):
//   a' = (a & M) | ((b << d) & ~M),   b' = ((a >> d) & M) | (b & ~M).
// d = 16, 8 move whole half-words and bytes: one byte permute (v_perm_b32) per output.  d = 4, 2, 1:
// one shift and one bit-field insert (v_bfi_b32) per output.  Four instructions per swap, two in
// the first two stages, where the xor form t = ((a >> d) ^ b) & M, a ^= t << d, b ^= t takes six.
#pragma once
#include "ff.h"

namespace zk {

// v_perm_b32: byte i of the result is byte s_i of the eight bytes {hi, lo} (0 - 3: lo, 4 - 7: hi),
// s_i = byte i of sel
ZK_HD uint32_t bt_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(hi, lo, sel);
#else
  const uint64_t v = ((uint64_t)hi << 32) | lo;
  uint32_t r = 0;
  for (int i = 0; i < 4; i++)
    r |= (uint32_t)((v >> (8 * ((sel >> (8 * i)) & 7u))) & 0xffu) << (8 * i);
  return r;
#endif
}

// v_bfi_b32: a where mask is set, b elsewhere.  There is no builtin, and from the C++ form the
// compiler selects it for a third of the swaps only: it first moves the masks across the shifts
// and then finds and / or pairs.  So the device names the instruction; the mask is wave-uniform
// (the one scalar operand a VOP3 instruction may take), a and b are vector registers.
ZK_HD uint32_t bt_bfi(uint32_t mask, uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t r;
  asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "s"(mask), "v"(a), "v"(b));
  return r;
#else
  return (a & mask) | (b & ~mask);
#endif
}

// Transposes m in place.  Rows 0 .. NLOW - 1 are read, and row 31 when TOP is set; every other row
// counts as zero whatever it holds, at compile time, so that the first stage's swaps against such
// a row are a mask and a shift.  Every word of the result is live.
template <int NLOW, bool TOP>
ZK_HD void bit_transpose32(uint32_t m[32]) {
  static_assert(NLOW >= 0 && NLOW <= (TOP ? 31 : 32), "rows");
#define ZK_BT_LIVE(r) ((r) < NLOW || (TOP && (r) == 31))
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int r = 0; r < 16; r++) {   // distance 16: a' = {a.lo16, b.lo16}, b' = {a.hi16, b.hi16}
    const uint32_t a = ZK_BT_LIVE(r) ? m[r] : 0u;
    if (ZK_BT_LIVE(r + 16)) {
      const uint32_t b = m[r + 16];
      m[r] = bt_perm(b, a, 0x05040100u);
      m[r + 16] = bt_perm(b, a, 0x07060302u);
    } else {
      m[r] = a & 0xffffu;
      m[r + 16] = a >> 16;
    }
  }
#undef ZK_BT_LIVE
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < 16; i++) {   // distance 8: a' = {a0, b0, a2, b2}, b' = {a1, b1, a3, b3}
    const int r = ((i & 8) << 1) | (i & 7);
    const uint32_t a = m[r], b = m[r + 8];
    m[r] = bt_perm(b, a, 0x06020400u);
    m[r + 8] = bt_perm(b, a, 0x07030501u);
  }
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int t = 0; t < 3; t++) {
    const int d = 4 >> t;
    const uint32_t M = d == 4 ? 0x0f0f0f0fu : d == 2 ? 0x33333333u : 0x55555555u;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 16; i++) {   // the 16 rows whose index has bit d clear
      const int r = ((i & ~(d - 1)) << 1) | (i & (d - 1));
      const uint32_t a = m[r], b = m[r + d];
      m[r] = bt_bfi(M, a, b << d);
      m[r + d] = bt_bfi(M, a >> d, b);
    }
  }
}

// Digit of a sign-pattern window from its word x: bits 0 .. k - 2 are the pattern's low bits, bit
// 31 is its top bit T (row k - 1 of the group goes into the transpose as row 31), low = 2^(k-1) - 1;
// the bits between do not matter.  The rule (top bit set: entry M & low; clear: entry ~M & low,
// negated, which is bit 31 of the digit) with n = x >>arith 31 = -T:
//   ~(x ^ n)        = T ? x : ~x          one xnor: the entry, before the mask
//   (n + 1) << 31   = T ? 0 : 2^31        the negate flag (one add-shift)
//   digit = (~(x ^ n) & low) | ((n + 1) << 31)          (one and-or)
// No bit k - 1 is extracted.  A complemented window (comb_sign_window's *complement) passes ~x:
// its top bit and its low bits are the complements, and the bits between are masked off.
ZK_HD uint32_t comb_sign_digit(uint32_t x, uint32_t low) {
  const uint32_t n = (uint32_t)((int32_t)x >> 31);
  return (~(x ^ n) & low) | ((n + 1u) << 31);
}

}  // namespace zk
