// Host check of csrc/comb_sign.h, the map from the bits of a scalar image to the windows of a
// sign-pattern comb table, and of the two image-conversion constants of csrc/ff29.h.
// Arguments: scalars t as 64 hex digits.  Prints, per scalar, the signs C_0 .. C_253 followed by the
// parity e as 255 characters; then the constants as nine limbs each.  The arithmetic is checked by
// tests/test_native_comb_sign.py in Python integers.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "comb_sign.h"
#include "ff29.h"

using namespace zk;

static bool parse_hex(const char* s, uint32_t t[8]) {
  if (std::strlen(s) != 64) return false;
  for (int w = 0; w < 8; w++) {
    char buf[9];
    std::memcpy(buf, s + 8 * (7 - w), 8);
    buf[8] = 0;
    char* end;
    t[w] = (uint32_t)std::strtoul(buf, &end, 16);
    if (*end) return false;
  }
  return true;
}

int main(int argc, char** argv) {
  // every window but the constant one is fed by exactly one bit; bits 254 and 255 feed none
  int fed[255] = {};
  for (int w = 0; w < 8; w++)
    for (int b = 0; b < 32; b++) {
      bool comp;
      const int j = comb_sign_window(w, b, &comp);
      if (j >= 255 || j < -1) return 2;
      if (j < 0) {
        if (w * 32 + b < 254) return 3;
        continue;
      }
      if (comp != (j == COMB_SIGN_PARITY)) return 4;
      fed[j]++;
    }
  for (int j = 0; j < 255; j++)
    if (fed[j] != (j == COMB_SIGN_ONES ? 0 : 1)) return 5;
  std::printf("ok map\n");
  for (int a = 1; a < argc; a++) {
    uint32_t t[8];
    if (!parse_hex(argv[a], t)) return 6;
    char line[256];
    for (int j = 0; j < 255; j++) line[j] = (char)('0' + comb_sign_bit(t, j));
    line[255] = 0;
    std::printf("%s\n", line);
  }
  std::printf("c256");
  for (int i = 0; i < 9; i++) std::printf(" %d", Fr29Params::c256(i));
  std::printf("\nc266");
  for (int i = 0; i < 9; i++) std::printf(" %d", Fr29Params::c266(i));
  std::printf("\n");
  return 0;
}
