// Host run of csrc/ff29.h's forms on an operand file written by tests/ff29_ref.py
// (write_operand_file): records of int32 {field, op, arity, n} followed by n x arity x 9 raw limbs,
// op numbered as zkmi_ff29_op.  Prints one line of nine integers per element.  An asm form runs
// as the C++ form it restates; mul_asm_s takes its b operand from element 64 * (i / 64).
//   g++ -O1 -g -std=c++17 -fsanitize=undefined,address -fno-sanitize-recover=all \
//       -I gnark_crypto_primitives_amd/csrc tests/native/ff29_ops.cpp -o ff29_ops && ./ff29_ops FILE
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ff29.h"

using namespace zk;

template <class P>
static F29<P> ld(const int32_t* p) {
  F29<P> r;
  for (int l = 0; l < 9; l++) r.v[l] = p[l];
  return r;
}

template <class P>
static int run(int op, int arity, const int32_t* in, size_t n) {
  for (size_t i = 0; i < n; i++) {
    const int32_t* e = in + i * arity * 9;
    const F29<P> a = ld<P>(e);
    F29<P> r = F29<P>::zero();
    uint32_t w[8];
    bool image = false;
    switch (op) {
      case 0: case 4: r = mul(a, ld<P>(e + 9)); break;
      case 7: r = mul_ilp(a, ld<P>(e + 9)); break;
      case 3: r = mul(a, ld<P>(in + (i - i % 64) * 18 + 9)); break;
      case 1: case 5: r = sqr(a); break;
      case 2: case 6: r = mul_add2(a, ld<P>(e + 9), ld<P>(e + 18), ld<P>(e + 27)); break;
      case 8: pack_canonical<P>(w, wred(a)); image = true; break;
      case 9: pack_canonical<P>(w, a); image = true; break;
      default: return 1;
    }
    if (image)
      printf("%u %u %u %u %u %u %u %u 0\n", w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]);
    else
      printf("%d %d %d %d %d %d %d %d %d\n", r.v[0], r.v[1], r.v[2], r.v[3], r.v[4], r.v[5],
             r.v[6], r.v[7], r.v[8]);
  }
  return 0;
}

int main(int argc, char** argv) {
  static const int arity_of[10] = {2, 1, 4, 2, 2, 1, 4, 2, 1, 1};
  FILE* f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
  if (!f) {
    fprintf(stderr, "usage: ff29_ops OPERAND_FILE\n");
    return 2;
  }
  int32_t h[4];
  while (fread(h, 4, 4, f) == 4) {
    if (h[0] < 0 || h[0] > 1 || h[1] < 0 || h[1] > 9 || h[2] != arity_of[h[1]] || h[3] < 0) {
      fprintf(stderr, "bad record header\n");
      return 2;
    }
    std::vector<int32_t> in((size_t)h[3] * h[2] * 9);
    if (fread(in.data(), 4, in.size(), f) != in.size()) {
      fprintf(stderr, "short record\n");
      return 2;
    }
    if (h[0] == 0 ? run<Fr29Params>(h[1], h[2], in.data(), h[3])
                  : run<Fq29Params>(h[1], h[2], in.data(), h[3]))
      return 2;
  }
  fclose(f);
  return 0;
}
