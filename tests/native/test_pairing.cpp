// Host driver of csrc/pairing.h for tests/test_native_pairing.py.  Reads commands from stdin, one per
// line, operands as hex strings of gnark's memory image (little-endian bytes, Montgomery form):
//   consts                      parameters, Frobenius constants, twist b, generators (plain integers)
//   pair P Q                    e(P, Q): 12 Fq coefficients, tower order c0.c0.c0 ... c1.c2.c1
//   prod2 P1 Q1 P2 Q2           1 when e(P1, Q1) e(P2, Q2) == 1
//   g2 Q                        "<on curve> <in subgroup>"
//   vk n K_0 .. K_(n-1) alpha beta gamma delta     1 when the key loads; it is kept for `verify`
//   verify PROOF PUBLICS        the decision of verify_one_host (PUBLICS may be "-" for none)
// Field elements are printed as hex integers out of Montgomery form.
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>

#include "pairing.h"

using namespace zk;

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoi(s.substr(i, 2), nullptr, 16));
  return out;
}
static std::vector<uint8_t> need(std::istringstream& in, size_t bytes) {
  std::string tok;
  in >> tok;
  std::vector<uint8_t> v = unhex(tok);
  if (v.size() != bytes) {
    fprintf(stderr, "operand of %zu bytes, want %zu\n", v.size(), bytes);
    exit(2);
  }
  return v;
}
static void print_fq(const Fq& a) {
  Fq x = from_mont(a);
  printf("0x");
  for (int i = 7; i >= 0; i--) printf("%08x", x.v[i]);
  printf(" ");
}
static void print_fq2(const Fq2& a) {
  print_fq(a.c0);
  print_fq(a.c1);
}
static void print_f12(const Fq12& a) {
  for (const Fq6* h : {&a.c0, &a.c1})
    for (const Fq2* c : {&h->c0, &h->c1, &h->c2}) print_fq2(*c);
  printf("\n");
}
static G1Affine g1_of(const std::vector<uint8_t>& v) {
  G1Affine p;
  memcpy(&p, v.data(), sizeof(p));
  return p;
}
static G2Affine g2_of(const std::vector<uint8_t>& v) {
  G2Affine p;
  memcpy(&p, v.data(), sizeof(p));
  return p;
}

int main() {
  static_assert(sizeof(G1Affine) == 64 && sizeof(G2Affine) == 128 && sizeof(Fq12) == 384, "images");
  PairingConsts pc;
  pairing_consts_init(pc);
  VkHost vk;
  bool have_vk = false;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    if (cmd == "consts") {
      printf("%llu %llu %d %d\n", (unsigned long long)BN_U, (unsigned long long)ATE_LO, ATE_BITS,
             ate_n_lines());
      for (const uint32_t* l : {HARD_L0, HARD_L1, HARD_L2}) printf("%u %u %u %u ", l[0], l[1], l[2], l[3]);
      printf("\n");
      for (int k = 0; k < 3; k++) {
        for (int i = 0; i < 6; i++) print_fq2(pc.frob[k][i]);
        printf("\n");
      }
      print_fq2(pc.twist_b);
      printf("\n");
      const G1Affine g1 = g1_generator();
      const G2Affine g2 = g2_generator();
      print_fq(g1.x);
      print_fq(g1.y);
      print_fq2(g2.x);
      print_fq2(g2.y);
      printf("\n");
    } else if (cmd == "pair") {
      const G1Affine p = g1_of(need(in, 64));
      const G2Affine q = g2_of(need(in, 128));
      Fq12 e;
      pairing(e, p, q, pc);
      print_f12(e);
    } else if (cmd == "prod2") {
      Fq12 e[2];
      for (int i = 0; i < 2; i++) {
        const G1Affine p = g1_of(need(in, 64));
        const G2Affine q = g2_of(need(in, 128));
        pairing(e[i], p, q, pc);
      }
      f12_mul(e[0], e[0], e[1]);
      printf("%d\n", f12_eq(e[0], f12_one()) ? 1 : 0);
    } else if (cmd == "g2") {
      const G2Affine q = g2_of(need(in, 128));
      printf("%d %d\n", g2_on_curve(q, pc) ? 1 : 0, g2_in_subgroup(q) ? 1 : 0);
    } else if (cmd == "vk") {
      uint32_t n = 0;
      in >> n;
      std::vector<uint8_t> k;
      for (uint32_t i = 0; i < n; i++) {
        std::vector<uint8_t> one = need(in, 64);
        k.insert(k.end(), one.begin(), one.end());
      }
      const std::vector<uint8_t> alpha = need(in, 64), beta = need(in, 128), gamma = need(in, 128),
                                 delta = need(in, 128);
      vk = VkHost();
      have_vk = vk_host_init(vk, n, k.data(), alpha.data(), beta.data(), gamma.data(), delta.data());
      printf("%d\n", have_vk ? 1 : 0);
    } else if (cmd == "verify") {
      if (!have_vk) {
        fprintf(stderr, "verify without a key\n");
        return 2;
      }
      const std::vector<uint8_t> proof = need(in, 256);
      const std::vector<uint8_t> pub = need(in, 32 * (vk.k.size() - 1));
      printf("%d\n", verify_one_host(vk, proof.data(), pub.data()) ? 1 : 0);
    } else {
      fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  printf("pairing driver ok\n");
  return 0;
}
