// Host build of csrc/scs_check.h, the loader checks of the PLONK witness entry.  Reads one case from
// standard input:
//   n_wires n_gates n_public log_n
//   n_gates x 3 wire indices (xa, then xb, then xc)
//   5 x n_gates selectors, 64 hex digits each (gnark's Montgomery image)
//   3 x 2^log_n permutation entries
// and prints what scs_validate, scs_perm_validate and scs_wiring_check say ("ok" for accepted), then
// the mark words of the gates.  Driven by tests/test_native_scs_check.py.
#include <cstdio>
#include <cstring>

#include "scs_check.h"

using namespace zk;

int main() {
  unsigned n_wires, n_gates, n_public, log_n;
  if (scanf("%u %u %u %u", &n_wires, &n_gates, &n_public, &log_n) != 4 || log_n > 24 ||
      n_gates > (1u << 25))
    return 2;
  const size_t n = (size_t)1 << log_n;
  std::vector<uint32_t> x[3], perm(3 * n), marks(n_gates);
  for (auto& col : x) {
    col.resize(n_gates);
    for (auto& v : col)
      if (scanf("%u", &v) != 1) return 2;
  }
  std::vector<Fr> sel((size_t)5 * n_gates);
  for (auto& s : sel) {
    char hex[80];
    if (scanf("%79s", hex) != 1 || strlen(hex) != 64) return 2;
    for (int w = 0; w < 8; w++) {
      char buf[9];
      memcpy(buf, hex + 8 * (7 - w), 8);
      buf[8] = 0;
      unsigned v;
      sscanf(buf, "%x", &v);
      s.v[w] = v;
    }
  }
  for (auto& v : perm)
    if (scanf("%u", &v) != 1) return 2;
  const ScsShape shape{n_wires, n_gates, n_public};
  const std::string e0 =
      scs_validate(shape, x[0].data(), x[1].data(), x[2].data(), sel.data(), marks.data());
  const std::string e1 = scs_perm_validate(perm.data(), n);
  // the loaders run the wiring check only on a system and a permutation they have accepted
  const std::string e2 = e0.empty() && e1.empty()
                             ? scs_wiring_check(shape, x[0].data(), x[1].data(), x[2].data(),
                                                perm.data(), n)
                             : "not run";
  printf("validate: %s\nperm: %s\nwiring: %s\nmarks:", e0.empty() ? "ok" : e0.c_str(),
         e1.empty() ? "ok" : e1.c_str(), e2.empty() ? "ok" : e2.c_str());
  if (e0.empty())
    for (uint32_t m : marks) printf(" %u", m);
  printf("\n");
  return 0;
}
