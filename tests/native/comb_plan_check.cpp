// Host check of csrc/comb_plan.h, the search for the comb group size of each MSM of a proving key.
// Arguments: n_a n_b1 n_k n_z n_b2 budget_bytes allow_signed phi guard.  Prints two lines,
//   equal  k*5 sg*5 fits bytes cost(1)
//   search k*5 sg*5 fits bytes cost(1) cost(phi)
// for the equal-k plan and the searched one.  tests/test_native_comb_plan.py recomputes bytes and
// costs in Python and checks the properties of the search.
#include <cstdio>
#include <cstdlib>

#include "comb_plan.h"

using namespace zk;

static void print_plan(const char* name, const size_t n[5], const CombPlan& p) {
  std::printf("%s", name);
  for (int i = 0; i < COMB_PLAN_MSMS; i++) std::printf(" %d", p.k[i]);
  for (int i = 0; i < COMB_PLAN_MSMS; i++) std::printf(" %d", p.sg[i] ? 1 : 0);
  std::printf(" %d %.0f %.6f", p.fits ? 1 : 0, comb_plan_bytes(n, p), comb_plan_cost(n, p, 1.0));
}

int main(int argc, char** argv) {
  if (argc != 10) return 2;
  size_t n[COMB_PLAN_MSMS];
  for (int i = 0; i < COMB_PLAN_MSMS; i++) n[i] = (size_t)std::strtoull(argv[1 + i], nullptr, 10);
  const double budget = std::strtod(argv[6], nullptr);
  const bool allow_signed = std::atoi(argv[7]) != 0;
  const double phi = std::strtod(argv[8], nullptr), guard = std::strtod(argv[9], nullptr);
  const CombPlan eq = comb_plan_equal5(n, budget, allow_signed);
  print_plan("equal", n, eq);
  std::printf("\n");
  const CombPlan p = comb_plan_search(n, budget, allow_signed, phi, guard);
  print_plan("search", n, p);
  std::printf(" %.6f\n", comb_plan_cost(n, p, phi));
  return 0;
}
