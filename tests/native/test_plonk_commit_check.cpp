// Host run of csrc/plonk_commit_check.h (tests/test_native_plonk_commit_check.py).  stdin:
//   n attached proved count
//   per commitment: n_rows row has_points lag_k, then its n_rows committed rows
// stdout: "validate: ok" or the refusal, then "auto_k: " for the point counts of the commitments.
#include <cstdio>
#include <iostream>
#include <vector>

#include "plonk_commit_check.h"

int main() {
  size_t n;
  int attached, proved;
  uint32_t count;
  if (!(std::cin >> n >> attached >> proved >> count)) return 2;
  std::vector<std::vector<uint32_t>> rows(count);
  std::vector<zk::PlonkCommitShape> shapes(count);
  for (uint32_t i = 0; i < count; i++) {
    uint32_t n_rows, row, lag_k;
    int has_points;
    if (!(std::cin >> n_rows >> row >> has_points >> lag_k)) return 2;
    rows[i].resize(n_rows);
    for (auto& r : rows[i])
      if (!(std::cin >> r)) return 2;
    shapes[i] = zk::PlonkCommitShape{n_rows, rows[i].data(), row, has_points != 0, lag_k};
  }
  const std::string bad = zk::plonk_commit_validate(
      shapes.data(), count, zk::PlonkCommitKeyState{n, attached != 0, proved != 0});
  printf("validate: %s\n", bad.empty() ? "ok" : bad.c_str());
  printf("auto_k:");
  for (uint32_t i = 0; i < count; i++) printf(" %u", zk::plonk_commit_auto_k(shapes[i].n_rows + 2));
  printf("\n");
  return 0;
}
