// Host check of csrc/msm_part_layout.h, the layout of an MSM partial-sum buffer.
// Arguments: elem chunks ngroups W Bp G common_sums, repeated for as many layouts as wanted.
// Prints, per layout, one line per region
//   <elem> <chunks> <ngroups> <W> <Bp> <G> <common> <region> <offset> <size> <align>
// and one line "... bytes <total>".  A layout of at most 16 MiB is also laid out in memory: every
// region is filled with its own number and read back after all are written, so that the sanitized
// build sees a region that overlaps another or runs past bytes().
// tests/test_native_msm_part_layout.py checks order, disjointness and alignment from the lines.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "msm_part_layout.h"

using namespace zk;

int main(int argc, char** argv) {
  if (argc < 8 || (argc - 1) % 7 != 0) return 2;
  for (int a = 1; a < argc; a += 7) {
    size_t v[7];
    for (int i = 0; i < 7; i++) v[i] = (size_t)std::strtoull(argv[a + i], nullptr, 10);
    const MsmPartLayout l = msm_part_layout(v[0], v[1], v[2], v[3], v[4], v[5], v[6] != 0);
    for (int r = 0; r < MSM_PART_REGIONS; r++)
      std::printf("%zu %zu %zu %zu %zu %zu %zu %s %zu %zu %zu\n", v[0], v[1], v[2], v[3], v[4], v[5],
                  v[6], msm_part_region_name(r), l.off[r], l.size[r], l.align[r]);
    std::printf("%zu %zu %zu %zu %zu %zu %zu bytes %zu\n", v[0], v[1], v[2], v[3], v[4], v[5], v[6],
                l.bytes());
    if (l.bytes() > ((size_t)16 << 20)) continue;
    unsigned char* buf = (unsigned char*)std::malloc(l.bytes());
    if (!buf) return 3;
    for (int r = 0; r < MSM_PART_REGIONS; r++) std::memset(buf + l.off[r], r + 1, l.size[r]);
    for (int r = 0; r < MSM_PART_REGIONS; r++)
      for (size_t i = 0; i < l.size[r]; i++)
        if (buf[l.off[r] + i] != r + 1) {
          std::printf("region %s overwritten at byte %zu\n", msm_part_region_name(r), i);
          return 1;
        }
    std::free(buf);
  }
  return 0;
}
