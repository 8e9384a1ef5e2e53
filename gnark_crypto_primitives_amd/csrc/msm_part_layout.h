// Layout of one MSM partial-sum buffer (zkmi_ctx::msm_part[pb]) of the comb and shared-table launch
// routines (msm_impl.h PartView).  Host only, no HIP types: the element size is passed as a number
// (128 bytes for a G1 accumulator, 256 for G2), so that the offsets are tested without a GPU
// (tests/native/msm_part_layout_check.cpp, tests/test_native_msm_part_layout.py).
//
// Regions, in this order:
//   partial [W][chunks][Bp]   elements   chunk partials of the accumulate launch
//   mid     [W][ngroups][Bp]  elements   group sums of the two-level reduction
//   wsum    [W][Bp]           elements   window sums (unused when the caller takes them)
// and for comb tables (common_sums), everything else that the tail of the MSM reads:
//   usum    [W]               elements   common sums of the uniform groups
//   counts  [2]               u32        {|vlist|, |ulist|} of comb_split_kernel
//   d0      [W][G]            u32        lane 0's digits of the uniform groups
//   ulist   [G]               u32        the uniform groups
// The element regions come first, so each starts at a multiple of the element size whenever the
// buffer does; the u32 regions follow and are 4-byte aligned.
#pragma once
#include <cstddef>
#include <cstdint>

namespace zk {

enum {
  MSM_PART_PARTIAL = 0,
  MSM_PART_MID,
  MSM_PART_WSUM,
  MSM_PART_USUM,
  MSM_PART_COUNTS,
  MSM_PART_D0,
  MSM_PART_ULIST,
  MSM_PART_REGIONS
};

struct MsmPartLayout {
  size_t off[MSM_PART_REGIONS];    // byte offset of every region
  size_t size[MSM_PART_REGIONS];   // its bytes (0: not part of this layout)
  size_t align[MSM_PART_REGIONS];  // bytes of one of its items
  size_t bytes() const { return off[MSM_PART_REGIONS - 1] + size[MSM_PART_REGIONS - 1]; }
};

inline const char* msm_part_region_name(int r) {
  static const char* const names[MSM_PART_REGIONS] = {"partial", "mid",  "wsum", "usum",
                                                      "counts",  "d0",   "ulist"};
  return names[r];
}

// elem = bytes of one accumulator; G = comb groups of the MSM (ignored without common_sums)
inline MsmPartLayout msm_part_layout(size_t elem, size_t chunks, size_t ngroups, size_t W, size_t Bp,
                                     size_t G, bool common_sums) {
  MsmPartLayout l;
  const size_t u32 = sizeof(uint32_t);
  const size_t size[MSM_PART_REGIONS] = {chunks * W * Bp * elem,
                                         ngroups * W * Bp * elem,
                                         W * Bp * elem,
                                         common_sums ? W * elem : 0,
                                         common_sums ? 2 * u32 : 0,
                                         common_sums ? W * G * u32 : 0,
                                         common_sums ? G * u32 : 0};
  size_t at = 0;
  for (int r = 0; r < MSM_PART_REGIONS; r++) {
    l.off[r] = at;
    l.size[r] = size[r];
    l.align[r] = r <= MSM_PART_USUM ? elem : u32;
    at += size[r];
  }
  return l;
}

}  // namespace zk
