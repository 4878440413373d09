// splat_merge.h -- the ordered splat merge (BLING_SPLAT_ORDERED, include/bling.h): an unordered buffer
// of splat records becomes, for every pixel that has records, img[p] = (((img[p] + r0) + r1) + ...) per
// channel in binary32, the records taken in ascending key order -- the order in which the reference's one
// thread splats (LightTracer.hs:41-50, Metropolis.hs:96-104).  No float atomic anywhere: integer atomics
// count and claim slots, and nothing depends on their order.  splat_merge.hip holds the kernels:
//   k_sm_count     per-pixel histogram of the records (integer atomics)
//   k_sm_sums / k_sm_scan_sums / k_sm_starts   exclusive scan of the W * H counts (1 024 per block)
//   k_sm_scatter   every record's key and XYZ into its pixel's segment, in any order
//   k_sm_short     one lane per pixel: a segment of at most SM_SHORT records is added by selection (the
//                  smallest key not yet added, len^2 / 2 key reads, no store, no array); longer ones are listed
//   k_sm_long      one block per listed segment: all-ascending bitonic network over (key, position) in LDS up
//                  to SM_LDS_RECORDS records, over keys and values in place in global memory beyond; then
//                  the values are staged 256 at a time and three lanes (X, Y, Z) add them one by one
#pragma once
#include <cstdint>

#include "dev_common.h"

namespace bd {

constexpr uint32_t SM_SHORT = 32;            // longest segment the one-lane path takes
constexpr uint32_t SM_LDS_RECORDS = 4096;    // longest segment sorted in LDS (48 KB of keys and positions)

// Record layouts the merge reads, 2 uint4 each.
//   SM_LAYOUT_SPLAT  bling_splat_rec: pixel, pad, key lo, key hi | X, Y, Z, pad
//   SM_LAYOUT_LIGHT  k_lt_photon's record (light_tracer.h): photon, depth, sx, sy | X, Y, Z, pad;
//                    pixel = sy * W + sx, key = photon << 32 | depth
enum : int { SM_LAYOUT_SPLAT = 0, SM_LAYOUT_LIGHT = 1 };

// tag: the record's spare word, which the merge does not read
DEV void sm_write_rec(uint4* __restrict__ rec, size_t slot, uint32_t pixel, unsigned long long key, float x, float y, float z,
                      uint32_t tag = 0u) {
  rec[2 * slot] = make_uint4(pixel, tag, (uint32_t)key, (uint32_t)(key >> 32));
  rec[2 * slot + 1] = make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(z), 0u);
}

}  // namespace bd
