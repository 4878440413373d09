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
// sm_bitonic, that network, is defined here: the image API's tile segments (image_ops.hip) are sorted by it too.
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

// The all-ascending bitonic network over len elements as if padded with +inf to a power of two: a
// comparator whose upper element is padding does nothing, and every comparator puts the larger element
// at the higher index, so padding never moves.  X::cswap(lo, hi) orders one pair.
template <class X>
DEV void sm_bitonic(X& x, uint32_t len) {
  uint32_t P = 1;
  while (P < len) P <<= 1;
  const uint32_t half = P >> 1;
  for (uint32_t k = 2; k <= P; k <<= 1) {
    const uint32_t hk = k >> 1;
    for (uint32_t i = threadIdx.x; i < half; i += blockDim.x) {        // the two sorted halves, mirrored
      const uint32_t blk = i / hk, off = i - blk * hk;
      const uint32_t lo = blk * k + off, hi = blk * k + (k - 1u - off);
      if (hi < len) x.cswap(lo, hi);
    }
    __syncthreads();
    for (uint32_t j = k >> 2; j > 0; j >>= 1) {                        // half-cleaners
      for (uint32_t i = threadIdx.x; i < half; i += blockDim.x) {
        const uint32_t blk = i / j, off = i - blk * j;
        const uint32_t lo = blk * 2u * j + off, hi = lo + j;
        if (hi < len) x.cswap(lo, hi);
      }
      __syncthreads();
    }
  }
}

}  // namespace bd
