// lbvh.h -- the linear BVH (Morton order + common-prefix hierarchy, Karras 2012) stated once for the
// device builder (core/bvh_device.hip) and its CPU restatement (host/lbvh_host.cpp, bling_host_lbvh):
// the key, its quantisation, the delta function, a node's range and split, and the box padding.
// Both sides compile these expressions without multiply-add contraction, so the two trees agree bit
// for bit.  The tree depends on nothing but the items: keys are unique (the item index is their low
// word), min / max / integer sums do not depend on the order they are formed in.
//
//   centre   c = lo + (hi - lo) * 0.5f per axis; cmin / cmax = their bounds over all items
//   key      q = min(1023, (uint32_t)((c - cmin) * (1024 / ext))) per axis (0 where ext <= 0), the
//            three interleaved to a 30-bit Morton code m; key = m << 32 | item index
//   order    ascending key
//   node i   (0 <= i < n - 1) covers the sorted positions [first, last] that node_range finds from
//            delta(i, j) = clz(key_i ^ key_j) (-1 outside the array) and splits behind `split`
//   leaves   a range of one or two items is a leaf: ~(first << 8 | count), refs in sorted order
//   emit     the nodes whose range holds three items or more, numbered ascending in i (root = 0),
//            16 floats each: the two child boxes widened by pad_box, the two links, two zero words
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BLBVH_FN __host__ __device__ __forceinline__
#else
#include <cmath>
#define BLBVH_FN static inline
#endif

namespace blbvh {

constexpr int kDepthCap = 31;                     // STACK_DEPTH - 1 of the traversal kernels
constexpr uint32_t kMaxItems = 1u << 24;          // a leaf code holds first < 2^24

BLBVH_FN float centre(float lo, float hi) { return lo + (hi - lo) * 0.5f; }

// 1024 / ext, or 0 for an axis without extent (every item then quantises to 0)
BLBVH_FN float axis_scale(float cmin, float cmax) {
  const float ext = cmax - cmin;
  return ext > 0.f ? 1024.f / ext : 0.f;
}

// min(1023, (uint32_t)((c - cmin) * scale)); a product that is no number below 1023 (an overflowed
// scale times zero) takes 1023 as well, so the conversion is defined for every input
BLBVH_FN uint32_t quantise(float c, float cmin, float scale) {
  if (!(scale > 0.f)) return 0u;
  const float f = (c - cmin) * scale;
  return f < 1023.f ? (uint32_t)f : 1023u;
}

// the 10 low bits of v, two zero bits between each
BLBVH_FN uint32_t spread10(uint32_t v) {
  v &= 0x3FFu;
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

BLBVH_FN uint32_t morton30(uint32_t qx, uint32_t qy, uint32_t qz) {
  return (spread10(qx) << 2) | (spread10(qy) << 1) | spread10(qz);
}

// box: lo.xyz, hi.xyz; cb: cmin.xyz, then the three axis scales
BLBVH_FN uint64_t make_key(const float* box, const float* cmin, const float* scale, uint32_t index) {
  uint32_t q[3];
  for (int a = 0; a < 3; ++a) q[a] = quantise(centre(box[a], box[3 + a]), cmin[a], scale[a]);
  return ((uint64_t)morton30(q[0], q[1], q[2]) << 32) | (uint64_t)index;
}

// length of the common prefix of keys i and j, -1 for a j outside [0, n)
BLBVH_FN int delta(const uint64_t* keys, uint32_t n, uint32_t i, int64_t j) {
  if (j < 0 || j >= (int64_t)n) return -1;
  return __builtin_clzll(keys[i] ^ keys[(uint32_t)j]);    // keys are unique: never 0
}

// internal node i of n sorted keys (n >= 2): its range [first, last] and the position `split` its left
// child ends at (the right one starts at split + 1)
BLBVH_FN void node_range(const uint64_t* keys, uint32_t n, uint32_t i, uint32_t* first, uint32_t* last, uint32_t* split) {
  const int d = delta(keys, n, i, (int64_t)i + 1) > delta(keys, n, i, (int64_t)i - 1) ? 1 : -1;
  const int dmin = delta(keys, n, i, (int64_t)i - d);
  int64_t lmax = 2;
  while (delta(keys, n, i, (int64_t)i + lmax * d) > dmin) lmax *= 2;
  int64_t l = 0;
  for (int64_t t = lmax / 2; t >= 1; t /= 2)
    if (delta(keys, n, i, (int64_t)i + (l + t) * d) > dmin) l += t;
  const int64_t j = (int64_t)i + l * d;
  const int dnode = delta(keys, n, i, j);
  int64_t s = 0;
  for (int64_t div = 2;; div *= 2) {
    const int64_t t = (l + div - 1) / div;
    if (delta(keys, n, i, (int64_t)i + (s + t) * d) > dnode) s += t;
    if (t <= 1) break;
  }
  const int64_t g = (int64_t)i + s * d + (d < 0 ? -1 : 0);
  *first = (uint32_t)(d > 0 ? (int64_t)i : j);
  *last = (uint32_t)(d > 0 ? j : (int64_t)i);
  *split = (uint32_t)g;
}

// a range of at most two items is a leaf of its parent
BLBVH_FN bool is_leaf_range(uint32_t first, uint32_t last) { return last - first < 2u; }
BLBVH_FN int32_t leaf_code(uint32_t first, uint32_t count) { return (int32_t)~((first << 8) | count); }

// the child-box widening of the SAH builder (bvh_build.cpp padded): a few ulps of the box magnitude
BLBVH_FN void pad_box(float* b) {
  float m = 0.f;
  for (int k = 0; k < 3; ++k) m = fmaxf(m, fmaxf(fabsf(b[k]), fabsf(b[3 + k])));
  const float e = m * 2e-6f + 1e-30f;
  for (int k = 0; k < 3; ++k) { b[k] -= e; b[3 + k] += e; }
}

}  // namespace blbvh
