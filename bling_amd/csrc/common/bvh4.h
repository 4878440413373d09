// bvh4.h -- what is derived from a BVH2 (bvh_build.h: 16 floats a node, two child boxes, two links), stated
// once for the host (core/bvh_build.cpp collapse4) and the device (core/bvh_derive.hip): how a BVH4 node opens
// its BVH2 children, how the BVH4 is numbered, and the leaf records.  Both sides compile these expressions
// without multiply-add contraction, so the two trees agree bit for bit: a fused area changes which child opens
// on a near-tie, and the whole tree below it.
//
//   link     >= 0 an inner BVH2 node, ~0 an empty child, any other negative value a leaf code
//   area     2 (d0 d1 + d0 d2 + d1 d2) of a child box, d = max(0, hi - lo) per axis, binary32, summed left to right
//   open     the non-empty children of the BVH2 node; then, while some inner child fits (size - 1 + its own
//            non-empty children <= 4), the one of strictly largest area (the lowest slot on a tie) is replaced
//            by its non-empty children, in place, child 0 before child 1.  (An inner child with an empty child
//            of its own never occurs: the builders leave an empty child in a root alone.)
//   number   level by level from the root (node 0): a level's nodes open in id order, and their inner slots take
//            the next ids in slot order -- the order of a queue.  A node of the level at position i therefore has
//            id = nodes of the earlier levels + i, and its r-th inner slot the id
//            nodes up to and including this level + inner slots of the positions before i + r
//   stack    pushes = max(0, children - 1); stk(root) = 0, stk(child) = stk(node) + pushes; the traversal stack
//            bound is the largest stk(node) + pushes, the depth the number of levels
//   node4    28 floats: child k's lo.x lo.y lo.z hi.x hi.y hi.z in lane k of words 0-5, the four links in word
//            6; an unused slot holds lo = +inf, hi = -inf and kEmpty4
//   leaf     three float4 per leaf ref j (dev_trace.h LeafRec) and one zero record behind the last: a
//            triangle's geo[3 idx], geo[3 idx + 1], (geo[3 idx + 2].x, ref bits, 0, 0); any other ref two zero
//            quads and (0, ref bits, 0, 0)
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BBVH4_FN __host__ __device__ __forceinline__
#else
#include <cmath>
#define BBVH4_FN static inline
#endif

namespace bbvh4 {

constexpr int32_t kEmpty2 = (int32_t)~0u;            // an empty BVH2 child
constexpr int32_t kEmpty4 = (int32_t)0x80000000;     // an unused BVH4 slot (bvh::EMPTY4)
constexpr uint32_t kMaxLevels = 32;                  // a BVH2 of depth <= 31 collapses into at most as many levels
constexpr uint32_t kThreadedMaxNodes = 16;           // BVH2s up to this size have a threaded list worth walking

struct Slot { float b[6]; int32_t link; };           // lo.xyz, hi.xyz, BVH2 link

BBVH4_FN int32_t float_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __float_as_int(f);
#else
  union { float f; int32_t i; } u;
  u.f = f;
  return u.i;
#endif
}
BBVH4_FN float bits_float(int32_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __int_as_float(i);
#else
  union { float f; int32_t i; } u;
  u.i = i;
  return u.f;
#endif
}

BBVH4_FN float area(const float* b) {
  float d[3];
  for (int k = 0; k < 3; ++k) { const float e = b[3 + k] - b[k]; d[k] = 0.f < e ? e : 0.f; }
  return 2.f * (d[0] * d[1] + d[0] * d[2] + d[1] * d[2]);
}

BBVH4_FN int32_t link2(const float* nodes2, int32_t node, int c) { return float_bits(nodes2[16 * (size_t)node + 12 + c]); }

BBVH4_FN Slot child2(const float* nodes2, int32_t node, int c) {
  const float* n = nodes2 + 16 * (size_t)node;
  Slot s;
  for (int k = 0; k < 6; ++k) s.b[k] = n[6 * c + k];
  s.link = float_bits(n[12 + c]);
  return s;
}

// the children of the BVH4 node opened from BVH2 node `node` (< n2), in slot order; returns how many (0 .. 4).  A
// link that names no node of the array (a malformed tree) is never followed: the callers refuse it.
BBVH4_FN int open4(const float* nodes2, uint32_t n2, int32_t node, Slot* v) {
  int n = 0;
  for (int c = 0; c < 2; ++c) {
    const Slot s = child2(nodes2, node, c);
    if (s.link != kEmpty2) v[n++] = s;
  }
  for (;;) {
    int best = -1;
    float ba = -1.f;
    for (int k = 0; k < n; ++k) {
      if (v[k].link < 0 || (uint32_t)v[k].link >= n2) continue;
      int grand = 0;
      for (int c = 0; c < 2; ++c) if (link2(nodes2, v[k].link, c) != kEmpty2) ++grand;
      if (n - 1 + grand > 4) continue;
      const float a = area(v[k].b);
      if (a > ba) { ba = a; best = k; }
    }
    if (best < 0) return n;
    Slot g[2];
    int ng = 0;
    for (int c = 0; c < 2; ++c) {
      const Slot s = child2(nodes2, v[best].link, c);
      if (s.link != kEmpty2) g[ng++] = s;
    }
    // ng children take the place of slot `best`: the slots behind it move by ng - 1
    if (ng == 2) { for (int k = n - 1; k > best; --k) v[k + 1] = v[k]; }
    else if (ng == 0) { for (int k = best + 1; k < n; ++k) v[k - 1] = v[k]; }
    for (int c = 0; c < ng; ++c) v[best + c] = g[c];
    n += ng - 1;
  }
}

// the 28 floats of the node with these children; inner slots keep their BVH2 link (the numbering replaces it).
// Returns the number of inner slots.
BBVH4_FN int node4(const Slot* v, int n, float* nd) {
  int inner = 0;
  for (int k = 0; k < 4; ++k) {
    int32_t link = kEmpty4;
    if (k < n) {
      for (int a = 0; a < 3; ++a) { nd[4 * a + k] = v[k].b[a]; nd[4 * (3 + a) + k] = v[k].b[3 + a]; }
      link = v[k].link;
      if (link >= 0) ++inner;
    } else {
      for (int a = 0; a < 3; ++a) { nd[4 * a + k] = INFINITY; nd[4 * (3 + a) + k] = -INFINITY; }
    }
    nd[24 + k] = bits_float(link);
  }
  return inner;
}

BBVH4_FN int pushes(int children) { return children > 1 ? children - 1 : 0; }

// float4 q (0 .. 3 (nrefs + 1) - 1) of the leaf records: x, y, z, w into out
BBVH4_FN void leaf_quad(const float* tri_geo /* 12 floats a triangle */, uint32_t n_tris, const uint32_t* refs, uint32_t nrefs,
                        uint32_t q, float* out) {
  out[0] = out[1] = out[2] = out[3] = 0.f;
  const uint32_t j = q / 3u, part = q - 3u * j;
  if (j >= nrefs) return;
  const uint32_t ref = refs[j], idx = ref & 0x3FFFFFFFu;
  const bool tri = (ref >> 30) == 0u && idx < n_tris;            // REF_TRI (dev_scene.h)
  if (part < 2u) {
    if (tri) for (int k = 0; k < 4; ++k) out[k] = tri_geo[12 * (size_t)idx + 4 * part + k];
    return;
  }
  if (tri) out[0] = tri_geo[12 * (size_t)idx + 8];
  out[1] = bits_float((int32_t)ref);
}

}  // namespace bbvh4
