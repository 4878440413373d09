// bvh_derive.hip -- what follows the BVH2, derived on the device from the tree in the context's buffers: the leaf
// records and the BVH4 of common/bvh4.h, each bit for bit the host's (scene_plan.cpp scene_derive, bvh_build.cpp
// collapse4).  Only counts come back: the BVH4's size, depth and stack bound, from which scene_plan_counts settles
// the plans on the host.
//
//   k_leaf_geo   one thread per output float4: a gather from tri_geo by the leaf refs, stores coalesced
//   k_d4_open    one thread per node of the level: opens its BVH2 node (bbvh4::open4), writes the 28 floats with
//                the inner slots' BVH2 links still in them, counts the inner slots, folds stk + pushes into the
//                stack bound (an integer maximum: LDS first, one global atomic per block)
//   sm_scan      the exclusive scan of the counts (splat_merge.hip), start[n] the next level's size
//   k_d4_link    one thread per node again: its inner slots get their ids, the next level gets their BVH2 nodes
//                and stack sums, in slot order -- the order of the host's queue
//
// The level loop reads each level's size back (4 bytes and a stream synchronisation per level, at most 32 levels),
// so every launch has its exact size and no kernel reads a count another one is still writing.  Nothing depends on
// the launch geometry: the numbering is a scan, the only atomic an integer maximum.
#include "core_internal.h"
#include "../common/bvh4.h"

using namespace bcore;

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kBadTree = 0xFFFFFFFFu;    // in the stack bound's word: a link that names no node, or more nodes than the BVH2 has

__global__ __launch_bounds__(kBlock) void k_leaf_geo(const float4* __restrict__ tri_geo, uint32_t n_tris, const uint32_t* __restrict__ refs,
                                                     uint32_t nrefs, float4* __restrict__ out, uint32_t n_quads) {
  const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
  if (q >= n_quads) return;
  float v[4];
  bbvh4::leaf_quad(reinterpret_cast<const float*>(tri_geo), n_tris, refs, nrefs, q, v);
  out[q] = make_float4(v[0], v[1], v[2], v[3]);
}

// src[i] / stk[i]: the BVH2 node and the stack sum of the level's i-th node, whose id is base + i
__global__ __launch_bounds__(kBlock) void k_d4_open(const float* __restrict__ nodes2, const uint32_t* __restrict__ src,
                                                    const uint32_t* __restrict__ stk, uint32_t n, uint32_t base, uint32_t n2,
                                                    float4* __restrict__ nodes4, uint32_t* __restrict__ cnt, uint32_t* __restrict__ need) {
  __shared__ uint32_t s_need;
  if (threadIdx.x == 0) s_need = 0u;
  __syncthreads();
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) {
    bbvh4::Slot v[4];
    const int m = bbvh4::open4(nodes2, n2, (int32_t)src[i], v);
    float nd[28];
    cnt[i] = (uint32_t)bbvh4::node4(v, m, nd);
    float4* o = nodes4 + 7 * (size_t)(base + i);
    for (int q = 0; q < 7; ++q) o[q] = make_float4(nd[4 * q], nd[4 * q + 1], nd[4 * q + 2], nd[4 * q + 3]);
    atomicMax(&s_need, stk[i] + (uint32_t)bbvh4::pushes(m));
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_need) atomicMax(need, s_need);
}

// start: the exclusive scan of cnt.  The level's inner slots are numbered behind the level (base + n + ...); cap
// (the BVH2's node count) bounds the next level's arrays and the links worth following.
__global__ __launch_bounds__(kBlock) void k_d4_link(float4* __restrict__ nodes4, uint32_t base, uint32_t n, const uint32_t* __restrict__ start,
                                                    const uint32_t* __restrict__ stk, uint32_t cap, uint32_t* __restrict__ next_src,
                                                    uint32_t* __restrict__ next_stk, uint32_t* __restrict__ need) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  float4* lq = nodes4 + 7 * (size_t)(base + i) + 6;
  const float4 w = *lq;
  int32_t link[4] = {__float_as_int(w.x), __float_as_int(w.y), __float_as_int(w.z), __float_as_int(w.w)};
  int children = 0;
  for (int k = 0; k < 4; ++k) if (link[k] != bbvh4::kEmpty4) ++children;
  const uint32_t s = stk[i] + (uint32_t)bbvh4::pushes(children);
  uint32_t r = start[i];
  for (int k = 0; k < 4; ++k) {
    if (link[k] < 0) continue;
    if (r < cap && (uint32_t)link[k] < cap) { next_src[r] = (uint32_t)link[k]; next_stk[r] = s; }
    else { if (r < cap) { next_src[r] = 0u; next_stk[r] = 0u; } atomicMax(need, kBadTree); }
    link[k] = (int32_t)(base + n + r);
    ++r;
  }
  *lq = make_float4(__int_as_float(link[0]), __int_as_float(link[1]), __int_as_float(link[2]), __int_as_float(link[3]));
}

inline uint32_t blocks_for(size_t n) { return (uint32_t)((n + kBlock - 1) / kBlock); }

}  // namespace

namespace bcore {

void bvh_derive_device(bling_ctx* c, uint32_t n_tris, bplan::DeriveCounts& k, bling_derive_info* info) {
  const uint32_t n2 = k.n2, nrefs = k.nrefs;
  if (n2 < 1 || c->nodes.n != (size_t)4 * n2 || c->refs.n != nrefs || c->tri_geo.n != (size_t)3 * n_tris)
    throw std::runtime_error("bvh derive: the context's tree does not have the sizes given");
  if (nrefs > (1u << 24)) throw std::runtime_error("bvh derive: more leaf refs than a leaf code can address");
  hipStream_t s = c->stream;
  HIPCHK(hipSetDevice(c->device));

  DBuf<uint32_t> d_src[2], d_stk[2], d_cnt, d_start, d_sums, d_need;
  DBuf<float4> d_nodes4;                                   // at most one BVH4 node per BVH2 node
  for (int b = 0; b < 2; ++b) { d_src[b].alloc(n2); d_stk[b].alloc(n2); }
  d_cnt.alloc(n2); d_start.alloc((size_t)n2 + 1); d_sums.alloc((size_t)n2 / 1024 + 2); d_need.alloc(1);
  d_nodes4.alloc((size_t)7 * n2);
  const uint32_t n_quads = leaf_geo_quads(nrefs);
  c->leaf_geo.alloc(n_quads);

  EventPair ev;
  ev.a.record(s);
  k_leaf_geo<<<blocks_for(n_quads), kBlock, 0, s>>>(c->tri_geo.p, n_tris, c->refs.p, nrefs, c->leaf_geo.p, n_quads);
  HIPCHK(hipMemsetAsync(d_src[0].p, 0, sizeof(uint32_t), s));          // the root: BVH2 node 0, nothing pushed above it
  HIPCHK(hipMemsetAsync(d_stk[0].p, 0, sizeof(uint32_t), s));
  HIPCHK(hipMemsetAsync(d_need.p, 0, sizeof(uint32_t), s));
  uint32_t base = 0, n = 1, levels = 0;
  int cur = 0;
  while (n > 0) {
    if (levels >= bbvh4::kMaxLevels || (size_t)base + n > n2) throw std::runtime_error("bvh derive: the BVH2 is no tree of depth <= 31");
    k_d4_open<<<blocks_for(n), kBlock, 0, s>>>(reinterpret_cast<const float*>(c->nodes.p), d_src[cur].p, d_stk[cur].p, n, base, n2, d_nodes4.p,
                                               d_cnt.p, d_need.p);
    sm_scan(s, d_cnt.p, n, d_sums.p, d_start.p);
    k_d4_link<<<blocks_for(n), kBlock, 0, s>>>(d_nodes4.p, base, n, d_start.p, d_stk[cur].p, n2, d_src[cur ^ 1].p, d_stk[cur ^ 1].p,
                                               d_need.p);
    HIPCHK(hipGetLastError());
    uint32_t next = 0;
    HIPCHK(hipMemcpyAsync(&next, d_start.p + n, sizeof next, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    base += n;
    n = next;
    cur ^= 1;
    ++levels;
  }
  const uint32_t n4 = base;
  c->nodes4.alloc((size_t)7 * n4);
  HIPCHK(hipMemcpyAsync(c->nodes4.p, d_nodes4.p, (size_t)7 * n4 * sizeof(float4), hipMemcpyDeviceToDevice, s));
  ev.b.record(s);
  uint32_t need = 0;
  HIPCHK(hipMemcpyAsync(&need, d_need.p, sizeof need, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (need == kBadTree) throw std::runtime_error("bvh derive: the BVH2 is no tree");
  k.n4 = n4; k.bvh4_depth = (int)levels; k.stack_need = (int)need;
  info->bvh4_nodes = n4; info->bvh4_depth = levels; info->stack_need = need;
  info->level_launches = levels;
  info->ms_derive_device = ev.elapsed_ms();
}

}  // namespace bcore
