// bvh_device.hip -- the scene BVH built on the device: the linear BVH of common/lbvh.h (Morton keys,
// radix sort, common-prefix hierarchy, bottom-up bounds, leaves of one or two items) in the node and
// leaf format of the host's SAH tree (bvh_build.h), read back once so that everything derived from a
// bvh::Result runs unchanged on it -- or left in the context's buffers for bvh_derive.hip.  The host
// restatement is bling_host_lbvh (host/lbvh_host.cpp).
//
//   k_lbvh_centres / k_lbvh_centres_final   bounds of the box centres (two-stage min / max) and the axis scales
//   k_lbvh_keys                             key = Morton code << 32 | item index
//   k_lbvh_sort_one                         n <= 1024: the whole sort in one block, keys in LDS
//   k_lbvh_hist, sm_scan, k_lbvh_scatter    larger n: per 8-bit digit, a histogram per 2048-key tile, one
//                                           exclusive scan (digit-major), a stable scatter
//   k_lbvh_hierarchy                        node i's range, split, children and parent links
//   k_lbvh_fit                              one thread per item climbs; the second arrival at a node
//                                           (an integer counter) forms the union and goes on
//   sm_scan, k_lbvh_emit                    the surviving nodes' numbers, then the 16-float nodes
//
// Nothing here depends on the launch geometry or on the order of arrival: a key's place within its
// tile is its rank among equal digits in index order (wave ballots, then per-wave counters summed in
// wave order), unions are min / max, and the only atomics are integer counters.
#include "core_internal.h"
#include "../common/lbvh.h"

using namespace bcore;

namespace {

using u64 = unsigned long long;

constexpr int kBlock = 256, kWaves = kBlock / 64;
constexpr int kRadix = 256, kPasses = 4, kKeyShift = 32;   // the Morton code's 30 bits, 8 at a time
constexpr int kOneRounds = 4, kOneMax = kBlock * kOneRounds;       // one-block sort: 1024 keys
constexpr int kTileRounds = 8, kTile = kBlock * kTileRounds;       // multi-block sort: 2048 keys a tile

// ---------------------------------------------------------------- centre bounds
__device__ void block_minmax(float (&mn)[3], float (&mx)[3], float* sh /* 6 * kBlock */) {
  for (int a = 0; a < 3; ++a) { sh[a * kBlock + threadIdx.x] = mn[a]; sh[(3 + a) * kBlock + threadIdx.x] = mx[a]; }
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s)
      for (int a = 0; a < 3; ++a) {
        sh[a * kBlock + threadIdx.x] = fminf(sh[a * kBlock + threadIdx.x], sh[a * kBlock + threadIdx.x + s]);
        sh[(3 + a) * kBlock + threadIdx.x] = fmaxf(sh[(3 + a) * kBlock + threadIdx.x], sh[(3 + a) * kBlock + threadIdx.x + s]);
      }
    __syncthreads();
  }
  for (int a = 0; a < 3; ++a) { mn[a] = sh[a * kBlock]; mx[a] = sh[(3 + a) * kBlock]; }
}

// part[6 b ..]: block b's centre minima and maxima
__global__ __launch_bounds__(kBlock) void k_lbvh_centres(const float* __restrict__ boxes, uint32_t n, float* __restrict__ part) {
  __shared__ float sh[6 * kBlock];
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock)
    for (int a = 0; a < 3; ++a) {
      const float c = blbvh::centre(boxes[6 * (size_t)i + a], boxes[6 * (size_t)i + 3 + a]);
      mn[a] = fminf(mn[a], c);
      mx[a] = fmaxf(mx[a], c);
    }
  block_minmax(mn, mx, sh);
  if (threadIdx.x < 3) { part[6 * blockIdx.x + threadIdx.x] = mn[threadIdx.x]; part[6 * blockIdx.x + 3 + threadIdx.x] = mx[threadIdx.x]; }
}

// cb[0..2] = cmin, cb[3..5] = the axis scales
__global__ __launch_bounds__(kBlock) void k_lbvh_centres_final(const float* __restrict__ part, uint32_t nparts, float* __restrict__ cb) {
  __shared__ float sh[6 * kBlock];
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t b = threadIdx.x; b < nparts; b += kBlock)
    for (int a = 0; a < 3; ++a) { mn[a] = fminf(mn[a], part[6 * b + a]); mx[a] = fmaxf(mx[a], part[6 * b + 3 + a]); }
  block_minmax(mn, mx, sh);
  if (threadIdx.x < 3) {
    cb[threadIdx.x] = mn[threadIdx.x];
    cb[3 + threadIdx.x] = blbvh::axis_scale(mn[threadIdx.x], mx[threadIdx.x]);
  }
}

__global__ __launch_bounds__(kBlock) void k_lbvh_keys(const float* __restrict__ boxes, uint32_t n, const float* __restrict__ cb,
                                                      u64* __restrict__ keys) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  float b[6], cmin[3], scale[3];
  for (int k = 0; k < 6; ++k) b[k] = boxes[6 * (size_t)i + k];
  for (int a = 0; a < 3; ++a) { cmin[a] = cb[a]; scale[a] = cb[3 + a]; }
  keys[i] = blbvh::make_key(b, cmin, scale, i);
}

// ---------------------------------------------------------------- radix sort
// the lanes of this wave that hold the same digit as this one (valid lanes only)
__device__ __forceinline__ u64 match_digit(uint32_t digit, bool valid) {
  u64 m = __ballot(valid);
  for (int b = 0; b < 8; ++b) {
    const bool bit = (digit >> b) & 1u;
    const u64 set = __ballot(valid && bit);
    m &= bit ? set : ~set;
  }
  return m;
}

// Stable ranks within a tile.  Wave w holds the tile's keys [w * 64 R, (w + 1) * 64 R), 64 consecutive
// ones per round.  Returns in local[r] the number of keys of the same digit before key r in this
// wave's part, and leaves in cnt[w][d] the wave's count of digit d.  Every thread of the block calls it.
template <int R>
__device__ void tile_rank(const u64 (&key)[R], const bool (&valid)[R], int shift, uint32_t (*cnt)[kRadix], uint32_t (&local)[R]) {
  const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  for (int k = threadIdx.x; k < kWaves * kRadix; k += kBlock) cnt[0][k] = 0u;
  __syncthreads();
  for (int r = 0; r < R; ++r) {
    const uint32_t d = (uint32_t)(key[r] >> shift) & (kRadix - 1u);
    const u64 peers = match_digit(d, valid[r]);
    const uint32_t before = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
    const uint32_t prior = valid[r] ? cnt[w][d] : 0u;
    __syncthreads();
    if (valid[r] && before == 0u) cnt[w][d] = prior + (uint32_t)__popcll(peers);
    __syncthreads();
    local[r] = prior + before;
  }
}

// n <= kOneMax keys sorted in place by one block
__global__ __launch_bounds__(kBlock) void k_lbvh_sort_one(u64* __restrict__ keys, uint32_t n) {
  __shared__ u64 buf[2][kOneMax];
  __shared__ uint32_t cnt[kWaves][kRadix];
  __shared__ uint32_t scan[kRadix];
  const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  for (uint32_t e = threadIdx.x; e < n; e += kBlock) buf[0][e] = keys[e];
  __syncthreads();
  int src = 0;
  for (int p = 0; p < kPasses; ++p) {
    const int shift = kKeyShift + 8 * p;
    u64 key[kOneRounds];
    bool valid[kOneRounds];
    uint32_t local[kOneRounds];
    for (int r = 0; r < kOneRounds; ++r) {
      const uint32_t e = w * 64u * kOneRounds + 64u * r + lane;
      valid[r] = e < n;
      key[r] = valid[r] ? buf[src][e] : 0ull;
    }
    tile_rank<kOneRounds>(key, valid, shift, cnt, local);
    // digit d starts behind every smaller digit; within it, wave after wave
    const uint32_t d = threadIdx.x;
    uint32_t t[kWaves], tot = 0u;
    for (int k = 0; k < kWaves; ++k) { t[k] = cnt[k][d]; tot += t[k]; }
    scan[d] = tot;
    __syncthreads();
    for (int s = 1; s < kRadix; s <<= 1) {
      const uint32_t v = (int)d >= s ? scan[d - s] : 0u;
      __syncthreads();
      scan[d] += v;
      __syncthreads();
    }
    uint32_t base = scan[d] - tot;
    for (int k = 0; k < kWaves; ++k) { cnt[k][d] = base; base += t[k]; }
    __syncthreads();
    for (int r = 0; r < kOneRounds; ++r)
      if (valid[r]) {
        const uint32_t dg = (uint32_t)(key[r] >> shift) & (kRadix - 1u);
        const uint32_t pos = cnt[w][dg] + local[r];
        if (pos < n) buf[src ^ 1][pos] = key[r];
      }
    __syncthreads();
    src ^= 1;
  }
  for (uint32_t e = threadIdx.x; e < n; e += kBlock) keys[e] = buf[src][e];
}

// hist[d * nblk + b]: keys of digit d in tile b
__global__ __launch_bounds__(kBlock) void k_lbvh_hist(const u64* __restrict__ keys, uint32_t n, int shift, uint32_t nblk,
                                                      uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[kRadix];
  h[threadIdx.x] = 0u;
  __syncthreads();
  const size_t base = (size_t)blockIdx.x * kTile;
  for (int r = 0; r < kTileRounds; ++r) {
    const size_t e = base + (size_t)r * kBlock + threadIdx.x;
    if (e < n) atomicAdd(&h[(uint32_t)(keys[e] >> shift) & (kRadix - 1u)], 1u);
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * nblk + blockIdx.x] = h[threadIdx.x];
}

// start: the exclusive scan of hist.  A key goes to start[d][tile] + its rank among the tile's keys of digit d.
__global__ __launch_bounds__(kBlock) void k_lbvh_scatter(const u64* __restrict__ in, u64* __restrict__ out, uint32_t n, int shift,
                                                         uint32_t nblk, const uint32_t* __restrict__ start) {
  __shared__ uint32_t cnt[kWaves][kRadix];
  const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const size_t base = (size_t)blockIdx.x * kTile + (size_t)w * 64u * kTileRounds;
  u64 key[kTileRounds];
  bool valid[kTileRounds];
  uint32_t local[kTileRounds];
  for (int r = 0; r < kTileRounds; ++r) {
    const size_t e = base + 64u * r + lane;
    valid[r] = e < n;
    key[r] = valid[r] ? in[e] : 0ull;
  }
  tile_rank<kTileRounds>(key, valid, shift, cnt, local);
  const uint32_t d = threadIdx.x;
  uint32_t pos0 = start[(size_t)d * nblk + blockIdx.x];
  uint32_t t[kWaves];
  for (int k = 0; k < kWaves; ++k) t[k] = cnt[k][d];
  __syncthreads();
  for (int k = 0; k < kWaves; ++k) { cnt[k][d] = pos0; pos0 += t[k]; }
  __syncthreads();
  for (int r = 0; r < kTileRounds; ++r)
    if (valid[r]) {
      const uint32_t dg = (uint32_t)(key[r] >> shift) & (kRadix - 1u);
      const uint32_t pos = cnt[w][dg] + local[r];
      if (pos < n) out[pos] = key[r];
    }
}

// ---------------------------------------------------------------- hierarchy
// children: >= 0 an internal node, ~position for an item.  parent[i]: of internal node i; parent[n - 1 + k]: of
// the item at sorted position k.
__global__ __launch_bounds__(kBlock) void k_lbvh_hierarchy(const u64* __restrict__ keys, uint32_t n, uint2* __restrict__ range,
                                                           int2* __restrict__ child, uint32_t* __restrict__ parent,
                                                           uint32_t* __restrict__ keep) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i + 1 >= n) return;
  uint32_t first, last, split;
  blbvh::node_range(reinterpret_cast<const uint64_t*>(keys), n, i, &first, &last, &split);
  range[i] = make_uint2(first, last);
  keep[i] = blbvh::is_leaf_range(first, last) ? 0u : 1u;
  int2 ch;
  if (first == split) { ch.x = ~(int)split; parent[n - 1 + split] = i; }
  else { ch.x = (int)split; parent[split] = i; }
  if (last == split + 1) { ch.y = ~(int)(split + 1); parent[n - 1 + split + 1] = i; }
  else { ch.y = (int)(split + 1); parent[split + 1] = i; }
  child[i] = ch;
  if (i == 0) parent[0] = 0xFFFFFFFFu;
}

__device__ __forceinline__ float load_agent(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// box[6 i ..] / height[i] of internal node i; box[6 (n - 1 + k) ..] of the item at sorted position k.  count[i]
// starts at 0.  A node's first arrival publishes its child's box and leaves; the second one reads the other
// child's (release before the counter, acquire after it, at agent scope: the two may run on different XCDs).
__global__ __launch_bounds__(kBlock) void k_lbvh_fit(const u64* __restrict__ keys, uint32_t n, const float* __restrict__ boxes,
                                                     const uint32_t* __restrict__ refs_in, const uint2* __restrict__ range,
                                                     const int2* __restrict__ child, const uint32_t* __restrict__ parent,
                                                     float* box, int* height, uint32_t* count, uint32_t* __restrict__ refs_out) {
  const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= n) return;
  const uint32_t item = (uint32_t)keys[k];
  float b[6];
  for (int a = 0; a < 6; ++a) b[a] = boxes[6 * (size_t)item + a];
  refs_out[k] = refs_in[item];
  uint32_t me = n - 1 + k;          // the slot of what this thread carries
  int h = 0;
  for (;;) {
    for (int a = 0; a < 6; ++a) box[6 * (size_t)me + a] = b[a];
    if (me < n - 1) height[me] = h;
    const uint32_t up = parent[me];
    if (up == 0xFFFFFFFFu) return;                       // the root is fitted
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (__hip_atomic_fetch_add(&count[up], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const int2 ch = child[up];
    const uint32_t l = ch.x < 0 ? n - 1 + (uint32_t)~ch.x : (uint32_t)ch.x;
    const uint32_t r = ch.y < 0 ? n - 1 + (uint32_t)~ch.y : (uint32_t)ch.y;
    const uint32_t other = l == me ? r : l;
    for (int a = 0; a < 3; ++a) {
      b[a] = fminf(b[a], load_agent(&box[6 * (size_t)other + a]));
      b[3 + a] = fmaxf(b[3 + a], load_agent(&box[6 * (size_t)other + 3 + a]));
    }
    const int ho = other < n - 1 ? __hip_atomic_load(&height[other], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    const uint2 rg = range[up];
    h = blbvh::is_leaf_range(rg.x, rg.y) ? 0 : 1 + max(h, ho);
    me = up;
  }
}

// stats: nodes, depth, leaves, max_leaf
__global__ __launch_bounds__(kBlock) void k_lbvh_emit(uint32_t n, const uint2* __restrict__ range, const int2* __restrict__ child,
                                                      const uint32_t* __restrict__ keep, const uint32_t* __restrict__ number,
                                                      const float* __restrict__ box, const int* __restrict__ height,
                                                      float4* __restrict__ nodes, uint32_t* __restrict__ stats) {
  __shared__ uint32_t s_leaves, s_max;
  if (threadIdx.x == 0) { s_leaves = 0u; s_max = 0u; }
  __syncthreads();
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i + 1 < n && keep[i]) {
    const int2 ch = child[i];
    float w[16];
    uint32_t leaves = 0u, mx = 0u;
    for (int c = 0; c < 2; ++c) {
      const int v = c == 0 ? ch.x : ch.y;
      float b[6];
      int32_t link;
      if (v < 0) {
        const uint32_t pos = (uint32_t)~v;
        for (int a = 0; a < 6; ++a) b[a] = box[6 * (size_t)(n - 1 + pos) + a];
        link = blbvh::leaf_code(pos, 1u);
      } else {
        for (int a = 0; a < 6; ++a) b[a] = box[6 * (size_t)v + a];
        link = keep[v] ? (int32_t)number[v] : blbvh::leaf_code(range[v].x, 2u);
      }
      if (link < 0) { ++leaves; mx = max(mx, (uint32_t)~link & 0xFFu); }
      blbvh::pad_box(b);
      for (int a = 0; a < 6; ++a) w[6 * c + a] = b[a];
      w[12 + c] = __int_as_float(link);
    }
    w[14] = w[15] = 0.f;
    float4* out = nodes + 4 * (size_t)number[i];
    for (int q = 0; q < 4; ++q) out[q] = make_float4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
    atomicAdd(&s_leaves, leaves);
    atomicMax(&s_max, mx);
    if (i == 0) { stats[0] = number[n - 1]; stats[1] = (uint32_t)height[0]; }
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_leaves) { atomicAdd(&stats[2], s_leaves); atomicMax(&stats[3], s_max); }
}

inline uint32_t blocks_for(size_t n, size_t per) { return (uint32_t)((n + per - 1) / per); }

}  // namespace

namespace bcore {

bool lbvh_build_device(bling_ctx* c, const std::vector<bvh::Box>& boxes, const std::vector<uint32_t>& refs, int depth_cap,
                       bvh::Result& R, float* ms, int* depth, uint32_t* n_kept) {
  static_assert(sizeof(bvh::Box) == 6 * sizeof(float), "a Box is lo.xyz, hi.xyz");
  const size_t n_items = boxes.size();
  if (n_items < 3 || n_items > blbvh::kMaxItems || refs.size() != n_items) throw std::invalid_argument("lbvh: item count out of range");
  const uint32_t n = (uint32_t)n_items;
  hipStream_t s = c->stream;
  HIPCHK(hipSetDevice(c->device));

  DBuf<float> d_boxes, d_part, d_cb, d_box;
  DBuf<uint32_t> d_refs, d_refs_out, d_hist, d_start, d_sums, d_parent, d_keep, d_number, d_count, d_stats;
  DBuf<u64> d_keys, d_keys2;
  DBuf<uint2> d_range;
  DBuf<int2> d_child;
  DBuf<int> d_height;
  DBuf<float4> d_nodes;

  const uint32_t nparts = std::min<uint32_t>(1024u, blocks_for(n, kBlock));
  const bool one = n <= (uint32_t)kOneMax;
  const uint32_t nblk = blocks_for(n, kTile);
  const uint32_t nh = (uint32_t)kRadix * nblk;
  d_boxes.upload(reinterpret_cast<const float*>(boxes.data()), (size_t)6 * n);
  d_refs.upload(refs.data(), n);
  d_part.alloc((size_t)6 * nparts); d_cb.alloc(6);
  d_keys.alloc(n);
  if (!one) { d_keys2.alloc(n); d_hist.alloc(nh); d_start.alloc((size_t)nh + 1); }
  d_sums.alloc((size_t)std::max(nh, n) / 1024 + 2);
  d_range.alloc(n - 1); d_child.alloc(n - 1); d_keep.alloc(n - 1); d_number.alloc(n); d_count.alloc(n - 1); d_height.alloc(n - 1);
  d_parent.alloc((size_t)2 * n - 1); d_box.alloc((size_t)6 * (2 * (size_t)n - 1));
  d_refs_out.alloc(n); d_stats.alloc(4);
  d_nodes.alloc((size_t)4 * (n - 1));

  EventPair ev;
  ev.a.record(s);
  HIPCHK(hipMemsetAsync(d_count.p, 0, (size_t)(n - 1) * sizeof(uint32_t), s));
  HIPCHK(hipMemsetAsync(d_stats.p, 0, 4 * sizeof(uint32_t), s));
  k_lbvh_centres<<<nparts, kBlock, 0, s>>>(d_boxes.p, n, d_part.p);
  k_lbvh_centres_final<<<1, kBlock, 0, s>>>(d_part.p, nparts, d_cb.p);
  k_lbvh_keys<<<blocks_for(n, kBlock), kBlock, 0, s>>>(d_boxes.p, n, d_cb.p, d_keys.p);
  u64* sorted = d_keys.p;
  if (one) {
    k_lbvh_sort_one<<<1, kBlock, 0, s>>>(d_keys.p, n);
  } else {
    u64* in = d_keys.p;
    u64* out = d_keys2.p;
    for (int p = 0; p < kPasses; ++p) {
      const int shift = kKeyShift + 8 * p;
      k_lbvh_hist<<<nblk, kBlock, 0, s>>>(in, n, shift, nblk, d_hist.p);
      sm_scan(s, d_hist.p, nh, d_sums.p, d_start.p);
      k_lbvh_scatter<<<nblk, kBlock, 0, s>>>(in, out, n, shift, nblk, d_start.p);
      std::swap(in, out);
    }
    sorted = in;                                           // an even number of passes: back in d_keys
  }
  HIPCHK(hipGetLastError());
  k_lbvh_hierarchy<<<blocks_for(n - 1, kBlock), kBlock, 0, s>>>(sorted, n, d_range.p, d_child.p, d_parent.p, d_keep.p);
  k_lbvh_fit<<<blocks_for(n, kBlock), kBlock, 0, s>>>(sorted, n, d_boxes.p, d_refs.p, d_range.p, d_child.p, d_parent.p, d_box.p,
                                                      d_height.p, d_count.p, d_refs_out.p);
  sm_scan(s, d_keep.p, n - 1, d_sums.p, d_number.p);       // number[n - 1] = the surviving nodes
  k_lbvh_emit<<<blocks_for(n - 1, kBlock), kBlock, 0, s>>>(n, d_range.p, d_child.p, d_keep.p, d_number.p, d_box.p, d_height.p,
                                                           d_nodes.p, d_stats.p);
  HIPCHK(hipGetLastError());
  ev.b.record(s);
  uint32_t stats[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(stats, d_stats.p, sizeof stats, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (ms) *ms = ev.elapsed_ms();
  if (depth) *depth = (int)stats[1];
  if (stats[0] < 1 || stats[0] > n - 1) throw std::runtime_error("lbvh: node count out of range");
  if ((int)stats[1] > depth_cap) return false;
  bvh::Result out;
  out.depth = (int)stats[1]; out.leaves = (int)stats[2]; out.max_leaf = (int)stats[3];
  if (n_kept) {                                            // the tree stays: the nodes at their size, the refs as they are
    c->nodes.alloc((size_t)4 * stats[0]);
    HIPCHK(hipMemcpy(c->nodes.p, d_nodes.p, (size_t)4 * stats[0] * sizeof(float4), hipMemcpyDeviceToDevice));
    std::swap(c->refs.p, d_refs_out.p);
    std::swap(c->refs.n, d_refs_out.n);
    *n_kept = stats[0];
    R = std::move(out);
    return true;
  }
  out.nodes.resize((size_t)16 * stats[0]);
  out.refs.resize(n);
  HIPCHK(hipMemcpy(out.nodes.data(), d_nodes.p, out.nodes.size() * sizeof(float), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(out.refs.data(), d_refs_out.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  R = std::move(out);
  return true;
}

}  // namespace bcore
