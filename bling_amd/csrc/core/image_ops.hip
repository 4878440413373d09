// image_ops.hip -- the image API on the device (include/bling.h, "the image API on the device"): samples the
// caller computed are filtered onto a film, or splatted, in the reference's order -- addSample,
// addUnfilteredSample and splatSample (Image.hs:201-299) applied to samples 0 .. n-1 by one thread -- without
// a float atomic.  Store, then sum per destination: a list is cut into chunks of consecutive samples, and per
// chunk
//   k_img_prep     one lane per sample: the drop rules, XYZ of the 16 bands, and a count of the sample for
//                  every 16 x 16 destination tile its pixel rectangle meets (integer atomics)
//   sm_scan        the exclusive scan of the tile counts (splat_merge.hip)
//   k_img_scatter  the sample's index into each of those tiles' segments, in any order
//   k_img_tile     one block per tile, one pixel per lane: the segment is sorted by sample index (the bitonic
//                  network of splat_merge.h, in LDS up to SM_LDS_RECORDS indices, in place in global memory
//                  beyond), then staged through LDS kStage records at a time; every lane adds to its pixel,
//                  in registers, the staged samples that reach it, one at a time in ascending index.
// The per-sample decisions are those of common/image_sample.h, which the host library's restatement shares.
//
// The windowed calls (bling_image_add_windowed[_device]) serve a renderer's use of its film: per SampleWindow a
// zeroed mkImageTile image takes the window's samples and addTile adds it to the film, film = film + tile.  A
// window owns consecutive samples, so a destination tile's segment sorted by sample index is sorted by window
// too; k_imgw_prep / k_imgw_scatter clip a sample's rectangle to the film pixels its own window's tile is added
// to, and k_imgw_tile keeps two accumulators a channel -- the film value and the current window's tile value,
// from +0 -- folding film = film + tile at every change of window.  A window that covers a pixel without reaching
// it adds +0, which changes nothing but a -0.0: k_imgw_cover turns every -0.0 under a tile into +0.0 first (the
// fix-up derived from the window rectangles; a tile value is never -0.0, so no later fold can make one).  A chunk
// ends at a window boundary where it can; one that ends inside a window leaves the lanes' tile values in a carry
// image that the next chunk starts from, so a window's tile sum is never split into two film additions.
#include "core_internal.h"
#include "../common/image_sample.h"

namespace bcore {
namespace {

using namespace bimgs;

constexpr uint32_t kStage = 1024;                 // sample records staged per round: 24 KiB of LDS
constexpr size_t kDefaultPairs = (size_t)64 << 18;   // 64 MiB of 4-byte pairs
constexpr size_t kMaxChunk = (size_t)1 << 22;     // samples per chunk at most: 64 MiB of per-sample results
enum : int { CTR_SPECTRUM = 0, CTR_POSITION = 1, CTR_PAIRS = 2, CTR_N = 3 };

struct ImgGeom {
  int w, h, ntx, nty;
  float fw, fh;
};
struct ImgTable { float v[256]; };

template <int OP>
__global__ __launch_bounds__(256) void k_img_prep(const float* __restrict__ xy, const float* __restrict__ spectra, uint32_t n,
                                                  ImgGeom G, float4* __restrict__ res, uint32_t* __restrict__ cnt,
                                                  unsigned long long* __restrict__ ctr) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float sx = xy[2 * (size_t)i], sy = xy[2 * (size_t)i + 1];
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!position_ok(sx, sy)) {
      atomicAdd(&ctr[CTR_POSITION], 1ull);
    } else {
      float b[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) b[q] = spectra[16 * (size_t)i + q];
      if (!spectrum_ok(b)) {
        atomicAdd(&ctr[CTR_SPECTRUM], 1ull);
      } else {
        to_xyz(b, &r.x, &r.y, &r.z);
        r.w = 1.f;
        int x0, x1, y0, y1;
        if (sample_rect(OP, sx, sy, G.fw, G.fh, G.w, G.h, &x0, &x1, &y0, &y1))
          for (int ty = y0 >> 4; ty <= y1 >> 4; ++ty)
            for (int tx = x0 >> 4; tx <= x1 >> 4; ++tx) atomicAdd(&cnt[ty * G.ntx + tx], 1u);
      }
    }
    res[i] = r;
  }
}

// cnt counts down: the slots of a tile are claimed in any order, each once.  cap bounds the pair buffer.
template <int OP>
__global__ __launch_bounds__(256) void k_img_scatter(const float* __restrict__ xy, const float4* __restrict__ res, uint32_t n, ImgGeom G,
                                                     const uint32_t* __restrict__ start, uint32_t* __restrict__ cnt,
                                                     uint32_t* __restrict__ pairs, uint32_t cap, unsigned long long* __restrict__ ctr) {
  if (blockIdx.x == 0 && threadIdx.x == 0) ctr[CTR_PAIRS] += start[G.ntx * G.nty];
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    if (res[i].w == 0.f) continue;
    int x0, x1, y0, y1;
    if (!sample_rect(OP, xy[2 * (size_t)i], xy[2 * (size_t)i + 1], G.fw, G.fh, G.w, G.h, &x0, &x1, &y0, &y1)) continue;
    for (int ty = y0 >> 4; ty <= y1 >> 4; ++ty)
      for (int tx = x0 >> 4; tx <= x1 >> 4; ++tx) {
        const int t = ty * G.ntx + tx;
        const uint32_t slot = start[t] + (atomicSub(&cnt[t], 1u) - 1u);
        if (slot < cap) pairs[slot] = i;
      }
  }
}

struct ImgLds {         // sample indices in LDS
  uint32_t* k;
  DEV void cswap(uint32_t lo, uint32_t hi) {
    const uint32_t a = k[lo], b = k[hi];
    if (a > b) { k[lo] = b; k[hi] = a; }
  }
};
struct ImgGlobal {      // one segment's sample indices, in place
  uint32_t* k;
  DEV void cswap(uint32_t lo, uint32_t hi) {
    const uint32_t a = k[lo], b = k[hi];
    if (a > b) { k[lo] = b; k[hi] = a; }
  }
};

// One block per tile.  A staged record is X, Y, Z and the sample's rectangle clipped to the tile, four nibbles
// (x0, x1, y0, y1 relative to the tile); its dx, dy go beside it.
template <int OP>
__global__ __launch_bounds__(256) void k_img_tile(const float* __restrict__ xy, const float4* __restrict__ res, ImgGeom G, ImgTable T,
                                                  const uint32_t* __restrict__ start, uint32_t* pairs, uint32_t cap,
                                                  float* __restrict__ target) {
  __shared__ uint32_t sk[SM_LDS_RECORDS];
  __shared__ float4 sres[kStage];
  __shared__ float2 spos[kStage];
  __shared__ float tbl[256];
  const uint32_t s = start[blockIdx.x], len = min(start[blockIdx.x + 1], cap) - min(s, cap);
  if (len == 0) return;
  tbl[threadIdx.x] = T.v[threadIdx.x];
  uint32_t* seg = pairs + s;
  if (len <= SM_LDS_RECORDS) {
    for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) sk[i] = seg[i];
    __syncthreads();
    ImgLds x{sk};
    sm_bitonic(x, len);
    for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) seg[i] = sk[i];
  } else {
    ImgGlobal x{seg};
    sm_bitonic(x, len);
  }
  constexpr int NC = OP == OP_SPLAT ? 3 : 4;
  const int tx0 = (int)(blockIdx.x % (uint32_t)G.ntx) * 16, ty0 = (int)(blockIdx.x / (uint32_t)G.ntx) * 16;
  const int lx = (int)(threadIdx.x & 15u), ly = (int)(threadIdx.x >> 4);
  const int x = tx0 + lx, y = ty0 + ly;
  const bool own = x < G.w && y < G.h;
  float* o = target + (size_t)NC * ((size_t)y * G.w + x);
  float a[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) a[c] = own ? o[c] : 0.f;
  const float ifw = 1.f / G.fw, ifh = 1.f / G.fw;                        // trap T12
  for (uint32_t base = 0; base < len; base += kStage) {
    const uint32_t m = min(kStage, len - base);
    __syncthreads();                                                    // the sorted segment is written; the previous round is consumed
    for (uint32_t e = threadIdx.x; e < m; e += blockDim.x) {
      const uint32_t i = seg[base + e];
      const float sx = xy[2 * (size_t)i], sy = xy[2 * (size_t)i + 1];
      int x0, x1, y0, y1;
      sample_rect(OP, sx, sy, G.fw, G.fh, G.w, G.h, &x0, &x1, &y0, &y1);
      const uint32_t rect = (uint32_t)(max(x0, tx0) - tx0) | (uint32_t)(min(x1, tx0 + 15) - tx0) << 4 |
                            (uint32_t)(max(y0, ty0) - ty0) << 8 | (uint32_t)(min(y1, ty0 + 15) - ty0) << 12;
      const float4 r = res[i];
      sres[e] = make_float4(r.x, r.y, r.z, __uint_as_float(rect));
      spos[e] = make_float2(sx - 0.5f, sy - 0.5f);
    }
    __syncthreads();
    if (own)
      for (uint32_t j = 0; j < m; ++j) {
        const float4 r = sres[j];
        const uint32_t rect = __float_as_uint(r.w);
        if (lx < (int)(rect & 15u) || lx > (int)(rect >> 4 & 15u) || ly < (int)(rect >> 8 & 15u) || ly > (int)(rect >> 12 & 15u)) continue;
        if (OP == OP_ADD) {
          // a = a + w, a = a + (v * w), the product rounded first (addSample, Image.hs:296-299)
          const float2 d = spos[j];
          const float fltw = tbl[table_index(y, d.y, ifh) * 16 + table_index(x, d.x, ifw)];
          const float vx = r.x * fltw, vy = r.y * fltw, vz = r.z * fltw;
          a[0] = a[0] + fltw; a[1] = a[1] + vx; a[2] = a[2] + vy; a[3] = a[3] + vz;
        } else if (OP == OP_UNFILTERED) {
          a[0] = a[0] + 1.f; a[1] = a[1] + r.x; a[2] = a[2] + r.y; a[3] = a[3] + r.z;
        } else {
          a[0] = a[0] + r.x; a[1] = a[1] + r.y; a[2] = a[2] + r.z;
        }
      }
  }
  if (own) {
#pragma unroll
    for (int c = 0; c < NC; ++c) o[c] = a[c];
  }
}

// ---- the windowed kernels ----
struct WinTable {
  const unsigned long long* first;   // n + 1 ascending sample offsets
  const int4* cover;                 // per window: the film pixels its tile is added to, x0, y0, x1, y1 inclusive
  uint32_t n;
};
DEV Rect win_cover(const WinTable& W, uint32_t k) {
  const int4 c = W.cover[k];
  return Rect{c.x, c.y, c.z, c.w};
}
// the window that owns sample g: the last k with first[k] <= g (an empty window owns nothing)
DEV uint32_t win_of(const WinTable& W, unsigned long long g) {
  uint32_t lo = 0, hi = W.n;         // first[lo] <= g < first[hi]
  while (hi - lo > 1u) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (W.first[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// addTile's zeros: a -0.0 of film or splat under any window's tile becomes +0.0.  One block a window at a time.
__global__ __launch_bounds__(256) void k_imgw_cover(WinTable W, int width, uint32_t* __restrict__ film, uint32_t* __restrict__ splat) {
  for (uint32_t k = blockIdx.x; k < W.n; k += gridDim.x) {
    const Rect c = win_cover(W, k);
    if (rect_empty(c)) continue;
    const uint32_t cw = (uint32_t)(c.x1 - c.x0 + 1);
    const unsigned long long px = (unsigned long long)cw * (uint32_t)(c.y1 - c.y0 + 1);
    for (unsigned long long i = threadIdx.x; i < px; i += blockDim.x) {
      const size_t p = (size_t)(c.y0 + (int)(i / cw)) * width + (size_t)(c.x0 + (int)(i % cw));
      if (film)
        for (int q = 0; q < 4; ++q)
          if (film[4 * p + q] == 0x80000000u) atomicCAS(&film[4 * p + q], 0x80000000u, 0u);
      if (splat)
        for (int q = 0; q < 3; ++q)
          if (splat[3 * p + q] == 0x80000000u) atomicCAS(&splat[3 * p + q], 0x80000000u, 0u);
    }
  }
}

// k_img_prep with the sample's window (off: the chunk's first sample in the list): win receives it, and the
// rectangle is the one inside its window's tile
template <int OP>
__global__ __launch_bounds__(256) void k_imgw_prep(const float* __restrict__ xy, const float* __restrict__ spectra, uint32_t n,
                                                   unsigned long long off, ImgGeom G, WinTable W, float4* __restrict__ res,
                                                   uint32_t* __restrict__ win, uint32_t* __restrict__ cnt,
                                                   unsigned long long* __restrict__ ctr) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float sx = xy[2 * (size_t)i], sy = xy[2 * (size_t)i + 1];
    const uint32_t k = win_of(W, off + i);
    win[i] = k;
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!position_ok(sx, sy)) {
      atomicAdd(&ctr[CTR_POSITION], 1ull);
    } else {
      float b[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) b[q] = spectra[16 * (size_t)i + q];
      if (!spectrum_ok(b)) {
        atomicAdd(&ctr[CTR_SPECTRUM], 1ull);
      } else {
        to_xyz(b, &r.x, &r.y, &r.z);
        r.w = 1.f;
        int x0, x1, y0, y1;
        if (sample_rect_in(OP, sx, sy, G.fw, G.fh, G.w, G.h, win_cover(W, k), &x0, &x1, &y0, &y1))
          for (int ty = y0 >> 4; ty <= y1 >> 4; ++ty)
            for (int tx = x0 >> 4; tx <= x1 >> 4; ++tx) atomicAdd(&cnt[ty * G.ntx + tx], 1u);
      }
    }
    res[i] = r;
  }
}

template <int OP>
__global__ __launch_bounds__(256) void k_imgw_scatter(const float* __restrict__ xy, const float4* __restrict__ res,
                                                      const uint32_t* __restrict__ win, uint32_t n, ImgGeom G, WinTable W,
                                                      const uint32_t* __restrict__ start, uint32_t* __restrict__ cnt,
                                                      uint32_t* __restrict__ pairs, uint32_t cap, unsigned long long* __restrict__ ctr) {
  if (blockIdx.x == 0 && threadIdx.x == 0) ctr[CTR_PAIRS] += start[G.ntx * G.nty];
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    if (res[i].w == 0.f) continue;
    int x0, x1, y0, y1;
    if (!sample_rect_in(OP, xy[2 * (size_t)i], xy[2 * (size_t)i + 1], G.fw, G.fh, G.w, G.h, win_cover(W, win[i]), &x0, &x1, &y0, &y1))
      continue;
    for (int ty = y0 >> 4; ty <= y1 >> 4; ++ty)
      for (int tx = x0 >> 4; tx <= x1 >> 4; ++tx) {
        const int t = ty * G.ntx + tx;
        const uint32_t slot = start[t] + (atomicSub(&cnt[t], 1u) - 1u);
        if (slot < cap) pairs[slot] = i;
      }
  }
}

// what a chunk's tile kernel needs to know of its place in the list: the windows of its first and last sample,
// and whether the first began in an earlier chunk (the carry image holds its tile so far) or the last goes on in
// the next (the carry image receives it)
struct WinChunk {
  uint32_t wfirst, wlast;
  int carry_in, carry_out;
};

// k_img_tile with a tile accumulator beside the film's: t sums the current window's samples from +0, and
// a = a + t at every change of window for the lanes whose pixel that window's tile is added to.
template <int OP>
__global__ __launch_bounds__(256) void k_imgw_tile(const float* __restrict__ xy, const float4* __restrict__ res,
                                                   const uint32_t* __restrict__ win, ImgGeom G, ImgTable T, WinTable W, WinChunk C,
                                                   const uint32_t* __restrict__ start, uint32_t* pairs, uint32_t cap,
                                                   float* __restrict__ target, float* __restrict__ carry) {
  __shared__ uint32_t sk[SM_LDS_RECORDS];
  __shared__ float4 sres[kStage];
  __shared__ float2 spos[kStage];
  __shared__ uint32_t swin[kStage];
  __shared__ float tbl[256];
  const uint32_t s = start[blockIdx.x], len = min(start[blockIdx.x + 1], cap) - min(s, cap);
  // nothing to add, and no carried tile to fold or to hand on
  if (len == 0 && ((!C.carry_in && !C.carry_out) || (C.carry_in && C.carry_out && C.wfirst == C.wlast))) return;
  tbl[threadIdx.x] = T.v[threadIdx.x];
  uint32_t* seg = pairs + s;
  if (len <= SM_LDS_RECORDS) {
    for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) sk[i] = seg[i];
    __syncthreads();
    ImgLds x{sk};
    sm_bitonic(x, len);
    for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) seg[i] = sk[i];
  } else {
    ImgGlobal x{seg};
    sm_bitonic(x, len);
  }
  constexpr int NC = OP == OP_SPLAT ? 3 : 4;
  const int tx0 = (int)(blockIdx.x % (uint32_t)G.ntx) * 16, ty0 = (int)(blockIdx.x / (uint32_t)G.ntx) * 16;
  const int lx = (int)(threadIdx.x & 15u), ly = (int)(threadIdx.x >> 4);
  const int x = tx0 + lx, y = ty0 + ly;
  const bool own = x < G.w && y < G.h;
  const size_t po = own ? (size_t)NC * ((size_t)y * G.w + x) : 0;
  float* o = target + po;
  float a[NC], t[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    a[c] = own ? o[c] : 0.f;
    t[c] = own && C.carry_in ? carry[po + c] : 0.f;
  }
  uint32_t cur = C.wfirst;
  // addTile of window k for this lane's pixel
  auto fold = [&](uint32_t k) {
    const Rect r = win_cover(W, k);
    const bool in = x >= r.x0 && x <= r.x1 && y >= r.y0 && y <= r.y1;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (in) a[c] = a[c] + t[c];
      t[c] = 0.f;
    }
  };
  const float ifw = 1.f / G.fw, ifh = 1.f / G.fw;                        // trap T12
  for (uint32_t base = 0; base < len; base += kStage) {
    const uint32_t m = min(kStage, len - base);
    __syncthreads();                                                    // the sorted segment is written; the previous round is consumed
    for (uint32_t e = threadIdx.x; e < m; e += blockDim.x) {
      const uint32_t i = seg[base + e];
      const float sx = xy[2 * (size_t)i], sy = xy[2 * (size_t)i + 1];
      const uint32_t k = win[i];
      int x0, x1, y0, y1;
      sample_rect_in(OP, sx, sy, G.fw, G.fh, G.w, G.h, win_cover(W, k), &x0, &x1, &y0, &y1);
      const uint32_t rect = (uint32_t)(max(x0, tx0) - tx0) | (uint32_t)(min(x1, tx0 + 15) - tx0) << 4 |
                            (uint32_t)(max(y0, ty0) - ty0) << 8 | (uint32_t)(min(y1, ty0 + 15) - ty0) << 12;
      const float4 r = res[i];
      sres[e] = make_float4(r.x, r.y, r.z, __uint_as_float(rect));
      spos[e] = make_float2(sx - 0.5f, sy - 0.5f);
      swin[e] = k;
    }
    __syncthreads();
    if (own)
      for (uint32_t j = 0; j < m; ++j) {
        const uint32_t k = swin[j];
        if (k != cur) { fold(cur); cur = k; }
        const float4 r = sres[j];
        const uint32_t rect = __float_as_uint(r.w);
        if (lx < (int)(rect & 15u) || lx > (int)(rect >> 4 & 15u) || ly < (int)(rect >> 8 & 15u) || ly > (int)(rect >> 12 & 15u)) continue;
        if (OP == OP_ADD) {
          const float2 d = spos[j];
          const float fltw = tbl[table_index(y, d.y, ifh) * 16 + table_index(x, d.x, ifw)];
          const float vx = r.x * fltw, vy = r.y * fltw, vz = r.z * fltw;
          t[0] = t[0] + fltw; t[1] = t[1] + vx; t[2] = t[2] + vy; t[3] = t[3] + vz;
        } else if (OP == OP_UNFILTERED) {
          t[0] = t[0] + 1.f; t[1] = t[1] + r.x; t[2] = t[2] + r.y; t[3] = t[3] + r.z;
        } else {
          t[0] = t[0] + r.x; t[1] = t[1] + r.y; t[2] = t[2] + r.z;
        }
      }
  }
  if (own) {
    if (C.carry_out && cur == C.wlast) {
#pragma unroll
      for (int c = 0; c < NC; ++c) carry[po + c] = t[c];               // the window goes on in the next chunk
    } else {
      fold(cur);
      if (C.carry_out) {
#pragma unroll
        for (int c = 0; c < NC; ++c) carry[po + c] = 0.f;              // the last window has not reached this tile yet
      }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) o[c] = a[c];
  }
}

// scaleSplats (Image.hs:93-106): one binary32 product a value
__global__ __launch_bounds__(256) void k_img_scale_splats(float* __restrict__ splat, const float* __restrict__ factors, float scalar,
                                                          size_t px) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < px; i += (size_t)gridDim.x * blockDim.x) {
    const float s = factors ? factors[i] : scalar;
    splat[3 * i] = splat[3 * i] * s; splat[3 * i + 1] = splat[3 * i + 1] * s; splat[3 * i + 2] = splat[3 * i + 2] * s;
  }
}

// the most tiles a sample's rectangle can meet along an axis of nt tiles: its span is at most
// floor (d + fw) - ceiling (d - fw) + 1 <= 2 fw + 1 pixels, widened for the binary32 roundings of d +- fw
// (|d| <= 2^20 + 1/2), and a span of S pixels meets at most (S + 14) / 16 + 1 tiles
uint32_t axis_tiles(int op, float fw, int nt) {
  if (op != OP_ADD) return 1u;
  const double span = std::floor(2.0 * (double)fw * (1.0 + 1e-6)) + 4.0;
  if (span >= 16.0 * nt) return (uint32_t)nt;
  return std::min<uint32_t>((uint32_t)nt, ((uint32_t)span + 14u) / 16u + 1u);
}

template <int OP>
void chunk_launch(bling_ctx* c, const float* xy, const float* spectra, uint32_t m, const ImgGeom& G, const ImgTable& T, uint32_t cap,
                  float* target) {
  ImageState& I = c->image;
  hipStream_t s = c->stream;
  const uint32_t nt = (uint32_t)G.ntx * (uint32_t)G.nty;
  HIPCHK(hipMemsetAsync(I.cnt.p, 0, (size_t)nt * sizeof(uint32_t), s));
  k_img_prep<OP><<<grid_for(m), 256, 0, s>>>(xy, spectra, m, G, I.res.p, I.cnt.p, I.ctr.p);
  sm_scan(s, I.cnt.p, nt, I.sums.p, I.start.p);
  k_img_scatter<OP><<<grid_for(m), 256, 0, s>>>(xy, I.res.p, m, G, I.start.p, I.cnt.p, I.pairs.p, cap, I.ctr.p);
  k_img_tile<OP><<<nt, 256, 0, s>>>(xy, I.res.p, G, T, I.start.p, I.pairs.p, cap, target);
  HIPCHK(hipGetLastError());
}

bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + nb && pb < pa + na;
}

void check_desc(const bling_image_desc* d) {
  if (d->width < 1 || d->height < 1) throw std::invalid_argument("image: width and height must be at least 1");
  if ((uint64_t)d->width * (uint64_t)d->height > ((uint64_t)1 << 28)) throw std::invalid_argument("image: more than 2^28 pixels");
}

size_t target_floats(const bling_image_desc* d, int op) { return (size_t)d->width * d->height * (op == OP_SPLAT ? 3 : 4); }

void check_add(const bling_ctx* c, const bling_image_desc* d, int op, const void* xy, const void* spectra, size_t n, const void* target) {
  if (!c || !d || !target || (n && (!xy || !spectra))) throw std::invalid_argument("null argument");
  if (op != OP_ADD && op != OP_UNFILTERED && op != OP_SPLAT) throw std::invalid_argument("image: unknown op " + std::to_string(op));
  check_desc(d);
  const float fw = d->filter.width, fh = d->filter.height;
  if (!(finite_f(fw) && finite_f(fh) && fw > 0.f && fh > 0.f)) throw std::invalid_argument("image: the filter size must be finite and positive");
  if ((((uintptr_t)xy | (uintptr_t)spectra | (uintptr_t)target) & 3u) != 0) throw std::invalid_argument("image: a buffer is not aligned to 4 bytes");
  const size_t nt = target_floats(d, op) * sizeof(float);
  if (n && (ranges_overlap(target, nt, xy, n * 8) || ranges_overlap(target, nt, spectra, n * 64)))
    throw std::invalid_argument("image: the target overlaps an input");
}

// the whole list, chunk after chunk, on the context's stream; returns after completion
void add_samples(bling_ctx* c, const bling_image_desc* d, int op, const float* xy, const float* spectra, size_t n, float* target,
                 bling_image_stats* st) {
  bling_image_stats out{};
  out.samples = n;
  if (n == 0) { if (st) *st = out; return; }
  HIPCHK(hipSetDevice(c->device));
  ImageState& I = c->image;
  ImgGeom G{d->width, d->height, (d->width + 15) / 16, (d->height + 15) / 16, d->filter.width, d->filter.height};
  ImgTable T;
  std::memcpy(T.v, d->filter.table, sizeof T.v);
  const uint32_t nt = (uint32_t)G.ntx * (uint32_t)G.nty;
  // a chunk's pairs fit the budget whatever its samples are; one sample alone may need more than a tiny budget
  const size_t per_sample = (size_t)axis_tiles(op, G.fw, G.ntx) * axis_tiles(op, G.fh, G.nty);
  const size_t budget = I.budget ? I.budget : kDefaultPairs;
  const size_t chunk = std::min(std::max<size_t>(1, budget / per_sample), kMaxChunk);
  const size_t cap = std::max(budget, per_sample);
  if (cap > 0x7FFFFFFFull) throw std::invalid_argument("image: pair budget beyond 2^31 - 1");
  if (I.cnt.n != nt) { I.cnt.alloc(nt); I.start.alloc((size_t)nt + 1); I.sums.alloc(((size_t)nt + 1023) / 1024 + 1); }
  if (I.pairs.n < std::min(cap, chunk * per_sample)) I.pairs.alloc(std::min(cap, chunk * per_sample));
  if (I.res.n < std::min(n, chunk)) I.res.alloc(std::min(n, chunk));
  if (!I.ctr.n) I.ctr.alloc(CTR_N);
  hipStream_t s = c->stream;
  HIPCHK(hipMemsetAsync(I.ctr.p, 0, CTR_N * sizeof(unsigned long long), s));
  EventPair ev;
  ev.a.record(s);
  for (size_t off = 0; off < n; off += chunk) {
    const uint32_t m = (uint32_t)std::min(chunk, n - off);
    const float *x = xy + 2 * off, *sp = spectra + 16 * off;
    const uint32_t pcap = (uint32_t)I.pairs.n;
    switch (op) {
      case OP_ADD: chunk_launch<OP_ADD>(c, x, sp, m, G, T, pcap, target); break;
      case OP_UNFILTERED: chunk_launch<OP_UNFILTERED>(c, x, sp, m, G, T, pcap, target); break;
      default: chunk_launch<OP_SPLAT>(c, x, sp, m, G, T, pcap, target); break;
    }
    ++out.chunks;
  }
  ev.b.record(s);
  unsigned long long ctr[CTR_N];
  HIPCHK(hipMemcpyAsync(ctr, I.ctr.p, sizeof ctr, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  out.dropped_spectrum = ctr[CTR_SPECTRUM];
  out.dropped_position = ctr[CTR_POSITION];
  out.tile_pairs = ctr[CTR_PAIRS];
  out.ms = ev.elapsed_ms();
  if (st) *st = out;
}

template <int OP>
void chunk_launch_windowed(bling_ctx* c, const float* xy, const float* spectra, uint32_t m, size_t off, const ImgGeom& G, const ImgTable& T,
                           const WinTable& W, const WinChunk& C, uint32_t cap, float* target) {
  ImageState& I = c->image;
  hipStream_t s = c->stream;
  const uint32_t nt = (uint32_t)G.ntx * (uint32_t)G.nty;
  HIPCHK(hipMemsetAsync(I.cnt.p, 0, (size_t)nt * sizeof(uint32_t), s));
  k_imgw_prep<OP><<<grid_for(m), 256, 0, s>>>(xy, spectra, m, (unsigned long long)off, G, W, I.res.p, I.win.p, I.cnt.p, I.ctr.p);
  sm_scan(s, I.cnt.p, nt, I.sums.p, I.start.p);
  k_imgw_scatter<OP><<<grid_for(m), 256, 0, s>>>(xy, I.res.p, I.win.p, m, G, W, I.start.p, I.cnt.p, I.pairs.p, cap, I.ctr.p);
  k_imgw_tile<OP><<<nt, 256, 0, s>>>(xy, I.res.p, I.win.p, G, T, W, C, I.start.p, I.pairs.p, cap, target, I.carry.p);
  HIPCHK(hipGetLastError());
}

// the cover rectangle of every window; throws for a first that does not ascend from 0 to n or a tile below 1 x 1
std::vector<int4> check_windows(const bling_image_desc* d, const bling_image_window* windows, const uint64_t* first, size_t nw, size_t n) {
  if (!first || (nw && !windows)) throw std::invalid_argument("null argument");
  if (nw > 0x7FFFFFFFull) throw std::invalid_argument("image: more than 2^31 - 1 windows");
  if (first[0] != 0 || first[nw] != n) throw std::invalid_argument("image: first must start at 0 and end at n");
  std::vector<int4> cover(nw);
  for (size_t k = 0; k < nw; ++k) {
    if (first[k] > first[k + 1]) throw std::invalid_argument("image: first is not ascending at window " + std::to_string(k));
    Tile t;
    if (!make_tile(windows[k].x0, windows[k].x1, windows[k].y0, windows[k].y1, d->filter.width, d->filter.height, &t))
      throw std::invalid_argument("image: window " + std::to_string(k) + ": its tile has a width or height below 1");
    const Rect r = tile_cover(t, d->width, d->height);
    cover[k] = make_int4(r.x0, r.y0, r.x1, r.y1);
  }
  return cover;
}

void check_add_windowed(const bling_ctx* c, const bling_image_desc* d, int op, const void* xy, const void* spectra, size_t n,
                        const void* film, const void* splat) {
  if (!c || !d) throw std::invalid_argument("null argument");
  const void* target = op == OP_SPLAT ? splat : film;
  check_add(c, d, op, xy, spectra, n, target);
  const void* other = op == OP_SPLAT ? film : splat;
  if (!other) return;
  const size_t no = target_floats(d, op == OP_SPLAT ? OP_ADD : OP_SPLAT) * sizeof(float);
  if (((uintptr_t)other & 3u) != 0) throw std::invalid_argument("image: a buffer is not aligned to 4 bytes");
  if (ranges_overlap(other, no, target, target_floats(d, op) * sizeof(float))) throw std::invalid_argument("image: film and splat overlap");
  if (n && (ranges_overlap(other, no, xy, n * 8) || ranges_overlap(other, no, spectra, n * 64)))
    throw std::invalid_argument("image: the target overlaps an input");
}

// the whole list window by window, chunk after chunk, on the context's stream; returns after completion
void add_windowed(bling_ctx* c, const bling_image_desc* d, int op, const std::vector<int4>& cover, const uint64_t* first, const float* xy,
                  const float* spectra, size_t n, float* film, float* splat, bling_image_stats* st) {
  bling_image_stats out{};
  out.samples = n;
  const size_t nw = cover.size();
  if (nw == 0) { if (st) *st = out; return; }
  HIPCHK(hipSetDevice(c->device));
  ImageState& I = c->image;
  ImgGeom G{d->width, d->height, (d->width + 15) / 16, (d->height + 15) / 16, d->filter.width, d->filter.height};
  ImgTable T;
  std::memcpy(T.v, d->filter.table, sizeof T.v);
  const uint32_t nt = (uint32_t)G.ntx * (uint32_t)G.nty;
  float* target = op == OP_SPLAT ? splat : film;
  const size_t per_sample = (size_t)axis_tiles(op, G.fw, G.ntx) * axis_tiles(op, G.fh, G.nty);
  const size_t budget = I.budget ? I.budget : kDefaultPairs;
  const size_t chunk = std::min(std::max<size_t>(1, budget / per_sample), kMaxChunk);
  const size_t cap = std::max(budget, per_sample);
  if (cap > 0x7FFFFFFFull) throw std::invalid_argument("image: pair budget beyond 2^31 - 1");
  // the chunks: each ends at the last window boundary within its budget, or inside a window longer than that
  struct Cut { size_t off, end; WinChunk C; };
  std::vector<Cut> cuts;
  bool carries = false;
  const uint64_t* fend = first + nw + 1;
  auto win_of_sample = [&](size_t g) { return (uint32_t)(std::upper_bound(first, fend, (uint64_t)g) - first - 1); };
  for (size_t off = 0; off < n;) {
    const size_t limit = std::min(off + chunk, n);
    const uint64_t boundary = *(std::upper_bound(first, fend, (uint64_t)limit) - 1);
    const size_t end = boundary > off ? (size_t)boundary : limit;
    WinChunk C{win_of_sample(off), win_of_sample(end - 1), 0, 0};
    C.carry_in = off > first[C.wfirst];
    C.carry_out = end < first[C.wlast + 1];
    carries = carries || C.carry_out;
    cuts.push_back(Cut{off, end, C});
    off = end;
  }
  if (n) {
    if (I.cnt.n != nt) { I.cnt.alloc(nt); I.start.alloc((size_t)nt + 1); I.sums.alloc(((size_t)nt + 1023) / 1024 + 1); }
    if (I.pairs.n < std::min(cap, chunk * per_sample)) I.pairs.alloc(std::min(cap, chunk * per_sample));
    if (I.res.n < std::min(n, chunk)) I.res.alloc(std::min(n, chunk));
    if (I.win.n < std::min(n, chunk)) I.win.alloc(std::min(n, chunk));
    if (carries && I.carry.n < target_floats(d, op)) I.carry.alloc(target_floats(d, op));
  }
  if (I.first.n < nw + 1) I.first.alloc(nw + 1);
  if (I.cover.n < nw) I.cover.alloc(nw);
  if (!I.ctr.n) I.ctr.alloc(CTR_N);
  hipStream_t s = c->stream;
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "first is uploaded as it is");
  HIPCHK(hipMemcpyAsync(I.first.p, first, (nw + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(I.cover.p, cover.data(), nw * sizeof(int4), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(I.ctr.p, 0, CTR_N * sizeof(unsigned long long), s));
  const WinTable W{I.first.p, I.cover.p, (uint32_t)nw};
  EventPair ev;
  ev.a.record(s);
  k_imgw_cover<<<grid_for((uint32_t)std::min<size_t>(nw, 1u << 19) * 256u), 256, 0, s>>>(W, G.w, reinterpret_cast<uint32_t*>(film),
                                                                                       reinterpret_cast<uint32_t*>(splat));
  HIPCHK(hipGetLastError());
  for (const Cut& q : cuts) {
    const uint32_t m = (uint32_t)(q.end - q.off);
    const float *x = xy + 2 * q.off, *sp = spectra + 16 * q.off;
    const uint32_t pcap = (uint32_t)I.pairs.n;
    switch (op) {
      case OP_ADD: chunk_launch_windowed<OP_ADD>(c, x, sp, m, q.off, G, T, W, q.C, pcap, target); break;
      case OP_UNFILTERED: chunk_launch_windowed<OP_UNFILTERED>(c, x, sp, m, q.off, G, T, W, q.C, pcap, target); break;
      default: chunk_launch_windowed<OP_SPLAT>(c, x, sp, m, q.off, G, T, W, q.C, pcap, target); break;
    }
    ++out.chunks;
  }
  ev.b.record(s);
  unsigned long long ctr[CTR_N];
  HIPCHK(hipMemcpyAsync(ctr, I.ctr.p, sizeof ctr, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  out.dropped_spectrum = ctr[CTR_SPECTRUM];
  out.dropped_position = ctr[CTR_POSITION];
  out.tile_pairs = ctr[CTR_PAIRS];
  out.ms = ev.elapsed_ms();
  if (st) *st = out;
}

}  // namespace
}  // namespace bcore

extern "C" {

int bling_image_add_samples_device(bling_ctx* c, const bling_image_desc* d, int op, const void* xy, const void* spectra, size_t n,
                                   void* target, bling_image_stats* st) {
  return guarded([&] {
    check_add(c, d, op, xy, spectra, n, target);
    add_samples(c, d, op, static_cast<const float*>(xy), static_cast<const float*>(spectra), n, static_cast<float*>(target), st);
    return BLING_OK;
  });
}

int bling_image_add_samples(bling_ctx* c, const bling_image_desc* d, int op, const float* xy, const float* spectra, size_t n,
                            float* target, bling_image_stats* st) {
  return guarded([&] {
    check_add(c, d, op, xy, spectra, n, target);
    if (n == 0) { add_samples(c, d, op, nullptr, nullptr, 0, nullptr, st); return BLING_OK; }
    HIPCHK(hipSetDevice(c->device));
    ImageState& I = c->image;
    const size_t nf = target_floats(d, op);
    if (I.xy.n < 2 * n) { I.xy.alloc(2 * n); I.spectra.alloc(16 * n); }
    if (I.target.n < nf) I.target.alloc(nf);
    hipStream_t s = c->stream;
    HIPCHK(hipMemcpyAsync(I.xy.p, xy, n * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(I.spectra.p, spectra, n * 64, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(I.target.p, target, nf * sizeof(float), hipMemcpyHostToDevice, s));
    add_samples(c, d, op, I.xy.p, I.spectra.p, n, I.target.p, st);
    HIPCHK(hipMemcpyAsync(target, I.target.p, nf * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return BLING_OK;
  });
}

int bling_image_add_windowed_device(bling_ctx* c, const bling_image_desc* d, int op, const bling_image_window* windows,
                                    const uint64_t* first, size_t n_windows, const void* xy, const void* spectra, size_t n, void* film,
                                    void* splat, bling_image_stats* st) {
  return guarded([&] {
    check_add_windowed(c, d, op, xy, spectra, n, film, splat);
    const std::vector<int4> cover = check_windows(d, windows, first, n_windows, n);
    add_windowed(c, d, op, cover, first, static_cast<const float*>(xy), static_cast<const float*>(spectra), n, static_cast<float*>(film),
                 static_cast<float*>(splat), st);
    return BLING_OK;
  });
}

int bling_image_add_windowed(bling_ctx* c, const bling_image_desc* d, int op, const bling_image_window* windows, const uint64_t* first,
                             size_t n_windows, const float* xy, const float* spectra, size_t n, float* film, float* splat,
                             bling_image_stats* st) {
  return guarded([&] {
    check_add_windowed(c, d, op, xy, spectra, n, film, splat);
    const std::vector<int4> cover = check_windows(d, windows, first, n_windows, n);
    HIPCHK(hipSetDevice(c->device));
    ImageState& I = c->image;
    const size_t nfilm = target_floats(d, OP_ADD), nsplat = target_floats(d, OP_SPLAT);
    if (n && I.xy.n < 2 * n) { I.xy.alloc(2 * n); I.spectra.alloc(16 * n); }
    if (film && I.target.n < nfilm) I.target.alloc(nfilm);
    if (splat && I.target2.n < nsplat) I.target2.alloc(nsplat);
    hipStream_t s = c->stream;
    if (n) {
      HIPCHK(hipMemcpyAsync(I.xy.p, xy, n * 8, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(I.spectra.p, spectra, n * 64, hipMemcpyHostToDevice, s));
    }
    if (film) HIPCHK(hipMemcpyAsync(I.target.p, film, nfilm * sizeof(float), hipMemcpyHostToDevice, s));
    if (splat) HIPCHK(hipMemcpyAsync(I.target2.p, splat, nsplat * sizeof(float), hipMemcpyHostToDevice, s));
    add_windowed(c, d, op, cover, first, I.xy.p, I.spectra.p, n, film ? I.target.p : nullptr, splat ? I.target2.p : nullptr, st);
    if (film) HIPCHK(hipMemcpyAsync(film, I.target.p, nfilm * sizeof(float), hipMemcpyDeviceToHost, s));
    if (splat) HIPCHK(hipMemcpyAsync(splat, I.target2.p, nsplat * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return BLING_OK;
  });
}

int bling_image_scale_splats_device(bling_ctx* c, const bling_image_desc* d, void* splat, const void* factors, float scalar) {
  return guarded([&] {
    if (!c || !d || !splat) throw std::invalid_argument("null argument");
    check_desc(d);
    const size_t px = (size_t)d->width * d->height;
    if ((((uintptr_t)splat | (uintptr_t)factors) & 3u) != 0) throw std::invalid_argument("image: a buffer is not aligned to 4 bytes");
    if (factors && ranges_overlap(splat, px * 12, factors, px * 4)) throw std::invalid_argument("image: splat overlaps factors");
    HIPCHK(hipSetDevice(c->device));
    k_img_scale_splats<<<grid_for((uint32_t)px), 256, 0, c->stream>>>(static_cast<float*>(splat), static_cast<const float*>(factors), scalar, px);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return BLING_OK;
  });
}

int bling_image_develop_device(bling_ctx* c, const bling_image_desc* d, const bling_develop_params* dp, const void* film,
                               const void* splat, void* out) {
  return guarded([&] {
    if (!c || !d || !dp || !film || !out) throw std::invalid_argument("null argument");
    check_desc(d);
    if (dp->format != BLING_DEVELOP_RGB_F32 && dp->format != BLING_DEVELOP_RGB8 && dp->format != BLING_DEVELOP_RGBE)
      throw std::invalid_argument("develop: unknown format " + std::to_string(dp->format));
    const size_t px = (size_t)d->width * d->height, nout = px * develop_pixel_bytes(dp->format);
    if (ranges_overlap(out, nout, film, px * 16) || (splat && ranges_overlap(out, nout, splat, px * 12)))
      throw std::invalid_argument("develop: out overlaps the film or the splat buffer");
    HIPCHK(hipSetDevice(c->device));
    develop_launch(c, dp, d->width, d->height, static_cast<const float*>(film), static_cast<const float*>(splat), out);
    HIPCHK(hipStreamSynchronize(c->stream));
    return BLING_OK;
  });
}

int bling_debug_set_image_budget(bling_ctx* c, size_t max_tile_pairs) {
  if (!c) { set_last_error("null argument"); return BLING_EINVAL; }
  c->image.budget = max_tile_pairs;
  return BLING_OK;
}

}  // extern "C"
