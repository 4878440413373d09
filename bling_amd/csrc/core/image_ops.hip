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

}  // namespace
}  // namespace bcore

extern "C" {

int bling_image_add_samples_device(bling_ctx* c, const bling_image_desc* d, int op, const void* xy, const void* spectra, size_t n,
                                   void* target, bling_image_stats* st) {
  return guarded([&] {
    check_add(c, d, op, xy, spectra, n, target);
    add_samples(c, d, op, static_cast<const float*>(xy), static_cast<const float*>(spectra), n, static_cast<float*>(target), st);
    return (int)BLING_OK;
  });
}

int bling_image_add_samples(bling_ctx* c, const bling_image_desc* d, int op, const float* xy, const float* spectra, size_t n,
                            float* target, bling_image_stats* st) {
  return guarded([&] {
    check_add(c, d, op, xy, spectra, n, target);
    if (n == 0) { add_samples(c, d, op, nullptr, nullptr, 0, nullptr, st); return (int)BLING_OK; }
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
    return (int)BLING_OK;
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
    return (int)BLING_OK;
  });
}

int bling_debug_set_image_budget(bling_ctx* c, size_t max_tile_pairs) {
  if (!c) { set_last_error("null argument"); return BLING_EINVAL; }
  c->image.budget = max_tile_pairs;
  return BLING_OK;
}

}  // extern "C"
