// mlt.h -- the Metropolis renderer (Renderer/Metropolis.hs) on the device: primary-sample-space
// Metropolis over the bidirectional integrator (mkBidirPathIntegrator md md, :46-49).  A pass runs C
// independent chains (the one departure); one mutation step of all live chains is
//   k_mlt_propose   one lane per chain: mutate (:191-219) -- the large-step test, then initialSample
//                   (:171-189) or one jitter (:221-239) per value -- into the proposal vectors
//   k_mlt_walk      bidir.h's two subpaths per chain, the sample values read from a primary sample
//   k_bd_connect, k_bd_finish   unchanged (they draw nothing)
//   k_mlt_accept    evalI (:241-242), a = min 1 (iProp / iCurr), the two guarded splats (:96-104) as
//                   float atomics or as splat records for the ordered merge (MltBufs::srec, splat_merge.h),
//                   the acceptance (:106-110) and the optional record
// Bootstrap samples (:142-169) and each chain's first evaluation (:84) go through the same walk
// (k_mlt_fill writes their vectors).  A primary sample is n1d + 2 n2d + 4 floats -- v1d, v2d, then the
// camera sample's x, y, lu, lv -- stored [value][chain], so a wave's loads and stores are contiguous.
//
// Keys (common/counter_rng.h; the pixel tags sit beside LT_PIXEL and SPPM_PHOTON_PIXEL, sppm.h): chain c
// draws from pixel_key(seed, pass, MLT_CHAIN_PIXEL | c), its mutation m from sample_key(pk, m), the
// start selection from sample_key(pk, MLT_START_SAMPLE); bootstrap sample i from
// sample_key(pixel_key(seed, pass, MLT_BOOT_PIXEL), i).  The dimension is DIM_FRESH1D + the ordinal of
// the draw in the reference's order (rnd2D = two draws).
#pragma once
#include "bidir.h"
#include "splat_merge.h"

namespace bd {

constexpr uint32_t MLT_CHAIN_PIXEL = 0x50000000u;    // | chain (< MLT_MAX_CHAINS)
constexpr uint32_t MLT_BOOT_PIXEL = 0x60000000u;
constexpr uint32_t MLT_START_SAMPLE = 0xFFFFFFFEu;   // no mutation index reaches it (M < 2^31)
constexpr uint32_t MLT_MAX_CHAINS = 1u << 20;

// The primary sample of lane j as a sample source of bd_walks: v[row * stride].  Nothing bounds dim here:
// with sd = md the largest dimensions bd_walks reads are 1D 12 md - 8 and 2D 9 md - 4, below n1d = 12 md + 1
// and n2d = 9 md + 2 (the rows of a sample).  tests/ref/mlt_ref.cpp aborts if an evaluation reads past them,
// and the device's records are pinned on it; a change of bidir.h's dimensions has to keep that.
struct PssKey { const float* v; uint32_t stride; int n1d; };
DEV float rnd1(const DevScene&, const PssKey& k, int dim) { return k.v[(size_t)dim * k.stride]; }
DEV void rnd2(const DevScene&, const PssKey& k, int dim, float* a, float* b) {
  *a = k.v[(size_t)(k.n1d + 2 * dim) * k.stride];
  *b = k.v[(size_t)(k.n1d + 2 * dim + 1) * k.stride];
}

// The chains' state of one pass; a record of record mode is 32 bytes (include/bling.h bling_mlt_record)
struct MltBufs {
  float* cur;                // [nv][cap] the chains' current primary samples
  float* prop;               // [nv][cap] the proposals (bootstrap: the chunk's samples)
  float* cur_l;              // [18][cap] the current sample's imageX, imageY and spectrum
  uint32_t* flags;           // per chain: bit 0 large step, bits 1.. the acceptance draw's ordinal
  float* splat;              // W * H * 3 (X, Y, Z), accumulated; nullptr = off
  unsigned long long* ctr;   // [0] large steps, [1] accepted, [2] dropped splats, [3] splats
  uint4* rec;                // record mode: 2 uint4 per (chain, mutation) of chains rec_first ..; nullptr = off
  uint32_t rec_first, rec_chains;
  uint4* srec;               // ordered mode: 2 uint4 per splat (splat_merge.h SM_LAYOUT_SPLAT), key = chain << 32 |
                             // mutation << 1 | proposal; nullptr = off
  uint32_t* srec_count;      // slots claimed
  uint32_t srec_cap;
  uint32_t cap;
  int n1d, n2d;
  float sx, sy;              // the image size (mutate's imgSize)
  float wt, plarge;          // 1 / mpp
};
DEV int mlt_nv(const MltBufs& B) { return B.n1d + 2 * B.n2d + 4; }

// jitter (:221-239): one rnd2D unless vmin == vmax; a = 1 / 1024, b = 1 / 256
DEV float mlt_jitter(const SampleKey& k, uint32_t& ord, float v, float vmin, float vmax) {
  if (vmin == vmax) return vmin;
  const float u1 = draw01(k, brng::DIM_FRESH1D + ord), u2 = draw01(k, brng::DIM_FRESH1D + ord + 1u);
  ord += 2u;
  const float a = 1.f / 1024.f, b = 1.f / 256.f;
  const float logRat = -bcr::logf(b / a);
  const float delta = (vmax - vmin) * b * bcr::expf(logRat * u1);
  const float x = u2 < 0.5f ? v + delta : v - delta;
  if (x >= vmax) return vmin + (x - vmax);                             // wrapAround
  if (x < vmin) return vmax - (vmin - x);
  return x;
}

// initialSample (:171-189) from ordinal ord on into column j of dst
DEV void mlt_initial(const MltBufs& B, const SampleKey& k, uint32_t& ord, float* dst, uint32_t j) {
  const int nr = B.n1d + 2 * B.n2d;
  for (int r = 0; r < nr; ++r) dst[(size_t)r * B.cap + j] = draw01(k, brng::DIM_FRESH1D + ord++);
  const float ox = draw01(k, brng::DIM_FRESH1D + ord), oy = draw01(k, brng::DIM_FRESH1D + ord + 1u);
  const float lu = draw01(k, brng::DIM_FRESH1D + ord + 2u), lv = draw01(k, brng::DIM_FRESH1D + ord + 3u);
  ord += 4u;
  dst[(size_t)nr * B.cap + j] = (1.f - ox) * 0.f + ox * B.sx;          // lerp ox 0 sx (Math.hs:108-110)
  dst[(size_t)(nr + 1) * B.cap + j] = (1.f - oy) * 0.f + oy * B.sy;
  dst[(size_t)(nr + 2) * B.cap + j] = lu;
  dst[(size_t)(nr + 3) * B.cap + j] = lv;
}

// Bootstrap samples: lane j < n writes sample list[j] (list != nullptr: a chain's start) or first + j
// into column j of dst.
static __global__ __launch_bounds__(256) void k_mlt_fill(MltBufs B, float* __restrict__ dst, const uint32_t* __restrict__ list,
                                                  uint32_t first, uint32_t n, uint32_t seed, uint32_t pass) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n || j >= B.cap) return;
  const uint32_t i = list ? list[j] : first + j;
  const SampleKey k = sample_key(seed, pass, MLT_BOOT_PIXEL, i);
  uint32_t ord = 0u;
  mlt_initial(B, k, ord, dst, j);
}

// mutate (:191-211) of chain c < n, mutation m
static __global__ __launch_bounds__(256) void k_mlt_propose(MltBufs B, uint32_t n, uint32_t m, uint32_t seed, uint32_t pass) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n || c >= B.cap) return;
  const SampleKey k = sample_key(seed, pass, MLT_CHAIN_PIXEL | c, m);
  uint32_t ord = 1u;
  const bool large = draw01(k, brng::DIM_FRESH1D) < B.plarge;
  if (large) {
    mlt_initial(B, k, ord, B.prop, c);
  } else {
    const int nr = B.n1d + 2 * B.n2d;
    for (int r = 0; r < nr + 4; ++r) {                                 // v1d, v2d (u1 then u2), then x, y, lu, lv
      const float vmax = r == nr ? B.sx : r == nr + 1 ? B.sy : 1.f;
      const size_t at = (size_t)r * B.cap + c;
      B.prop[at] = mlt_jitter(k, ord, B.cur[at], 0.f, vmax);
    }
  }
  B.flags[c] = (ord << 1) | (large ? 1u : 0u);
}

// evalSample (:244-252) of the primary samples in vec: both subpaths of lane j < n, as k_bd_walk
template <uint32_t F>
static __global__ __launch_bounds__(256) void k_mlt_walk(const DevScene* __restrict__ Sptr, WaveState W, BdBufs B,
                                                  const float* __restrict__ vec, uint32_t stride, int n1d, int n2d,
                                                  uint32_t n, Counters* __restrict__ C) {
  extern __shared__ float4 smem[];
  const DevScene& S = *Sptr;
  const LdsScene L = lds_setup(S, smem);
  const uint32_t sid = blockIdx.x * blockDim.x + threadIdx.x;
  BdRays R{0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
  if (sid < n && sid < B.cap && sid < stride) {
    const PssKey k{vec + sid, stride, n1d};
    const float* cs = vec + (size_t)(n1d + 2 * n2d) * stride + sid;
    const float imx = cs[0], imy = cs[stride];
    const Ray cam = fire_ray(S.camera, imx, imy, cs[2 * (size_t)stride], cs[3 * (size_t)stride]);
    W.img[sid] = make_float2(imx, imy);
    uint32_t emask, lmask;
    int ne, nl;
    Sp le = sconst(0.f), lalpha;
    Ray lray;
    V3 lwi;
    bd_light_start<F, PssKey>(S, k, lray, lwi, lalpha);
    bd_walks<F, PssKey>(S, L, B, sid, k, lray, lwi, lalpha, cam, ne, nl, emask, lmask, le, R);
    bd_store_sp(B.le, sid, le);
    B.info[sid] = make_uint4((uint32_t)ne, (uint32_t)nl, emask, lmask);
  }
  bd_flush(C, R);
}

// evalI (:241-242) of a chunk's bootstrap samples
static __global__ __launch_bounds__(256) void k_mlt_boot_i(const float4* __restrict__ Lfull, uint32_t n, float* __restrict__ out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) out[j] = sY(bd_load_sp(Lfull, j));
}

// The chains' start: the evaluated start sample (in prop) becomes the current one (:83-84)
static __global__ __launch_bounds__(256) void k_mlt_adopt(MltBufs B, const float4* __restrict__ Lfull, uint32_t n) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n || c >= B.cap) return;
  const int nv = mlt_nv(B);
  for (int r = 0; r < nv; ++r) B.cur[(size_t)r * B.cap + c] = B.prop[(size_t)r * B.cap + c];
  B.cur_l[c] = B.prop[(size_t)(nv - 4) * B.cap + c];
  B.cur_l[(size_t)B.cap + c] = B.prop[(size_t)(nv - 3) * B.cap + c];
  const Sp l = bd_load_sp(Lfull, c);
#pragma unroll
  for (int q = 0; q < 16; ++q) B.cur_l[(size_t)(2 + q) * B.cap + c] = l.v[q];
}

// splat (:68-69) then splatSample (Image.hs:201-221): outside the image first, then the NaN / infinite filter
DEV void mlt_splat(const DevScene& S, const MltBufs& B, float x, float y, const Sp& s, unsigned long long key,
                   unsigned long long& splats, unsigned long long& dropped) {
  const float fx = floorf(x), fy = floorf(y);
  if (!(fx >= 0.f && fy >= 0.f && fx < (float)S.width && fy < (float)S.height)) return;
  if (s_bad(s)) { ++dropped; return; }
  float X, Y, Z;
  to_xyz(s, &X, &Y, &Z);
  ++splats;
  if (B.splat) {
    float* o = B.splat + 3 * ((size_t)(int)fy * S.width + (int)fx);
    atomicAdd(&o[0], X); atomicAdd(&o[1], Y); atomicAdd(&o[2], Z);
  }
  if (B.srec) {
    const uint32_t slot = atomicAdd(B.srec_count, 1u);
    if (slot < B.srec_cap) sm_write_rec(B.srec, slot, (uint32_t)(int)fy * (uint32_t)S.width + (uint32_t)(int)fx, key, X, Y, Z);
  }
}

// The body of the mutation loop after evalSample (:90-110) for chain c < n, mutation m
static __global__ __launch_bounds__(256) void k_mlt_accept(const DevScene* __restrict__ Sptr, MltBufs B,
                                                    const float4* __restrict__ Lfull, uint32_t n, uint32_t m, uint32_t seed,
                                                    uint32_t pass) {
  const DevScene& S = *Sptr;
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long larges = 0, accepted = 0, dropped = 0, splats = 0;
  if (c < n && c < B.cap) {
    const int nv = mlt_nv(B);
    const Sp lp = bd_load_sp(Lfull, c);
    const float xp = B.prop[(size_t)(nv - 4) * B.cap + c], yp = B.prop[(size_t)(nv - 3) * B.cap + c];
    Sp lc;
#pragma unroll
    for (int q = 0; q < 16; ++q) lc.v[q] = B.cur_l[(size_t)(2 + q) * B.cap + c];
    const float xc = B.cur_l[c], yc = B.cur_l[(size_t)B.cap + c];
    const float iProp = sY(lp), iCurr = sY(lc);
    const float q = iProp / iCurr;
    const float a = 1.f <= q ? 1.f : q;                                // GHC's min 1 q: NaN stays NaN
    const unsigned long long okey = ((unsigned long long)c << 32) | ((unsigned long long)m << 1);   // the current sample first
    if (iCurr > 0.f && !__builtin_isinf(1.f / iCurr)) mlt_splat(S, B, xc, yc, sscale(lc, (1.f - a) / iCurr * B.wt), okey, splats, dropped);
    if (iProp > 0.f && !__builtin_isinf(1.f / iProp)) mlt_splat(S, B, xp, yp, sscale(lp, a / iProp * B.wt), okey | 1ull, splats, dropped);
    const uint32_t fl = B.flags[c];
    const SampleKey k = sample_key(seed, pass, MLT_CHAIN_PIXEL | c, m);
    const float r = draw01(k, brng::DIM_FRESH1D + (fl >> 1));
    const bool acc = r < a;
    if (fl & 1u) ++larges;
    if (acc) {
      ++accepted;
      for (int rr = 0; rr < nv; ++rr) B.cur[(size_t)rr * B.cap + c] = B.prop[(size_t)rr * B.cap + c];
      B.cur_l[c] = xp; B.cur_l[(size_t)B.cap + c] = yp;
#pragma unroll
      for (int qq = 0; qq < 16; ++qq) B.cur_l[(size_t)(2 + qq) * B.cap + c] = lp.v[qq];
    }
    if (B.rec && c >= B.rec_first && c - B.rec_first < B.rec_chains) {
      const size_t slot = (size_t)m * B.rec_chains + (c - B.rec_first);
      B.rec[2 * slot] = make_uint4(c, m, __float_as_uint(xp), __float_as_uint(yp));
      B.rec[2 * slot + 1] = make_uint4(__float_as_uint(iProp), __float_as_uint(a), (fl & 1u) | (acc ? 2u : 0u), 0u);
    }
  }
  const unsigned long long wl = wave_sum_u64(larges), wa = wave_sum_u64(accepted), wd = wave_sum_u64(dropped),
                           ws = wave_sum_u64(splats);
  if ((threadIdx.x & 63) == 0) {
    if (wl) atomicAdd(&B.ctr[0], wl);
    if (wa) atomicAdd(&B.ctr[1], wa);
    if (wd) atomicAdd(&B.ctr[2], wd);
    if (ws) atomicAdd(&B.ctr[3], ws);
  }
}

}  // namespace bd
