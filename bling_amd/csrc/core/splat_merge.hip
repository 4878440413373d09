// splat_merge.hip -- the kernels and the host driver of the ordered splat merge (splat_merge.h).
#include "core_internal.h"

namespace bcore {

namespace {

constexpr uint32_t kScanChunk = 1024;        // counts per block of the scan: 256 lanes x 4
constexpr uint32_t kStage = 256;             // values staged per round of the sequential add
constexpr uint32_t kStageStride = kStage + 1;   // the three channels' rows start in different banks

DEV void sm_load(const uint4* __restrict__ recs, size_t i, int layout, uint32_t W, uint32_t& pixel, unsigned long long& key) {
  const uint4 a = recs[2 * i];
  if (layout == SM_LAYOUT_LIGHT) {
    pixel = a.z < W ? a.w * W + a.z : 0xFFFFFFFFu;
    key = ((unsigned long long)a.x << 32) | a.y;
  } else {
    pixel = a.x;
    key = ((unsigned long long)a.w << 32) | a.z;
  }
}

__global__ __launch_bounds__(256) void k_sm_count(const uint4* __restrict__ recs, size_t n, int layout, uint32_t W,
                                                  uint32_t npix, uint32_t* __restrict__ cnt) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    uint32_t p;
    unsigned long long k;
    sm_load(recs, i, layout, W, p, k);
    if (p < npix) atomicAdd(&cnt[p], 1u);
  }
}

// the sum of the block's 256 values, in every lane
DEV uint32_t block_sum(uint32_t v, uint32_t* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (uint32_t s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  const uint32_t t = sh[0];
  __syncthreads();
  return t;
}

// the exclusive prefix of the block's 256 values (Hillis-Steele in LDS); *total receives their sum
DEV uint32_t block_excl(uint32_t v, uint32_t* sh, uint32_t* total) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {
    const uint32_t add = threadIdx.x >= d ? sh[threadIdx.x - d] : 0u;
    __syncthreads();
    sh[threadIdx.x] += add;
    __syncthreads();
  }
  const uint32_t incl = sh[threadIdx.x];
  *total = sh[255];
  __syncthreads();
  return incl - v;
}

__global__ __launch_bounds__(256) void k_sm_sums(const uint32_t* __restrict__ cnt, uint32_t npix, uint32_t* __restrict__ sums) {
  __shared__ uint32_t sh[256];
  const size_t base = (size_t)blockIdx.x * kScanChunk + 4u * threadIdx.x;
  uint32_t t = 0;
  for (uint32_t q = 0; q < 4; ++q)
    if (base + q < npix) t += cnt[base + q];
  const uint32_t s = block_sum(t, sh);
  if (threadIdx.x == 0) sums[blockIdx.x] = s;
}

// one block: sums[0 .. nb) becomes its exclusive prefix, sums[nb] the total
__global__ __launch_bounds__(256) void k_sm_scan_sums(uint32_t* __restrict__ sums, uint32_t nb) {
  __shared__ uint32_t sh[256];
  uint32_t carry = 0;
  for (uint32_t base = 0; base < nb; base += 256) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < nb ? sums[i] : 0u;
    uint32_t total;
    const uint32_t ex = block_excl(v, sh, &total);
    if (i < nb) sums[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) sums[nb] = carry;
}

__global__ __launch_bounds__(256) void k_sm_starts(const uint32_t* __restrict__ cnt, uint32_t npix, const uint32_t* __restrict__ sums,
                                                   uint32_t nb, uint32_t* __restrict__ start) {
  __shared__ uint32_t sh[256];
  const size_t base = (size_t)blockIdx.x * kScanChunk + 4u * threadIdx.x;
  uint32_t v[4], t = 0;
  for (uint32_t q = 0; q < 4; ++q) {
    v[q] = base + q < npix ? cnt[base + q] : 0u;
    t += v[q];
  }
  uint32_t total;
  uint32_t at = sums[blockIdx.x] + block_excl(t, sh, &total);
  for (uint32_t q = 0; q < 4; ++q) {
    if (base + q < npix) start[base + q] = at;
    at += v[q];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) start[npix] = sums[nb];
}

// cnt counts down: the slots of a pixel are claimed in any order, each once
__global__ __launch_bounds__(256) void k_sm_scatter(const uint4* __restrict__ recs, size_t n, int layout, uint32_t W, uint32_t npix,
                                                    const uint32_t* __restrict__ start, uint32_t* __restrict__ cnt,
                                                    unsigned long long* __restrict__ key, float4* __restrict__ val) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    uint32_t p;
    unsigned long long k;
    sm_load(recs, i, layout, W, p, k);
    if (p >= npix) continue;
    const uint32_t slot = start[p] + (atomicSub(&cnt[p], 1u) - 1u);
    const uint4 b = recs[2 * i + 1];
    key[slot] = k;
    val[slot] = make_float4(__uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z), 0.f);
  }
}

// One lane per pixel.  A short segment is added by selection: the record with the smallest (key, position)
// beyond the last one added -- the position only so that equal keys (the debug hook may pass some) are all
// added.  longs[0] counts the listed pixels, longs[1 ..] holds them.
__global__ __launch_bounds__(256) void k_sm_short(const uint32_t* __restrict__ start, uint32_t npix,
                                                  const unsigned long long* __restrict__ key, const float4* __restrict__ val,
                                                  float* __restrict__ img, uint32_t* __restrict__ longs) {
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += gridDim.x * blockDim.x) {
    const uint32_t s = start[p], len = start[p + 1] - s;
    if (len == 0) continue;
    if (len > SM_SHORT) {
      longs[1u + atomicAdd(&longs[0], 1u)] = p;
      continue;
    }
    float* o = img + 3 * (size_t)p;
    float ax = o[0], ay = o[1], az = o[2];
    unsigned long long lastk = 0ull;
    uint32_t lastj = 0u;
    for (uint32_t t = 0; t < len; ++t) {
      unsigned long long bk = ~0ull;
      uint32_t bj = ~0u;
      for (uint32_t j = 0; j < len; ++j) {
        const unsigned long long k = key[s + j];
        const bool after = t == 0 || k > lastk || (k == lastk && j > lastj);
        const bool better = k < bk || (k == bk && j < bj);
        if (after && better) { bk = k; bj = j; }
      }
      const float4 v = val[s + bj];
      ax = ax + v.x; ay = ay + v.y; az = az + v.z;
      lastk = bk; lastj = bj;
    }
    o[0] = ax; o[1] = ay; o[2] = az;
  }
}

struct SmLds {          // (key, position) pairs in LDS
  unsigned long long* k;
  uint32_t* j;
  DEV void cswap(uint32_t lo, uint32_t hi) {
    const unsigned long long a = k[lo], b = k[hi];
    if (a > b) {
      k[lo] = b; k[hi] = a;
      const uint32_t t = j[lo]; j[lo] = j[hi]; j[hi] = t;
    }
  }
};

struct SmGlobal {       // keys and values of one segment, in place
  unsigned long long* k;
  float4* v;
  DEV void cswap(uint32_t lo, uint32_t hi) {
    const unsigned long long a = k[lo], b = k[hi];
    if (a > b) {
      k[lo] = b; k[hi] = a;
      const float4 t = v[lo]; v[lo] = v[hi]; v[hi] = t;
    }
  }
};

// One block per listed segment (grid-stride over the list).
__global__ __launch_bounds__(256) void k_sm_long(const uint32_t* __restrict__ start, unsigned long long* __restrict__ key,
                                                 float4* __restrict__ val, float* __restrict__ img, const uint32_t* __restrict__ longs) {
  __shared__ unsigned long long sk[SM_LDS_RECORDS];
  __shared__ uint32_t sj[SM_LDS_RECORDS];
  __shared__ float sv[3 * kStageStride];
  const uint32_t nlong = longs[0];
  for (uint32_t li = blockIdx.x; li < nlong; li += gridDim.x) {
    const uint32_t p = longs[1u + li];
    const uint32_t s = start[p], len = start[p + 1] - s;
    const bool in_lds = len <= SM_LDS_RECORDS;
    if (in_lds) {
      for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) { sk[i] = key[s + i]; sj[i] = i; }
      __syncthreads();
      SmLds x{sk, sj};
      sm_bitonic(x, len);
    } else {
      __syncthreads();
      SmGlobal x{key + s, val + s};
      sm_bitonic(x, len);
    }
    float acc = threadIdx.x < 3 ? img[3 * (size_t)p + threadIdx.x] : 0.f;
    for (uint32_t base = 0; base < len; base += kStage) {
      const uint32_t i = base + threadIdx.x;
      if (i < len) {
        const float4 v = val[s + (in_lds ? sj[i] : i)];
        sv[threadIdx.x] = v.x; sv[kStageStride + threadIdx.x] = v.y; sv[2 * kStageStride + threadIdx.x] = v.z;
      }
      __syncthreads();
      if (threadIdx.x < 3) {
        const uint32_t m = min(kStage, len - base);
        const float* row = sv + threadIdx.x * kStageStride;
        for (uint32_t q = 0; q < m; ++q) acc = acc + row[q];           // one at a time: the contract
      }
      __syncthreads();
    }
    if (threadIdx.x < 3) img[3 * (size_t)p + threadIdx.x] = acc;
  }
}

unsigned stride_grid(size_t items) { return (unsigned)std::max<size_t>(1, std::min<size_t>((items + 255) / 256, 4096)); }

}  // namespace

size_t splat_budget(bling_ctx* c) {
  if (c->merge.budget) return c->merge.budget;
  if (!c->merge.default_budget) {
    // a sixteenth of the device's memory at 56 bytes a record (32 the record, 8 its key and 16 its value
    // in the segments), within [2^16, 2^27] records
    size_t total = 0;
    if (hipDeviceTotalMem(&total, c->device) != hipSuccess) total = 0;
    c->merge.default_budget = std::min<size_t>(std::max<size_t>(total / 16 / 56, (size_t)1 << 16), (size_t)1 << 27);
  }
  return c->merge.default_budget;
}

void sm_scan(hipStream_t s, const uint32_t* cnt, uint32_t n, uint32_t* sums, uint32_t* start) {
  const uint32_t nb = (n + kScanChunk - 1) / kScanChunk;
  k_sm_sums<<<nb, 256, 0, s>>>(cnt, n, sums);
  k_sm_scan_sums<<<1, 256, 0, s>>>(sums, nb);
  k_sm_starts<<<nb, 256, 0, s>>>(cnt, n, sums, nb, start);
}

void splat_merge(bling_ctx* c, const uint4* recs, size_t n, int layout, float* img) {
  if (n == 0) return;
  if (n > 0x7FFFFFFFull) throw std::invalid_argument("splat merge: more than 2^31 - 1 records");
  MergeState& M = c->merge;
  hipStream_t s = c->stream;
  const uint32_t W = (uint32_t)c->S.width, npix = W * (uint32_t)c->S.height;
  const uint32_t nb = (npix + kScanChunk - 1) / kScanChunk;
  if (M.cnt.n != npix) { M.cnt.alloc(npix); M.start.alloc((size_t)npix + 1); M.longs.alloc((size_t)npix + 1); M.sums.alloc((size_t)nb + 1); }
  if (M.key.n < n) { M.key.alloc(n); M.val.alloc(n); }
  HIPCHK(hipMemsetAsync(M.cnt.p, 0, (size_t)npix * sizeof(uint32_t), s));
  HIPCHK(hipMemsetAsync(M.longs.p, 0, sizeof(uint32_t), s));
  k_sm_count<<<stride_grid(n), 256, 0, s>>>(recs, n, layout, W, npix, M.cnt.p);
  sm_scan(s, M.cnt.p, npix, M.sums.p, M.start.p);
  k_sm_scatter<<<stride_grid(n), 256, 0, s>>>(recs, n, layout, W, npix, M.start.p, M.cnt.p, M.key.p, M.val.p);
  k_sm_short<<<stride_grid(npix), 256, 0, s>>>(M.start.p, npix, M.key.p, M.val.p, img, M.longs.p);
  k_sm_long<<<(unsigned)std::min<size_t>(1024, std::max<size_t>(1, n / (SM_SHORT + 1))), 256, 0, s>>>(M.start.p, M.key.p, M.val.p, img,
                                                                                                    M.longs.p);
  HIPCHK(hipGetLastError());
}

}  // namespace bcore
