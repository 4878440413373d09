// li_rays.h -- the integrator seam for a caller's rays (bling_surface_li[_device], include/bling.h):
// SurfaceIntegrator.surfaceLi :: Scene -> Ray -> Sampled s Spectrum (Integrator.hs:32-36) for rays the
// caller made itself, with the sample streams of ids it names.
//
// A wave of at most the context's path capacity takes a chunk of consecutive rays: k_li_intake puts them
// where k_raygen puts the camera's (init_path_ray, slot = the ray's index in the chunk), the wave pipeline
// (run_wave_prof, normals_wave) runs unchanged with WaveState::Lfull set, and k_li_store copies the
// wave's 16-band records to the caller's rows.  A ray's arithmetic depends on its seven floats, its two
// ids, the seed and the pass only: not on its slot, its chunk or its neighbours.
#pragma once
#include "wavefront.h"

namespace bd {

// A chunk of the caller's buffers, already offset to its first ray: the seven planes (ox, oy, oz, dx,
// dy, dz, tmin) and the (pixel, n) id pairs.
struct LiChunk {
  const float* plane[7];
  const uint32_t* ids;
};

// NaN and both infinities fail
DEV bool li_finite(float x) { return fabsf(x) < INFINITY; }

// One thread per ray of the chunk.  Lane l of a wave reads word l of each plane (seven coalesced 256-B
// loads) and its id pair (one 512-B load), so the intake moves 36 B per ray in and the path records out.
// A dropped ray (include/bling.h: a NaN or infinite float other than tmin = +inf, a zero direction, n >=
// spp) never reaches a traversal kernel: its slot holds a unit ray from the origin made as a miss, its
// flag byte tells k_li_store to write zeros, and it is counted once.  tmin = +inf is a valid ray that
// can hit nothing (no t exceeds it): it too is made as a miss, and keeps its own direction for the
// environment term.
static __global__ __launch_bounds__(256) void k_li_intake(const DevScene* __restrict__ Sptr, WaveState W, LiChunk in, uint32_t n,
                                                   uint8_t* __restrict__ drop, unsigned long long* __restrict__ n_dropped) {
  const DevScene& S = *Sptr;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float v[7];
#pragma unroll
  for (int p = 0; p < 7; ++p) v[p] = in.plane[p][i];
  const uint32_t pixel = in.ids[2 * (size_t)i], sn = in.ids[2 * (size_t)i + 1];
  bool ok = true;
#pragma unroll
  for (int p = 0; p < 6; ++p) ok = ok && li_finite(v[p]);
  ok = ok && (li_finite(v[6]) || v[6] == INFINITY);
  ok = ok && !(v[3] == 0.f && v[4] == 0.f && v[5] == 0.f);
  ok = ok && sn < (uint32_t)S.spp;
  const Ray r = ok ? Ray{mk(v[0], v[1], v[2]), mk(v[3], v[4], v[5]), v[6], INFINITY}
                   : Ray{mk(0.f, 0.f, 0.f), mk(0.f, 0.f, 1.f), 0.f, INFINITY};
  init_path_ray(S, W, i, r, ok ? pixel : 0u, ok ? sn : 0u, !ok || v[6] == INFINITY);
  drop[i] = ok ? (uint8_t)0 : (uint8_t)1;
  const unsigned long long m = __ballot(!ok);
  if (m != 0ull && (threadIdx.x & 63u) == (uint32_t)__ffsll((long long)__ballot(1)) - 1u)
    atomicAdd(n_dropped, (unsigned long long)__popcll(m));
}

// The wave's Lfull records (64 B per slot, finalize's store_sp) to rows of the caller's n x 16 buffer:
// one float4 per thread, four threads per ray, so a wave reads and writes 1 KiB of consecutive bytes per
// instruction.  A dropped ray's row is +0.0.  ALIGNED: the caller's buffer is 16-byte aligned (one
// 16-byte store per thread; else four 4-byte ones).
template <bool ALIGNED>
static __global__ __launch_bounds__(256) void k_li_store(const float4* __restrict__ lfull, const uint8_t* __restrict__ drop,
                                                  uint32_t n, float* __restrict__ out) {
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // float4 index: n <= 2^31 rays, 4 n quads
  if (q >= (size_t)4 * n) return;
  float4 v = lfull[q];
  if (drop[q >> 2]) v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ALIGNED) {
    reinterpret_cast<float4*>(out)[q] = v;
  } else {
    float* o = out + 4 * q;
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  }
}

}  // namespace bd
