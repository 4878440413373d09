// cam_samples.h -- the sampler and camera seam (bling_camera_samples[_device], include/bling.h): the samples
// and camera rays of a list of SampleWindows, written to the caller's buffers instead of a wave's path set.
// `sample sampler window` (Sampling.hs:101-132) walks a window's pixels y outer, x inner, n innermost
// (coverWindow), and every sample fires fireRay (Camera.hs:49-76).
//
// The arithmetic is init_path's (wavefront.h): sample_key, camera_sample and fire_ray of dev_shade.h, called
// with the same arguments, so a slot's floats are the floats k_raygen puts into a path set for that sample --
// and, with the host library's restatement (host/camera_samples.h), bling_host_camera_samples' bit for bit.
// A slot's values depend on its window, its offset in it, the seed, the pass and the scene only.
#pragma once
#include "dev_shade.h"

namespace bd {

// A window as the kernel reads it: its first pixel and its width as an exact divisor (pt / w, pt % w).
// 32 B, so a lane's record is two 16-B loads.
struct CamWin {
  int32_t x0, y0;
  FastDiv fw;
  uint32_t pad[3];
};
static_assert(sizeof(CamWin) == 32, "CamWin is 32 bytes");

// The caller's buffers, indexed by the 64-bit slot; a NULL one is not produced.  pairs8: xy, ids and lens are
// 8-byte aligned (one 8-B store per lane; else two 4-B ones).
struct CamOut {
  float* xy;
  uint32_t* ids;
  float* plane[7];      // ox, oy, oz, dx, dy, dz, tmin; all NULL or none
  float* lens;
  uint32_t pairs8;
};

DEV void cam_store_pair(void* base, uint64_t i, uint32_t a, uint32_t b, bool wide) {
  if (wide) {
    reinterpret_cast<uint2*>(base)[i] = make_uint2(a, b);
  } else {
    uint32_t* o = reinterpret_cast<uint32_t*>(base) + 2 * i;
    o[0] = a; o[1] = b;
  }
}

// One thread per sample: slot = base + the thread's index in the launch, count slots from base on.
// first (n_windows + 1 ascending offsets, first[n_windows] > every slot of the launch) and wins live in
// device memory, copied once per call.  A wave finds the window of its first slot by binary search over first
// -- the same addresses in every lane -- and every lane walks forward from there: most waves sit inside one
// window, and a wave over many small windows crosses them at arbitrary lanes.  Then the sample of the slot's
// offset in its window, init_path's camera sample and ray, and the stores: lane l of a wave writes word l of
// each ray plane (seven 256-B rows per wave) and pair l of xy, ids and lens (512-B rows), every output once.
// fire_ray feeds the ray planes only and is skipped without them; nothing else depends on which outputs exist.
static __global__ __launch_bounds__(256) void k_cam_samples(const DevScene* __restrict__ Sptr, const CamWin* __restrict__ wins,
                                                     const unsigned long long* __restrict__ first, uint32_t n_windows,
                                                     uint64_t base, uint32_t count, CamOut out, uint32_t seed, uint32_t pass) {
  const DevScene& S = *Sptr;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const uint64_t slot = base + t;
  // the wave's first slot (lane 0 is active whenever any lane is)
  const uint64_t slot0 = base + (t & ~63u);
  const uint32_t s0lo = __builtin_amdgcn_readfirstlane((uint32_t)slot0), s0hi = __builtin_amdgcn_readfirstlane((uint32_t)(slot0 >> 32));
  const uint64_t w0 = ((uint64_t)s0hi << 32) | s0lo;
  uint32_t lo = 0, hi = n_windows;                 // first[lo] <= w0 < first[hi]
  while (hi - lo > 1u) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (first[mid] <= w0) lo = mid; else hi = mid;
  }
  uint32_t k = lo;
  while (slot >= first[k + 1]) ++k;                // ends: slot < first[n_windows]
  const uint64_t off = slot - first[k];
  const CamWin w = wins[k];
  // a window holds fewer than 2^32 pixels (the stream id is 32 bits), so pt fits; its samples may not
  const uint32_t spp = (uint32_t)S.spp;
  uint32_t pt, n;
  if ((off >> 32) == 0) {
    pt = S.fd_spp.div((uint32_t)off); n = (uint32_t)off - pt * spp;
  } else {
    const uint64_t q = off / spp;
    pt = (uint32_t)q; n = (uint32_t)(off - q * spp);
  }
  const uint32_t py = w.fw.div(pt), px = pt - py * w.fw.d;             // coverWindow: y outer
  const int ix = w.x0 + (int)px, iy = w.y0 + (int)py;
  // from here on: init_path (wavefront.h)
  const uint32_t pixel = (uint32_t)((iy - S.ey0) * S.ext_w + (ix - S.ex0));
  const SampleKey key = sample_key(seed, pass, pixel, n);
  float ox, oy, lu, lv;
  camera_sample(S, key, &ox, &oy, &lu, &lv);
  const float imx = (float)ix + ox, imy = (float)iy + oy;
  const bool wide = out.pairs8 != 0u;
  if (out.xy) cam_store_pair(out.xy, slot, __float_as_uint(imx), __float_as_uint(imy), wide);
  if (out.ids) cam_store_pair(out.ids, slot, pixel, n, wide);
  if (out.lens) cam_store_pair(out.lens, slot, __float_as_uint(lu), __float_as_uint(lv), wide);
  if (out.plane[0]) {
    const Ray r = fire_ray(S.camera, imx, imy, lu, lv);
    out.plane[0][slot] = r.o.x; out.plane[1][slot] = r.o.y; out.plane[2][slot] = r.o.z;
    out.plane[3][slot] = r.d.x; out.plane[4][slot] = r.d.y; out.plane[5][slot] = r.d.z;
    out.plane[6][slot] = r.tmin;
  }
}

}  // namespace bd
