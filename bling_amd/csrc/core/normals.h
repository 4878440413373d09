// normals.h -- the normal-map integrator `integrator { debug normals }` (mkNormalMap,
// Integrator/Debug.hs:25-34): li = rgbToSpectrumRefl ((1 + n) / 2) of the BSDF's shading normal at the
// camera ray's hit, black on a miss (no environment term).  It asks for no sample dimensions.
//
// One wave = the camera rays (k_raygen), the scene's planned closest-hit launch over them, k_shade_nm
// and the film.  No queue compaction, no second path set: slot = sample id, as k_raygen leaves it.
//
// k_shade_nm rebuilds the hit with hit_geometry (the per-triangle frames, shape_dg, the fractal
// normal) and applies the bump step of make_bsdf (bump_dg) where the profile has FT_BUMP: the normal
// is the cs.n make_bsdf would put in the frame, also for a material without lobes (mkBsdf [] dgs ng).
// No material spectrum is evaluated; only a bump displacement texture is.
#pragma once
#include "wavefront.h"

namespace bd {

// The seven reflectance bases (r, g, b, c, m, y, w) of common/spectral_data.h as device constant data:
// the two a lane adds to the white one depend on its normal, so they are loaded by index.
struct NmBases { float v[7][16]; };
constexpr NmBases nm_bases() {
  NmBases b{};
  for (int k = 0; k < 7; ++k)
    for (int i = 0; i < 16; ++i) b.v[k][i] = BLING_RGB_REFL_BANDS[k][i];
  return b;
}
__constant__ const NmBases kNmBases = nm_bases();

// rgbToSpectrumRefl (Spectrum.hs:140-159): three ordered cases, each sScale wb a0 + (sScale b1 a1 +
// sScale b2 a2) with b1 of {c, m, y} and b2 of {r, g, b}; the third case's `r <= b` is kept as written
DEV Sp nm_rgb_to_spectrum(float r, float g, float b) {
  int w1, w2;
  float a0, a1, a2;
  if (r <= g && r <= b) {
    a0 = r;
    if (g <= b) { w1 = 3; a1 = g - r; w2 = 2; a2 = b - g; } else { w1 = 3; a1 = b - r; w2 = 1; a2 = g - b; }
  } else if (g <= r && g <= b) {
    a0 = g;
    if (r <= b) { w1 = 4; a1 = r - g; w2 = 2; a2 = b - r; } else { w1 = 4; a1 = b - g; w2 = 0; a2 = r - b; }
  } else {
    a0 = b;
    if (r <= b) { w1 = 5; a1 = r - b; w2 = 1; a2 = g - r; } else { w1 = 5; a1 = g - b; w2 = 0; a2 = r - g; }
  }
  const float* b1 = kNmBases.v[w1];
  const float* b2 = kNmBases.v[w2];
  Sp s;
  SP_LOOP s.v[i] = kNmBases.v[6][i] * a0 + (b1[i] * a1 + b2[i] * a2);
  return s;
}

// intToSpectrum (Debug.hs:31-34): (vpromote 1 + n) / 2 componentwise
DEV Sp nm_colour(V3 n) { return nm_rgb_to_spectrum((1.f + n.x) / 2.f, (1.f + n.y) / 2.f, (1.f + n.z) / 2.f); }

// bsdfShadingNormal (intBsdf int): the shading DG's normal after the material's bump step
template <uint32_t F>
DEV V3 nm_shading_normal(const DevScene& S, const Ray& ray, const float4 hv) {
  DG dgg, dgs;
  float eps;
  int mat, hit_light;
  hit_geometry<F>(S, ray, hv, dgg, dgs, eps, mat, hit_light);
  if constexpr ((F & FT_BUMP) != 0) {
    const int bump_tex = gen(S.materials[mat]).stex[3];
    if (bump_tex >= 0) return bump_dg<F>(S, bump_tex, dgg, dgs).n;        // bumpMapped (Reflection.hs:344-377)
  }
  return dgs.n;
}

// The n camera samples of a wave, slot = sample id: W.cur.hit holds their closest hits.  Counts the
// samples as camera rays and the hits as path vertices.
template <uint32_t F>
static __global__ __launch_bounds__(256) void k_shade_nm(const DevScene* __restrict__ Sptr, WaveState W, uint32_t n,
                                                         Counters* __restrict__ C) {
  const DevScene& S = *Sptr;
  unsigned long long n_drop = 0, n_hit = 0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float4 hv = W.cur.hit[i];
    Sp L = sconst(0.f);
    if (__float_as_uint(hv.y) != REF_NONE) {
      const float4 ro = W.cur.org[i], rdv = W.cur.dir[i];
      const Ray ray{mk(ro.x, ro.y, ro.z), mk(rdv.x, rdv.y, rdv.z), ro.w, INFINITY};
      L = nm_colour(nm_shading_normal<F>(S, ray, hv));
      ++n_hit;
    }
    finalize(W, i, L, n_drop);
  }
  flush_dropped(C, n_drop);
  n_hit = wave_sum_u64(n_hit);
  if ((threadIdx.x & 63u) == 0u && n_hit) atomicAdd(&C->vertices, n_hit);
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&C->cam, (unsigned long long)n);
}

}  // namespace bd
