// light_tracer.h -- the light tracer (Renderer/LightTracer.hs) on the device, the third consumer of
// the trace core.  One pass traces passPhotons photons (oneRay, :54-66); every vertex of a photon's
// walk (nextVertex, :84-109) is connected to the camera's pinhole (connectCam, :68-82) and splatted.
//   k_lt_photon     one thread per photon: sampleLightRay, then per vertex sampleAdjBsdf, the camera
//                   connection (sampleCam, the adjoint evalBsdf, an any-hit shadow ray, splatSample as
//                   three float atomics) and Russian roulette (0.8 beyond depth 3, no depth limit)
// The LDS scene set-up, light_ray, the closest / any-hit trace, hit_geometry, make_bsdf and the adjoint
// sample_bsdf are the SPPM photon kernel's (sppm.h).  Float atomics make the film's sums
// order-dependent; the set of contributions is not, and record mode (LtBufs::rec) writes each one out.
#pragma once
#include "sppm.h"

namespace bd {

// one splat, 32 bytes (include/bling.h bling_light_record): photon, depth, sx, sy | X, Y, Z, pad
struct LtBufs {
  float* splat;              // W * H * 3 (X, Y, Z), accumulated
  unsigned long long* ctr;   // [0] photon rays, [1] shadow rays, [2] splats, [3] dropped
  uint4* rec;                // record mode: 2 uint4 per splat; nullptr = off
  uint32_t* rec_count;       // slots claimed (may exceed rec_cap: the host reports the overflow)
  uint32_t rec_cap;
};

// sampleCam (Camera.hs:90-100) of the projective camera: the raster position of p, the pinhole and
// the pdf ap * cost^3.  Nothing tests that p lies in front of the camera (trap T20).
DEV void sample_cam(const DevScene& S, V3 p, float& px, float& py, V3& pLens, float& cPdf) {
  const V3 pRas = xpoint(S.lt_w2r, p);
  px = pRas.x; py = pRas.y;
  pLens = xpoint(S.camera.c2w, mk(0.f, 0.f, 0.f));
  const float cost = fabsf(normalize(xpoint(S.camera.r2c, pRas)).z);
  const float cost3 = cost * cost * cost;
  cPdf = S.lt_pixel_area * cost3;
}

// evalBsdf True (Reflection.hs:318-332): the lobes sideTest selects, evaluated unflipped
// (bxdfEval b wo wi) and scaled by |sideTest|
template <uint32_t F>
DEV Sp eval_bsdf_adj(const Bsdf& bs, V3 woW, V3 wiW) {
  const float cosWo = dot(woW, bs.ng);
  const float side = dot(wiW, bs.ng) / cosWo;
  if (side == 0.f) return sconst(0.f);
  if (fabsf(cosWo) < 1e-5f) return sconst(0.f);
  const int flt = side < 0.f ? F_TRANS : F_REFL;
  const V3 wo = world_to_local(bs.cs, woW), wi = world_to_local(bs.cs, wiW);
  Sp f = sconst(0.f);
#pragma unroll
  for (int i = 0; i < max_lobes<F>(); ++i)
    if (i < bs.n && has_flag(bs.b[i], flt)) f = f + bxdf_eval<F>(bs.b[i], wo, wi);
  return sscale(f, fabsf(side));
}

template <uint32_t F>
static __global__ __launch_bounds__(256) void k_lt_photon(const DevScene* __restrict__ Sptr, LtBufs B, uint32_t first,
                                                   uint32_t count, uint32_t seed, uint32_t pass) {
  extern __shared__ float4 smem[];
  const DevScene& S = *Sptr;
  const LdsScene L = lds_setup(S, smem);
  const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long rays = 0, shadows = 0, splats = 0, dropped = 0;
  if (gid < count) {
    const uint32_t i = first + gid;
    // plain i.i.d. rnd (runWithSeed, LightTracer.hs:46): the counter RNG's fresh dimensions only
    const uint32_t sk = brng::sample_key(brng::pixel_key(seed, pass, LT_PIXEL | (i >> 16)), i & 0xFFFFu);
    auto rnd1 = [&](uint32_t dim) { return brng::u01(brng::draw(sk, brng::DIM_FRESH1D + dim)); };
    auto rnd2 = [&](uint32_t dim, float* a, float* b) {
      *a = brng::u01(brng::draw(sk, brng::DIM_FRESH2D + 2u * dim));
      *b = brng::u01(brng::draw(sk, brng::DIM_FRESH2D + 2u * dim + 1u));
    };
    const float ul = rnd1(LT_DIM_UL);                                   // oneRay (LightTracer.hs:54-66)
    float uo1, uo2, ud1, ud2;
    rnd2(LT_DIM_ULO, &uo1, &uo2);
    rnd2(LT_DIM_ULD, &ud1, &ud2);
    float pdf = 0.f;                                                    // sampleLightRay (Scene.hs:121-135)
    Sp li; Ray ray; V3 nl;
    if (S.num_lights > 0) {
      const int lc = S.num_lights;
      const int ln = lc == 1 ? 0 : min((int)floorf(ul * (float)lc), lc - 1);
      pdf = light_ray<F>(S, gen(S.lights[ln]), uo1, uo2, ud1, ud2, li, ray, nl);
      if (lc > 1) pdf = pdf / (float)lc;
    }
    bool alive = pdf > 0.f;
    V3 wi = mk(0.f, 1.f, 0.f);
    if (alive) {
      const V3 wo = normalize(ray.d);
      li = sscale(li, fabsf(dot(nl, wo)) / pdf);
      alive = !is_black(li);
      wi = -wo;
    }
    for (int d = 0; alive && d < SPPM_PHOTON_BOUNCES; ++d) {           // nextVertex (:84-109)
      ++rays;
      HitRec h;
      TraceCount tc{0u, 0u, 0u, 0u};
      if (!trace<false, F>(S, L, ray, h, tc)) break;
      if (is_black(li)) break;
      const float ubc = rnd1(LT_DIM_UBC + 2u * (uint32_t)d);
      float ub1, ub2;
      rnd2(LT_DIM_UBD + (uint32_t)d, &ub1, &ub2);
      const float4 hv = make_float4(h.t, __uint_as_float(h.ref), h.b1, h.b2);
      DG dgg, dgs;
      float eps;
      int mat, hit_light;
      hit_geometry<F>(S, ray, hv, dgg, dgs, eps, mat, hit_light);
      const Bsdf bsdf = make_bsdf<F>(S, mat, dgg, dgs);
      const V3 p = bsdf.p;
      Sp bf; V3 wo; int fl;
      const float spdf = sample_bsdf<F, true>(bsdf, wi, ubc, ub1, ub2, bf, wo, fl);   // sampleAdjBsdf
      const float pcont = d > 3 ? 0.8f : 1.f;
      {                                                                 // connectCam (:68-82)
        float px, py, cPdf;
        V3 pCam;
        sample_cam(S, p, px, py, pCam, cPdf);
        const V3 dCam = pCam - p;
        const V3 we = normalize(dCam);
        const Sp f = eval_bsdf_adj<F>(bsdf, wi, we);
        if (!(is_black(f) || cPdf == 0.f)) {
          const float dCam2 = sqlen(dCam);
          ++shadows;
          HitRec hs;
          if (!trace<true, F>(S, L, Ray{p, we, eps, sqrtf(dCam2)}, hs, tc)) {
            const Sp lr = sscale(li * f, 1.f / (cPdf * dCam2));
            // splatSample (Image.hs:201-221); a raster position that is NaN or beyond Int is outside
            const float fx = floorf(px), fy = floorf(py);
            if (fx >= 0.f && fy >= 0.f && fx < (float)S.width && fy < (float)S.height) {
              if (s_bad(lr)) ++dropped;
              else {
                const int sx = (int)fx, sy = (int)fy;
                float x, y, z;
                to_xyz(lr, &x, &y, &z);
                ++splats;
                if (B.splat) {
                  float* o = B.splat + 3 * ((size_t)sy * S.width + sx);
                  atomicAdd(&o[0], x); atomicAdd(&o[1], y); atomicAdd(&o[2], z);
                }
                if (B.rec) {
                  const uint32_t slot = atomicAdd(B.rec_count, 1u);
                  if (slot < B.rec_cap) {
                    B.rec[2 * (size_t)slot] = make_uint4(i, (uint32_t)d, (uint32_t)sx, (uint32_t)sy);
                    B.rec[2 * (size_t)slot + 1] = make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(z), 0u);
                  }
                }
              }
            }
          }
        }
      }
      if (is_black(bf) || spdf == 0.f) break;
      if (rnd1(LT_DIM_ROULETTE + 2u * (uint32_t)d) > pcont) break;     // drawn even when pcont = 1
      li = sscale(li * bf, 1.f / pcont);
      ray = Ray{p, wo, eps, INFINITY};
      wi = -wo;
    }
  }
  const unsigned long long wr = wave_sum_u64(rays), ws = wave_sum_u64(shadows), wp = wave_sum_u64(splats),
                           wd = wave_sum_u64(dropped);
  if ((threadIdx.x & 63) == 0) {
    if (wr) atomicAdd(&B.ctr[0], wr);
    if (ws) atomicAdd(&B.ctr[1], ws);
    if (wp) atomicAdd(&B.ctr[2], wp);
    if (wd) atomicAdd(&B.ctr[3], wd);
  }
}

}  // namespace bd
