// lighttracer_ref.cpp -- CPU restatement of the light tracer (Renderer/LightTracer.hs), test
// infrastructure only: never linked into the product libraries.
//
// It includes the oracle's translation unit, whose internals sit in an anonymous namespace, and so
// shares its binary32 restatements of sampleLightRay, sampleAdjBsdf, bxdfEval, scIntersect /
// occluded, the hit's BSDF, spectrumToXYZ and the counter RNG; it adds only oneRay, nextVertex,
// connectCam, sampleCam and the adjoint evalBsdf.  Citations are File.hs:line relative to
// src/lib/Graphics/Bling/ of the reference, in the oracle's style.  Build: make ltref
// (HOSTFLAGS: -ffp-contract=off, no fast-math).
#include "../../oracle/oracle.cpp"

#include <algorithm>

#include "coverage.h"

namespace {

// sampler keys of the device's light tracer (bling_amd/csrc/core/sppm.h LT_*): photon i
// of a pass is "sample" i & 0xFFFF of "pixel" LT_PIXEL | i >> 16; plain rnd -> fresh dimensions
constexpr uint32_t LT_PIXEL = 0x40000000u;
struct LtRnd {
  uint32_t seed, pass, i;
  float r1(uint32_t dim) const { return u01(hash5(seed, pass, LT_PIXEL | (i >> 16), i & 0xFFFFu, DIM_FRESH1D + dim)); }
  void r2(uint32_t dim, float* a, float* b) const {
    *a = u01(hash5(seed, pass, LT_PIXEL | (i >> 16), i & 0xFFFFu, DIM_FRESH2D + 2u * dim));
    *b = u01(hash5(seed, pass, LT_PIXEL | (i >> 16), i & 0xFFFFu, DIM_FRESH2D + 2u * dim + 1u));
  }
};

// sampleCam (Camera.hs:90-100), ProjectiveCamera only (`sampleCam c _ = error`, :102)
struct CamSample { V pLens; float px, py, pdf; };
CamSample sample_cam(const bling_scene_desc* d, V p) {
  const V pRas = xpoint(d->light.w2r, p);                                      // transPoint w2r p
  const V pLens = xpoint(d->camera.c2w, mk(0.f, 0.f, 0.f));                    // transPoint c2w (0 0 0)
  const float cost = std::fabs(normalize(xpoint(d->camera.r2c, pRas)).z);
  const float cost3 = cost * cost * cost;
  return CamSample{pLens, pRas.x, pRas.y, d->light.pixel_area * cost3};        // ap * cost3
}

// evalBsdf True (Reflection.hs:318-332): eval b = bxdfEval b (not flipped), scaled by |sideTest|
S eval_bsdf_adj(const Bsdf& bs, V woW, V wiW) {
  const float cosWo = dot(woW, bs.ng);
  const float side = dot(wiW, bs.ng) / cosWo;
  if (side == 0.f) return black();
  if (std::fabs(cosWo) < 1e-5f) return black();
  const int flt = side < 0.f ? B_TRANS : B_REFL;
  const V wo = world_to_local(bs.cs, woW), wi = world_to_local(bs.cs, wiW);
  S f = black();
  for (int i = 0; i < bs.n; ++i)
    if (has_flag(bs.b[i], flt)) f = f + bxdf_eval(bs.b[i], wo, wi);
  return sscale(f, std::fabs(side));
}

struct LtRecord { uint32_t photon, depth; int32_t sx, sy; float x, y, z; uint32_t pad; };
struct LtSplat { LtRecord r; float camz; };   // camz: the vertex's camera-space z (transPoint (inverse c2w) p)
struct LtCount { uint64_t rays = 0, shadows = 0, splats = 0, dropped = 0; Cov cov; };

// connectCam (LightTracer.hs:68-82) followed by splatSample (Image.hs:201-221)
void connect_cam(const Scene& Sc, const S& li, const Bsdf& bsdf, V wi, float eps, uint32_t photon, uint32_t depth,
                 std::vector<LtSplat>& out, LtCount& C) {
  const V p = bsdf.p;
  const CamSample cs = sample_cam(Sc.d, p);
  const V dCam = cs.pLens - p;
  const V we = normalize(dCam);
  const S f = eval_bsdf_adj(bsdf, wi, we);
  if (is_black(f) || cs.pdf == 0.f) return;                                    // csf is white
  const float dCam2 = sqlen(dCam);
  TStats ts;
  C.shadows++;
  if (sc_occluded(Sc, Ray{p, we, eps, std::sqrt(dCam2)}, ts)) return;
  const S lr = sscale(li * f, 1.f / (cs.pdf * dCam2));
  // splatSample: px = floor sx.  A raster position that is NaN or beyond Int has no pixel.
  const float fx = std::floor(cs.px), fy = std::floor(cs.py);
  if (!(fx >= 0.f && fy >= 0.f && fx < (float)Sc.d->config.width && fy < (float)Sc.d->config.height)) return;
  if (s_nan(lr) || s_inf(lr)) { C.dropped++; return; }
  LtRecord r{photon, depth, (int32_t)fx, (int32_t)fy, 0.f, 0.f, 0.f, 0u};
  to_xyz(lr, &r.x, &r.y, &r.z);
  C.splats++;
  out.push_back(LtSplat{r, xpoint(Sc.d->camera.c2w_inv, p).z});
}

// oneRay (LightTracer.hs:54-66) and nextVertex (:84-109), the recursion as a loop.  No depth limit;
// the walk is cut after 1 << 16 bounces like the SPPM photon walk's.
void one_ray(const Scene& Sc, const LtRnd& R, std::vector<LtSplat>& out, LtCount& C) {
  const float ul = R.r1(0);
  float uo1, uo2, ud1, ud2;
  R.r2(0, &uo1, &uo2);
  R.r2(1, &ud1, &ud2);
  const LightRay lr = sample_light_ray(Sc, ul, uo1, uo2, ud1, ud2);
  if (!(lr.pdf > 0.f)) return;
  const V wo0 = normalize(lr.ray.d);
  S li = sscale(lr.li, absdot(lr.n, wo0) / lr.pdf);
  if (is_black(li)) return;
  cov_light_ray(C.cov, Sc, ul);
  Ray ray = lr.ray;
  V wi = -wo0;
  for (int d = 0; d < (1 << 16); ++d) {
    Hit h;
    TStats ts;
    C.rays++;
    if (!sc_intersect(Sc, ray, &h, ts)) return;                                // nextVertex _ _ Nothing
    if (is_black(li)) return;
    const float ubc = R.r1(1u + 2u * (uint32_t)d);
    float ub1, ub2;
    R.r2(2u + (uint32_t)d, &ub1, &ub2);
    const float pcont = d > 3 ? 0.8f : 1.f;
    const Bsdf bsdf = hit_bsdf(Sc, h);
    const BsdfSample bs = sample_bsdf_t(bsdf, B_ALL, wi, ubc, ub1, ub2, true);  // sampleAdjBsdf
    cov_vertex(C.cov, Sc, h, bsdf, ubc);
    connect_cam(Sc, li, bsdf, wi, h.eps, R.i, (uint32_t)d, out, C);
    if (is_black(bs.f) || bs.pdf == 0.f) return;
    if (R.r1(2u + 2u * (uint32_t)d) > pcont) return;                          // rnd, drawn even when pcont = 1
    li = sscale(li * bs.f, 1.f / pcont);
    ray = Ray{bsdf.p, bs.wi, h.eps, INF};
    wi = -bs.wi;
  }
}

}  // namespace

extern "C" {

struct lt_ref_stats { uint64_t photons, photon_rays, shadow_rays, splats, dropped; double seconds; };

// what the photons of the last lt_ref_pass met (coverage.h)
static Cov g_lt_cov;
void lt_ref_coverage(uint64_t* out) { std::memcpy(out, g_lt_cov.c, sizeof g_lt_cov.c); }

// Photons first .. first + count - 1 of a pass.  The walks run in parallel; their records are then
// taken in photon order: splatted sequentially into splat (W * H * 3, accumulated, may be NULL) and
// copied to rec and their vertices' camera-space z to camz (at most cap each, may be NULL).
// Returns the number of records.
size_t lt_ref_pass(const oracle_scene* os, uint32_t seed, uint32_t pass, uint32_t first, uint32_t count, int threads,
                   float* splat, LtRecord* rec, float* camz, size_t cap, lt_ref_stats* st) {
  const Scene& Sc = os->s;
  auto t0 = std::chrono::steady_clock::now();
#ifdef _OPENMP
  if (threads > 0) omp_set_num_threads(threads);
#endif
  const uint32_t chunk = 256;
  const uint32_t nch = (count + chunk - 1) / chunk;
  std::vector<std::vector<LtSplat>> recs(nch);
  std::vector<LtCount> cnt(nch);
#pragma omp parallel for schedule(dynamic, 1)
  for (int64_t c = 0; c < (int64_t)nch; ++c) {
    const uint32_t b = (uint32_t)c * chunk, e = std::min(count, b + chunk);
    for (uint32_t k = b; k < e; ++k) one_ray(Sc, LtRnd{seed, pass, first + k}, recs[c], cnt[c]);
  }
  LtCount T;
  g_lt_cov = Cov{};
  for (uint32_t c = 0; c < nch; ++c) g_lt_cov.add(cnt[c].cov);
  size_t n = 0;
  const int W = Sc.d->config.width;
  for (uint32_t c = 0; c < nch; ++c) {
    T.rays += cnt[c].rays; T.shadows += cnt[c].shadows; T.splats += cnt[c].splats; T.dropped += cnt[c].dropped;
    for (const LtSplat& sp : recs[c]) {
      const LtRecord& r = sp.r;
      if (splat) {
        float* o = &splat[3 * ((size_t)r.sx + (size_t)r.sy * W)];
        o[0] = o[0] + r.x; o[1] = o[1] + r.y; o[2] = o[2] + r.z;
      }
      if (rec && n < cap) rec[n] = r;
      if (camz && n < cap) camz[n] = sp.camz;
      ++n;
    }
  }
  if (st) {
    st->photons = count; st->photon_rays = T.rays; st->shadow_rays = T.shadows; st->splats = T.splats;
    st->dropped = T.dropped;
    st->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
  return n;
}

// probes for the known-answer tests
// sampleCam of a world point: out = px, py, pLens xyz, pdf, and the point's camera-space z
void lt_ref_sample_cam(const oracle_scene* os, const float* p3, float* out7) {
  const bling_scene_desc* d = os->s.d;
  const V p = mk(p3[0], p3[1], p3[2]);
  const CamSample cs = sample_cam(d, p);
  out7[0] = cs.px; out7[1] = cs.py; out7[2] = cs.pLens.x; out7[3] = cs.pLens.y; out7[4] = cs.pLens.z; out7[5] = cs.pdf;
  out7[6] = xpoint(d->camera.c2w_inv, p).z;
}

// evalBsdf True of material mi's BSDF built on a geometric normal ng and a shading frame (ns, dpdu):
// frame9 = ng, ns, dpdu; out16 = the spectrum
void lt_ref_eval_adj(const oracle_scene* os, int mi, const float* frame9, const float* wo3, const float* wi3, float* out16) {
  const V ng = mk(frame9[0], frame9[1], frame9[2]), ns = mk(frame9[3], frame9[4], frame9[5]);
  const V dpdu = mk(frame9[6], frame9[7], frame9[8]);
  const DG dgg = mk_dg2(mk(0.f, 0.f, 0.f), ng);
  DG dgs = dgg;
  dgs.n = ns; dgs.dpdu = dpdu; dgs.dpdv = cross(ns, dpdu);
  const Bsdf bs = make_bsdf(os->s.d, mi, dgg, dgs);
  const S f = eval_bsdf_adj(bs, mk(wo3[0], wo3[1], wo3[2]), mk(wi3[0], wi3[1], wi3[2]));
  std::memcpy(out16, f.v, sizeof f.v);
}

// the first hit of a ray: out = hit (0 / 1), emitter (the hit shape's light index, -1 if none), for
// the convergence test's pixel mask
void lt_ref_first_hit(const oracle_scene* os, const float* ray6, int* out2) {
  const Scene& Sc = os->s;
  Hit h;
  TStats ts;
  out2[0] = 0; out2[1] = -1;
  if (!sc_intersect(Sc, Ray{mk(ray6[0], ray6[1], ray6[2]), mk(ray6[3], ray6[4], ray6[5]), 0.f, INF}, &h, ts)) return;
  out2[0] = 1;
  const Prim& pr = Sc.prims[h.prim];
  if (pr.kind == 1) out2[1] = Sc.d->shapes[pr.index].light;
}

}  // extern "C"
