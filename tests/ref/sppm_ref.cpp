// sppm_ref.cpp -- the per-splat records of SPPM's photon pass (Renderer/SPPM.hs), test infrastructure
// only: never linked into the product libraries.
//
// It includes the oracle's translation unit and runs the oracle's own eye pass (trace_cam over the
// extent tiles, as oracle_sppm_pass does), hash (sppm_hash) and photon walk: tracePhoton is
// restated below from the oracle's trace_photon line for line, with the one difference that a
// (vertex, hit point) pair whose splat splatSample would add is written out as a record instead of
// being added to an image.  tests/test_sppm_ordered.py folds the records in the reference's two
// levels and requires oracle_sppm_pass's splat image bit for bit, which pins this restatement to
// the oracle's.  Build: make sppmref (HOSTFLAGS: -ffp-contract=off, no fast-math).
#include "../../oracle/oracle.cpp"

#include <algorithm>

namespace {

struct SpRecord { uint32_t thread, photon, seq, depth; int32_t sx, sy; float x, y, z; uint32_t pad; };
struct SpCount { uint64_t rays = 0, pairs = 0, dropped = 0; };

// mkHitPoints (SPPM.hs:133-164) as oracle_sppm_pass runs it, without the film: tile by tile, a
// tile's pixels by (iy, ix), for the radii r2
std::vector<HitPoint> eye_pass(const Scene& Sc, const std::vector<float>& r2, uint32_t seed, uint32_t pass) {
  const int nt = (int)Sc.tiles.size(), extW = Sc.ex1 - Sc.ex0 + 1;
  std::vector<std::vector<HitPoint>> thp(nt);
#pragma omp parallel for schedule(dynamic, 1)
  for (int t = 0; t < nt; ++t) {
    const Scene::Tile& w = Sc.tiles[t];
    for (int iy = w.y0; iy <= w.y1; ++iy)
      for (int ix = w.x0; ix <= w.x1; ++ix) {
        SampleCtx sc{&Sc, seed, pass, (uint32_t)((iy - Sc.ey0) * extW + (ix - Sc.ex0)), 0u, 0, 0,
                     SamplerCfg{BLING_SAMPLER_RANDOM, 1, 1}};
        float ox, oy, lu, lv;
        camera_sample(sc, &ox, &oy, &lu, &lv);
        const float px = (float)ix + ox, py = (float)iy + oy;
        const Ray ray = fire_ray(Sc.d->camera, px, py, lu, lv);
        EyeCtx E{&Sc, seed, pass, sc.pixel, px, py, r2[(size_t)sppm_sidx(Sc, px, py)], &thp[t], 0};
        trace_cam(E, ray, 0, 1u, white());
      }
  }
  std::vector<HitPoint> hps;
  for (int t = 0; t < nt; ++t) hps.insert(hps.end(), thp[t].begin(), thp[t].end());
  return hps;
}

// trace_photon (oracle.cpp; tracePhoton / followPhoton, SPPM.hs:181-239) with splat_sample's accepted
// splats as records
void trace_photon_rec(const Scene& Sc, const SppmHash& Hs, const std::vector<HitPoint>& hps, const SampleCtx& sc, uint32_t thread,
                      std::vector<SpRecord>& out, SpCount& C) {
  float ul = rnd1(sc, 0);
  float uo1, uo2, ud1, ud2;
  rnd2(sc, 0, &uo1, &uo2);
  rnd2(sc, 1, &ud1, &ud2);
  LightRay lr = sample_light_ray(Sc, ul, uo1, uo2, ud1, ud2);
  V wi0 = -lr.ray.d;
  if (!(lr.pdf > 0.f)) return;
  S li = sscale(lr.li, absdot(lr.n, wi0) / lr.pdf);
  if (is_black(li)) return;
  Ray ray = lr.ray;
  const int64_t cnt = (int64_t)hps.size();
  const int W = Sc.d->config.width, H = Sc.d->config.height;
  uint32_t seq = 0;
  for (int d = 0; d < (1 << 16); ++d) {
    V wi = -ray.d;
    Hit h;
    TStats ts;
    C.rays++;
    if (!sc_intersect(Sc, ray, &h, ts)) return;
    Bsdf bsdf = hit_bsdf(Sc, h);
    V p = bsdf.p, ng = bsdf.ng;
    if (has_non_specular(bsdf) && cnt > 0) {                                             // hashLookup (:307-314)
      V q = p - Hs.bounds.mn;
      int64_t x = (int64_t)std::fabs(q.x * Hs.scale), y = (int64_t)std::fabs(q.y * Hs.scale), z = (int64_t)std::fabs(q.z * Hs.scale);
      const size_t b = (size_t)sppm_bucket(x, y, z, cnt);
      sppm_kd_lookup(Hs.buckets[b], Hs.mr[b], hps, 0, (int)Hs.buckets[b].size(), 0, p, [&](const HitPoint& hp) {
        const uint32_t my = seq++;
        C.pairs++;
        S f = eval_bsdf(hp.bsdf, hp.w, wi);
        S l = sscale(hp.f * f * li, 1.f / (absdot(wi, ng) * hp.r2 * PI));
        // splatSample (Image.hs:201-221), as the oracle's splat_sample
        int px = (int)std::floor(hp.px), py = (int)std::floor(hp.py);
        if (px >= W || py >= H || px < 0 || py < 0) return;
        if (s_nan(l) || s_inf(l)) { C.dropped++; return; }
        SpRecord r{thread, sc.n, my, (uint32_t)d, px, py, 0.f, 0.f, 0.f, 0u};
        to_xyz(l, &r.x, &r.y, &r.z);
        out.push_back(r);
      });
    }
    float ubc = rnd1(sc, 1 + d * 2);
    float ub1, ub2;
    rnd2(sc, 2 + d, &ub1, &ub2);
    BsdfSample bs = sample_bsdf_t(bsdf, B_ALL, wi, ubc, ub1, ub2, true);                 // sampleAdjBsdf
    float pcont = d > 7 ? 0.8f : 1.f;
    S li2 = sscale(bs.f * li, 1.f / pcont);
    if (bs.pdf == 0.f || is_black(li2)) return;
    if (rnd1(sc, 2 + d * 2) > pcont) return;
    ray = Ray{p, bs.wi, h.eps, INF};
    li = li2;
  }
}

}  // namespace

extern "C" {

struct sppm_ref_stats { uint64_t hitpoints, photons, photon_rays, photon_hits; };

// The records of every sampler's photons of pass `pass`, for P's CURRENT radii (call it before
// oracle_sppm_pass of the same pass, which updates them): sampler by sampler, photon by photon, in
// the order the walk meets the pairs.  At most cap are copied to rec (may be NULL); returns their
// number.  P is not changed.
size_t sppm_ref_records(const oracle_sppm* P, uint32_t seed, uint32_t pass, int threads, SpRecord* rec, size_t cap,
                        sppm_ref_stats* st) {
  const Scene& Sc = P->os->s;
  const bling_render_config& cfg = Sc.d->config;
#ifdef _OPENMP
  if (threads > 0) omp_set_num_threads(threads);
#endif
  const std::vector<HitPoint> hps = eye_pass(Sc, P->r2, seed, pass);
  const SppmHash Hs = sppm_hash(hps);
  const int nth = std::max(1, cfg.sppm_threads);
  const int sn = std::max(1, (int)std::ceil(std::sqrt((float)cfg.sppm_photons / (float)nth)));
  std::vector<std::vector<SpRecord>> outs(nth);
  std::vector<SpCount> cnt(nth);
#pragma omp parallel for schedule(dynamic, 1)
  for (int k = 0; k < nth; ++k) {
    SampleCtx sc{&Sc, seed, pass, SPPM_PHOTON_PIXEL | (uint32_t)k, 0u, 7, 5, SamplerCfg{BLING_SAMPLER_STRATIFIED, sn, sn}};
    for (int s = 0; s < sn * sn; ++s) { sc.n = (uint32_t)s; trace_photon_rec(Sc, Hs, hps, sc, (uint32_t)k, outs[k], cnt[k]); }
  }
  size_t n = 0;
  sppm_ref_stats T{hps.size(), (uint64_t)nth * (uint64_t)sn * (uint64_t)sn, 0, 0};
  for (int k = 0; k < nth; ++k) {
    T.photon_rays += cnt[k].rays; T.photon_hits += cnt[k].pairs;
    for (const SpRecord& r : outs[k]) {
      if (rec && n < cap) rec[n] = r;
      ++n;
    }
  }
  if (st) *st = T;
  return n;
}

// sn of the scene's photon samplers (SPPM.hs:449, 474), as oracle_sppm_pass forms it
int sppm_ref_sn(const oracle_sppm* P) {
  const bling_render_config& cfg = P->os->s.d->config;
  const int nth = std::max(1, cfg.sppm_threads);
  return std::max(1, (int)std::ceil(std::sqrt((float)cfg.sppm_photons / (float)nth)));
}

}  // extern "C"
