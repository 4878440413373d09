// bidir_ref.cpp -- CPU restatement of the bidirectional path integrator (Integrator/BidirPath.hs),
// test infrastructure only: never linked into the product libraries.
//
// It includes the oracle's translation unit, whose internals sit in an anonymous namespace, and so
// shares its binary32 restatements of sampleLightRay, sampleBsdf / sampleAdjBsdf, evalBsdf,
// sampleOneLight, intLe, scIntersect / occluded, the hit's BSDF, the sampler and the tile film; it adds
// only contrib, countSpec, connect, estimateDirect, eyePath, lightPath, nextVertex and the adjoint
// evalBsdf.  Citations are BidirPath.hs:line unless a file is named (relative to
// src/lib/Graphics/Bling/ of the reference).  The reference's oddities (DESIGN.md traps T25-T31) are
// restated as written.  Build: make bdref (HOSTFLAGS: -ffp-contract=off, no fast-math).
#include "../../oracle/oracle.cpp"

#include <algorithm>

#include "coverage.h"

namespace {

// evalBsdf True (Reflection.hs:318-332): eval b = bxdfEval b (not flipped), scaled by |sideTest|
S bd_eval_bsdf_adj(const Bsdf& bs, V woW, V wiW) {
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

constexpr int BD_MAX_DEPTH = 16;

// Vert wi wo int type alpha (:21-27); the intersection's BSDF (intBsdf int) is kept beside it
struct Vert { V wi, wo; Hit h; Bsdf bsdf; int type; S alpha; };
inline bool v_spec(const Vert& v) { return (v.type & B_SPEC) == B_SPEC; }              // bxdfIs Specular

struct BdCount { uint64_t cam = 0, cont = 0, mis = 0, shadow = 0, verts = 0; Cov cov; };

// sampler dimensions of mkBidirPathIntegrator (:44-48): smps1D * sd * 3 + 1, smps2D * sd * 3 + 2
SampleCtx bd_sample_ctx(const Scene& Sc, uint32_t seed, uint32_t pass) {
  const bling_render_config& cfg = Sc.d->config;
  return SampleCtx{&Sc, seed, pass, 0, 0, 12 * cfg.sample_depth + 1, 9 * cfg.sample_depth + 2,
                   SamplerCfg{cfg.sampler, cfg.nu, cfg.nv}};
}

// nextVertex (:175-213), the recursion as a loop.  The first clause matches the intersection before
// the depth guard, so the segment after vertex md - 1 is intersected too; a vertex whose sample is
// black or has pdf 0 is kept and ends the walk without a next segment.  The roulette draw (1 + f1d)
// is compared against rrProb = 1 and never read.  first: the walk's first segment (already counted).
void next_vertex(bool adj, const Scene& Sc, const SampleCtx& sc, V wi, bool hit, Hit h, S alpha, int md, int f1d0,
                 int f2d0, std::vector<Vert>& out, BdCount& C) {
  TStats ts;
  for (int depth = 0;; ++depth) {
    if (!hit) return;                                                          // :187
    if (depth == md) return;                                                   // :189
    const float ubc = rnd1(sc, f1d0 + 12 * depth);                             // :191
    float u1, u2;
    rnd2(sc, f2d0 + 9 * depth, &u1, &u2);                                      // :192
    const Bsdf bsdf = hit_bsdf(Sc, h);
    const BsdfSample bs = sample_bsdf_t(bsdf, B_ALL, wi, ubc, u1, u2, adj);    // :194-195
    if (adj) cov_vertex(C.cov, Sc, h, bsdf, ubc);
    out.push_back(Vert{wi, bs.wi, h, bsdf, bs.flags, alpha});                  // :198
    C.verts++;
    if (is_black(bs.f) || bs.pdf == 0.f) return;                               // :207-208
    alpha = sscale(bs.f * alpha, 1.f / 1.f);                                   // :199-201 (pathScale = f, rrProb = 1)
    C.cont++;
    hit = sc_intersect(Sc, Ray{bsdf.p, bs.wi, h.eps, INF}, &h, ts);           // :196
    wi = -bs.wi;                                                               // :197
  }
}

// countSpec (:103-112): x[i + j + 2] counts the pairs with a specular eye or light vertex
void count_spec(const int* espec, int ne, const int* lspec, int nl, float* x) {
  for (int k = 0; k < ne + nl + 2; ++k) x[k] = 0.f;
  for (int i = 0; i < ne; ++i)
    for (int j = 0; j < nl; ++j)
      if (espec[i] || lspec[j]) x[i + j + 2] = x[i + j + 2] + 1.f;
}

// connect (:114-140) as called at :90-92 with ((vl, s), (ve, t)): the first component -- the light
// vertex -- takes the pattern's eye role (evalBsdf False), the eye vertex the light role (evalBsdf
// True); `Vert _ wie ...` binds the second field, the vertex's sampled wo.
S connect(const Scene& Sc, const float* nspec, const Vert& a, int i, const Vert& b, int j, BdCount& C) {
  if (v_spec(a)) return black();                                               // :118
  if (v_spec(b)) return black();                                               // :119
  const V pe = a.bsdf.p, pl = b.bsdf.p;
  const V dv = pl - pe;
  const float l2 = sqlen(dv);
  const float wl = l2 != 0.f ? std::sqrt(l2) : 0.f;                            // normLen (Math.hs:356-363)
  const V w = l2 != 0.f ? vs(dv, 1.f / wl) : dv;
  const S fe = eval_bsdf(a.bsdf, a.wo, w);                                     // :130
  if (is_black(fe)) return black();                                            // :120
  const S fl = bd_eval_bsdf_adj(b.bsdf, b.wo, -w);                             // :134
  if (is_black(fl)) return black();
  TStats ts;
  C.shadow++;
  if (sc_occluded(Sc, Ray{pe, w, a.h.eps, wl - b.h.eps}, ts)) return black();  // :121, :136
  const float pathWt = 1.f / ((float)(i + j + 2) - nspec[i + j + 2]);          // :124
  const float g = 1.f / sqlen(pl - pe);                                        // :125
  return sscale(a.alpha * fe * b.alpha * fl, g * pathWt);                      // :122
}

struct BdTerms { S ld, le, l; int ne, nl; uint32_t emask, lmask; };

// contrib False md (:50-96) of one camera ray
S contrib(const Scene& Sc, const SampleCtx& sc, const Ray& r, BdTerms* T, BdCount& C) {
  const int md = Sc.d->config.max_depth;
  TStats ts;
  const float ul = rnd1(sc, 0);                                                // :52-54
  float uo1, uo2, ud1, ud2;
  rnd2(sc, 0, &uo1, &uo2);
  rnd2(sc, 1, &ud1, &ud2);
  std::vector<Vert> lp, ep;
  {                                                                            // lightPath (:167-173)
    const LightRay lr = sample_light_ray(Sc, ul, uo1, uo2, ud1, ud2);
    cov_light_ray(C.cov, Sc, ul);
    const V wo = -lr.ray.d;                                                    // not normalised, pdf not tested
    const S li = sscale(lr.li, absdot(lr.n, wo) / lr.pdf);
    Hit h;
    C.cont++;
    const bool hit = sc_intersect(Sc, lr.ray, &h, ts);
    next_vertex(true, Sc, sc, wo, hit, h, li, md, 4, 5, lp, C);
  }
  {                                                                            // eyePath (:161-164)
    Hit h;
    C.cam++;
    const bool hit = sc_intersect(Sc, r, &h, ts);
    next_vertex(false, Sc, sc, -r.d, hit, h, white(), md, 3, 4, ep, C);
  }
  const int ne = (int)ep.size(), nl = (int)lp.size();
  int espec[BD_MAX_DEPTH], lspec[BD_MAX_DEPTH];
  uint32_t emask = 0, lmask = 0;
  for (int i = 0; i < ne; ++i) { espec[i] = v_spec(ep[i]); emask |= (uint32_t)espec[i] << i; }
  for (int j = 0; j < nl; ++j) { lspec[j] = v_spec(lp[j]); lmask |= (uint32_t)lspec[j] << j; }
  float nspec[2 * BD_MAX_DEPTH + 2];
  count_spec(espec, ne, lspec, nl, nspec);                                     // :61
  S ld = black();                                                              // :70-72
  for (int i = 0; i < ne; ++i) {
    const Vert& v = ep[i];                                                     // estimateDirect (:142-154)
    const float lNumU = rnd1(sc, 1 + 12 * i);
    float ld1, ld2, lb1, lb2;
    rnd2(sc, 2 + 9 * i, &ld1, &ld2);
    const float lBc = rnd1(sc, 2 + 12 * i);
    rnd2(sc, 3 + 9 * i, &lb1, &lb2);
    Counters oc;
    const S lHere = sample_one_light(Sc, v.bsdf.p, v.h.eps, v.wi, v.bsdf, lNumU, ld1, ld2, lBc, lb1, lb2, oc);
    C.mis += oc.mis; C.shadow += oc.shadow;
    const S d = lHere * v.alpha;
    ld = ld + sscale(d, 1.f / (1.f + (float)i - nspec[i + 1]));
  }
  S le = black();                                                              // :75-82
  for (int i = 0; i < ne; ++i) {
    const bool prev_spec = i == 0 ? true : espec[i - 1] != 0;
    if (prev_spec) le = le + ep[i].alpha * int_le(Sc, ep[i].h, ep[i].wo);      // towards the sampled wo
  }
  S l = black();                                                               // :90-92
  for (int s = 0; s < nl; ++s) {
    S inner = black();
    for (int t = 0; t < ne; ++t) inner = inner + connect(Sc, nspec, lp[s], s, ep[t], t, C);
    l = l + inner;
  }
  if (T) { T->ld = ld; T->le = le; T->l = l; T->ne = ne; T->nl = nl; T->emask = emask; T->lmask = lmask; }
  if (ne == 0 || nl == 0) return ld + le;                                      // :94-96
  return ld + le + l;
}

struct BdSampleOut { S L; float imx, imy; };

BdSampleOut bd_sample(const Scene& Sc, SampleCtx sc, int px, int py, int n, BdTerms* T, BdCount& C) {
  const int extW = Sc.ex1 - Sc.ex0 + 1;
  sc.pixel = (uint32_t)((py - Sc.ey0) * extW + (px - Sc.ex0));
  sc.n = (uint32_t)n;
  float ox, oy, lu, lv;
  camera_sample(sc, &ox, &oy, &lu, &lv);
  const float imx = (float)px + ox, imy = (float)py + oy;
  const Ray r = fire_ray(Sc.d->camera, imx, imy, lu, lv);
  return BdSampleOut{contrib(Sc, sc, r, T, C), imx, imy};
}

}  // namespace

extern "C" {

struct bd_ref_stats { uint64_t samples, rays_camera, rays_continuation, rays_mis, rays_shadow, path_vertices, dropped; double seconds; };

// what the light subpaths of the last bd_ref_sample_li / bd_ref_render met (coverage.h)
static Cov g_bd_cov;
void bd_ref_coverage(uint64_t* out) { std::memcpy(out, g_bd_cov.c, sizeof g_bd_cov.c); }

static void bd_add(bd_ref_stats* st, const BdCount& C) {
  st->rays_camera += C.cam; st->rays_continuation += C.cont; st->rays_mis += C.mis; st->rays_shadow += C.shadow;
  st->path_vertices += C.verts;
}

// Radiance of n camera samples (x, y, n each): L = 16 n floats; terms (may be NULL) = 3 x 16 floats per
// sample (ld, le, l); lens (may be NULL) = 4 ints per sample (eye length, light length, eye specular
// mask, light specular mask); st accumulates the ray counts.
int bd_ref_sample_li(const oracle_scene* os, uint32_t seed, uint32_t pass, const int* samples, size_t n, float* L,
                     float* terms, int* lens, int threads, bd_ref_stats* st) {
  const Scene& Sc = os->s;
  const int md = Sc.d->config.max_depth;
  if (md < 1 || md > BD_MAX_DEPTH) return -1;
  const SampleCtx sc0 = bd_sample_ctx(Sc, seed, pass);
#ifdef _OPENMP
  if (threads > 0) omp_set_num_threads(threads);
#endif
  std::vector<BdCount> cnt(n);
#pragma omp parallel for schedule(dynamic, 16)
  for (long i = 0; i < (long)n; ++i) {
    BdTerms T;
    const BdSampleOut o = bd_sample(Sc, sc0, samples[3 * i], samples[3 * i + 1], samples[3 * i + 2], &T, cnt[i]);
    std::memcpy(L + 16 * i, o.L.v, sizeof o.L.v);
    if (terms) {
      std::memcpy(terms + 48 * i, T.ld.v, 64); std::memcpy(terms + 48 * i + 16, T.le.v, 64);
      std::memcpy(terms + 48 * i + 32, T.l.v, 64);
    }
    if (lens) { lens[4 * i] = T.ne; lens[4 * i + 1] = T.nl; lens[4 * i + 2] = (int)T.emask; lens[4 * i + 3] = (int)T.lmask; }
  }
  g_bd_cov = Cov{};
  for (size_t i = 0; i < n; ++i) g_bd_cov.add(cnt[i].cov);
  if (st) {
    for (size_t i = 0; i < n; ++i) bd_add(st, cnt[i]);
    st->samples += n;
  }
  return 0;
}

// One pass of the sampler renderer with this integrator into film (W * H * 4, accumulated), the tiles
// k with k % shard_world == shard_rank, added in tile order like oracle_render_shard.  term_mask
// selects what a sample contributes: 7 = contrib's radiance; otherwise the sum, from 0, of the terms
// whose bit is set (1 ld, 2 le, 4 l) -- for the convergence test's findings.  Counter RNG only.
int bd_ref_render(const oracle_scene* os, uint32_t seed, uint32_t pass, int shard_rank, int shard_world, int term_mask,
                  int threads, float* film, bd_ref_stats* st) {
  const Scene& Sc = os->s;
  const bling_render_config& cfg = Sc.d->config;
  if (cfg.max_depth < 1 || cfg.max_depth > BD_MAX_DEPTH) return -1;
  if (shard_world < 1 || shard_rank < 0 || shard_rank >= shard_world) return -1;
  auto t0 = std::chrono::steady_clock::now();
  std::vector<int> todo;
  for (int k = 0; k < (int)Sc.tiles.size(); ++k)
    if (k % shard_world == shard_rank) todo.push_back(k);
  std::vector<TileImg> imgs(todo.size());
  std::vector<BdCount> cs(todo.size());
  std::vector<uint64_t> smp(todo.size(), 0), drp(todo.size(), 0);
  const SampleCtx sc0 = bd_sample_ctx(Sc, seed, pass);
#ifdef _OPENMP
  if (threads > 0) omp_set_num_threads(threads);
#endif
#pragma omp parallel for schedule(dynamic, 1)
  for (int i = 0; i < (int)todo.size(); ++i) {
    const Scene::Tile& w = Sc.tiles[todo[i]];
    imgs[i] = make_tile(Sc, w);
    for (int iy = w.y0; iy <= w.y1; ++iy)                                      // coverWindow: y outer
      for (int ix = w.x0; ix <= w.x1; ++ix)
        for (int n = 0; n < cfg.spp; ++n) {
          BdTerms T;
          const BdSampleOut o = bd_sample(Sc, sc0, ix, iy, n, &T, cs[i]);
          S L = o.L;
          if (term_mask != 7) {
            L = black();
            if (term_mask & 1) L = L + T.ld;
            if (term_mask & 2) L = L + T.le;
            if (term_mask & 4) L = L + T.l;
          }
          add_sample(imgs[i], Sc.d->filter, o.imx, o.imy, L, drp[i]);
          smp[i]++;
        }
  }
  const int W = cfg.width, H = cfg.height;
  for (size_t i = 0; i < todo.size(); ++i) {                                   // addTile in tile order (Image.hs:178-199)
    const TileImg& T = imgs[i];
    for (int y = 0; y < T.h; ++y)
      for (int x = 0; x < T.w; ++x) {
        const int gx = x + T.ox, gy = y + T.oy;
        if (gy >= H || gx >= W) continue;
        float* o = film + 4 * ((size_t)gy * W + gx);
        const float* q = &T.px[4 * ((size_t)y * T.w + x)];
        for (int c = 0; c < 4; ++c) o[c] = o[c] + q[c];
      }
  }
  g_bd_cov = Cov{};
  for (size_t i = 0; i < todo.size(); ++i) g_bd_cov.add(cs[i].cov);
  if (st) {
    for (size_t i = 0; i < todo.size(); ++i) { bd_add(st, cs[i]); st->samples += smp[i]; st->dropped += drp[i]; }
    st->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
  return 0;
}

// What addSample keeps of n spectra (Image.hs:253-256, spectrumToXYZ): X, Y, Z, 1 per sample, zeros for
// a NaN / Inf one -- the per-sample result the device's film kernels read (bling_debug_pass_results)
void bd_ref_results(const float* L, size_t n, float* out4) {
  for (size_t i = 0; i < n; ++i) {
    S s;
    std::memcpy(s.v, L + 16 * i, sizeof s.v);
    float* o = out4 + 4 * i;
    o[0] = o[1] = o[2] = o[3] = 0.f;
    if (s_nan(s) || s_inf(s)) continue;
    to_xyz(s, &o[0], &o[1], &o[2]);
    o[3] = 1.f;
  }
}

// countSpec probe: nspec[0 .. ne + nl + 1] for subpath lengths and specular masks (bit i = vertex i)
int bd_ref_count_spec(int ne, int nl, uint32_t emask, uint32_t lmask, float* out) {
  if (ne < 0 || nl < 0 || ne > BD_MAX_DEPTH || nl > BD_MAX_DEPTH) return -1;
  int es[BD_MAX_DEPTH], ls[BD_MAX_DEPTH];
  for (int i = 0; i < ne; ++i) es[i] = (emask >> i) & 1u;
  for (int j = 0; j < nl; ++j) ls[j] = (lmask >> j) & 1u;
  count_spec(es, ne, ls, nl, out);
  return 0;
}

}  // extern "C"
