// normals_ref.cpp -- CPU restatement of the normal-map integrator (mkNormalMap,
// Integrator/Debug.hs:25-34), test infrastructure only: never linked into the product libraries.
//
// It includes the oracle's translation unit, whose internals sit in an anonymous namespace, and so
// shares its binary32 restatements of the camera, the sampler, scIntersect, the hit's BSDF (shading
// geometry, bump mapping, mkBsdf's frame) and the tile film; it adds only li -- scIntersect, the
// shading normal of the hit's BSDF, rgbToSpectrumRefl -- and the per-tile film loop.  Citations are
// File.hs:line relative to src/lib/Graphics/Bling/ of the reference.  Build: make nmref (HOSTFLAGS:
// -ffp-contract=off, no fast-math).
#include "../../oracle/oracle.cpp"

namespace {

// rgbToSpectrumRefl (Spectrum.hs:140-159): rgbToSpectrum over the reflectance bases r, g, b, c, m, y, w;
// three ordered cases, sScale of the bases, the sums in the order written
S nm_rgb_to_spectrum_refl(float r, float g, float b) {
  const float (*B)[16] = BLING_RGB_REFL_BANDS;
  auto sc = [&](int k, float f) { return sscale(from_array(B[k]), f); };
  if (r <= g && r <= b) return sc(6, r) + (g <= b ? sc(3, g - r) + sc(2, b - g) : sc(3, b - r) + sc(1, g - b));
  if (g <= r && g <= b) return sc(6, g) + (r <= b ? sc(4, r - g) + sc(2, b - r) : sc(4, b - g) + sc(0, r - b));
  return sc(6, b) + (r <= b ? sc(5, r - b) + sc(1, g - r) : sc(5, g - b) + sc(0, r - g));
}

// intToSpectrum (Debug.hs:31-34): (vpromote 1 + n) / 2 componentwise
S nm_colour(V n) { return nm_rgb_to_spectrum_refl((1.f + n.x) / 2.f, (1.f + n.y) / 2.f, (1.f + n.z) / 2.f); }

struct NmOut { S L; float imx, imy; bool hit; V ns, ng; };

// li (Debug.hs:27-29) of sample n of extent pixel (px, py): no sample dimensions (SurfaceIntegrator li 0 0)
NmOut nm_sample(const Scene& Sc, SampleCtx sc, int px, int py, int n) {
  const int extW = Sc.ex1 - Sc.ex0 + 1;
  sc.pixel = (uint32_t)((py - Sc.ey0) * extW + (px - Sc.ex0));
  sc.n = (uint32_t)n;
  float ox, oy, lu, lv;
  camera_sample(sc, &ox, &oy, &lu, &lv);
  NmOut o{black(), (float)px + ox, (float)py + oy, false, mk(0.f, 0.f, 0.f), mk(0.f, 0.f, 0.f)};
  const Ray r = fire_ray(Sc.d->camera, o.imx, o.imy, lu, lv);
  Hit h;
  TStats ts;
  if (!sc_intersect(Sc, r, &h, ts)) return o;                                  // Nothing -> black
  const Bsdf bs = hit_bsdf(Sc, h);                                             // intBsdf int
  o.hit = true;
  o.ns = bs.cs.n;                                                              // bsdfShadingNormal
  o.ng = h.dg.n;
  o.L = nm_colour(o.ns);
  return o;
}

SampleCtx nm_sample_ctx(const Scene& Sc, uint32_t seed, uint32_t pass) {
  const bling_render_config& cfg = Sc.d->config;
  return SampleCtx{&Sc, seed, pass, 0, 0, 0, 0, SamplerCfg{cfg.sampler, cfg.nu, cfg.nv}};
}

}  // namespace

extern "C" {

struct nm_ref_stats { uint64_t samples, hits, dropped; };

// The colour of a normal, for known-answer tests: out = 16 floats
void nm_ref_colour(const float* n3, float* out) {
  const S s = nm_colour(mk(n3[0], n3[1], n3[2]));
  std::memcpy(out, s.v, sizeof s.v);
}

// li of n camera samples (x, y, n each): L = 16 n floats; img (may be NULL) = imageX, imageY per
// sample; geo (may be NULL) = 7 floats per sample: hit (0 / 1), the shading normal, the geometric normal
int nm_ref_sample_li(const oracle_scene* os, uint32_t seed, uint32_t pass, const int* samples, size_t n, float* L,
                     float* img, float* geo, int threads, nm_ref_stats* st) {
  const Scene& Sc = os->s;
  const SampleCtx sc0 = nm_sample_ctx(Sc, seed, pass);
#ifdef _OPENMP
  if (threads > 0) omp_set_num_threads(threads);
#endif
  uint64_t hits = 0;
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : hits)
  for (long i = 0; i < (long)n; ++i) {
    const NmOut o = nm_sample(Sc, sc0, samples[3 * i], samples[3 * i + 1], samples[3 * i + 2]);
    std::memcpy(L + 16 * i, o.L.v, sizeof o.L.v);
    if (img) { img[2 * i] = o.imx; img[2 * i + 1] = o.imy; }
    if (geo) {
      float* g = geo + 7 * i;
      g[0] = o.hit ? 1.f : 0.f;
      g[1] = o.ns.x; g[2] = o.ns.y; g[3] = o.ns.z;
      g[4] = o.ng.x; g[5] = o.ng.y; g[6] = o.ng.z;
    }
    hits += o.hit ? 1u : 0u;
  }
  if (st) { st->samples += n; st->hits += hits; }
  return 0;
}

// One pass of the sampler renderer with this integrator into film (W * H * 4, accumulated): the tiles
// k with k % shard_world == shard_rank, each sample added to its tile image in coverWindow order, the
// tile images added in tile order (Image.hs:178-199), like oracle_render_shard.
int nm_ref_render(const oracle_scene* os, uint32_t seed, uint32_t pass, int shard_rank, int shard_world, int threads,
                  float* film, nm_ref_stats* st) {
  const Scene& Sc = os->s;
  const bling_render_config& cfg = Sc.d->config;
  if (shard_world < 1 || shard_rank < 0 || shard_rank >= shard_world) return -1;
  std::vector<int> todo;
  for (int k = 0; k < (int)Sc.tiles.size(); ++k)
    if (k % shard_world == shard_rank) todo.push_back(k);
  std::vector<TileImg> imgs(todo.size());
  std::vector<uint64_t> smp(todo.size(), 0), hit(todo.size(), 0), drp(todo.size(), 0);
  const SampleCtx sc0 = nm_sample_ctx(Sc, seed, pass);
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
          const NmOut o = nm_sample(Sc, sc0, ix, iy, n);
          add_sample(imgs[i], Sc.d->filter, o.imx, o.imy, o.L, drp[i]);
          smp[i]++;
          hit[i] += o.hit ? 1u : 0u;
        }
  }
  const int W = cfg.width, H = cfg.height;
  for (size_t i = 0; i < todo.size(); ++i) {                                   // addTile in tile order
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
  if (st)
    for (size_t i = 0; i < todo.size(); ++i) { st->samples += smp[i]; st->hits += hit[i]; st->dropped += drp[i]; }
  return 0;
}

}  // extern "C"
