// mlt_ref.cpp -- CPU restatement of the Metropolis renderer (Renderer/Metropolis.hs), test
// infrastructure only: never linked into the product libraries.
//
// It includes the bidirectional integrator's restatement (and through it the oracle's translation
// unit): a chain sample is evaluated with contrib False md on a PrecomSample, which here is the
// oracle's precomputed-sample context (rnd' / rnd2D', Sampling.hs:203-221) holding the primary sample.
// Citations are Metropolis.hs:line unless a file is named.  The one departure:
// C independent chains, every draw keyed by (seed, pass, tag, index, ordinal) -- chains = 1 is the
// reference's structure.  Traps T32-T35 are restated as written.  Build: make mltref.
#include "bidir_ref.cpp"

namespace {

constexpr uint32_t MLT_CHAIN_PIXEL = 0x50000000u, MLT_BOOT_PIXEL = 0x60000000u, MLT_START_SAMPLE = 0xFFFFFFFEu;

// PrecomSample cs v1d v2d (Sampling.hs)
struct Pss { std::vector<float> v1d; std::vector<std::pair<float, float>> v2d; float x, y, lu, lv; };

// R.rnd number `ord` of a keyed stream
struct Stream {
  uint32_t seed, pass, pixel, sample, ord;
  float rnd() { return u01(hash5(seed, pass, pixel, sample, DIM_FRESH1D + ord++)); }
};

inline float lerp_hs(float t, float v1, float v2) { return (1.f - t) * v1 + t * v2; }        // Math.hs:108-110

// initialSample (:171-189)
Pss initial_sample(Stream& g, float sx, float sy, int n1d, int n2d) {
  Pss p;
  p.v1d.resize(n1d); p.v2d.resize(n2d);
  for (int i = 0; i < n1d; ++i) p.v1d[i] = g.rnd();
  for (int i = 0; i < n2d; ++i) { const float a = g.rnd(); const float b = g.rnd(); p.v2d[i] = {a, b}; }
  const float ox = g.rnd(), oy = g.rnd();
  const float lu = g.rnd(), lv = g.rnd();
  p.x = lerp_hs(ox, 0.f, sx); p.y = lerp_hs(oy, 0.f, sy); p.lu = lu; p.lv = lv;
  return p;
}

// jitter's pure part (:226-239) of v in [vmin, vmax) with the rnd2D (u1, u2)
float jitter_go(float v, float vmin, float vmax, float u1, float u2) {
  const float a = 1.f / 1024.f, b = 1.f / 256.f;
  const float logRat = -bcr::logf(b / a);
  const float delta = (vmax - vmin) * b * bcr::expf(logRat * u1);
  const float x = u2 < 0.5f ? v + delta : v - delta;
  if (x >= vmax) return vmin + (x - vmax);
  if (x < vmin) return vmax - (vmin - x);
  return x;
}
float jitter(Stream& g, float v, float vmin, float vmax) {                                      // :221-225
  if (vmin == vmax) return vmin;
  const float u1 = g.rnd(), u2 = g.rnd();
  return jitter_go(v, vmin, vmax, u1, u2);
}

// mutate (:191-219); *large: which branch the first draw took
Pss mutate(Stream& g, float sx, float sy, int n1d, int n2d, float plarge, const Pss& s, bool* large) {
  const float x = g.rnd();
  *large = x < plarge;
  if (*large) return initial_sample(g, sx, sy, n1d, n2d);
  Pss p;
  p.v1d.resize(n1d); p.v2d.resize(n2d);
  for (int i = 0; i < n1d; ++i) p.v1d[i] = jitter(g, s.v1d[i], 0.f, 1.f);
  for (int i = 0; i < n2d; ++i) {
    const float u1 = jitter(g, s.v2d[i].first, 0.f, 1.f);
    const float u2 = jitter(g, s.v2d[i].second, 0.f, 1.f);
    p.v2d[i] = {u1, u2};
  }
  p.x = jitter(g, s.x, 0.f, sx); p.y = jitter(g, s.y, 0.f, sy);                                // mutateCamaraSample (:213-219)
  p.lu = jitter(g, s.lu, 0.f, 1.f); p.lv = jitter(g, s.lv, 0.f, 1.f);
  return p;
}

struct Eval { S l; float x, y, i; };

// evalSample (:244-252) and evalI (:241-242) of the one (imageX, imageY, li) triple.  With sd = md every
// dimension contrib reads is precomputed; a read past them would draw from the chain's stream, which
// the untouched generator state below rules out.
Eval eval_sample(const Scene& Sc, const Pss& p, int n1d, int n2d, BdCount& C) {
  Mwc g(0u, 0u, 0u);
  const uint32_t gi = g.i, gc = g.c;
  MwcPixel mp;
  mp.g = &g; mp.v1d = p.v1d; mp.v2d = p.v2d;
  SampleCtx sc{&Sc, 0u, 0u, 0u, 0u, n1d, n2d, SamplerCfg{BLING_SAMPLER_STRATIFIED, 1, 1}, &mp};
  const Ray r = fire_ray(Sc.d->camera, p.x, p.y, p.lu, p.lv);
  Eval e;
  e.l = contrib(Sc, sc, r, nullptr, C);
  if (g.i != gi || g.c != gc) { std::fprintf(stderr, "mlt_ref: an evaluation drew from the chain's stream\n"); std::abort(); }
  e.x = p.x; e.y = p.y; e.i = sY(e.l);
  return e;
}

// mkDist1D's cdf (Montecarlo.hs:40-48) and upperBound (:53-54)
std::vector<float> dist1d_cdf(const std::vector<float>& f) {
  const int n = (int)f.size();
  std::vector<float> c(n + 1);
  c[0] = 0.f;
  for (int i = 0; i < n; ++i) c[i + 1] = c[i] + f[i] / (float)n;
  const float fi = c[n];
  std::vector<float> cdf(n + 1);
  for (int j = 0; j <= n; ++j) cdf[j] = fi != 0.f ? c[j] / fi : (float)j / (float)n;
  return cdf;
}
int upper_bound(const std::vector<float>& v, float u) {
  const int len = (int)v.size();
  int found = len - 1;
  for (int i = 0; i < len; ++i)
    if (v[i] >= u) { found = i - 1; break; }
  return std::min(len - 2, std::max(0, found));
}

// bootstrap's bookkeeping (:150-167), literally: `is` is consed (reversed), smps is written at n - i - 1,
// a NaN sample is dropped from `is` and leaves its slot unwritten (trap T34)
struct Boot { float sumI; std::vector<float> cdf; std::vector<uint8_t> written; };
Boot boot_tables(const float* I, int n) {
  Boot B;
  B.sumI = 0.f;
  B.written.assign(n, 0);
  std::vector<float> is;
  for (int i = 0; i < n; ++i) {
    if (std::isnan(I[i])) { B.sumI = B.sumI + 0.f; continue; }
    B.written[n - i - 1] = 1;
    is.insert(is.begin(), I[i]);
    B.sumI = B.sumI + I[i];
  }
  if (!is.empty()) B.cdf = dist1d_cdf(is);
  return B;
}
// the slot sampleDiscrete1D selects, or -1 where MV.read would fail; *sample = the bootstrap sample in it
int boot_select(const Boot& B, float u, int* sample) {
  const int n = (int)B.written.size();
  const int slot = B.cdf.empty() ? -1 : upper_bound(B.cdf, u);
  if (slot < 0 || slot >= n || !B.written[slot]) return -1;
  *sample = n - 1 - slot;
  return slot;
}

struct Splat { int px, py; float X, Y, Z; };
struct ChainOut { std::vector<Splat> splats; uint64_t large = 0, accepted = 0, dropped = 0; BdCount cnt; };

// splat (:68-69) then splatSample (Image.hs:201-221)
void splat(const Scene& Sc, ChainOut& O, float f, float wt, const Eval& e) {
  const S s = sscale(e.l, f * wt);
  const int W = Sc.d->config.width, H = Sc.d->config.height;
  const float fx = std::floor(e.x), fy = std::floor(e.y);
  if (!(fx >= 0.f && fy >= 0.f && fx < (float)W && fy < (float)H)) return;
  if (s_nan(s) || s_inf(s)) { O.dropped++; return; }
  Splat sp{(int)fx, (int)fy, 0.f, 0.f, 0.f};
  to_xyz(s, &sp.X, &sp.Y, &sp.Z);
  O.splats.push_back(sp);
}

}  // namespace

extern "C" {

struct mlt_ref_record { uint32_t chain, mutation; float x, y, i_prop, a; uint32_t flags, pad; };
struct mlt_ref_stats {
  double b;
  uint64_t mutations, large_steps, accepted, splats, dropped, rays_camera, rays_continuation, rays_mis, rays_shadow, path_vertices;
  double seconds;
};

// what the light subpaths of the last mlt_ref_pass met, bootstrap and chain evaluations together (coverage.h)
static Cov g_mlt_cov;
void mlt_ref_coverage(uint64_t* out) { std::memcpy(out, g_mlt_cov.c, sizeof g_mlt_cov.c); }

// One pass with the scene's metropolis block: splat64 / splat32 (W * H * 3, accumulated in (chain,
// mutation, current-then-proposal) order; may be NULL), the records of every chain sorted by (chain,
// mutation) (rec of cap entries, may be NULL; the count is M), starts (chains entries, may be NULL),
// abs64 / cnt (W * H * 3 / W * H, may be NULL): per channel the sum of |contribution|, per pixel the splats.
// Returns 0, -1 for a bad block, -2 where the bootstrap selection reads an unwritten slot.
int mlt_ref_pass(const oracle_scene* os, uint32_t seed, uint32_t pass, int threads, double* splat64, float* splat32,
                 mlt_ref_record* rec, size_t cap, uint32_t* starts, mlt_ref_stats* st, double* abs64, uint32_t* cnt_px) {
  const Scene& Sc = os->s;
  const bling_metropolis& mp = Sc.d->metropolis;
  const int md = mp.max_depth, W = Sc.d->config.width, H = Sc.d->config.height;
  if (md < 1 || md > BD_MAX_DEPTH || Sc.d->config.max_depth != md || mp.bootstrap < 1 || mp.chains < 1) return -1;
  const float mf = std::floor(mp.mpp * (float)(W * H));                                        // :86
  if (!(mf >= 1.f) || !(mf < 2147483648.f)) return -1;
  auto t0 = std::chrono::steady_clock::now();
  const uint64_t M = (uint64_t)mf, C = (uint64_t)mp.chains, per = M / C, extra = M % C;
  const int n1d = 12 * md + 1, n2d = 9 * md + 2, nboot = mp.bootstrap;
  const float sx = (float)W, sy = (float)H, wt = 1.f / mp.mpp;
#ifdef _OPENMP
  if (threads > 0) omp_set_num_threads(threads);
#endif
  std::vector<float> I(nboot);
  std::vector<BdCount> bc(nboot);
#pragma omp parallel for schedule(dynamic, 16)
  for (int i = 0; i < nboot; ++i) {
    Stream g{seed, pass, MLT_BOOT_PIXEL, (uint32_t)i, 0u};
    I[i] = eval_sample(Sc, initial_sample(g, sx, sy, n1d, n2d), n1d, n2d, bc[i]).i;
  }
  const Boot B = boot_tables(I.data(), nboot);
  const float b = B.sumI / (float)nboot;                                                       // :169
  std::vector<int> start(C);
  for (uint64_t c = 0; c < C; ++c) {
    Stream g{seed, pass, MLT_CHAIN_PIXEL | (uint32_t)c, MLT_START_SAMPLE, 0u};
    if (boot_select(B, g.rnd(), &start[c]) < 0) return -2;
  }
  std::vector<ChainOut> out(C);
  std::vector<uint64_t> first(C);
  for (uint64_t c = 0, at = 0; c < C; ++c) { first[c] = at; at += per + (c < extra ? 1 : 0); }
  const bool want_rec = rec && cap >= M;
#pragma omp parallel for schedule(dynamic, 1)
  for (long c = 0; c < (long)C; ++c) {
    ChainOut& O = out[c];
    Stream gb{seed, pass, MLT_BOOT_PIXEL, (uint32_t)start[c], 0u};
    Pss sCurr = initial_sample(gb, sx, sy, n1d, n2d);
    Eval lCurr = eval_sample(Sc, sCurr, n1d, n2d, O.cnt);                                      // :84
    const uint64_t mine = per + ((uint64_t)c < extra ? 1 : 0);
    for (uint64_t m = 0; m < mine; ++m) {
      Stream g{seed, pass, MLT_CHAIN_PIXEL | (uint32_t)c, (uint32_t)m, 0u};
      bool large;
      const Pss sProp = mutate(g, sx, sy, n1d, n2d, mp.plarge, sCurr, &large);
      const Eval lProp = eval_sample(Sc, sProp, n1d, n2d, O.cnt);
      const float iProp = lProp.i, iCurr = lCurr.i;
      const float q = iProp / iCurr;
      const float a = 1.f <= q ? 1.f : q;                                                      // GHC's min 1 q (trap T33)
      if (iCurr > 0.f && !std::isinf(1.f / iCurr)) splat(Sc, O, (1.f - a) / iCurr, wt, lCurr);
      if (iProp > 0.f && !std::isinf(1.f / iProp)) splat(Sc, O, a / iProp, wt, lProp);
      const float r = g.rnd();
      const bool acc = r < a;
      if (large) O.large++;
      if (acc) { O.accepted++; sCurr = sProp; lCurr = lProp; }
      if (want_rec) rec[first[c] + m] = mlt_ref_record{(uint32_t)c, (uint32_t)m, lProp.x, lProp.y, iProp, a,
                                                       (large ? 1u : 0u) | (acc ? 2u : 0u), 0u};
    }
  }
  mlt_ref_stats T{};
  BdCount cnt;
  auto add = [&](const BdCount& x) { cnt.cam += x.cam; cnt.cont += x.cont; cnt.mis += x.mis; cnt.shadow += x.shadow; cnt.verts += x.verts; cnt.cov.add(x.cov); };
  for (int i = 0; i < nboot; ++i) add(bc[i]);
  for (uint64_t c = 0; c < C; ++c) {
    add(out[c].cnt);
    T.large_steps += out[c].large; T.accepted += out[c].accepted; T.dropped += out[c].dropped; T.splats += out[c].splats.size();
    for (const Splat& s : out[c].splats) {
      const size_t o = 3 * ((size_t)s.px + (size_t)s.py * W);
      if (abs64) { abs64[o] += std::fabs((double)s.X); abs64[o + 1] += std::fabs((double)s.Y); abs64[o + 2] += std::fabs((double)s.Z); }
      if (cnt_px) cnt_px[o / 3]++;
      if (splat64) { splat64[o] += s.X; splat64[o + 1] += s.Y; splat64[o + 2] += s.Z; }
      if (splat32) { splat32[o] = splat32[o] + s.X; splat32[o + 1] = splat32[o + 1] + s.Y; splat32[o + 2] = splat32[o + 2] + s.Z; }
    }
    if (starts) starts[c] = (uint32_t)start[c];
  }
  g_mlt_cov = cnt.cov;
  if (st) {
    T.b = b; T.mutations = M;
    T.rays_camera = cnt.cam; T.rays_continuation = cnt.cont; T.rays_mis = cnt.mis; T.rays_shadow = cnt.shadow;
    T.path_vertices = cnt.verts;
    T.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    *st = T;
  }
  return 0;
}

// Probes for the known-answer tests.
float mlt_ref_jitter(float v, float vmin, float vmax, float u1, float u2) { return jitter_go(v, vmin, vmax, u1, u2); }

// One mutation of chain `chain`, mutation m, of the primary sample cur (n1d + 2 n2d + 4 floats: v1d, v2d
// pairs, x, y, lu, lv) into prop; returns the number of draws taken, *large the branch.
int mlt_ref_mutate(uint32_t seed, uint32_t pass, uint32_t chain, uint32_t m, int md, float sx, float sy, float plarge,
                   const float* cur, float* prop, int* large) {
  const int n1d = 12 * md + 1, n2d = 9 * md + 2;
  Pss s;
  s.v1d.assign(cur, cur + n1d);
  s.v2d.resize(n2d);
  for (int i = 0; i < n2d; ++i) s.v2d[i] = {cur[n1d + 2 * i], cur[n1d + 2 * i + 1]};
  const float* cs = cur + n1d + 2 * n2d;
  s.x = cs[0]; s.y = cs[1]; s.lu = cs[2]; s.lv = cs[3];
  Stream g{seed, pass, MLT_CHAIN_PIXEL | chain, m, 0u};
  bool lg;
  const Pss p = mutate(g, sx, sy, n1d, n2d, plarge, s, &lg);
  std::copy(p.v1d.begin(), p.v1d.end(), prop);
  for (int i = 0; i < n2d; ++i) { prop[n1d + 2 * i] = p.v2d[i].first; prop[n1d + 2 * i + 1] = p.v2d[i].second; }
  float* ps = prop + n1d + 2 * n2d;
  ps[0] = p.x; ps[1] = p.y; ps[2] = p.lu; ps[3] = p.lv;
  *large = lg ? 1 : 0;
  return (int)g.ord;
}

// Bootstrap bookkeeping of hand-built I values: *b = sumI / n, the selected slot for u (-1: unwritten,
// an error in the reference) and the bootstrap sample it holds.
int mlt_ref_boot_select(const float* I, int n, float u, float* b, int* sample) {
  const Boot B = boot_tables(I, n);
  *b = B.sumI / (float)n;
  *sample = -1;
  return boot_select(B, u, sample);
}

// The same for every chain of a pass with its own keys: *b and starts (chains entries); -2 where a chain's
// selection reads an unwritten slot (*bad = that chain).
int mlt_ref_boot_starts(const float* I, int n, uint32_t seed, uint32_t pass, uint32_t chains, float* b, uint32_t* starts,
                        uint32_t* bad) {
  const Boot B = boot_tables(I, n);
  *b = B.sumI / (float)n;
  for (uint32_t c = 0; c < chains; ++c) {
    Stream g{seed, pass, MLT_CHAIN_PIXEL | c, MLT_START_SAMPLE, 0u};
    int smp = -1;
    if (boot_select(B, g.rnd(), &smp) < 0) { *bad = c; return -2; }
    starts[c] = (uint32_t)smp;
  }
  return 0;
}

// The mutations of chain c of C when a pass does M
uint64_t mlt_ref_chain_mutations(uint64_t M, uint64_t C, uint64_t c) { return M / C + (c < M % C ? 1 : 0); }

}  // extern "C"
