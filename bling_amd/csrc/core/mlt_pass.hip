// mlt_pass.hip -- host driver of one pass of the Metropolis renderer (Renderer/Metropolis.hs `pass`,
// :76-120) over the kernels of mlt.h and bidir.h.
//
// k_mlt_walk exists for two feature sets, like k_bd_walk (bidir_pass.hip): the cornell profile, compiled
// here with the driver, and every feature (FT_ALL), compiled in mlt_pass_walk.hip, which includes this
// file with BLING_MLT_UNIT_WALK_ALL set.
#include "core_internal.h"

namespace bcore {

template <uint32_t F>
void mlt_walk_launch(bling_ctx* c, const WaveState& W, const BdBufs& B, const float* vec, uint32_t stride, int n1d, int n2d,
                     uint32_t n) {
  k_mlt_walk<F><<<(n + 255) / 256, TRACE_BLOCK, c->lds_trace, c->stream>>>(c->dscene.p, W, B, vec, stride, n1d, n2d, n,
                                                                          c->counters.p);
}

#define BLING_MLT_WALK_ARGS bling_ctx*, const WaveState&, const BdBufs&, const float*, uint32_t, int, int, uint32_t
#if defined(BLING_MLT_UNIT_WALK_ALL)
template void mlt_walk_launch<FT_ALL>(BLING_MLT_WALK_ARGS);
#else
extern template void mlt_walk_launch<FT_ALL>(BLING_MLT_WALK_ARGS);

namespace {

// evalSample of the first n primary samples of vec into lfull: walk, connect, finish
void mlt_eval(bling_ctx* c, const WaveState& W, const MltBufs& M, const float* vec, uint32_t n) {
  if (n == 0) return;
  const BdBufs B = bidir_bufs(c, n, nullptr);
  if ((c->features & ~kProfiles[0]) == 0u) mlt_walk_launch<kProfiles[0]>(c, W, B, vec, M.cap, M.n1d, M.n2d, n);
  else mlt_walk_launch<FT_ALL>(c, W, B, vec, M.cap, M.n1d, M.n2d, n);
  bidir_connect_finish(c, W, B, n);
}

// mkDist1D's cdf (Montecarlo.hs:40-48) from the loader's builder (sky_model.h), which only the host pass sees
std::vector<float> dist1d_cdf(const std::vector<float>& f) {
  std::vector<float> cdf;
#if !defined(__HIP_DEVICE_COMPILE__)
  bling_dist1d(f, cdf);
#endif
  return cdf;
}

// upperBound (Montecarlo.hs:53-54) of sampleDiscrete1D
int upper_bound(const std::vector<float>& v, float u) {
  const int len = (int)v.size();
  int found = len - 1;                                               // maybe (length v - 1) ...
  for (int i = 0; i < len; ++i)
    if (v[i] >= u) { found = i - 1; break; }                         // ... (\i -> i - 1) $ findIndex (>= u) v
  return std::min(len - 2, std::max(0, found));
}

}  // namespace

// bootstrap's bookkeeping (:150-167) from the samples' I values, literally: sumI in foldl order (a NaN
// counts 0), the consed list `is` (reversed), smps written at n - i - 1 (a NaN leaves its slot unwritten,
// trap T34), mkDist1D, and every chain's own sampleDiscrete1D draw.  Returns b' = sumI / n and the chains'
// start samples; throws std::invalid_argument where MV.read would fail in the reference.
float mlt_boot_select(const float* I, uint32_t nboot, uint32_t seed, uint32_t pass, uint32_t chains, uint32_t* start) {
  float sumI = 0.f;
  std::vector<float> is;
  std::vector<uint8_t> written(nboot, 0);
  for (uint32_t i = 0; i < nboot; ++i) {
    if (I[i] != I[i]) { sumI = sumI + 0.f; continue; }
    written[nboot - i - 1] = 1;
    is.push_back(I[i]);
    sumI = sumI + I[i];
  }
  std::reverse(is.begin(), is.end());
  const std::vector<float> cdf = is.empty() ? std::vector<float>() : dist1d_cdf(is);
  for (uint32_t ch = 0; ch < chains; ++ch) {                         // every chain's own selection (:165-167)
    const float u = brng::u01(brng::draw(brng::sample_key(brng::pixel_key(seed, pass, MLT_CHAIN_PIXEL | ch), MLT_START_SAMPLE),
                                         brng::DIM_FRESH1D));
    const int slot = is.empty() ? -1 : upper_bound(cdf, u);
    if (slot < 0 || slot >= (int)nboot || !written[slot])
      throw std::invalid_argument("metropolis: the bootstrap selection of chain " + std::to_string(ch) + " reads slot " +
                                  std::to_string(slot) + ", which a NaN bootstrap sample left unwritten (an error in the reference)");
    start[ch] = nboot - 1u - (uint32_t)slot;                         // smps[slot] holds sample n - slot - 1
  }
  return sumI / (float)nboot;
}

void mlt_pass_run(bling_ctx* c, uint32_t seed, uint32_t pass, float* splat, bool ordered, uint32_t rec_first, uint32_t rec_chains,
                  bling_mlt_stats* st, MltOut* out) {
  const bling_metropolis& mp = c->mp;
  const DevScene& S = c->S;
  const int md = mp.max_depth, n1d = 12 * md + 1, n2d = 9 * md + 2, nv = n1d + 2 * n2d + 4;
  const uint64_t M = (uint64_t)mlt_mutations(mp, S.width, S.height);
  const uint32_t C = (uint32_t)mp.chains, nboot = (uint32_t)mp.bootstrap;
  const uint64_t per = M / C, extra = M % C;
  const uint64_t nsteps = per + (extra ? 1 : 0);
  ordered = ordered && splat;
  // ordered: the order is chain-major, the launches are mutation-major, so every splat of the pass (two a
  // mutation at most) is recorded and merged once
  if (ordered && 2 * M > (uint64_t)splat_budget(c))
    throw std::invalid_argument("metropolis: an ordered pass may write 2 M = " + std::to_string(2 * M) +
                                " splat records, more than the record budget " + std::to_string(splat_budget(c)));
  // the wave: every chain, and bootstrap chunks of at most kMltBootChunk samples
  const uint32_t wave = std::max(C, std::min(nboot, kMltBootChunk));
  const uint32_t cap = (wave + 255u) & ~255u;
  c->ensure_paths(cap);
  MltState& P = c->mlt;
  hipStream_t s = c->stream;
  if (P.cur.n != (size_t)nv * cap) { P.cur.alloc((size_t)nv * cap); P.prop.alloc((size_t)nv * cap); }
  if (P.cur_l.n != (size_t)18 * cap) { P.cur_l.alloc((size_t)18 * cap); P.flags.alloc(cap); P.start.alloc(cap); P.lfull.alloc((size_t)4 * cap); }
  if (P.boot_i.n < nboot) P.boot_i.alloc(nboot);
  if (P.ctr.n != 4) P.ctr.alloc(4);
  const size_t nrec = (size_t)nsteps * rec_chains;
  if (nrec && P.rec.n < 2 * nrec) P.rec.alloc(2 * nrec);
  MltBufs B{};
  B.cur = P.cur.p; B.prop = P.prop.p; B.cur_l = P.cur_l.p; B.flags = P.flags.p;
  B.splat = ordered ? nullptr : splat;
  MergeState& G = c->merge;
  if (ordered) {
    if (G.rec.n < (size_t)4 * M) G.rec.alloc((size_t)4 * M);
    if (G.rec_count.n != 1) G.rec_count.alloc(1);
    B.srec = G.rec.p; B.srec_count = G.rec_count.p; B.srec_cap = (uint32_t)(2 * M);
    HIPCHK(hipMemsetAsync(G.rec_count.p, 0, sizeof(uint32_t), s));
  }
  B.ctr = P.ctr.p;
  B.rec = nrec ? P.rec.p : nullptr;
  B.rec_first = rec_first; B.rec_chains = rec_chains;
  B.cap = cap; B.n1d = n1d; B.n2d = n2d;
  B.sx = (float)S.width; B.sy = (float)S.height;
  B.wt = 1.f / mp.mpp; B.plarge = mp.plarge;
  WaveState W = c->state();
  W.Lfull = P.lfull.p;
  const EventPair ev;                    // the pass's two timing events
  HIPCHK(hipMemsetAsync(P.ctr.p, 0, 4 * sizeof(unsigned long long), s));
  HIPCHK(hipMemsetAsync(c->counters.p, 0, sizeof(Counters), s));
  ev.a.record(s);
  // bootstrap (:142-169): evalI of nboot initialSamples, in chunks of the wave
  for (uint32_t first = 0; first < nboot; first += cap) {
    const uint32_t n = std::min(cap, nboot - first);
    k_mlt_fill<<<(n + 255) / 256, 256, 0, s>>>(B, B.prop, nullptr, first, n, seed, pass);
    mlt_eval(c, W, B, B.prop, n);
    k_mlt_boot_i<<<(n + 255) / 256, 256, 0, s>>>(P.lfull.p, n, P.boot_i.p + first);
  }
  HIPCHK(hipGetLastError());
  std::vector<float> I(nboot);
  HIPCHK(hipMemcpyAsync(I.data(), P.boot_i.p, (size_t)nboot * sizeof(float), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (c->mlt_boot_override.size() == nboot) I = c->mlt_boot_override;   // bling_debug_mlt_set_boot
  std::vector<uint32_t> start(C);
  const float b = mlt_boot_select(I.data(), nboot, seed, pass, C, start.data());
  HIPCHK(hipMemcpyAsync(P.start.p, start.data(), (size_t)C * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  // sCurr, lCurr (:83-84)
  k_mlt_fill<<<(C + 255) / 256, 256, 0, s>>>(B, B.prop, P.start.p, 0u, C, seed, pass);
  mlt_eval(c, W, B, B.prop, C);
  k_mlt_adopt<<<(C + 255) / 256, 256, 0, s>>>(B, P.lfull.p, C);
  if (nrec) HIPCHK(hipMemsetAsync(P.rec.p, 0xFF, 2 * nrec * sizeof(uint4), s));
  for (uint64_t m = 0; m < nsteps; ++m) {                            // chains whose share is exhausted sit out the last step
    const uint32_t live = m < per ? C : (uint32_t)extra;
    k_mlt_propose<<<(live + 255) / 256, 256, 0, s>>>(B, live, (uint32_t)m, seed, pass);
    mlt_eval(c, W, B, B.prop, live);
    k_mlt_accept<<<(live + 255) / 256, 256, 0, s>>>(c->dscene.p, B, P.lfull.p, live, (uint32_t)m, seed, pass);
  }
  HIPCHK(hipGetLastError());
  const EventPair evm;                   // the ordered merge's share of the pass
  if (ordered) {
    uint32_t nsplat = 0;
    HIPCHK(hipMemcpyAsync(&nsplat, G.rec_count.p, sizeof nsplat, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (nsplat > B.srec_cap) throw std::runtime_error("metropolis: splat record count beyond 2 M");
    evm.a.record(s);
    splat_merge(c, G.rec.p, nsplat, SM_LAYOUT_SPLAT, splat);
    evm.b.record(s);
  }
  ev.b.record(s);
  unsigned long long ctr[4];
  Counters hc;
  HIPCHK(hipMemcpyAsync(ctr, P.ctr.p, sizeof ctr, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&hc, c->counters.p, sizeof hc, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (st) {
    std::memset(st, 0, sizeof *st);
    st->b = b;
    st->mutations = M; st->large_steps = ctr[0]; st->accepted = ctr[1]; st->dropped = ctr[2]; st->splats = ctr[3];
    st->rays_camera = hc.cam; st->rays_continuation = hc.cont; st->rays_mis = hc.mis; st->rays_shadow = hc.shadow;
    st->path_vertices = hc.vertices;
    st->ms_total = ev.elapsed_ms();
  }
  if (ordered) { G.ms_merge = evm.elapsed_ms(); G.ms_kernel = ev.elapsed_ms() - G.ms_merge; }
  if (out) {
    out->b = b;
    out->start = start;
    out->rec.clear();
    if (nrec) {
      std::vector<bling_mlt_record> raw(nrec);
      static_assert(sizeof(bling_mlt_record) == 2 * sizeof(uint4), "record layout");
      HIPCHK(hipMemcpy(raw.data(), P.rec.p, nrec * sizeof(bling_mlt_record), hipMemcpyDeviceToHost));
      for (uint32_t k = 0; k < rec_chains; ++k) {
        const uint64_t mine = per + ((uint64_t)(rec_first + k) < extra ? 1 : 0);
        for (uint64_t m = 0; m < mine; ++m) out->rec.push_back(raw[(size_t)m * rec_chains + k]);
      }
    }
  }
}
#endif

}  // namespace bcore
