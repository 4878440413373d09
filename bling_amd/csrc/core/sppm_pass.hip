// sppm_pass.hip -- host driver of one SPPM pass (Renderer/SPPM.hs onePass) over the kernels of sppm.h.
#include "core_internal.h"
#include "ordered_ranges.h"

namespace bcore {

// ------------------------------------------------------------------ SPPM pass (sppm.h)
static SppmBufs sppm_bufs(bling_ctx* c) {
  SppmState& P = c->sppm;
  SppmBufs B{};
  B.hp_pos = P.hp_pos.p; B.hp_hit = P.hp_hit.p; B.hp_o = P.hp_o.p; B.hp_d = P.hp_d.p; B.hp_f = P.hp_f.p;
  B.hp_bsdf = P.hp_bsdf.p;
  B.hp_count = P.hp_count.p; B.hp_cap = P.hp_cap;
  B.r2 = P.r2.p; B.nacc = P.nacc.p; B.cnt = P.cnt.p; B.n_stats = P.n_stats;
  B.grid = P.grid.p; B.bstart = P.bstart.p; B.bcur = P.bcur.p; B.items = P.items.p; B.items_cap = P.items_cap;
  B.hp_key = P.hp_key.p; B.kd_mr = P.kd_mr.p; B.kd_c = P.kd_c.p;
  B.splat = P.splat.p; B.ctr = P.ctr.p;
  return B;
}


static void sppm_alloc_hitpoints(SppmState& P, uint32_t cap) {
  P.hp_cap = cap;
  for (auto* b : {&P.hp_pos, &P.hp_hit, &P.hp_o, &P.hp_d}) b->alloc(cap);
  P.hp_f.alloc((size_t)4 * cap);
  P.hp_bsdf.alloc(cap);
  P.hp_key.alloc(cap);
  P.bstart.alloc((size_t)cap + 1);
  P.bcur.alloc(cap);
}

void sppm_init(bling_ctx* c) {
  SppmState& P = c->sppm;
  const DevScene& S = c->S;
  const int ext_h = S.ey1 - S.ey0 + 1;
  P.n_ext = (uint32_t)S.ext_w * (uint32_t)ext_h;
  P.n_stats = P.n_ext;                                                 // windowPixels (Sampling.hs:60-62)
  P.nth = (uint32_t)std::max(1, c->cfg.sppm_threads);
  std::vector<float> r2(P.n_stats, c->cfg.sppm_radius * c->cfg.sppm_radius);
  P.r2.upload(r2.data(), r2.size());
  P.nacc.alloc(P.n_stats);
  HIPCHK(hipMemset(P.nacc.p, 0, P.n_stats * sizeof(float)));
  P.cnt.alloc((size_t)P.nth * P.n_stats);
  // the extent's 16 x 16 tiles (splitWindow), one camera sample per pixel, in tile order
  std::vector<TileDesc> tl;
  uint32_t off = 0;
  for (int y = S.ey0; y <= S.ey1; y += 16)
    for (int x = S.ex0; x <= S.ex1; x += 16) {
      TileDesc t{x, std::min(x + 15, S.ex1), y, std::min(y + 15, S.ey1), off, 0u};
      t.count = (uint32_t)((t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1));
      off += t.count;
      tl.push_back(t);
    }
  P.n_tiles = (uint32_t)tl.size();
  P.tiles.upload(tl.data(), tl.size());
  P.result.alloc(P.n_ext); P.img.alloc(P.n_ext);
  P.hp_count.alloc(1); P.grid.alloc(1); P.ctr.alloc(4);
  sppm_alloc_hitpoints(P, 2 * P.n_ext);
  P.splat.alloc((size_t)S.width * S.height * 3);
  P.film.alloc((size_t)S.width * S.height * 4);
  P.ready = true;
}

template <uint32_t F>
static void sppm_launch_eye(bling_ctx* c, const WaveState& W, uint32_t seed, uint32_t pass) {
  SppmState& P = c->sppm;
  HIPCHK(hipMemsetAsync(P.hp_count.p, 0, sizeof(uint32_t), c->stream));
  HIPCHK(hipMemsetAsync(P.ctr.p, 0, 4 * sizeof(unsigned long long), c->stream));
  k_sppm_eye<F><<<dim3(1, P.n_tiles), TRACE_BLOCK, c->lds_trace, c->stream>>>(c->dscene.p, sppm_bufs(c), W, P.tiles.p,
                                                                             seed, pass);
  HIPCHK(hipGetLastError());
}

uint32_t sppm_sn(const bling_ctx* c) {
  const uint32_t nth = (uint32_t)std::max(1, c->cfg.sppm_threads);
  const uint32_t sn = (uint32_t)std::max(1, (int)std::ceil(std::sqrt((float)c->cfg.sppm_photons / (float)nth)));
  const uint64_t nph = (uint64_t)nth * sn * sn;
  if (nph > 0xFFFFFFFFull || (uint64_t)sn * sn > (1u << 24)) throw std::invalid_argument("too many photons per pass");
  return sn;
}

// mkHitPoints and mkHash: the eye pass (an overflowing hit-point buffer is grown and the deterministic pass
// re-run), the film through `film` (called with the hit point count, between the two), then grid, bucket
// counts, offsets, entries and kd-trees; ordered: the never-sorted small buckets in the reference's order.
// Returns the hit points appended (which the buffer now holds).
template <uint32_t F, class Film>
static uint32_t sppm_eye_and_hash(bling_ctx* c, const WaveState& W, uint32_t seed, uint32_t pass, bool ordered, const Event& e1,
                                  Film&& film) {
  SppmState& P = c->sppm;
  hipStream_t s = c->stream;
  sppm_launch_eye<F>(c, W, seed, pass);
  uint32_t nhp = 0;
  HIPCHK(hipMemcpyAsync(&nhp, P.hp_count.p, sizeof nhp, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (nhp > P.hp_cap) {
    sppm_alloc_hitpoints(P, nhp + nhp / 4 + 1024);
    sppm_launch_eye<F>(c, W, seed, pass);
  }
  film();
  e1.record(s);
  HIPCHK(hipMemsetAsync(P.grid.p, 0, sizeof(SppmGrid), s));
  if (nhp > 0) {
    k_sppm_reduce<<<1, 1024, 0, s>>>(sppm_bufs(c));
    HIPCHK(hipMemsetAsync(P.bstart.p, 0, ((size_t)nhp + 1) * sizeof(uint32_t), s));
    const unsigned gb = (nhp + 255u) / 256u;
    k_sppm_cells<false><<<gb, 256, 0, s>>>(sppm_bufs(c));
    k_sppm_scan<<<1, 1024, 0, s>>>(sppm_bufs(c));
    SppmGrid g;
    HIPCHK(hipMemcpyAsync(&g, P.grid.p, sizeof g, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (g.items > P.items_cap) {
      P.items_cap = g.items + g.items / 4 + 1024;
      P.items.alloc(P.items_cap); P.kd_mr.alloc(P.items_cap); P.kd_c.alloc(P.items_cap);
    }
    k_sppm_cells<true><<<gb, 256, 0, s>>>(sppm_bufs(c));
    k_sppm_kd<<<gb, 256, 0, s>>>(sppm_bufs(c));                           // a kd-tree per bucket
    if (ordered) k_sppm_leaf_order<<<gb, 256, 0, s>>>(c->dscene.p, sppm_bufs(c));
    HIPCHK(hipGetLastError());
  }
  return nhp;
}

// One record-mode launch: photons first .. first + count - 1 of sampler k into the launch's own counts,
// counters and (rec_cap > 0) records.  Returns the records claimed; ctr receives the four counters.
template <uint32_t F>
static uint32_t sppm_launch_rec(bling_ctx* c, uint32_t seed, uint32_t pass, uint32_t sn, uint32_t k, uint32_t first, uint32_t count,
                                uint32_t rec_cap, unsigned long long ctr[4], const EventPair& ev) {
  SppmState& P = c->sppm;
  hipStream_t s = c->stream;
  if (P.cnt_tmp.n != P.n_stats) P.cnt_tmp.alloc(P.n_stats);
  if (P.rctr.n != 4) P.rctr.alloc(4);
  if (P.rec_count.n != 1) P.rec_count.alloc(1);
  if (rec_cap > 0 && P.rec.n < (size_t)2 * rec_cap) P.rec.alloc((size_t)2 * rec_cap);
  HIPCHK(hipMemsetAsync(P.cnt_tmp.p, 0, (size_t)P.n_stats * sizeof(uint32_t), s));
  HIPCHK(hipMemsetAsync(P.rctr.p, 0, 4 * sizeof(unsigned long long), s));
  HIPCHK(hipMemsetAsync(P.rec_count.p, 0, sizeof(uint32_t), s));
  SppmBufs B = sppm_bufs(c);
  B.cnt = P.cnt_tmp.p; B.ctr = P.rctr.p; B.splat = nullptr;
  const SppmRec R{rec_cap > 0 ? P.rec.p : nullptr, P.rec_count.p, rec_cap, k, first, count};
  ev.a.record(s);
  k_sppm_photon<F, true><<<(count + 255u) / 256u, TRACE_BLOCK, c->lds_trace, s>>>(c->dscene.p, B, P.nth, sn, seed, pass, R);
  HIPCHK(hipGetLastError());
  ev.b.record(s);
  uint32_t nrec = 0;
  HIPCHK(hipMemcpyAsync(ctr, P.rctr.p, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&nrec, P.rec_count.p, sizeof nrec, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return nrec;
}

// film / splat: device images accumulated into (nullptr: not produced).  flags 0: k_film and the photons'
// float atomics; BLING_SPLAT_ORDERED: the reference's order, no float atomic (include/bling.h).
template <uint32_t F>
void sppm_pass_t(bling_ctx* c, uint32_t seed, uint32_t pass, float* film, float* splat, uint32_t flags, bling_sppm_stats* st) {
  SppmState& P = c->sppm;
  hipStream_t s = c->stream;
  const bool ordered = (flags & BLING_SPLAT_ORDERED) != 0u;
  const uint32_t sn = sppm_sn(c);
  const uint64_t nph = (uint64_t)P.nth * sn * sn;
  const size_t npix = (size_t)c->S.width * c->S.height;
  const Event e0, e1, e2, e3;
  e0.record(s);
  WaveState W{};
  W.result = P.result.p; W.img = P.img.p;
  const uint32_t nhp = sppm_eye_and_hash<F>(c, W, seed, pass, ordered, e1, [&] {
    if (!ordered) {                                                     // an unwanted film goes to the context's own
      k_film<<<P.n_tiles, 256, 0, s>>>(c->dscene.p, W, P.tiles.p, film ? film : P.film.p, nullptr, 0, 0);
    } else if (film) {
      const size_t nt = (size_t)P.n_tiles * FILM_TILE_MAX * FILM_TILE_MAX;
      if (P.timg.n != nt) P.timg.alloc(nt);
      k_sppm_film_ordered<<<P.n_tiles, 256, 0, s>>>(c->dscene.p, W, P.tiles.p, P.timg.p);
      k_sppm_film_add<<<(unsigned)((npix + 255) / 256), 256, 0, s>>>(c->dscene.p, P.tiles.p, P.n_tiles, P.timg.p, film);
    }
    HIPCHK(hipGetLastError());
  });
  e2.record(s);
  // photons (threads x sn^2, SPPM.hs:441-453, 474)
  HIPCHK(hipMemsetAsync(P.cnt.p, 0, (size_t)P.nth * P.n_stats * sizeof(uint32_t), s));
  unsigned long long sum[4] = {0, 0, 0, 0};
  std::vector<EventPair> launches, merges;
  if (!ordered) {
    SppmBufs B = sppm_bufs(c);
    if (splat) B.splat = splat;
    k_sppm_photon<F, false><<<(unsigned)((nph + 255) / 256), TRACE_BLOCK, c->lds_trace, s>>>(c->dscene.p, B, P.nth, sn, seed, pass,
                                                                                            SppmRec{});
    HIPCHK(hipGetLastError());
  } else {
    // Sampler k's image from zero: its photons over the ascending ranges of ordered_ranges.h, each merged
    // (splat_merge.h) before the next, then splat = splat + image_k.  A launch's counts, counters and records
    // live in its own buffers and are taken over only once the range fits, so nothing of a redone range counts
    // twice; the record capacity is carried from sampler to sampler.
    const uint32_t spp = sn * sn;
    const size_t budget = std::min<size_t>(splat_budget(c), 0x7FFFFFFFull);
    uint32_t cap = splat ? ordered_ranges::initial_cap(budget, P.rec.n / 2, spp) : 0u;
    if (splat && P.thread_img.n != 3 * npix) P.thread_img.alloc(3 * npix);
    for (uint32_t k = 0; k < P.nth; ++k) {
      if (splat) HIPCHK(hipMemsetAsync(P.thread_img.p, 0, 3 * npix * sizeof(float), s));
      unsigned long long ctr[4];
      ordered_ranges::run(
          spp, budget, cap,
          [&](uint32_t first, uint32_t count, uint32_t rec_cap) {
            launches.emplace_back();
            return sppm_launch_rec<F>(c, seed, pass, sn, k, first, count, rec_cap, ctr, launches.back());
          },
          [&](uint32_t, uint32_t, uint32_t got) {
            merges.emplace_back();
            merges.back().a.record(s);
            k_sppm_add_u32<<<(P.n_stats + 255) / 256, 256, 0, s>>>(P.cnt.p + (size_t)k * P.n_stats, P.cnt_tmp.p, P.n_stats);
            if (splat) splat_merge(c, P.rec.p, got, SM_LAYOUT_SPLAT, P.thread_img.p);
            merges.back().b.record(s);
            for (int q = 1; q < 4; ++q) sum[q] += ctr[q];
          },
          [&](uint32_t photon) { return "sppm: photon " + std::to_string(photon) + " of sampler " + std::to_string(k); });
      if (splat) {
        merges.emplace_back();
        merges.back().a.record(s);
        k_sppm_add_f32<<<(unsigned)((3 * npix + 255) / 256), 256, 0, s>>>(splat, P.thread_img.p, 3 * npix);
        merges.back().b.record(s);
      }
      HIPCHK(hipGetLastError());
    }
  }
  k_sppm_stats<<<(P.n_stats + 255) / 256, 256, 0, s>>>(sppm_bufs(c), P.nth, c->cfg.sppm_alpha);
  e3.record(s);
  unsigned long long ctr[4];
  HIPCHK(hipMemcpyAsync(ctr, P.ctr.p, sizeof ctr, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (ordered) {
    double mk = 0., mm = 0.;
    for (const EventPair& p : launches) mk += p.elapsed_ms();
    for (const EventPair& p : merges) mm += p.elapsed_ms();
    c->merge.ms_kernel = mk; c->merge.ms_merge = mm;
  }
  if (st) {
    const float a = elapsed_ms(e0, e1), b = elapsed_ms(e1, e2), t = elapsed_ms(e0, e3);
    st->hitpoints = std::min(nhp, P.hp_cap);
    st->photons = nph;
    st->cam_rays = ctr[0]; st->photon_rays = ctr[1] + sum[1]; st->photon_hits = ctr[2] + sum[2]; st->dropped = ctr[3] + sum[3];
    st->ms_eye = a; st->ms_hash = b; st->ms_photon = t - a - b; st->ms_total = t;
  }
}

template <uint32_t F>
uint32_t sppm_records_t(bling_ctx* c, uint32_t seed, uint32_t pass, uint32_t k, uint32_t first, uint32_t count, uint32_t rec_cap) {
  SppmState& P = c->sppm;
  const uint32_t sn = sppm_sn(c);
  const Event e1(false);
  WaveState W{};
  W.result = P.result.p; W.img = P.img.p;
  sppm_eye_and_hash<F>(c, W, seed, pass, true, e1, [] {});
  unsigned long long ctr[4];
  const EventPair ev;
  return sppm_launch_rec<F>(c, seed, pass, sn, k, first, count, rec_cap, ctr, ev);
}

template void sppm_pass_t<kProfiles[0]>(bling_ctx*, uint32_t, uint32_t, float*, float*, uint32_t, bling_sppm_stats*);
template void sppm_pass_t<kSppmAll>(bling_ctx*, uint32_t, uint32_t, float*, float*, uint32_t, bling_sppm_stats*);
template uint32_t sppm_records_t<kProfiles[0]>(bling_ctx*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t);
template uint32_t sppm_records_t<kSppmAll>(bling_ctx*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t);

}  // namespace bcore
