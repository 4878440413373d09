// splat_renderers.hip -- the entry points of the three renderers that splat light paths onto the image: SPPM
// (sppm.h, sppm_pass.hip), the light tracer (light_tracer.h, light_pass.hip) and Metropolis (mlt.h,
// mlt_pass.hip), on host and on device images, with their record, statistics and reset calls, and the ordered
// splat film's merge, budget and timing hooks (splat_merge.h).  Nothing of the wavefront pass driver (core.hip).
#include "core_internal.h"
#include "ordered_ranges.h"

using namespace bd;
using namespace bcore;

namespace {

// The kernels of these renderers exist for two feature sets: the cornell profile and everything SPPM serves.
// fn takes the set as a std::integral_constant, as with_profile's does.
template <class Fn>
auto with_splat_profile(uint32_t need, Fn&& fn) {
  if ((need & ~kProfiles[0]) == 0u) return fn(std::integral_constant<uint32_t, kProfiles[0]>{});
  return fn(std::integral_constant<uint32_t, kSppmAll>{});
}

void single_device(const bling_ctx* c, const char* who) {
  if (!c->peers.empty()) throw std::invalid_argument(std::string(who) + " on a single-device context");
}

void splat_device_args(uint32_t flags, const void* splat_device) {
  if (flags & ~BLING_SPLAT_ORDERED) throw std::invalid_argument("unknown splat flag bits " + std::to_string(flags & ~BLING_SPLAT_ORDERED));
  if (!splat_device) throw std::invalid_argument("null splat_device");
}

size_t film_floats(const bling_ctx* c) { return (size_t)c->S.width * c->S.height * 4; }
size_t splat_floats(const bling_ctx* c) { return (size_t)c->S.width * c->S.height * 3; }

// ---- SPPM (sppm.h, sppm_pass.hip)
void sppm_ready(const bling_ctx* c) {
  need_scene(c);
  if (c->cfg.renderer != BLING_RENDERER_SPPM) throw std::invalid_argument("the uploaded scene's renderer is not sppm");
  if (c->features & FT_PROCTEX)
    throw Refusal(BLING_EUNSUPPORTED, "sppm: blend / gradient / checker / cellNoise textures are not supported by the SPPM renderer");
}

void sppm_launch(bling_ctx* c, uint32_t seed, uint32_t pass, float* film, float* splat, uint32_t flags, bling_sppm_stats* st) {
  with_splat_profile(c->features, [&](auto prof) { sppm_pass_t<decltype(prof)::value>(c, seed, pass, film, splat, flags, st); });
}

// ---- light tracer (light_tracer.h, light_pass.hip)
void light_ready(const bling_ctx* c) {
  need_scene(c);
  if (c->cfg.renderer != BLING_RENDERER_LIGHT) throw std::invalid_argument("the uploaded scene's renderer is not the light tracer");
  single_device(c, "the light tracer runs");
  if (c->S.camera.kind != BLING_CAM_PERSPECTIVE)
    throw Refusal(BLING_EUNSUPPORTED, "light tracer: an environment camera cannot be sampled (sampleCam, Camera.hs:102)");
  if (c->features & FT_PROCTEX)
    throw Refusal(BLING_EUNSUPPORTED, "light tracer: blend / gradient / checker / cellNoise textures are not supported by the light tracer");
}

uint32_t light_launch(bling_ctx* c, uint32_t seed, uint32_t pass, uint32_t first, uint32_t count, float* splat, uint32_t rec_cap,
                      bling_light_stats* st) {
  return with_splat_profile(c->features, [&](auto prof) {
    return light_pass_t<decltype(prof)::value>(c, seed, pass, first, count, splat, rec_cap, st);
  });
}

// The ordered light tracer pass: k_lt_photon in record mode over the ascending photon ranges of
// ordered_ranges.h, each merged (splat_merge.h) before the next.  A launch that is run again is timed like
// any other.  Every launch returns with the stream synchronised, so nothing runs when a photon is refused.
void light_pass_ordered(bling_ctx* c, uint32_t seed, uint32_t pass, float* img, bling_light_stats* st) {
  const uint32_t total = (uint32_t)c->lt.pass_photons;
  const size_t budget = std::min<size_t>(splat_budget(c), 0x7FFFFFFFull);
  uint32_t cap = ordered_ranges::initial_cap(budget, c->light.rec.n / 2, total);
  bling_light_stats sum{}, one{};
  std::vector<EventPair> merges;
  double ms_kernel = 0.;
  ordered_ranges::run(
      total, budget, cap,
      [&](uint32_t first, uint32_t count, uint32_t rec_cap) {
        one = bling_light_stats{};
        const uint32_t got = light_launch(c, seed, pass, first, count, nullptr, rec_cap, &one);
        ms_kernel += one.ms_total;
        return got;
      },
      [&](uint32_t, uint32_t, uint32_t got) {
        merges.emplace_back();
        merges.back().a.record(c->stream);
        splat_merge(c, c->light.rec.p, got, SM_LAYOUT_LIGHT, img);
        merges.back().b.record(c->stream);
        sum.photon_rays += one.photon_rays; sum.shadow_rays += one.shadow_rays; sum.splats += one.splats; sum.dropped += one.dropped;
      },
      [](uint32_t photon) { return "light tracer: photon " + std::to_string(photon); });
  HIPCHK(hipStreamSynchronize(c->stream));
  double ms_merge = 0.;
  for (const EventPair& p : merges) ms_merge += p.elapsed_ms();
  c->merge.ms_kernel = ms_kernel; c->merge.ms_merge = ms_merge;
  if (st) {
    *st = sum;
    st->photons = total;
    st->ms_total = ms_kernel + ms_merge;
  }
}

// ---- Metropolis renderer (mlt.h, mlt_pass.hip)
void mlt_ready(const bling_ctx* c) {
  need_scene(c);
  if (c->cfg.renderer != BLING_RENDERER_METROPOLIS) throw std::invalid_argument("the uploaded scene's renderer is not metropolis");
  single_device(c, "the Metropolis renderer runs");
}

}  // namespace

extern "C" {

int bling_sppm_pass(bling_ctx* c, uint32_t seed, uint32_t pass_index, float* film_out, float* splat_out,
                    bling_sppm_stats* st) {
  return guarded([&] {
    if (!c) throw std::invalid_argument("null argument");
    sppm_ready(c);
    HIPCHK(hipSetDevice(c->device));
    if (!c->sppm.ready) sppm_init(c);
    SppmState& P = c->sppm;
    stage_in(P.film, film_out, film_floats(c));
    stage_in(P.splat, splat_out, splat_floats(c));
    if (st) std::memset(st, 0, sizeof *st);
    sppm_launch(c, seed, pass_index, P.film.p, P.splat.p, 0u, st);
    stage_out(film_out, P.film, film_floats(c));
    stage_out(splat_out, P.splat, splat_floats(c));
    return BLING_OK;
  });
}

int bling_sppm_pass_device(bling_ctx* c, uint32_t seed, uint32_t pass_index, uint32_t flags, void* film_device, void* splat_device,
                           bling_sppm_stats* st) {
  return guarded([&] {
    if (!c) throw std::invalid_argument("null argument");
    if (flags & ~BLING_SPLAT_ORDERED) throw std::invalid_argument("unknown splat flag bits " + std::to_string(flags & ~BLING_SPLAT_ORDERED));
    sppm_ready(c);
    single_device(c, "bling_sppm_pass_device runs");
    HIPCHK(hipSetDevice(c->device));
    if (!c->sppm.ready) sppm_init(c);
    if (st) std::memset(st, 0, sizeof *st);
    sppm_launch(c, seed, pass_index, static_cast<float*>(film_device), static_cast<float*>(splat_device), flags, st);
    return BLING_OK;
  });
}

int bling_debug_sppm_records(bling_ctx* c, uint32_t seed, uint32_t pass_index, uint32_t thread, uint32_t first_photon,
                             uint32_t n_photons, bling_sppm_record* records, size_t cap, size_t* n) {
  return guarded([&] {
    if (!c || !n || (cap && !records)) throw std::invalid_argument("null argument");
    *n = 0;
    sppm_ready(c);
    single_device(c, "bling_debug_sppm_records runs");
    const uint32_t sn = sppm_sn(c);
    if (thread >= (uint32_t)std::max(1, c->cfg.sppm_threads)) throw std::invalid_argument("sampler beyond sppm_threads");
    if ((uint64_t)first_photon + n_photons > (uint64_t)sn * sn) throw std::invalid_argument("photon range beyond the sampler's sn^2");
    if (cap > 0x7FFFFFFFull) throw std::invalid_argument("record capacity too large");
    if (n_photons == 0) return BLING_OK;
    HIPCHK(hipSetDevice(c->device));
    if (!c->sppm.ready) sppm_init(c);
    // a launch needs a buffer to claim slots in: one record at least, so the count is always known
    const uint32_t rcap = (uint32_t)std::max<size_t>(cap, 1);
    const uint32_t got = with_splat_profile(c->features, [&](auto prof) {
      return sppm_records_t<decltype(prof)::value>(c, seed, pass_index, thread, first_photon, n_photons, rcap);
    });
    *n = got;
    if (got > cap) throw std::invalid_argument("sppm records: " + std::to_string(got) + " records exceed the capacity " + std::to_string(cap));
    std::vector<uint4> raw((size_t)2 * got);
    if (got) HIPCHK(hipMemcpy(raw.data(), c->sppm.rec.p, raw.size() * sizeof(uint4), hipMemcpyDeviceToHost));
    const uint32_t W = (uint32_t)c->S.width;
    for (uint32_t i = 0; i < got; ++i) {
      const uint4 a = raw[2 * (size_t)i], b = raw[2 * (size_t)i + 1];
      bling_sppm_record& r = records[i];
      r.thread = thread; r.photon = a.w; r.seq = a.z; r.depth = a.y;
      r.sx = (int32_t)(a.x % W); r.sy = (int32_t)(a.x / W);
      std::memcpy(&r.x, &b.x, 3 * sizeof(float));
      r.pad = 0u;
    }
    std::sort(records, records + got, [](const bling_sppm_record& p, const bling_sppm_record& q) {
      return p.photon != q.photon ? p.photon < q.photon : p.seq < q.seq;
    });
    return BLING_OK;
  });
}

int bling_sppm_pixel_stats(bling_ctx* c, float* r2_out, float* n_out, size_t* n_pixels) {
  return guarded([&] {
    if (!c) throw std::invalid_argument("null argument");
    sppm_ready(c);
    HIPCHK(hipSetDevice(c->device));
    if (!c->sppm.ready) sppm_init(c);
    SppmState& P = c->sppm;
    if (n_pixels) *n_pixels = P.n_stats;
    if (r2_out) HIPCHK(hipMemcpy(r2_out, P.r2.p, P.n_stats * sizeof(float), hipMemcpyDeviceToHost));
    if (n_out) HIPCHK(hipMemcpy(n_out, P.nacc.p, P.n_stats * sizeof(float), hipMemcpyDeviceToHost));
    return BLING_OK;
  });
}

int bling_debug_sppm_hitpoints(bling_ctx* c, float* pos_r2, uint64_t* keys, size_t cap, size_t* n) {
  return guarded([&] {
    if (!c) throw std::invalid_argument("null argument");
    if (!c->sppm.ready) throw std::invalid_argument("no SPPM pass has run");
    HIPCHK(hipSetDevice(c->device));
    SppmState& P = c->sppm;
    uint32_t cnt = 0;
    HIPCHK(hipMemcpy(&cnt, P.hp_count.p, sizeof cnt, hipMemcpyDeviceToHost));
    const size_t m = std::min<size_t>(cnt, P.hp_cap);
    if (n) *n = m;
    const size_t k = std::min(m, cap);
    if (pos_r2 && k) HIPCHK(hipMemcpy(pos_r2, P.hp_pos.p, k * sizeof(float4), hipMemcpyDeviceToHost));
    if (keys && k) HIPCHK(hipMemcpy(keys, P.hp_key.p, k * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return BLING_OK;
  });
}

int bling_debug_sppm_buckets(bling_ctx* c, uint32_t* bstart, uint32_t* items, float* mr, size_t cap_b, size_t cap_i,
                             size_t* nb, size_t* ni) {
  return guarded([&] {
    if (!c) throw std::invalid_argument("null argument");
    if (!c->sppm.ready) throw std::invalid_argument("no SPPM pass has run");
    HIPCHK(hipSetDevice(c->device));
    SppmState& P = c->sppm;
    SppmGrid g;
    HIPCHK(hipMemcpy(&g, P.grid.p, sizeof g, hipMemcpyDeviceToHost));
    if (nb) *nb = (size_t)g.cnt + 1;
    if (ni) *ni = g.items;
    if (bstart && cap_b >= (size_t)g.cnt + 1) HIPCHK(hipMemcpy(bstart, P.bstart.p, ((size_t)g.cnt + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (items && cap_i >= g.items && g.items) HIPCHK(hipMemcpy(items, P.items.p, (size_t)g.items * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (mr && cap_i >= g.items && g.items) HIPCHK(hipMemcpy(mr, P.kd_mr.p, (size_t)g.items * sizeof(float), hipMemcpyDeviceToHost));
    return BLING_OK;
  });
}

int bling_sppm_reset(bling_ctx* c) {
  return guarded([&] {
    if (!c) throw std::invalid_argument("null argument");
    HIPCHK(hipSetDevice(c->device));
    c->sppm.free_all();
    return BLING_OK;
  });
}

int bling_light_pass(bling_ctx* c, uint32_t seed, uint32_t pass_index, float* splat_inout, bling_light_stats* st) {
  return guarded([&] {
    if (!c) throw std::invalid_argument("null argument");
    light_ready(c);
    HIPCHK(hipSetDevice(c->device));
    LightState& P = c->light;
    stage_in(P.splat, splat_inout, splat_floats(c));
    if (st) std::memset(st, 0, sizeof *st);
    light_launch(c, seed, pass_index, 0u, (uint32_t)c->lt.pass_photons, P.splat.p, 0u, st);
    stage_out(splat_inout, P.splat, splat_floats(c));
    return BLING_OK;
  });
}

int bling_light_pass_device(bling_ctx* c, uint32_t seed, uint32_t pass_index, uint32_t flags, void* splat_device,
                            bling_light_stats* st) {
  return guarded([&] {
    if (!c) throw std::invalid_argument("null argument");
    splat_device_args(flags, splat_device);
    light_ready(c);
    HIPCHK(hipSetDevice(c->device));
    if (st) std::memset(st, 0, sizeof *st);
    float* img = static_cast<float*>(splat_device);
    if (flags & BLING_SPLAT_ORDERED) light_pass_ordered(c, seed, pass_index, img, st);
    else light_launch(c, seed, pass_index, 0u, (uint32_t)c->lt.pass_photons, img, 0u, st);
    return BLING_OK;
  });
}

int bling_debug_light_records(bling_ctx* c, uint32_t seed, uint32_t pass_index, uint32_t first_photon, uint32_t n_photons,
                              bling_light_record* records, size_t cap, size_t* n) {
  return guarded([&] {
    if (!c || !n || (cap && !records)) throw std::invalid_argument("null argument");
    *n = 0;
    light_ready(c);
    if ((uint64_t)first_photon + n_photons > (uint64_t)c->lt.pass_photons) throw std::invalid_argument("photon range beyond passPhotons");
    if (cap > 0x7FFFFFFFull) throw std::invalid_argument("record capacity too large");
    if (n_photons == 0) return BLING_OK;
    HIPCHK(hipSetDevice(c->device));
    // a launch needs a buffer to claim slots in: one record at least, so the count is always known
    const uint32_t rcap = (uint32_t)std::max<size_t>(cap, 1);
    const uint32_t got = light_launch(c, seed, pass_index, first_photon, n_photons, nullptr, rcap, nullptr);
    *n = got;
    if (got > cap) throw std::invalid_argument("light records: " + std::to_string(got) + " records exceed the capacity " + std::to_string(cap));
    static_assert(sizeof(bling_light_record) == 2 * sizeof(uint4), "record layout");
    if (got) HIPCHK(hipMemcpy(records, c->light.rec.p, (size_t)got * sizeof(bling_light_record), hipMemcpyDeviceToHost));
    std::sort(records, records + got, [](const bling_light_record& a, const bling_light_record& b) {
      return a.photon != b.photon ? a.photon < b.photon : a.depth < b.depth;
    });
    return BLING_OK;
  });
}

int bling_mlt_pass(bling_ctx* c, uint32_t seed, uint32_t pass_index, float* splat_inout, bling_mlt_stats* st) {
  return guarded([&] {
    if (!c) throw std::invalid_argument("null argument");
    mlt_ready(c);
    HIPCHK(hipSetDevice(c->device));
    LightState& P = c->light;
    stage_in(P.splat, splat_inout, splat_floats(c));
    if (st) std::memset(st, 0, sizeof *st);
    mlt_pass_run(c, seed, pass_index, P.splat.p, false, 0u, 0u, st, nullptr);
    stage_out(splat_inout, P.splat, splat_floats(c));
    return BLING_OK;
  });
}

int bling_mlt_pass_device(bling_ctx* c, uint32_t seed, uint32_t pass_index, uint32_t flags, void* splat_device,
                          bling_mlt_stats* st) {
  return guarded([&] {
    if (!c) throw std::invalid_argument("null argument");
    splat_device_args(flags, splat_device);
    mlt_ready(c);
    HIPCHK(hipSetDevice(c->device));
    if (st) std::memset(st, 0, sizeof *st);
    mlt_pass_run(c, seed, pass_index, static_cast<float*>(splat_device), (flags & BLING_SPLAT_ORDERED) != 0u, 0u, 0u, st, nullptr);
    return BLING_OK;
  });
}

int bling_debug_mlt_records(bling_ctx* c, uint32_t seed, uint32_t pass_index, uint32_t first_chain, uint32_t n_chains,
                            bling_mlt_record* records, size_t cap, size_t* n, uint32_t* starts, float* b) {
  return guarded([&] {
    if (!c || !n || (cap && !records)) throw std::invalid_argument("null argument");
    *n = 0;
    mlt_ready(c);
    const uint64_t C = (uint64_t)c->mp.chains;
    if ((uint64_t)first_chain + n_chains > C) throw std::invalid_argument("chain range beyond chains");
    if (n_chains == 0) return BLING_OK;
    const uint64_t M = (uint64_t)mlt_mutations(c->mp, c->S.width, c->S.height);
    uint64_t need = 0;
    for (uint64_t k = first_chain; k < (uint64_t)first_chain + n_chains; ++k) need += M / C + (k < M % C ? 1 : 0);
    *n = (size_t)need;
    if (need > cap) throw std::invalid_argument("mlt records: " + std::to_string(need) + " records exceed the capacity " + std::to_string(cap));
    HIPCHK(hipSetDevice(c->device));
    MltOut out;
    mlt_pass_run(c, seed, pass_index, nullptr, false, first_chain, n_chains, nullptr, &out);
    if (out.rec.size() != need) throw std::runtime_error("mlt records: count mismatch");
    if (need) std::memcpy(records, out.rec.data(), need * sizeof(bling_mlt_record));
    if (starts) std::memcpy(starts, out.start.data() + first_chain, (size_t)n_chains * sizeof(uint32_t));
    if (b) *b = out.b;
    return BLING_OK;
  });
}

int bling_debug_mlt_boot(const float* I, uint32_t n, uint32_t seed, uint32_t pass_index, uint32_t chains, float* b,
                         uint32_t* starts) {
  return guarded([&] {
    if (!I || !b || !starts || n < 1 || chains < 1) throw std::invalid_argument("null argument");
    *b = mlt_boot_select(I, n, seed, pass_index, chains, starts);
    return BLING_OK;
  });
}

int bling_debug_mlt_set_boot(bling_ctx* c, const float* I, uint32_t n) {
  return guarded([&] {
    if (!c || (n && !I)) throw std::invalid_argument("null argument");
    c->mlt_boot_override.assign(I, I + n);
    return BLING_OK;
  });
}

// ---- ordered splat films and caller-owned device splat images (splat_merge.h)
int bling_debug_splat_merge(bling_ctx* c, const bling_splat_rec* recs, size_t n, void* splat_device) {
  return guarded([&] {
    if (!c || !splat_device || (n && !recs)) throw std::invalid_argument("null argument");
    need_scene(c);
    if (n > 0x7FFFFFFFull) throw std::invalid_argument("splat merge: more than 2^31 - 1 records");
    const size_t npix = (size_t)c->S.width * c->S.height;
    for (size_t i = 0; i < n; ++i)
      if (recs[i].pixel >= npix) throw std::invalid_argument("splat merge: record " + std::to_string(i) + " names pixel " +
                                                             std::to_string(recs[i].pixel) + " of " + std::to_string(npix));
    if (n == 0) return BLING_OK;
    HIPCHK(hipSetDevice(c->device));
    static_assert(sizeof(bling_splat_rec) == 2 * sizeof(uint4), "record layout");
    MergeState& G = c->merge;
    if (G.rec.n < 2 * n) G.rec.alloc(2 * n);
    HIPCHK(hipMemcpyAsync(G.rec.p, recs, n * sizeof(bling_splat_rec), hipMemcpyHostToDevice, c->stream));
    splat_merge(c, G.rec.p, n, SM_LAYOUT_SPLAT, static_cast<float*>(splat_device));
    HIPCHK(hipStreamSynchronize(c->stream));
    return BLING_OK;
  });
}

int bling_debug_set_splat_budget(bling_ctx* c, size_t max_records) {
  return guarded([&] {
    if (!c) throw std::invalid_argument("null argument");
    c->merge.budget = max_records;
    return BLING_OK;
  });
}

int bling_debug_splat_times(bling_ctx* c, double* ms_kernel, double* ms_merge) {
  return guarded([&] {
    if (!c || !ms_kernel || !ms_merge) throw std::invalid_argument("null argument");
    *ms_kernel = c->merge.ms_kernel; *ms_merge = c->merge.ms_merge;
    return BLING_OK;
  });
}

}  // extern "C"
