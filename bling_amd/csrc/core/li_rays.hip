// li_rays.hip -- the integrator seam (include/bling.h, "the integrator seam"): surfaceLi of the uploaded
// scene's integrator along rays the caller made, device buffers in, 16-band spectra out in the layout
// bling_image_add_*_device takes.  Per chunk of at most the context's path capacity:
//   k_reset_queues   the wave's queue counters (wavefront.h)
//   k_li_intake      validation, the sample key's ids and the path records of the chunk's rays (li_rays.h)
//   run_wave_prof / normals_wave   the wave pipeline of bling_render_pass and bling_sample_li, unchanged
//   k_li_store       the wave's spectra to the caller's rows
// all on the context's stream.  The counters of the waves add up on the device and are read once.
#include "core_internal.h"
#include "li_rays.h"

namespace bcore {
namespace {

// rays per wave when the context holds no larger path capacity yet (4 Mi paths: at most 3 GiB of path state)
constexpr size_t kLiDefaultChunk = (size_t)1 << 22;

bool li_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + nb && pb < pa + na;
}

// everything the two entry points refuse, in the order include/bling.h lists it
void li_ready(bling_ctx* c) {
  if (!c) throw std::invalid_argument("null argument");
  need_scene(c);
  if (c->cfg.renderer != BLING_RENDERER_SAMPLER_PATH)
    throw std::invalid_argument("surface_li: the uploaded scene's renderer is not the sampler renderer");
  if (c->S.integrator == BLING_INTEGRATOR_BIDIR)
    throw Refusal(BLING_EUNSUPPORTED, "surface_li: the bidirectional integrator makes its camera ray inside its walk");
}

int li_wave(bling_ctx* c, const WaveState& W, uint32_t n, uint32_t seed, uint32_t pass) {
  if (c->S.integrator == BLING_INTEGRATOR_NORMALS) return normals_wave(c, W, n, nullptr);
  int launches = 0;
  with_profile(c->features, [&](auto prof) { launches = run_wave_prof<decltype(prof)::value>(c, W, n, seed, pass, false, nullptr); });
  return launches;
}

// n > 0 rays on device buffers, wave after wave; returns after completion
void li_run(bling_ctx* c, uint32_t seed, uint32_t pass, const float* rays, const uint32_t* ids, size_t n, float* L,
            bling_li_stats* st) {
  HIPCHK(hipSetDevice(c->device));
  LiState& I = c->li;
  const size_t cap = std::min(I.chunk ? I.chunk : std::max<size_t>(c->cap, kLiDefaultChunk), (size_t)1 << 31);
  const size_t waves = (n + cap - 1) / cap;
  const size_t chunk = (n + waves - 1) / waves;      // equal waves of at most cap rays, not full ones and a remainder
  c->ensure_paths((uint32_t)chunk);
  if (I.lfull.n < (size_t)4 * c->cap) I.lfull.alloc((size_t)4 * c->cap);
  if (I.drop.n < c->cap) I.drop.alloc(c->cap);
  if (!I.ctr.n) I.ctr.alloc(1);
  WaveState P = c->state();
  P.Lfull = I.lfull.p;
  const hipStream_t s = c->stream;
  const bool aligned = ((uintptr_t)L & 15u) == 0;
  HIPCHK(hipMemsetAsync(c->counters.p, 0, sizeof(Counters), s));
  HIPCHK(hipMemsetAsync(I.ctr.p, 0, sizeof(unsigned long long), s));
  const EventPair ev;
  ev.a.record(s);
  for (size_t off = 0; off < n; off += chunk) {
    const uint32_t m = (uint32_t)std::min(chunk, n - off);
    LiChunk in;
    for (int p = 0; p < 7; ++p) in.plane[p] = rays + (size_t)p * n + off;
    in.ids = ids + 2 * off;
    k_reset_queues<<<1, 64, 0, s>>>(P.qcount, m);
    k_li_intake<<<(m + 255u) / 256u, 256, 0, s>>>(c->dscene.p, P, in, m, I.drop.p, I.ctr.p);
    li_wave(c, P, m, seed, pass);
    const unsigned blocks = (unsigned)(((size_t)4 * m + 255) / 256);
    if (aligned) k_li_store<true><<<blocks, 256, 0, s>>>(I.lfull.p, I.drop.p, m, L + 16 * off);
    else k_li_store<false><<<blocks, 256, 0, s>>>(I.lfull.p, I.drop.p, m, L + 16 * off);
    HIPCHK(hipGetLastError());
  }
  ev.b.record(s);
  Counters hc;
  unsigned long long dropped = 0;
  HIPCHK(hipMemcpyAsync(&hc, c->counters.p, sizeof hc, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&dropped, I.ctr.p, sizeof dropped, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (!st) return;
  bling_li_stats out{};
  out.rays = n;
  out.dropped = dropped;
  out.rays_continuation = hc.cont; out.rays_mis = hc.mis; out.rays_shadow = hc.shadow;
  // a dropped ray's stand-in enters the first launch of the path pipelines and ends there: it is no vertex
  // (the normal-map integrator counts hits only)
  out.path_vertices = c->S.integrator == BLING_INTEGRATOR_NORMALS ? hc.vertices : hc.vertices - dropped;
  out.waves = waves;
  out.ms_total = ev.elapsed_ms();
  *st = out;
}

void li_zero_stats(bling_li_stats* st) { if (st) *st = bling_li_stats{}; }

}  // namespace
}  // namespace bcore

extern "C" {

int bling_surface_li_device(bling_ctx* c, uint32_t seed, uint32_t pass_index, const void* rays_soa_dev, const void* ids_dev,
                            size_t n, void* L_dev, bling_li_stats* st) {
  return guarded([&] {
    li_ready(c);
    li_zero_stats(st);
    if (n == 0) return BLING_OK;
    if (!rays_soa_dev || !ids_dev || !L_dev) throw std::invalid_argument("null argument");
    if (n > ((size_t)1 << 40)) throw std::invalid_argument("surface_li: more than 2^40 rays");
    if ((((uintptr_t)rays_soa_dev | (uintptr_t)ids_dev | (uintptr_t)L_dev) & 3u) != 0)
      throw std::invalid_argument("surface_li: a buffer is not aligned to 4 bytes");
    if (li_overlap(L_dev, n * 64, rays_soa_dev, n * 28) || li_overlap(L_dev, n * 64, ids_dev, n * 8))
      throw std::invalid_argument("surface_li: L overlaps an input");
    li_run(c, seed, pass_index, static_cast<const float*>(rays_soa_dev), static_cast<const uint32_t*>(ids_dev), n,
           static_cast<float*>(L_dev), st);
    return BLING_OK;
  });
}

int bling_surface_li(bling_ctx* c, uint32_t seed, uint32_t pass_index, const float* rays_soa, const uint32_t* ids, size_t n,
                     float* L_out, bling_li_stats* st) {
  return guarded([&] {
    li_ready(c);
    li_zero_stats(st);
    if (n == 0) return BLING_OK;
    if (!rays_soa || !ids || !L_out) throw std::invalid_argument("null argument");
    if (n > ((size_t)1 << 40)) throw std::invalid_argument("surface_li: more than 2^40 rays");
    if (li_overlap(L_out, n * 64, rays_soa, n * 28) || li_overlap(L_out, n * 64, ids, n * 8))
      throw std::invalid_argument("surface_li: L overlaps an input");
    HIPCHK(hipSetDevice(c->device));
    LiState& I = c->li;
    if (I.rays.n < 7 * n) I.rays.alloc(7 * n);
    if (I.ids.n < 2 * n) I.ids.alloc(2 * n);
    if (I.L.n < 16 * n) I.L.alloc(16 * n);
    // the staged planes keep the caller's stride n, whatever the buffer's capacity
    HIPCHK(hipMemcpy(I.rays.p, rays_soa, 7 * n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(I.ids.p, ids, 2 * n * sizeof(uint32_t), hipMemcpyHostToDevice));
    li_run(c, seed, pass_index, I.rays.p, I.ids.p, n, I.L.p, st);
    HIPCHK(hipMemcpy(L_out, I.L.p, 16 * n * sizeof(float), hipMemcpyDeviceToHost));
    return BLING_OK;
  });
}

int bling_debug_set_li_chunk(bling_ctx* c, size_t max_rays) {
  return guarded([&] {
    if (!c) throw std::invalid_argument("null argument");
    if (max_rays > ((size_t)1 << 31)) throw std::invalid_argument("surface_li: a chunk beyond 2^31 rays");
    c->li.chunk = max_rays;
    return BLING_OK;
  });
}

}  // extern "C"
