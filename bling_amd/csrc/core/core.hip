// core.hip -- the MI355X path-tracing core behind include/bling.h.
//
// One render pass (Rendering.hs:127-140) runs as a wavefront of paths in HBM, chunked by tiles:
//   k_raygen          camera samples of the chunk's 16x16 tiles (Sampling.hs:112-132, Camera.hs:49-76)
//   per path vertex   k_trace_closest -> k_trace_any -> k_resolve -> k_shade over compacted queues
//                     (wavefront.h; Integrator/Path.hs:41-87, Scene.hs:61-118)
//   k_film            per-tile filtered splat into LDS + merge into the film (Image.hs:108-299)
// Path state is SoA (one 64-B record per spectrum) indexed through compacted queues.  Traversal
// uses the LDS stack of dev_trace.h.
// This unit holds the pass driver, the film, tile and develop calls, bling_render and the debug and trace
// calls.  What a scene becomes before a pass is planned on the host in scene_plan.cpp and put on the devices
// by scene_upload.hip; the SPPM, light tracer and Metropolis entries are in splat_renderers.hip.
#include "core_internal.h"
#include "pass_plan.h"
#include "pass_stats.h"

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <thread>

using namespace bd;
using namespace bcore;

namespace {

thread_local std::string g_err;

// A pass whose paths fit one wave runs as two half-waves on two streams (core_wave.h run_wave_pair_t)
// where that measured faster: the cornell profile; BLING_PASS_NO_PIPELINE and
// bling_debug_set_pipeline override.  Legal for the Path integrator of a product build, and only
// while the traversal keeps its stack in LDS: the BVH4 overflow rows are indexed by a grid's thread
// id, so two traversal launches in flight would share them.
bool pipeline_wanted(const bling_ctx* c, const bling_pass_params* p) {
  if (BLING_DEBUG_VERTEX || BLING_STREAM_STATS) return false;
  if (p->flags & BLING_PASS_NO_PIPELINE) return false;
  if (c->S.integrator != BLING_INTEGRATOR_PATH) return false;
  if (c->S.stack4_need > c->S.stack4_lds) return false;
  if (c->pipeline_mode >= 0) return c->pipeline_mode != 0;
  return profile_of(c->features) == kProfiles[0];
}

int run_wave_pair(bling_ctx* c, const HalfWave* h, uint32_t seed, uint32_t pass, bool stats, WaveTiming* tm) {
  int launches = 0;
  with_profile(c->features, [&](auto prof) {
    launches = run_wave_pair_prof<decltype(prof)::value>(c, h, seed, pass, stats, tm);
  });
  return launches;
}

int run_wave(bling_ctx* c, const WaveState& W, uint32_t n, uint32_t seed, uint32_t pass, bool stats,
             WaveTiming* tm = nullptr) {
  int launches = 0;
  with_profile(c->features, [&](auto prof) {
    launches = run_wave_prof<decltype(prof)::value>(c, W, n, seed, pass, stats, tm);
  });
  return launches;
}

void launch_trace(bling_ctx* c, const float* rays, uint32_t n, int any_hit, float* t, uint32_t* prim, float* bary) {
  with_profile(c->features, [&](auto prof) { launch_trace_prof<decltype(prof)::value>(c, rays, n, any_hit, t, prim, bary); });
}

// The tile-image slot of a filter (BLING_PASS_TILE_IMAGES): the largest mkImageTile image
// (Image.hs:108-120), w = x1 - max(0, x0) + floor(0.5 + fw) <= 15 + floor(0.5 + fw).
void tile_slot(const DevScene& S, int* sw, int* sh) {
  *sw = 15 + (int)std::floor(0.5f + S.filter_w);
  *sh = 15 + (int)std::floor(0.5f + S.filter_h);
}

// splitWindow over the sample extent (Sampling.hs:55-58), filtered by the stride (a sub-sample of
// the pass) and dealt round-robin to the shard
std::vector<TileDesc> pass_tiles(const DevScene& S, int rank, int world, int stride) {
  world = std::max(1, world); stride = std::max(1, stride);
  if (rank < 0 || rank >= world) throw std::invalid_argument("shard rank outside [0, world)");
  const uint32_t spp = (uint32_t)S.spp;
  std::vector<TileDesc> tiles;
  int k = 0;
  for (int y = S.ey0; y <= S.ey1; y += 16)
    for (int x = S.ex0; x <= S.ex1; x += 16, ++k) {
      if (k % stride != 0 || (k / stride) % world != rank) continue;
      TileDesc t{x, std::min(x + 15, S.ex1), y, std::min(y + 15, S.ey1), 0, 0};
      t.count = (uint32_t)((t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1)) * spp;
      tiles.push_back(t);
    }
  return tiles;
}

// Film splat of a chunk's tiles: the register-window kernel for the filter widths the configs use,
// the per-sample LDS-atomic kernel otherwise.  timg != NULL: the chunk's tile images into their slots.
// td: the chunk's tile table on the device (n_tiles entries).
// ordered (BLING_PASS_ORDERED_FILM): the tile images in the reference's order, without atomics, always
// into their slots (k_film_ordered: the window kernel for the square K = 3, 5, 7, else the generic one).
void launch_film(bling_ctx* c, const WaveState& P, const TileDesc* td, unsigned n_tiles, float* film_dev, float* timg,
                 bool ordered = false) {
  const float fw = c->S.filter_w, fh = c->S.filter_h;
  const int kx = 2 * (int)std::floor(0.5f + fw) + 1, ky = 2 * (int)std::floor(0.5f + fh) + 1;
  int sw, sh;
  tile_slot(c->S, &sw, &sh);
  hipStream_t s = c->stream;
  if (ordered) {
    if (!timg) throw std::logic_error("ordered film without tile images");
    if (kx == ky && kx == 3) k_film_ordered<3><<<n_tiles, 256, 0, s>>>(c->dscene.p, P, td, timg, sw, sh);
    else if (kx == ky && kx == 5) k_film_ordered<5><<<n_tiles, 256, 0, s>>>(c->dscene.p, P, td, timg, sw, sh);
    else if (kx == ky && kx == 7) k_film_ordered<7><<<n_tiles, 256, 0, s>>>(c->dscene.p, P, td, timg, sw, sh);
    else k_film_ordered<0><<<n_tiles, 256, 0, s>>>(c->dscene.p, P, td, timg, sw, sh);
    return;
  }
  if (kx == 5 && ky == 5)
    k_film_gather<5><<<n_tiles, 256 * film_split<5>(), 0, s>>>(c->dscene.p, P, td, film_dev, timg, sw, sh);
  else if (kx == 7 && ky == 7)
    k_film_gather<7><<<n_tiles, 256 * film_split<7>(), 0, s>>>(c->dscene.p, P, td, film_dev, timg, sw, sh);
  else
    k_film<<<n_tiles, 256, 0, s>>>(c->dscene.p, P, td, film_dev, timg, sw, sh);
}

// addTile in tile order (k_film_add_ordered) of the tile images of p's stride into a device film: one
// rank's (rank >= 0, from `one`) or every rank's of p's world (rank < 0, ranks_dev: the buffers' device
// pointers on the device)
void add_tiles_ordered(bling_ctx* c, const bling_pass_params* p, int rank, const float* one, const float4* const* ranks_dev,
                       float* film_dev) {
  int sw, sh;
  tile_slot(c->S, &sw, &sh);
  const FilmOrderedSrc src{reinterpret_cast<const float4*>(one), ranks_dev, rank, std::max(1, p->shard_world), std::max(1, p->tile_stride)};
  const size_t npix = (size_t)c->S.width * c->S.height;
  k_film_add_ordered<<<(unsigned)((npix + 255) / 256), 256, 0, c->stream>>>(c->dscene.p, src, film_dev, sw, sh);
  HIPCHK(hipGetLastError());
}

// BLING_PASS_ORDERED_FILM is served on single-device contexts
void check_ordered(const bling_ctx* c, const bling_pass_params* p) {
  if ((p->flags & BLING_PASS_ORDERED_FILM) && !c->peers.empty())
    throw std::invalid_argument("BLING_PASS_ORDERED_FILM on a multi-device context");
}

struct PassPlan {                 // what render() settles before its first launch
  std::vector<TileDesc> tiles;
  std::vector<uint32_t> counts;   // the tiles' samples, for pass_plan.h
  uint64_t total = 0;             // the pass's paths
  uint32_t chunk = 0;             // paths per wave
  bool pipe = false;              // one wave, at least two tiles: two half-waves cut at a tile boundary, in flight together
  float* timg = nullptr;          // BLING_PASS_TILE_IMAGES: the tile images, slot_floats per tile
  size_t slot_floats = 0;
  bool ordered = false;           // BLING_PASS_ORDERED_FILM: the film kernels write ordered tile images
  bool add_film = false;          // ... into the context's own buffer (timg), added into the film after the last wave
  float* timg_at(size_t tile) const { return timg ? timg + tile * slot_floats : nullptr; }
};

// Checks the pass's parameters, sizes its waves (pass_plan.h wave_chunk) and allocates their path state.
PassPlan plan_pass(bling_ctx* c, const bling_pass_params* p) {
  PassPlan pl;
  pl.tiles = pass_tiles(c->S, p->shard_rank, p->shard_world, p->tile_stride);
  pl.timg = (p->flags & BLING_PASS_TILE_IMAGES) ? static_cast<float*>(p->tiles_device) : nullptr;
  if ((p->flags & BLING_PASS_TILE_IMAGES) && !pl.timg) throw std::invalid_argument("BLING_PASS_TILE_IMAGES without tiles_device");
  int slot_w, slot_h;
  tile_slot(c->S, &slot_w, &slot_h);
  pl.slot_floats = (size_t)slot_w * slot_h * 4;
  if (pl.timg && p->tiles_capacity < pl.tiles.size() * pl.slot_floats)
    throw std::invalid_argument("tiles_capacity " + std::to_string(p->tiles_capacity) + " floats < the " +
                                std::to_string(pl.tiles.size() * pl.slot_floats) + " this shard's tile images need");
  pl.ordered = (p->flags & BLING_PASS_ORDERED_FILM) != 0;
  if (pl.ordered && !pl.timg) {
    // a film pixel is covered by tiles of different waves: the pass keeps all its tile images and forms
    // the film once, after the last wave
    const size_t need = std::max<size_t>(1, pl.tiles.size() * pl.slot_floats);
    if (c->pass_tiles.n < need) c->pass_tiles.alloc(need);
    pl.timg = c->pass_tiles.p;
    pl.add_film = true;
  }
  uint32_t max_tile = 0;
  for (auto& t : pl.tiles) { pl.counts.push_back(t.count); pl.total += t.count; max_tile = std::max(max_tile, t.count); }
  size_t free_b = 0, total_b = 0;
  const bool mem = p->chunk_paths <= 0 && hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0;
  const uint64_t pb = c->path_bytes();
  pl.chunk = pass_plan::wave_chunk(pl.total, max_tile, (uint32_t)c->S.spp, p->chunk_paths, mem, free_b, (uint64_t)c->cap * pb, pb);
  pl.pipe = pl.total > 0 && pl.total <= pl.chunk && pl.total + 256 < ((uint64_t)1 << 31) && pl.tiles.size() >= 2 && pipeline_wanted(c, p);
  // (the first half's slots are rounded up to 256, so the pair needs up to 255 more than one wave)
  c->ensure_paths((uint32_t)(std::min<uint64_t>(pl.chunk, std::max<uint64_t>(pl.total, 1)) + (pl.pipe ? 256u : 0u)));
  pl.chunk = std::min<uint32_t>(pl.chunk, c->cap);
  return pl;
}

struct PassRun {                  // what a pass adds up wave by wave, and the events it reuses for each wave
  EventPair bounce;               // around a wave's path-vertex launches
  Event film_end;                 // after its film
  WaveTiming tm;
  bling_stats st{};               // the samples, launches and times so far
  std::vector<TileDesc> batch;    // the host's copy of a wave's tile table, kept until the wave's sync
};

// After the stream has finished a wave of n0 samples (waves = -2: the two half-waves of n0 and n1, the
// second one's results off1 slots in): what bling_debug_pass_results reads, and the wave's times.
void wave_done(bling_ctx* c, PassRun& r, int waves, uint32_t n0, uint32_t n1, uint32_t off1) {
  r.st.camera_samples += (uint64_t)n0 + n1;
  c->last_pass_waves = waves; c->last_n[0] = n0; c->last_n[1] = n1; c->last_off[1] = off1;
  r.st.ms_bounce += r.bounce.elapsed_ms();
  r.st.ms_film += elapsed_ms(r.bounce.b, r.film_end);
  r.tm.harvest(r.st.ms_closest, r.st.closest_launches, r.st.ms_shade, r.st.shade_launches);
}

// Tiles t0 .. t0 + offset.size() - 1 with these sample offsets into the device's tile table.
void upload_tiles(bling_ctx* c, const PassPlan& pl, PassRun& r, size_t t0, const std::vector<uint32_t>& offset) {
  r.batch.assign(pl.tiles.begin() + t0, pl.tiles.begin() + t0 + offset.size());
  for (size_t k = 0; k < offset.size(); ++k) r.batch[k].offset = offset[k];
  HIPCHK(hipMemcpyAsync(c->tiles_dev.p, r.batch.data(), offset.size() * sizeof(TileDesc), hipMemcpyHostToDevice, c->stream));
}

// The pass as two half-waves on two streams (pass_plan.h half_cut, core_wave.h run_wave_pair_t).
void render_pair(bling_ctx* c, const bling_pass_params* p, const PassPlan& pl, const WaveState& P, float* film_dev, PassRun& r) {
  const pass_plan::HalfCut hc = pass_plan::half_cut(pl.counts);
  const uint32_t cap_a = (hc.nh[0] + 255u) & ~255u;
  if ((uint64_t)cap_a + hc.nh[1] > c->cap) throw std::runtime_error("half-waves exceed the path capacity");
  c->ensure_half_streams();
  const hipStream_t s = c->stream, hs[2] = {c->half_stream[0], c->half_stream[1]};
  HalfWave H[2] = {{c->state_half(0, cap_a), hc.nh[0], hs[0], c->tiles_dev.p, (unsigned)hc.cut, hc.maxc[0]},
                   {c->state_half(1, cap_a), hc.nh[1], hs[1], c->tiles_dev.p + hc.cut, (unsigned)(pl.tiles.size() - hc.cut), hc.maxc[1]}};
  for (auto& h : H) h.W.mis_cull = P.mis_cull;
  upload_tiles(c, pl, r, 0, hc.offset);
  r.bounce.a.record(s);
  // the halves start after everything enqueued so far (the tile table, the counters' reset, the
  // previous pass's film), and the film waits for each of them
  HIPCHK(hipEventRecord(c->half_fork, s));
  try {
    for (int h = 0; h < 2; ++h) HIPCHK(hipStreamWaitEvent(hs[h], c->half_fork, 0));
    r.st.bounce_launches += (uint64_t)run_wave_pair(c, H, p->seed, p->pass_index, (p->flags & BLING_PASS_TRAVERSAL_STATS) != 0, &r.tm);
    for (int h = 0; h < 2; ++h) {
      HIPCHK(hipEventRecord(c->half_done[h], hs[h]));
      HIPCHK(hipStreamWaitEvent(s, c->half_done[h], 0));
      if (h == 1) r.bounce.b.record(s);
      launch_film(c, H[h].W, H[h].td, H[h].n_tiles, film_dev, pl.timg_at(h ? hc.cut : 0), pl.ordered);
    }
    r.film_end.record(s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
  } catch (...) {
    // an error between the fork and the join: nothing of the halves may still run on the context's
    // buffers when the caller sees it (the next pass, or ensure_paths, would reuse or free them)
    for (int h = 0; h < 2; ++h) (void)hipStreamSynchronize(hs[h]);
    (void)hipStreamSynchronize(s);
    throw;
  }
  // ms_film: the second half's film only (the first half's runs beside the second half's last
  // launches); ms_bounce: from the halves' start to the end of the later one
  wave_done(c, r, -2, hc.nh[0], hc.nh[1], cap_a);
}

// st with a pass's device counters filled in.  bling_sample_li reports path_vertices for the
// bidirectional and the normal-map integrator only, and no traversal counts.
bling_stats stats_from_counters(const Counters& hc, bling_stats st, bool vertices, bool traversal) {
  st.rays_camera = hc.cam; st.rays_continuation = hc.cont; st.rays_mis = hc.mis; st.rays_shadow = hc.shadow;
  st.dropped_samples = hc.dropped; st.path_vertices = vertices ? hc.vertices : 0;
  if (traversal) {
    st.node_visits = hc.node_visits; st.tri_tests = hc.tri_tests; st.shape_tests = hc.shape_tests; st.march_ticks = hc.march_ticks;
    st.closest_node_visits = hc.c_node_visits; st.closest_tri_tests = hc.c_tri_tests;
    st.closest_shape_tests = hc.c_shape_tests; st.closest_march_ticks = hc.c_march_ticks;
  }
  return st;
}

int render(bling_ctx* c, const bling_pass_params* p, float* film_dev, bling_stats* st) {
  check_ordered(c, p);
  const PassPlan pl = plan_pass(c, p);
  if (pl.add_film && !film_dev) throw std::invalid_argument("null argument");
  WaveState P = c->state();
  if (p->flags & BLING_PASS_NO_MIS_CULL) P.mis_cull = 0u;
  c->last_pass_waves = 0;
  hipStream_t s = c->stream;
  HIPCHK(hipMemsetAsync(c->counters.p, 0, sizeof(Counters), s));
  const EventPair pass;
  pass.a.record(s);
  PassRun r;
  r.tm.on = (p->flags & BLING_PASS_KERNEL_TIMING) != 0;
  c->tiles_dev.alloc(std::max<size_t>(1, pl.tiles.size()));
  if (pl.pipe) render_pair(c, p, pl, P, film_dev, r);
  for (size_t t0 = pl.pipe ? pl.tiles.size() : 0; t0 < pl.tiles.size();) {
    const pass_plan::Wave w = pass_plan::next_wave(pl.counts, t0, pl.chunk);
    const unsigned nt = (unsigned)(w.t1 - t0);
    upload_tiles(c, pl, r, t0, w.offset);
    if (c->S.integrator == BLING_INTEGRATOR_BIDIR) {
      r.bounce.a.record(s);
      r.st.bounce_launches += (uint64_t)bidir_wave(c, P, c->tiles_dev.p, nt, w.maxc, nullptr, w.off, p->seed, p->pass_index, nullptr);
    } else {
      k_reset_queues<<<1, 64, 0, s>>>(P.qcount, w.off);
      k_raygen<<<dim3((w.maxc + 255) / 256, nt), 256, 0, s>>>(c->dscene.p, P, c->tiles_dev.p, p->seed, p->pass_index);
      r.bounce.a.record(s);
      if (c->S.integrator == BLING_INTEGRATOR_NORMALS) r.st.bounce_launches += (uint64_t)normals_wave(c, P, w.off, &r.tm);
      else r.st.bounce_launches += (uint64_t)run_wave(c, P, w.off, p->seed, p->pass_index, (p->flags & BLING_PASS_TRAVERSAL_STATS) != 0, &r.tm);
    }
    r.bounce.b.record(s);
    launch_film(c, P, c->tiles_dev.p, nt, film_dev, pl.timg_at(t0), pl.ordered);
    r.film_end.record(s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));   // the tile table is reused by the next chunk
    wave_done(c, r, c->last_pass_waves + 1, w.off, 0, 0);
    t0 = w.t1;
  }
  const EventPair add;
  if (pl.add_film) {
    add.a.record(s);
    add_tiles_ordered(c, p, p->shard_rank, pl.timg, nullptr, film_dev);
    add.b.record(s);
  }
  pass.b.record(s);
  HIPCHK(hipEventSynchronize(pass.b));
  if (pl.add_film) r.st.ms_film += add.elapsed_ms();
  Counters hc;
  HIPCHK(hipMemcpy(&hc, c->counters.p, sizeof hc, hipMemcpyDeviceToHost));
  std::memcpy(c->stream_bytes, hc.sb, sizeof c->stream_bytes);
  c->mis_culled = hc.mis_culled;
  if (st) {
    *st = stats_from_counters(hc, r.st, true, true);
    st->tiles = pl.tiles.size();
    st->ms_total = pass.elapsed_ms();
  }
  return BLING_OK;
}

// addTile of tile images into a device film: for each (tile list, buffer) pair, slot k of the buffer
// holds tile k of the list (slots of this context's tile_slot); one launch over all of them
void add_tiles(bling_ctx* c, const std::vector<std::pair<const std::vector<TileDesc>*, const float*>>& sets,
               float* film_dev) {
  int sw, sh;
  tile_slot(c->S, &sw, &sh);
  const size_t slot = (size_t)sw * sh;
  std::vector<TileSrc> t;
  for (const auto& s : sets)
    for (size_t k = 0; k < s.first->size(); ++k) {
      const TileDesc& d = (*s.first)[k];
      t.push_back(TileSrc{reinterpret_cast<const float4*>(s.second) + k * slot, std::max(0, d.x0), std::max(0, d.y0)});
    }
  if (t.empty()) return;
  c->tile_src.upload(t.data(), t.size());
  k_add_tiles<<<(unsigned)t.size(), 256, 0, c->stream>>>(c->tile_src.p, film_dev, c->S.width, c->S.height, sw, sh);
  HIPCHK(hipGetLastError());
}

// One pass over every device of the context (bling_create with n_devices > 1).  The caller's shard
// (rank, world) is dealt further over the n devices: device j renders the tiles of shard
// (rank + world j, world n), i.e. tile k (after the stride) when k % (world n) == rank + world j.
// Devices render concurrently, one host thread each, every one into its own tile-image buffer
// (BLING_PASS_TILE_IMAGES: ~1/n of the pass's tiles with their aprons, 2.4 MB per device for C2 at
// n = 8 instead of a 16 MiB film).  Once all succeeded, each peer pushes its buffer into its landing
// buffer on the primary with its own stream (the copies run concurrently over the xGMI links), the
// primary waits for them and adds every device's tile images into the caller's film (addTile).  A
// failed pass leaves the caller's film untouched.  Replaces the spark fan-out `parBuffer
// numCapabilities` of prender (Rendering.hs:111-140, :118) and its addTile merge.
int render_fanout(bling_ctx* c, const bling_pass_params* p, float* film_dev, bling_stats* st) {
  if (c->peers.empty()) return render(c, p, film_dev, st);
  check_ordered(c, p);
  if (p->flags & BLING_PASS_TILE_IMAGES) throw std::invalid_argument("BLING_PASS_TILE_IMAGES on a multi-device context");
  const int nd = 1 + (int)c->peers.size();
  const int world = std::max(1, p->shard_world), rank = p->shard_rank;
  int sw, sh;
  tile_slot(c->S, &sw, &sh);
  const size_t slot_floats = (size_t)sw * sh * 4;
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<bling_stats> sts(nd);
  std::vector<std::string> errs(nd);
  std::vector<int> rcs(nd, BLING_OK);
  std::vector<std::vector<TileDesc>> dtiles(nd);
  for (int j = 0; j < nd; ++j) dtiles[j] = pass_tiles(c->S, rank + world * j, world * nd, p->tile_stride);
  std::vector<std::thread> th;
  for (int j = 0; j < nd; ++j) {
    th.emplace_back([&, j] {
      try {
        bling_ctx* d = j == 0 ? c : c->peers[j - 1].get();
        HIPCHK(hipSetDevice(d->device));
        bling_pass_params pp = *p;
        pp.shard_world = world * nd;
        pp.shard_rank = rank + world * j;
        const size_t need = std::max<size_t>(1, dtiles[j].size() * slot_floats);
        if (d->pass_tiles.n < need) d->pass_tiles.alloc(need);
        pp.flags |= BLING_PASS_TILE_IMAGES;
        pp.tiles_device = d->pass_tiles.p;
        pp.tiles_capacity = d->pass_tiles.n;
        rcs[j] = render(d, &pp, nullptr, &sts[j]);
      } catch (const std::exception& e) {
        errs[j] = e.what();
        rcs[j] = BLING_EHIP;
      }
    });
  }
  for (auto& t : th) t.join();
  for (int j = 0; j < nd; ++j)
    if (rcs[j] != BLING_OK) throw HipError("device " + std::to_string(j) + ": " + (errs[j].empty() ? "render failed" : errs[j]));
  // merge: peers push concurrently, the primary adds after their copies
  while (c->stage.size() < (size_t)nd) c->stage.emplace_back(new DBuf<float>());
  struct Events {                      // destroyed on every exit path, after the streams drained
    std::vector<Event> done;           // one per peer that copies (members go after the destructor's body)
    std::vector<hipStream_t> drain;
    ~Events() { for (hipStream_t s : drain) (void)hipStreamSynchronize(s); }
  } ev;
  for (int j = 1; j < nd; ++j) {
    bling_ctx* d = c->peers[j - 1].get();
    const size_t bytes = dtiles[j].size() * slot_floats * sizeof(float);
    if (!bytes) continue;
    HIPCHK(hipSetDevice(c->device));
    if (c->stage[j]->n < dtiles[j].size() * slot_floats) c->stage[j]->alloc(dtiles[j].size() * slot_floats);
    HIPCHK(hipSetDevice(d->device));
    ev.drain.push_back(d->stream);
    HIPCHK(hipMemcpyPeerAsync(c->stage[j]->p, c->device, d->pass_tiles.p, d->device, bytes, d->stream));
    ev.done.emplace_back(false);
    ev.done.back().record(d->stream);
  }
  HIPCHK(hipSetDevice(c->device));
  for (const Event& done : ev.done) HIPCHK(hipStreamWaitEvent(c->stream, done, 0));
  std::vector<std::pair<const std::vector<TileDesc>*, const float*>> sets;
  for (int j = 0; j < nd; ++j) sets.emplace_back(&dtiles[j], j == 0 ? c->pass_tiles.p : c->stage[j]->p);
  ev.drain.push_back(c->stream);
  // one launch over every device's tile images.  Not bit-reproducible, like the single-device pass:
  // the film pixels under overlapping aprons, and each tile image's own LDS accumulation, take their
  // float additions in arrival order (tests/test_multidevice.py checks the sums to a tolerance;
  // INTEGRATION.md "Reproducibility" tells callers)
  add_tiles(c, sets, film_dev);
  if (st) {
    bling_stats a = sts[0];
    // counts summed, times the slowest device's, timed launches counted once (pass_stats.h)
    for (int j = 1; j < nd; ++j) pass_stats::stats_add(a, sts[j], pass_stats::StatsFold::Devices);
    a.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *st = a;
  }
  return BLING_OK;
}

}  // namespace

namespace bcore {
void set_last_error(const std::string& msg) { g_err = msg; }
}  // namespace bcore

extern "C" {

int bling_create(const int* device_ids, int n_devices, bling_ctx** out) {
  return guarded([&] {
    if (!out) throw std::invalid_argument("out is NULL");
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) { g_err = "no HIP device"; return BLING_ENODEV; }
    if (n_devices < 0 || (n_devices > 0 && !device_ids)) throw std::invalid_argument("bad device list");
    if (n_devices > 64) throw std::invalid_argument("more than 64 devices");
    const int nd = std::max(1, n_devices);
    std::vector<int> ids(nd, 0);
    for (int j = 0; j < n_devices; ++j) {
      ids[j] = device_ids[j];
      if (ids[j] < 0 || ids[j] >= count) throw std::invalid_argument("bad device id " + std::to_string(ids[j]));
    }
    // a repeated id would silently fan a multi-GPU caller out onto one device: refused, except under
    // the test hook that exercises the fan-out on a one-GPU box (BLING_ALLOW_REPEATED_DEVICES=1)
    const char* rep = std::getenv("BLING_ALLOW_REPEATED_DEVICES");
    if (!(rep && rep[0] == '1'))
      for (int j = 0; j < n_devices; ++j)
        for (int k = 0; k < j; ++k)
          if (ids[j] == ids[k])
            throw std::invalid_argument("device id " + std::to_string(ids[j]) + " repeated in the device list");
    auto make = [](int dev) {
      auto x = std::make_unique<bling_ctx>();
      x->device = dev;
      HIPCHK(hipSetDevice(dev));
      HIPCHK(hipStreamCreateWithFlags(&x->stream, hipStreamNonBlocking));
      return x;
    };
    auto c = make(ids[0]);
    develop_table(c.get());   // rgbPixels' thresholds (bling_film_develop runs on the first device only)
    // further devices: peer contexts of the fan-out (render_fanout); the primary reads their films
    // over xGMI, so peer access is enabled where the pair supports it (a repeated id -- test hook
    // only -- runs two contexts on one device)
    for (int j = 1; j < nd; ++j) {
      c->peers.push_back(make(ids[j]));
      if (ids[j] != ids[0]) {
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, ids[0], ids[j]) == hipSuccess && can) {
          HIPCHK(hipSetDevice(ids[0]));
          hipError_t e = hipDeviceEnablePeerAccess(ids[j], 0);
          if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) HIPCHK(e);
          (void)hipGetLastError();
        }
      }
    }
    HIPCHK(hipSetDevice(ids[0]));
    *out = c.release();
    return BLING_OK;
  });
}

int bling_render_pass_device(bling_ctx* c, const bling_pass_params* p, void* film, bling_stats* st) {
  return guarded([&] {
    if (!c || !p || (!film && !(p->flags & BLING_PASS_TILE_IMAGES))) throw std::invalid_argument("null argument");
    need_scene(c);
    HIPCHK(hipSetDevice(c->device));
    return render_fanout(c, p, static_cast<float*>(film), st);
  });
}

int bling_render_pass(bling_ctx* c, const bling_pass_params* p, float* film_out, bling_stats* st) {
  return guarded([&] {
    if (!c || !p) throw std::invalid_argument("null argument");
    need_scene(c);
    HIPCHK(hipSetDevice(c->device));
    const size_t n = (size_t)c->S.width * c->S.height * 4;
    stage_in(c->film_dev, film_out, n);
    const int rc = render_fanout(c, p, c->film_dev.p, st);
    if (rc == BLING_OK) stage_out(film_out, c->film_dev, n);
    return rc;
  });
}

static int sample_li_impl(bling_ctx* c, uint32_t seed, uint32_t pass_index, const int32_t* samples, size_t n, float* L_out,
                   float* img_out, bling_stats* st, float* vtx_out, float* terms_out = nullptr, int32_t* lens_out = nullptr) {
  return guarded([&] {
    if (!c || !samples || !L_out) throw std::invalid_argument("null argument");
    need_scene(c);
    if (n == 0) return BLING_OK;
    if (n > (1u << 24)) throw std::invalid_argument("too many samples");
    HIPCHK(hipSetDevice(c->device));
    const DevScene& S = c->S;
    for (size_t k = 0; k < n; ++k) {
      int x = samples[3 * k], y = samples[3 * k + 1], m = samples[3 * k + 2];
      if (x < S.ex0 || x > S.ex1 || y < S.ey0 || y > S.ey1 || m < 0 || m >= S.spp)
        throw std::invalid_argument("sample outside the sample extent");
    }
    c->ensure_paths((uint32_t)n);
    DBuf<float4> lfull;
    lfull.alloc((size_t)4 * c->cap);
    DBuf<int32_t> list;
    list.upload(samples, 3 * n);
    WaveState P = c->state();
    P.Lfull = lfull.p;
    DBuf<float> vtx;
    if (vtx_out) {
      const size_t nv = n * BLING_DV_DEPTHS * BLING_DV_FIELDS;
      std::vector<float> nan(nv, std::numeric_limits<float>::quiet_NaN());
      vtx.upload(nan.data(), nv);
      P.dbg = vtx.p;
    }
    hipStream_t s = c->stream;
    HIPCHK(hipMemsetAsync(c->counters.p, 0, sizeof(Counters), s));
    DBuf<float> terms;
    if (S.integrator == BLING_INTEGRATOR_BIDIR) {
      if (terms_out) terms.alloc(n * 48);
      bidir_wave(c, P, nullptr, 0u, 0u, list.p, (uint32_t)n, seed, pass_index, terms.p);
    } else {
      unsigned blocks = (unsigned)((n + 255) / 256);
      k_reset_queues<<<1, 64, 0, s>>>(P.qcount, (uint32_t)n);
      k_raygen_list<<<blocks, 256, 0, s>>>(c->dscene.p, P, list.p, (uint32_t)n, seed, pass_index);
      if (S.integrator == BLING_INTEGRATOR_NORMALS) normals_wave(c, P, (uint32_t)n, nullptr);
      else run_wave(c, P, (uint32_t)n, seed, pass_index, false);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    if (terms.p) HIPCHK(hipMemcpy(terms_out, terms.p, n * 48 * sizeof(float), hipMemcpyDeviceToHost));
    if (lens_out && c->bidir.info.p) HIPCHK(hipMemcpy(lens_out, c->bidir.info.p, n * sizeof(uint4), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(L_out, lfull.p, n * 16 * sizeof(float), hipMemcpyDeviceToHost));
    if (vtx_out) HIPCHK(hipMemcpy(vtx_out, vtx.p, vtx.n * sizeof(float), hipMemcpyDeviceToHost));
    if (img_out) {
      std::vector<float2> im(n);
      HIPCHK(hipMemcpy(im.data(), c->img.p, n * sizeof(float2), hipMemcpyDeviceToHost));
      for (size_t k = 0; k < n; ++k) { img_out[2 * k] = im[k].x; img_out[2 * k + 1] = im[k].y; }
    }
    if (st) {
      Counters hc;
      HIPCHK(hipMemcpy(&hc, c->counters.p, sizeof hc, hipMemcpyDeviceToHost));
      bling_stats samples{}; samples.camera_samples = n;
      *st = stats_from_counters(hc, samples, S.integrator == BLING_INTEGRATOR_BIDIR || S.integrator == BLING_INTEGRATOR_NORMALS, false);
    }
    return BLING_OK;
  });
}

int bling_pass_tile_layout(bling_ctx* c, const bling_pass_params* p, int32_t* origins_out, size_t* n_tiles,
                           int32_t* slot_w, int32_t* slot_h) {
  return guarded([&] {
    if (!c || !p || !n_tiles) throw std::invalid_argument("null argument");
    need_scene(c);
    const std::vector<TileDesc> tiles = pass_tiles(c->S, p->shard_rank, p->shard_world, p->tile_stride);
    *n_tiles = tiles.size();
    int sw, sh;
    tile_slot(c->S, &sw, &sh);
    if (slot_w) *slot_w = sw;
    if (slot_h) *slot_h = sh;
    if (origins_out)
      for (size_t k = 0; k < tiles.size(); ++k) {
        origins_out[2 * k] = std::max(0, tiles[k].x0);
        origins_out[2 * k + 1] = std::max(0, tiles[k].y0);
      }
    return BLING_OK;
  });
}

static void check_tiles_capacity(bling_ctx* c, const bling_pass_params* p, size_t n_tiles) {
  int sw, sh;
  tile_slot(c->S, &sw, &sh);
  const size_t need = n_tiles * (size_t)sw * sh * 4;
  if (p->tiles_capacity < need)
    throw std::invalid_argument("tiles_capacity " + std::to_string(p->tiles_capacity) + " floats < the " +
                                std::to_string(need) + " a shard's tile images need");
}

int bling_film_add_tiles(bling_ctx* c, const bling_pass_params* p, const void* tiles_device, void* film_device) {
  return guarded([&] {
    if (!c || !p || !tiles_device || !film_device) throw std::invalid_argument("null argument");
    need_scene(c);
    HIPCHK(hipSetDevice(c->device));
    const std::vector<TileDesc> tiles = pass_tiles(c->S, p->shard_rank, p->shard_world, p->tile_stride);
    check_tiles_capacity(c, p, tiles.size());
    check_ordered(c, p);
    if (p->flags & BLING_PASS_ORDERED_FILM)
      add_tiles_ordered(c, p, p->shard_rank, static_cast<const float*>(tiles_device), nullptr, static_cast<float*>(film_device));
    else
      add_tiles(c, {{&tiles, static_cast<const float*>(tiles_device)}}, static_cast<float*>(film_device));
    HIPCHK(hipStreamSynchronize(c->stream));
    return BLING_OK;
  });
}

int bling_film_add_shards(bling_ctx* c, const bling_pass_params* p, const void* const* tiles_devices, void* film_device) {
  return guarded([&] {
    if (!c || !p || !tiles_devices || !film_device) throw std::invalid_argument("null argument");
    need_scene(c);
    HIPCHK(hipSetDevice(c->device));
    const int world = std::max(1, p->shard_world);
    std::vector<std::vector<TileDesc>> tiles(world);
    std::vector<std::pair<const std::vector<TileDesc>*, const float*>> sets;
    for (int r = 0; r < world; ++r) {
      if (!tiles_devices[r]) throw std::invalid_argument("null tile buffer");
      tiles[r] = pass_tiles(c->S, r, world, p->tile_stride);
      check_tiles_capacity(c, p, tiles[r].size());
      sets.emplace_back(&tiles[r], static_cast<const float*>(tiles_devices[r]));
    }
    check_ordered(c, p);
    if (p->flags & BLING_PASS_ORDERED_FILM) {
      std::vector<const float4*> bufs(world);
      for (int r = 0; r < world; ++r) bufs[r] = static_cast<const float4*>(tiles_devices[r]);
      c->rank_bufs.upload(bufs.data(), bufs.size());
      add_tiles_ordered(c, p, -1, nullptr, c->rank_bufs.p, static_cast<float*>(film_device));
    } else {
      add_tiles(c, sets, static_cast<float*>(film_device));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return BLING_OK;
  });
}

namespace {
// the checks the two develop calls share
void develop_check(bling_ctx* c, const bling_develop_params* dp, const void* film, const void* out) {
  if (!c || !dp || !film || !out) throw std::invalid_argument("null argument");
  need_scene(c);
  if (dp->format != BLING_DEVELOP_RGB_F32 && dp->format != BLING_DEVELOP_RGB8 && dp->format != BLING_DEVELOP_RGBE)
    throw std::invalid_argument("develop: unknown format " + std::to_string(dp->format));
}
bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + nb && pb < pa + na;
}
}  // namespace

int bling_film_develop_device(bling_ctx* c, const bling_develop_params* dp, const void* film, const void* splat, void* out) {
  return guarded([&] {
    develop_check(c, dp, film, out);
    const size_t px = (size_t)c->S.width * c->S.height, nout = px * develop_pixel_bytes(dp->format);
    if (ranges_overlap(out, nout, film, px * 16) || (splat && ranges_overlap(out, nout, splat, px * 12)))
      throw std::invalid_argument("develop: out overlaps the film or the splat buffer");
    HIPCHK(hipSetDevice(c->device));
    develop_launch(c, dp, static_cast<const float*>(film), static_cast<const float*>(splat), out);
    HIPCHK(hipStreamSynchronize(c->stream));
    return BLING_OK;
  });
}

int bling_film_develop(bling_ctx* c, const bling_develop_params* dp, const float* film, const float* splat, void* out) {
  return guarded([&] {
    develop_check(c, dp, film, out);
    int x0, x1, y0, y1;
    if (!develop_clip(c, dp->window, &x0, &x1, &y0, &y1)) return BLING_OK;   // nothing to write
    HIPCHK(hipSetDevice(c->device));
    const size_t w = (size_t)c->S.width, px = w * c->S.height, bpp = develop_pixel_bytes(dp->format);
    if (c->film_dev.n != px * 4) c->film_dev.alloc(px * 4);
    if (splat && c->develop_splat.n != px * 3) c->develop_splat.alloc(px * 3);
    if (c->develop_out.n < px * bpp) c->develop_out.alloc(px * 12);   // the largest format: allocated once
    hipStream_t s = c->stream;
    // the window's rows only, in both directions: they are one contiguous range of each buffer
    const size_t r0 = (size_t)y0 * w, nr = (size_t)(y1 - y0 + 1) * w;
    HIPCHK(hipMemcpyAsync(c->film_dev.p + r0 * 4, film + r0 * 4, nr * 16, hipMemcpyHostToDevice, s));
    if (splat) HIPCHK(hipMemcpyAsync(c->develop_splat.p + r0 * 3, splat + r0 * 3, nr * 12, hipMemcpyHostToDevice, s));
    uint8_t* o = c->develop_out.p + r0 * bpp;
    uint8_t* oh = static_cast<uint8_t*>(out) + r0 * bpp;
    // a window narrower than the image leaves pixels of its rows untouched: they go up first
    if (x0 != 0 || x1 != c->S.width - 1) HIPCHK(hipMemcpyAsync(o, oh, nr * bpp, hipMemcpyHostToDevice, s));
    develop_launch(c, dp, c->film_dev.p, splat ? c->develop_splat.p : nullptr, c->develop_out.p);
    HIPCHK(hipMemcpyAsync(oh, o, nr * bpp, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return BLING_OK;
  });
}

namespace {
// One pass of bling_render with exact per-window reports (single-device contexts, host film): the
// pass is rendered into its tile images on the device (BLING_PASS_TILE_IMAGES), which come back to
// the host; bling_render then adds them into the film one window after another, in the pass's
// window order, reporting SamplesAdded with the film up to that window (Rendering.hs:130-134).
int region_pass(bling_ctx* c, const bling_pass_params& p, bling_stats* st, std::vector<TileDesc>& tiles,
                std::vector<float>& images, int& sw, int& sh) {
  return guarded([&] {
    need_scene(c);
    HIPCHK(hipSetDevice(c->device));
    tiles = pass_tiles(c->S, p.shard_rank, p.shard_world, p.tile_stride);
    tile_slot(c->S, &sw, &sh);
    const size_t slot = (size_t)sw * sh * 4, need = std::max<size_t>(1, tiles.size() * slot);
    if (c->pass_tiles.n < need) c->pass_tiles.alloc(need);
    bling_pass_params pt = p;
    pt.flags |= BLING_PASS_TILE_IMAGES;
    pt.tiles_device = c->pass_tiles.p;
    pt.tiles_capacity = c->pass_tiles.n;
    const int rc = render(c, &pt, nullptr, st);
    if (rc != BLING_OK) return rc;
    images.resize(tiles.size() * slot);
    HIPCHK(hipMemcpy(images.data(), c->pass_tiles.p, images.size() * sizeof(float), hipMemcpyDeviceToHost));
    return BLING_OK;
  });
}
// addTile of one tile image slot (the layout film_flush writes) into a host film: k_add_tiles' rule
// (zero pixels and pixels past the film skipped), one tile at a time in the caller's order
// (all: zero pixels are added too, as the ordered film does: film = film + tile for every covered pixel)
void add_tile_host(float* film, int width, int height, const float* img, int ox, int oy, int sw, int sh, bool all) {
  for (int y = 0; y < sh; ++y)
    for (int x = 0; x < sw; ++x) {
      const int gx = ox + x, gy = oy + y;
      if (gx >= width || gy >= height) continue;
      const float* v = img + 4 * ((size_t)y * sw + x);
      if (!all && v[0] == 0.f && v[1] == 0.f && v[2] == 0.f && v[3] == 0.f) continue;
      float* o = film + 4 * ((size_t)gy * width + gx);
      o[0] += v[0]; o[1] += v[1]; o[2] += v[2]; o[3] += v[3];
    }
}
}  // namespace

int bling_render(bling_ctx* c, const bling_pass_params* p, float* film_out, bling_progress_fn report, void* user,
                 bling_stats* st) {
  if (!report) { g_err = "bling_render needs a progress reporter"; return BLING_EINVAL; }
  if (!p) { g_err = "null argument"; return BLING_EINVAL; }
  bling_pass_params pp = *p;
  bling_stats sum;
  std::memset(&sum, 0, sizeof sum);
  // per-window reports with the film up to each window need the tile images on the host: single
  // device, host film (a multi-device pass merges on the device; its reports follow the pass)
  const bool exact = (pp.flags & BLING_PASS_REGION_EVENTS) && film_out && c && c->peers.empty();
  std::vector<TileDesc> rtiles;
  std::vector<float> rimages;
  int rsw = 0, rsh = 0;
  for (;;) {
    bling_stats one;
    const int rc = exact ? region_pass(c, pp, &one, rtiles, rimages, rsw, rsh) : bling_render_pass(c, &pp, film_out, &one);
    if (rc != BLING_OK) return rc;
    pass_stats::stats_add(sum, one, pass_stats::StatsFold::Passes);
    if (st) *st = sum;
    if (pp.flags & BLING_PASS_REGION_EVENTS) {                     // forM_ ... RegionStarted w, SamplesAdded w img'
      const std::vector<TileDesc> tiles = exact ? rtiles : pass_tiles(c->S, pp.shard_rank, pp.shard_world, pp.tile_stride);
      for (size_t k = 0; k < tiles.size(); ++k) {
        const TileDesc& t = tiles[k];
        const bling_progress rs{BLING_PROGRESS_REGION_STARTED, (int32_t)pp.pass_index, nullptr, 1.f, nullptr,
                                {t.x0, t.x1, t.y0, t.y1}};
        (void)report(user, &rs);
        if (exact)                                                    // addTile of this window (Rendering.hs:133)
          add_tile_host(film_out, c->S.width, c->S.height, rimages.data() + k * (size_t)rsw * rsh * 4,
                        std::max(0, t.x0), std::max(0, t.y0), rsw, rsh, (pp.flags & BLING_PASS_ORDERED_FILM) != 0);
        const bling_progress sa{BLING_PROGRESS_SAMPLES_ADDED, (int32_t)pp.pass_index, film_out, 1.f, nullptr,
                                {t.x0, t.x1, t.y0, t.y1}};
        (void)report(user, &sa);
      }
    }
    const bling_progress ev{BLING_PROGRESS_PASS_DONE, (int32_t)pp.pass_index, film_out, 1.f, &one, {0, 0, 0, 0}};
    if (!report(user, &ev)) return BLING_OK;                      // PassDone ... >>= \cont -> ...
    ++pp.pass_index;
  }
}

int bling_debug_set_mis_cull(bling_ctx* c, int on) {
  if (!c) { g_err = "null argument"; return BLING_EINVAL; }
  c->mis_cull_off = !on;
  for (auto& p : c->peers) p->mis_cull_off = !on;
  return BLING_OK;
}

int bling_debug_set_pipeline(bling_ctx* c, int mode) {
  if (!c || mode < -1 || mode > 1) { g_err = "bad argument"; return BLING_EINVAL; }
  c->pipeline_mode = mode;
  for (auto& p : c->peers) p->pipeline_mode = mode;
  return BLING_OK;
}

int bling_debug_pass_results(bling_ctx* c, float* out, size_t cap, size_t* n, int* waves) {
  return guarded([&] {
    if (!c || !n) throw std::invalid_argument("null argument");
    if (!c->peers.empty()) throw std::invalid_argument("single-device contexts only");
    if (waves) *waves = c->last_pass_waves;
    if (c->last_pass_waves != 1 && c->last_pass_waves != -2) throw std::invalid_argument("the last pass did not keep its samples' results");
    *n = (size_t)c->last_n[0] + c->last_n[1];
    if (!out) return BLING_OK;
    if (cap < *n) throw std::invalid_argument("capacity below the pass's samples");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpy(out, c->result.p, (size_t)c->last_n[0] * sizeof(float4), hipMemcpyDeviceToHost));
    if (c->last_n[1])
      HIPCHK(hipMemcpy(out + 4 * (size_t)c->last_n[0], c->result.p + c->last_off[1], (size_t)c->last_n[1] * sizeof(float4),
                       hipMemcpyDeviceToHost));
    return BLING_OK;
  });
}

int bling_debug_compact(bling_ctx* c, const uint8_t* flags, const uint32_t* queue_in, size_t n, size_t capacity, int fused,
                        uint32_t* queues_out, uint32_t* qcount_out) {
  return guarded([&] {
    if (!c || !flags || !queue_in || !queues_out || !qcount_out) throw std::invalid_argument("null argument");
    if (capacity == 0 || n > capacity || capacity > (1u << 24)) throw std::invalid_argument("bad queue length or capacity");
    HIPCHK(hipSetDevice(c->device));
    c->ensure_paths((uint32_t)capacity);
    WaveState W = c->state();
    hipStream_t s = c->stream;
    const uint32_t nb = (uint32_t)((capacity + COMPACT_CHUNK - 1) / COMPACT_CHUNK);
    // every flag past the queue's end set, every output word poisoned: neither may show in the result
    HIPCHK(hipMemsetAsync(W.qflag, 0xFF, c->cap, s));
    HIPCHK(hipMemsetAsync(c->qmem.p, 0xEE, (size_t)6 * c->cap * sizeof(uint32_t), s));
    if (n) {
      HIPCHK(hipMemcpyAsync(W.qflag, flags, n, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(W.queue[Q_SHADE0], queue_in, n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    }
    k_reset_queues<<<1, 64, 0, s>>>(W.qcount, (uint32_t)n);
    k_compact_count<<<nb, 256, 0, s>>>(W, nb, 0);
    k_compact_scan<<<1, 1024, 0, s>>>(W, nb, 0, fused);
    k_compact_scatter<<<nb, 256, 0, s>>>(W, nb, 0, fused);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemcpy(qcount_out, W.qcount, QC_N * sizeof(uint32_t), hipMemcpyDeviceToHost));
    const int ids[5] = {Q_SHADE0, Q_SHADE1, Q_CLOSEST, Q_ANY, Q_RESOLVE};
    const size_t at[5] = {0, 1, 2, 4, 5};
    for (int k = 0; k < 5; ++k)
      HIPCHK(hipMemcpy(queues_out + at[k] * capacity, W.queue[ids[k]], (ids[k] == Q_CLOSEST ? 2 : 1) * capacity * sizeof(uint32_t),
                       hipMemcpyDeviceToHost));
    return BLING_OK;
  });
}

int bling_debug_mis_culled(bling_ctx* c, uint64_t* out) {
  if (!c || !out) { g_err = "null argument"; return BLING_EINVAL; }
  uint64_t n = c->mis_culled;
  for (const auto& p : c->peers) n += p->mis_culled;
  *out = n;
  return BLING_OK;
}

int bling_debug_stream_bytes(bling_ctx* c, uint64_t* out, size_t n, size_t* n_streams) {
  if (!c) { g_err = "null argument"; return BLING_EINVAL; }
  if (n_streams) *n_streams = BLING_N_STREAMS;
  if (!BLING_STREAM_STATS) { g_err = "stream byte counts need a BLING_STREAM_STATS build"; return BLING_EUNSUPPORTED; }
  if (out) std::memcpy(out, c->stream_bytes, std::min<size_t>(n, 2 * BLING_N_STREAMS) * sizeof(uint64_t));
  return BLING_OK;
}

int bling_sample_li(bling_ctx* c, uint32_t seed, uint32_t pass_index, const int32_t* samples, size_t n, float* L_out,
                    float* img_out, bling_stats* st) {
  return sample_li_impl(c, seed, pass_index, samples, n, L_out, img_out, st, nullptr);
}

int bling_debug_bidir_terms(bling_ctx* c, uint32_t seed, uint32_t pass_index, const int32_t* samples, size_t n,
                            float* terms_out, int32_t* lens_out) {
  if (!terms_out || !lens_out) { g_err = "null argument"; return BLING_EINVAL; }
  if (c && c->has_scene && c->S.integrator != BLING_INTEGRATOR_BIDIR) {
    g_err = "the uploaded scene's integrator is not bidir";
    return BLING_EINVAL;
  }
  std::vector<float> L(16 * std::max<size_t>(n, 1));
  return sample_li_impl(c, seed, pass_index, samples, n, L.data(), nullptr, nullptr, nullptr, terms_out, lens_out);
}

int bling_sample_li_vertices(bling_ctx* c, uint32_t seed, uint32_t pass_index, const int32_t* samples, size_t n,
                             float* L_out, float* vtx_out) {
  if (!BLING_DEBUG_VERTEX) { g_err = "per-vertex records need a BLING_DEBUG_VERTEX build"; return BLING_EUNSUPPORTED; }
  if (!vtx_out) { g_err = "vtx_out is NULL"; return BLING_EINVAL; }
  if (c && c->S.integrator != BLING_INTEGRATOR_PATH) { g_err = "per-vertex records: Path integrator only"; return BLING_EUNSUPPORTED; }
  return sample_li_impl(c, seed, pass_index, samples, n, L_out, nullptr, nullptr, vtx_out);
}

int bling_trace(bling_ctx* c, const float* rays, size_t n, int any_hit, float* t_out, uint32_t* prim_out, float* bary_out) {
  return guarded([&] {
    if (!c || !rays || !prim_out) throw std::invalid_argument("null argument");
    need_scene(c);
    if (n == 0) return BLING_OK;
    HIPCHK(hipSetDevice(c->device));
    c->tr_rays.upload(rays, 8 * n);
    c->tr_t.alloc(n); c->tr_prim.alloc(n); c->tr_bary.alloc(2 * n);
    HIPCHK(hipMemsetAsync(c->counters.p, 0, sizeof(Counters), c->stream));
    launch_trace(c, c->tr_rays.p, (uint32_t)n, any_hit, c->tr_t.p, c->tr_prim.p, c->tr_bary.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(prim_out, c->tr_prim.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (t_out) HIPCHK(hipMemcpy(t_out, c->tr_t.p, n * sizeof(float), hipMemcpyDeviceToHost));
    if (bary_out) HIPCHK(hipMemcpy(bary_out, c->tr_bary.p, 2 * n * sizeof(float), hipMemcpyDeviceToHost));
    return BLING_OK;
  });
}

int bling_trace_device(bling_ctx* c, const void* rays, size_t n, int any_hit, void* t_dev, void* prim_dev, void* bary_dev,
                       int repeats, double* ms_out) {
  return guarded([&] {
    if (!c || !rays || !prim_dev) throw std::invalid_argument("null argument");
    need_scene(c);
    HIPCHK(hipSetDevice(c->device));
    const EventPair ev;
    ev.a.record(c->stream);
    for (int r = 0; r < std::max(1, repeats); ++r)
      launch_trace(c, static_cast<const float*>(rays), (uint32_t)n, any_hit, static_cast<float*>(t_dev),
                   static_cast<uint32_t*>(prim_dev), static_cast<float*>(bary_dev));
    HIPCHK(hipGetLastError());
    ev.b.record(c->stream);
    HIPCHK(hipEventSynchronize(ev.b));
    if (ms_out) *ms_out = ev.elapsed_ms() / std::max(1, repeats);
    return BLING_OK;
  });
}

void bling_destroy(bling_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  delete c;
}

const char* bling_last_error(void) { return g_err.c_str(); }

const char* bling_version(void) { return "bling-mi355x core 0.1 (gfx950, wavefront path tracer, BVH2 + LDS stack)"; }

}  // extern "C"
