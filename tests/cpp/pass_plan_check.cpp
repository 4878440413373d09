// pass_plan_check.cpp -- the pass driver's integer arithmetic (bling_amd/csrc/core/pass_plan.h) and the
// bling_stats field table (pass_stats.h) on the CPU: hand-derived cases of wave sizing, the half-wave
// cut and the greedy tile batching, their properties over random tile lists, and both folds of the
// statistics.  Built and run by tests/test_pass_plan.py; exit status 0 = every check held.
#include <cstdio>
#include <cstring>
#include <random>

#include "../../bling_amd/csrc/core/pass_plan.h"
#include "../../bling_amd/csrc/core/pass_stats.h"

using namespace pass_plan;

static int fails = 0;
#define CHECK(x)                                                            \
  do {                                                                      \
    if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++fails; } \
  } while (0)

// every wave of a pass over counts: {tiles, samples} per wave, checking each wave's invariants
static std::vector<std::pair<size_t, uint32_t>> waves_of(const std::vector<uint32_t>& counts, uint32_t chunk) {
  std::vector<std::pair<size_t, uint32_t>> out;
  for (size_t t0 = 0; t0 < counts.size();) {
    const Wave w = next_wave(counts, t0, chunk);
    CHECK(w.t1 > t0 && w.t1 <= counts.size());           // in order, never empty
    CHECK(w.offset.size() == w.t1 - t0);
    uint32_t run = 0, maxc = 0;
    for (size_t k = t0; k < w.t1; ++k) {
      CHECK(w.offset[k - t0] == run);                    // offsets are prefix sums
      run += counts[k];
      if (counts[k] > maxc) maxc = counts[k];
    }
    CHECK(w.off == run && w.off <= chunk && w.maxc == maxc);
    CHECK(w.t1 == counts.size() || (uint64_t)w.off + counts[w.t1] > chunk);   // greedy: the next tile did not fit
    out.emplace_back(w.t1 - t0, w.off);
    t0 = w.t1;
  }
  return out;
}

static void sizing() {
  // an explicit chunk: nine tiles of 1024 samples, spp 4, chunk_paths 1024 -> nine waves of one tile
  const std::vector<uint32_t> nine(9, 1024u);
  const uint32_t c1 = wave_chunk(9 * 1024, 1024, 4, 1024, false, 0, 0, 560);
  CHECK(c1 == 1024);
  const auto w1 = waves_of(nine, c1);
  CHECK(w1.size() == 9);
  for (const auto& w : w1) CHECK(w.first == 1 && w.second == 1024);
  for (size_t t0 = 0; t0 < 9; ++t0) CHECK(next_wave(nine, t0, c1).offset == std::vector<uint32_t>{0u});
  // auto sizing: 5120 tiles of 1024 (5 242 880 paths) where 2^21 fit -> three equal waves plus a tile of slack
  const std::vector<uint32_t> many(5120, 1024u);
  const uint64_t total = 5120ull * 1024;
  const uint32_t c2 = wave_chunk(total, 1024, 4, 0, true, 2ull * 560 * (1u << 21), 0, 560);
  CHECK(c2 == 1747627u + 1024u && c2 == 1748651u);
  CHECK(wave_chunk(total, 1024, 4, 0, true, 560ull * (1u << 21), 560ull * (1u << 21), 560) == c2);   // free + held
  CHECK(wave_chunk(total, 1024, 4, 0, true, 2ull * 560 * (1u << 21) + 1119, 0, 560) == c2);          // fit == 2^21 still
  const auto w2 = waves_of(many, c2);
  CHECK(w2.size() == 3 && w2[0].first == 1707 && w2[1].first == 1707 && w2[2].first == 1706);
  // a pass that fits is one wave; little free memory still gives 2^20 paths
  CHECK(wave_chunk(total, 1024, 4, 0, true, 2ull * 560 * total, 0, 560) == total);
  CHECK(wave_chunk(1u << 20, 1024, 4, 0, true, 1, 0, 560) == (1u << 20));
  // no memory info: 2^22 at the most; the floor of 256 spp; the ceiling of 2^31
  CHECK(wave_chunk(1u << 23, 1024, 4, 0, false, 0, 0, 560) == (1u << 22));
  CHECK(wave_chunk(100, 100, 4, 0, false, 0, 0, 560) == 1024);
  CHECK(wave_chunk(100, 100, 4, 0, true, 1ull << 40, 0, 560) == 1024);
  CHECK(wave_chunk(100, 100, 4, 1, false, 0, 0, 560) == 1024);
  CHECK(wave_chunk(1ull << 33, 1024, 4, 0, true, 1ull << 60, 0, 560) == (1u << 31));
}

static void cuts() {
  const HalfCut a = half_cut(std::vector<uint32_t>(9, 1024u));         // the 5 / 4 cut of a 40 x 40 image
  CHECK(a.cut == 5 && a.nh[0] == 5120 && a.nh[1] == 4096 && a.maxc[0] == 1024 && a.maxc[1] == 1024);
  for (size_t k = 0; k < 9; ++k) CHECK(a.offset[k] == 1024u * (k < 5 ? k : k - 5));   // the second half restarts at 0
  const HalfCut b = half_cut({100u, 900u});                             // the second half is never empty
  CHECK(b.cut == 1 && b.nh[0] == 100 && b.nh[1] == 900 && b.offset[0] == 0 && b.offset[1] == 0);
  CHECK(b.maxc[0] == 100 && b.maxc[1] == 900);
  const HalfCut c = half_cut({900u, 100u});
  CHECK(c.cut == 1 && c.nh[0] == 900 && c.nh[1] == 100);
  const HalfCut d = half_cut({777u});                                   // one tile: nothing read past the end
  CHECK(d.cut == 0 && d.nh[0] == 0 && d.nh[1] == 777 && d.offset.size() == 1 && d.offset[0] == 0);
  const HalfCut e = half_cut({});
  CHECK(e.cut == 0 && e.nh[0] == 0 && e.nh[1] == 0 && e.offset.empty());
}

static void properties() {
  std::mt19937 rng(20240917u);
  for (int it = 0; it < 400; ++it) {
    std::vector<uint32_t> counts(1 + rng() % 200);
    for (auto& n : counts) n = 1 + rng() % 1024;
    const uint32_t chunk = 1024 + rng() % ((1u << 16) - 1024 + 1);
    uint64_t total = 0, seen = 0;
    size_t tiles = 0;
    for (uint32_t n : counts) total += n;
    for (const auto& w : waves_of(counts, chunk)) { tiles += w.first; seen += w.second; }
    CHECK(tiles == counts.size() && seen == total);      // the waves partition the list
    // the cut: the first boundary at or past half of the samples, each half's offsets its own prefix sums
    const HalfCut h = half_cut(counts);
    CHECK((uint64_t)h.nh[0] + h.nh[1] == total && h.cut < counts.size());
    if (counts.size() >= 2) {
      CHECK(h.cut >= 1);
      CHECK(2 * (uint64_t)h.nh[0] >= total || h.cut + 1 == counts.size());
      CHECK(2 * (uint64_t)(h.nh[0] - counts[h.cut - 1]) < total);
    }
    uint32_t run[2] = {0u, 0u}, maxc[2] = {0u, 0u};
    for (size_t k = 0; k < counts.size(); ++k) {
      const int s = k < h.cut ? 0 : 1;
      CHECK(h.offset[k] == run[s]);
      run[s] += counts[k];
      if (counts[k] > maxc[s]) maxc[s] = counts[k];
    }
    CHECK(run[0] == h.nh[0] && run[1] == h.nh[1] && maxc[0] == h.maxc[0] && maxc[1] == h.maxc[1]);
  }
  // a tile larger than the chunk: refused, where the loop would not have advanced
  bool threw = false;
  try { next_wave({512u, 2048u, 512u}, 1, 1024); } catch (const std::runtime_error&) { threw = true; }
  CHECK(threw);
  CHECK(next_wave({512u, 2048u, 512u}, 0, 1024).t1 == 1);
}

static void stats() {
  using pass_stats::StatsFold;
  // a: field k holds 1000 + 10 k, b: 2000 + k for the even fields, 3 + k for the odd ones, so that the
  // maximum comes from either side; the fields in the order of include/bling.h
  bling_stats a, b;
  const auto fill = [](bling_stats& s, int which) {
    int k = 0;
    const auto v = [&] { const int x = which == 0 ? 1000 + 10 * k : (k % 2 == 0 ? 2000 + k : 3 + k); ++k; return x; };
    s.camera_samples = v(); s.rays_camera = v(); s.rays_continuation = v(); s.rays_mis = v(); s.rays_shadow = v();
    s.dropped_samples = v(); s.tiles = v(); s.ms_total = v(); s.ms_bounce = v(); s.ms_film = v();
    s.bounce_launches = v(); s.path_vertices = v(); s.node_visits = v(); s.tri_tests = v(); s.shape_tests = v();
    s.ms_closest = v(); s.closest_launches = v(); s.march_ticks = v(); s.closest_node_visits = v();
    s.closest_tri_tests = v(); s.closest_shape_tests = v(); s.closest_march_ticks = v(); s.ms_shade = v();
    s.shade_launches = v();
  };
  fill(a, 0);
  fill(b, 1);
  // over passes: every field added
  bling_stats want;
  want.camera_samples = 1000 + 2000; want.rays_camera = 1010 + 4; want.rays_continuation = 1020 + 2002;
  want.rays_mis = 1030 + 6; want.rays_shadow = 1040 + 2004; want.dropped_samples = 1050 + 8; want.tiles = 1060 + 2006;
  want.ms_total = 1070 + 10; want.ms_bounce = 1080 + 2008; want.ms_film = 1090 + 12;
  want.bounce_launches = 1100 + 2010; want.path_vertices = 1110 + 14; want.node_visits = 1120 + 2012;
  want.tri_tests = 1130 + 16; want.shape_tests = 1140 + 2014; want.ms_closest = 1150 + 18;
  want.closest_launches = 1160 + 2016; want.march_ticks = 1170 + 20; want.closest_node_visits = 1180 + 2018;
  want.closest_tri_tests = 1190 + 22; want.closest_shape_tests = 1200 + 2020; want.closest_march_ticks = 1210 + 24;
  want.ms_shade = 1220 + 2022; want.shade_launches = 1230 + 26;
  bling_stats got = a;
  pass_stats::stats_add(got, b, StatsFold::Passes);
  CHECK(std::memcmp(&got, &want, sizeof got) == 0);
  // over devices: counts added, the four device times the larger one, the timed launches and the
  // wall clock the left operand's
  want.ms_total = 1070;
  want.ms_bounce = 2008; want.ms_film = 1090; want.ms_closest = 1150; want.ms_shade = 2022;
  want.closest_launches = 1160; want.shade_launches = 1230;
  got = a;
  pass_stats::stats_add(got, b, StatsFold::Devices);
  CHECK(std::memcmp(&got, &want, sizeof got) == 0);
  // and the other way round: the maxima stay, the kept fields are b's
  want.ms_total = 10; want.closest_launches = 2016; want.shade_launches = 26;
  got = b;
  pass_stats::stats_add(got, a, StatsFold::Devices);
  CHECK(std::memcmp(&got, &want, sizeof got) == 0);
}

int main() {
  sizing();
  cuts();
  properties();
  stats();
  std::printf("pass_plan: %d checks failed\n", fails);
  return fails ? 1 : 0;
}
