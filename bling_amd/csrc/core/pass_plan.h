// pass_plan.h -- the integer arithmetic of a render pass (core.hip render): the paths a wave holds, the
// cut of a pipelined pass into two half-waves, the tiles of the next wave.  Nothing of HIP in here:
// tests/cpp/pass_plan_check.cpp checks it on the CPU.  A tile is its sample count, in the pass's order.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <vector>

namespace pass_plan {

// Paths per wave, before the caller clamps it to the capacity it allocates.  chunk_paths > 0 is the
// caller's own size; otherwise the whole pass when it fits in half of the free HBM (C2: 67.7 M paths,
// ~33 GB of path state on a 288 GB MI355X) -- one wave means 8 launches per bounce in total instead of
// per chunk, and full-device waves at the deep bounces.  Never less than a tile (256 spp).
inline uint32_t wave_chunk(uint64_t total, uint32_t max_tile, uint32_t spp, int64_t chunk_paths, bool have_mem_info,
                           uint64_t free_bytes, uint64_t held_bytes, uint64_t path_bytes) {
  const auto min = [](uint64_t a, uint64_t b) { return a < b ? a : b; };
  uint64_t want = chunk_paths > 0 ? (uint64_t)chunk_paths : total;
  if (chunk_paths <= 0 && have_mem_info) {
    // half of (free + what the context already holds): the same answer on every pass, so a pass
    // never re-allocates the path state the previous one sized (C3: 140 GB per hipMalloc)
    uint64_t fit = (free_bytes + held_bytes) / 2 / path_bytes;
    if (fit < (1u << 20)) fit = 1u << 20;
    // equal waves, not full ones plus a small remainder; a tile of slack: waves are cut at tile boundaries
    const uint64_t waves = (total + fit - 1) / fit;
    if (want > fit) want = min(fit, (total + waves - 1) / waves + max_tile);
  } else if (chunk_paths <= 0) {
    want = min(want, 1u << 22);
  }
  want = min(want, (uint64_t)1 << 31);
  return (uint32_t)(want > 256u * (uint64_t)spp ? want : 256u * (uint64_t)spp);
}

// A pipelined pass's two half-waves: tiles [0, cut) and [cut, n), each half's sample ids from 0.  The cut
// is the first tile boundary at or past half of the paths; with two tiles or more the second half is
// never empty (the driver does not pipeline below that; one tile gives cut == 0).
struct HalfCut {
  size_t cut = 0;
  uint32_t nh[2] = {0u, 0u}, maxc[2] = {0u, 0u};   // samples and largest tile of each half
  std::vector<uint32_t> offset;                    // per tile, within its half
};
inline HalfCut half_cut(const std::vector<uint32_t>& counts) {
  HalfCut h;
  uint64_t total = 0, first = 0;
  for (uint32_t n : counts) total += n;
  while (h.cut + 1 < counts.size() && 2 * first < total) first += counts[h.cut++];
  for (size_t k = 0; k < counts.size(); ++k) {
    const int s = k < h.cut ? 0 : 1;
    h.offset.push_back(h.nh[s]);
    h.nh[s] += counts[k];
    if (counts[k] > h.maxc[s]) h.maxc[s] = counts[k];
  }
  return h;
}

// One wave of a pass that runs wave after wave: tiles [t0, t1), off samples, the largest of maxc.
// Greedy: whole tiles while they fit in chunk.  A tile larger than chunk would never be taken and the
// caller's loop would spin: wave_chunk's floor of 256 spp, at least a tile, rules that out, and
// next_wave throws if it ever stops holding.
struct Wave {
  size_t t1 = 0;
  uint32_t off = 0, maxc = 0;
  std::vector<uint32_t> offset;   // per tile of the wave
};
inline Wave next_wave(const std::vector<uint32_t>& counts, size_t t0, uint32_t chunk) {
  Wave w;
  for (w.t1 = t0; w.t1 < counts.size() && (uint64_t)w.off + counts[w.t1] <= chunk; ++w.t1) {
    w.offset.push_back(w.off);
    w.off += counts[w.t1];
    if (counts[w.t1] > w.maxc) w.maxc = counts[w.t1];
  }
  if (w.t1 == t0) throw std::runtime_error("a tile holds more samples than a wave");
  return w;
}

}  // namespace pass_plan
