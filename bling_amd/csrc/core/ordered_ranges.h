// ordered_ranges.h -- the range loop of the ordered splat films (the light tracer's and SPPM's ordered passes,
// splat_renderers.hip and sppm_pass.hip): a sequence of photons is launched in record mode over ascending
// ranges, each taken over before the next.  Nothing of HIP in here: tests/cpp/ordered_ranges_check.cpp checks
// it on the CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>

namespace ordered_ranges {

// The record capacity a pass starts with: what the record buffer already holds (`held` records) or four
// records per photon of a sequence and some slack, whichever is more, within the budget.
inline uint32_t initial_cap(size_t budget, size_t held, uint32_t total) {
  return (uint32_t)std::min<size_t>(budget, std::max<size_t>(held, (size_t)4 * total + 1024));
}

// Photons [0, total) as ascending ranges.  launch(first, count, cap) runs a range into a buffer of cap records
// and returns the records it claimed; accept(first, count, got) takes a range over, once per range that fit.
// A range that claimed more than cap is run again: into a buffer that holds it (cap only grows, and stays with
// the caller for its next sequence) or, beyond the budget, as two halves -- and the shorter length holds for
// the rest of the sequence.  Nothing of a range is accepted before it fits.  A single photon beyond the budget
// throws std::invalid_argument; name(first) says which photon that is ("light tracer: photon 7").
template <class Launch, class Accept, class Name>
void run(uint32_t total, size_t budget, uint32_t& cap, Launch&& launch, Accept&& accept, Name&& name) {
  uint32_t first = 0, len = total;
  while (first < total) {
    const uint32_t count = std::min(len, total - first);
    const uint32_t got = launch(first, count, cap);
    if (got > cap) {
      if ((size_t)got <= budget) { cap = got; continue; }              // the same range, into a buffer that holds it
      if (count == 1)
        throw std::invalid_argument(name(first) + " alone writes " + std::to_string(got) +
                                    " splat records, more than the record budget " + std::to_string(budget));
      len = (count + 1) / 2;
      continue;
    }
    accept(first, count, got);
    first += count;
  }
}

}  // namespace ordered_ranges
