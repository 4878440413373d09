// ordered_ranges_check.cpp -- the range loop of the ordered splat films (bling_amd/csrc/core/ordered_ranges.h)
// on the CPU.  A script says how many records each photon writes; a launch of a range claims their sum, whatever
// its buffer holds, as the device's record mode does.  The full sequences of launches (first, count, cap) and
// of accepted ranges (first, count, got) are compared with hand-derived lists, then their properties are checked
// over seeded random scripts.  Built and run by tests/test_ordered_ranges.py; exit status 0 = every check held.
#include <cstdio>
#include <numeric>
#include <random>
#include <tuple>
#include <vector>

#include "../../bling_amd/csrc/core/ordered_ranges.h"

static int fails = 0;
#define CHECK(x)                                                            \
  do {                                                                      \
    if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++fails; } \
  } while (0)

using Call = std::tuple<uint32_t, uint32_t, uint32_t>;
using Calls = std::vector<Call>;

struct Trace {
  Calls launches, accepts;   // (first, count, cap) and (first, count, got)
  std::string error;         // what() of the refusal, empty without one
};

// one sequence over the script w (records per photon), from and into cap
static Trace drive(const std::vector<uint32_t>& w, size_t budget, uint32_t& cap, const char* who = "light tracer: photon ",
                   const char* of = "") {
  Trace t;
  try {
    ordered_ranges::run(
        (uint32_t)w.size(), budget, cap,
        [&](uint32_t first, uint32_t count, uint32_t c) {
          t.launches.emplace_back(first, count, c);
          return std::accumulate(w.begin() + first, w.begin() + first + count, 0u);
        },
        [&](uint32_t first, uint32_t count, uint32_t got) { t.accepts.emplace_back(first, count, got); },
        [&](uint32_t photon) { return who + std::to_string(photon) + of; });
  } catch (const std::invalid_argument& e) {
    t.error = e.what();
  }
  return t;
}

static void by_hand() {
  // the starting capacity: four records per photon and 1024, or what the buffer holds, within the budget
  CHECK(ordered_ranges::initial_cap(1u << 20, 0, 100) == 4 * 100 + 1024);
  CHECK(ordered_ranges::initial_cap(1u << 20, 5000, 100) == 5000);
  CHECK(ordered_ranges::initial_cap(300, 5000, 100) == 300);
  CHECK(ordered_ranges::initial_cap(1, 0, 0) == 1);
  CHECK(ordered_ranges::initial_cap(0x7FFFFFFFull, 0, 0xFFFFFFFFu) == 0x7FFFFFFFu);   // 4 total does not wrap

  {  // no photons: no launch
    uint32_t cap = 8;
    const Trace t = drive({}, 100, cap);
    CHECK(t.launches.empty() && t.accepts.empty() && t.error.empty() && cap == 8);
  }
  {  // everything fits: one launch, one accept of [0, total)
    uint32_t cap = 100;
    const Trace t = drive(std::vector<uint32_t>(10, 1u), 1000, cap);
    CHECK((t.launches == Calls{{0, 10, 100}}));
    CHECK((t.accepts == Calls{{0, 10, 10}}));
    CHECK(t.error.empty() && cap == 100);
  }
  {  // cap < got <= budget: the same range once more with cap == got, and cap is kept for the next sequence
    uint32_t cap = 20;
    const Trace t = drive(std::vector<uint32_t>(10, 3u), 100, cap);
    CHECK((t.launches == Calls{{0, 10, 20}, {0, 10, 30}}));
    CHECK((t.accepts == Calls{{0, 10, 30}}));
    CHECK(cap == 30);
    const Trace u = drive(std::vector<uint32_t>(4, 2u), 100, cap);   // SPPM's next sampler
    CHECK((u.launches == Calls{{0, 4, 30}}));
    CHECK((u.accepts == Calls{{0, 4, 8}}));
    CHECK(cap == 30);
  }
  {  // got > budget on a range of 5: 3, then the 2 that are left
    uint32_t cap = 4;
    const Trace t = drive(std::vector<uint32_t>(5, 1u), 4, cap);
    CHECK((t.launches == Calls{{0, 5, 4}, {0, 3, 4}, {3, 2, 4}}));
    CHECK((t.accepts == Calls{{0, 3, 3}, {3, 2, 2}}));
    CHECK(t.error.empty() && cap == 4);
  }
  {  // 10 -> 5 -> 3, and the length stays 3 for what follows
    uint32_t cap = 4;
    const Trace t = drive(std::vector<uint32_t>(10, 1u), 4, cap);
    CHECK((t.launches == Calls{{0, 10, 4}, {0, 5, 4}, {0, 3, 4}, {3, 3, 4}, {6, 3, 4}, {9, 1, 4}}));
    CHECK((t.accepts == Calls{{0, 3, 3}, {3, 3, 3}, {6, 3, 3}, {9, 1, 1}}));
  }
  {  // the length stays short even where a longer range would fit again: four heavy photons, then four that write nothing
    uint32_t cap = 8;
    const Trace t = drive({4, 4, 4, 4, 0, 0, 0, 0}, 8, cap);
    CHECK((t.launches == Calls{{0, 8, 8}, {0, 4, 8}, {0, 2, 8}, {2, 2, 8}, {4, 2, 8}, {6, 2, 8}}));
    CHECK((t.accepts == Calls{{0, 2, 8}, {2, 2, 8}, {4, 2, 0}, {6, 2, 0}}));
  }
  {  // a range is retried into the larger buffer before any halving, and halved only beyond the budget
    uint32_t cap = 2;
    const Trace t = drive(std::vector<uint32_t>(4, 2u), 5, cap);
    CHECK((t.launches == Calls{{0, 4, 2}, {0, 2, 2}, {0, 2, 4}, {2, 2, 4}}));
    CHECK((t.accepts == Calls{{0, 2, 4}, {2, 2, 4}}));
    CHECK(cap == 4);
  }
  {  // nested halving down to single photons
    uint32_t cap = 1;
    const Trace t = drive(std::vector<uint32_t>(8, 1u), 1, cap);
    CHECK((t.launches == Calls{{0, 8, 1}, {0, 4, 1}, {0, 2, 1}, {0, 1, 1}, {1, 1, 1}, {2, 1, 1}, {3, 1, 1}, {4, 1, 1}, {5, 1, 1},
                               {6, 1, 1}, {7, 1, 1}}));
    Calls each;
    for (uint32_t i = 0; i < 8; ++i) each.emplace_back(i, 1u, 1u);
    CHECK(t.accepts == each);
  }
  {  // an odd length halves upwards: 7 -> 4, then the 3 that are left
    uint32_t cap = 1;
    const Trace t = drive({1, 0, 0, 0, 0, 0, 1}, 1, cap);
    CHECK((t.launches == Calls{{0, 7, 1}, {0, 4, 1}, {4, 3, 1}}));
    CHECK((t.accepts == Calls{{0, 4, 1}, {4, 3, 1}}));
  }
  {  // one photon beyond the budget: refused with its index and the budget, and never accepted
    uint32_t cap = 2;
    const Trace t = drive({1, 1, 5, 1}, 2, cap);
    CHECK((t.launches == Calls{{0, 4, 2}, {0, 2, 2}, {2, 2, 2}, {2, 1, 2}}));
    CHECK((t.accepts == Calls{{0, 2, 2}}));
    CHECK(t.error == "light tracer: photon 2 alone writes 5 splat records, more than the record budget 2");
    CHECK(t.error.find("alone writes") != std::string::npos && t.error.find("budget 2") != std::string::npos);
    uint32_t cap2 = 1;
    const Trace u = drive({3}, 1, cap2, "sppm: photon ", " of sampler 3");
    CHECK((u.launches == Calls{{0, 1, 1}}) && u.accepts.empty());
    CHECK(u.error == "sppm: photon 0 of sampler 3 alone writes 3 splat records, more than the record budget 1");
  }
  {  // two sequences share cap, as SPPM's samplers do: the second starts in the buffer the first grew
    uint32_t cap = 5;
    const Trace a = drive(std::vector<uint32_t>(4, 3u), 100, cap);
    CHECK((a.launches == Calls{{0, 4, 5}, {0, 4, 12}}));
    CHECK((a.accepts == Calls{{0, 4, 12}}));
    const Trace b = drive(std::vector<uint32_t>(4, 2u), 100, cap);
    CHECK((b.launches == Calls{{0, 4, 12}}));
    CHECK((b.accepts == Calls{{0, 4, 8}}));
    CHECK(cap == 12);
    // but the halved length is the sequence's own: the next one starts from its whole length again
    uint32_t c2 = 2;
    const Trace d = drive({1, 1, 1, 1}, 2, c2);
    const Trace e = drive({0, 0, 1, 1}, 2, c2);
    CHECK((d.launches == Calls{{0, 4, 2}, {0, 2, 2}, {2, 2, 2}}));
    CHECK((e.launches == Calls{{0, 4, 2}}));
  }
}

// Over random scripts: the accepted ranges are ascending, disjoint and cover [0, total) exactly once (up to the
// refused photon, where there is one); every accepted got is the range's own sum and got <= cap <= budget; cap
// never shrinks and a sequence's ranges never grow; a range is launched again only after it did not fit.
static void properties() {
  int refused = 0, grown = 0, halved = 0;
  for (uint32_t seed = 1; seed <= 48; ++seed) {
    std::mt19937 rng(seed);
    const uint32_t total = rng() % 200;
    const size_t budget = 1 + rng() % (seed % 3 ? 64 : 1024);
    std::vector<uint32_t> w(total);
    for (uint32_t& x : w) x = rng() % 7 == 0 ? rng() % 40 : rng() % 5;
    uint32_t cap = (uint32_t)(rng() % (budget + 1));
    for (int sequence = 0; sequence < 2; ++sequence) {      // the second one starts from the first one's cap
      const uint32_t cap0 = cap;
      std::vector<uint32_t> caps;                            // cap at each accept
      Trace t;
      try {
        ordered_ranges::run(
            total, budget, cap,
            [&](uint32_t first, uint32_t count, uint32_t c) {
              t.launches.emplace_back(first, count, c);
              return std::accumulate(w.begin() + first, w.begin() + first + count, 0u);
            },
            [&](uint32_t first, uint32_t count, uint32_t got) { t.accepts.emplace_back(first, count, got); caps.push_back(cap); },
            [](uint32_t photon) { return "photon " + std::to_string(photon); });
      } catch (const std::invalid_argument& e) {
        t.error = e.what();
      }
      uint32_t next = 0;
      for (size_t k = 0; k < t.accepts.size(); ++k) {
        const auto [first, count, got] = t.accepts[k];
        CHECK(first == next && count >= 1 && first + count <= total);
        CHECK(got == std::accumulate(w.begin() + first, w.begin() + first + count, 0u));
        CHECK(got <= caps[k] && caps[k] <= budget);
        next = first + count;
      }
      if (t.error.empty()) {
        CHECK(next == total);
        for (uint32_t x : w) CHECK(x <= budget);
      } else {
        ++refused;
        CHECK(next < total && w[next] > budget);             // everything before the refused photon, nothing of it
        CHECK(t.error.find("photon " + std::to_string(next) + " alone writes " + std::to_string(w[next])) != std::string::npos);
        CHECK(t.error.find("budget " + std::to_string(budget)) != std::string::npos);
        CHECK((t.launches.back() == Call{next, 1u, cap}));
      }
      uint32_t c_prev = cap0, n_prev = total;
      for (size_t k = 0; k < t.launches.size(); ++k) {
        const auto [first, count, c] = t.launches[k];
        CHECK(c >= c_prev && c <= std::max<size_t>(budget, cap0) && count <= n_prev && count >= 1);
        if (k > 0 && first == std::get<0>(t.launches[k - 1])) {   // the range before it did not fit
          const auto [pf, pn, pc] = t.launches[k - 1];
          const uint32_t pgot = std::accumulate(w.begin() + pf, w.begin() + pf + pn, 0u);
          CHECK(pgot > pc);
          if (pgot <= budget) { CHECK(count == pn && c == pgot); ++grown; }
          else { CHECK(c == pc && count == std::min((pn + 1) / 2, total - first)); ++halved; }
        }
        c_prev = c; n_prev = count;
      }
      CHECK(cap == c_prev);
    }
  }
  CHECK(refused > 0 && grown > 0 && halved > 0);             // the scripts reach every branch
}

int main() {
  by_hand();
  properties();
  std::printf("ordered_ranges: %d checks failed\n", fails);
  return fails ? 1 : 0;
}
