// pass_stats.h -- the one table of bling_stats' fields and the two ways they are folded: over the
// passes of bling_render and over the devices of a fanned-out pass (core.hip render_fanout).
#pragma once
#include "../../../include/bling.h"

namespace pass_stats {

enum class StatsFold { Passes, Devices };
using S = bling_stats;
// counts: added either way
constexpr uint64_t S::* kCounts[] = {
    &S::camera_samples, &S::rays_camera, &S::rays_continuation, &S::rays_mis, &S::rays_shadow, &S::dropped_samples,
    &S::tiles, &S::bounce_launches, &S::path_vertices, &S::node_visits, &S::tri_tests, &S::shape_tests, &S::march_ticks,
    &S::closest_node_visits, &S::closest_tri_tests, &S::closest_shape_tests, &S::closest_march_ticks};
// device times: added over passes; over devices the slowest device's
constexpr double S::* kTimes[] = {&S::ms_bounce, &S::ms_film, &S::ms_closest, &S::ms_shade};
// added over passes; over devices the first device's (every device launches the same sequence, and the
// caller puts its own wall clock into ms_total)
constexpr uint64_t S::* kLaunches[] = {&S::closest_launches, &S::shade_launches};
constexpr double S::* kWall = &S::ms_total;
static_assert(sizeof(bling_stats) == 24 * 8, "a new field of bling_stats belongs in one of the lists above");
static_assert(sizeof kCounts / 8 + sizeof kTimes / 8 + sizeof kLaunches / 8 + 1 == 24, "every field once");

inline void stats_add(bling_stats& sum, const bling_stats& one, StatsFold how) {
  for (auto f : kCounts) sum.*f += one.*f;
  for (auto f : kTimes)
    if (how == StatsFold::Passes) sum.*f += one.*f;
    else if (one.*f > sum.*f) sum.*f = one.*f;
  if (how == StatsFold::Devices) return;
  for (auto f : kLaunches) sum.*f += one.*f;
  sum.*kWall += one.*kWall;
}

}  // namespace pass_stats
