// scene_plan.h -- what a scene description becomes before any device sees it, in three host-only stages:
//   validate_scene   everything the later stages and the kernels assume of a description
//   scene_items      triangle records, the primitives' boxes and refs in reference order, world bounds
//   scene_derive     everything after the BVH2 (built by either builder, scene_upload.hip): leaf records, BVH4,
//                    threaded list, the LDS plans and kernel switches, shape records, light tables and the
//                    scalar half of DevScene; scene_plan_counts is its second half, which the sizes alone decide
// scene_plan.cpp makes no HIP runtime call: bling_debug_scene_plan answers on a machine without a GPU, and a
// multi-device upload derives once and copies the one plan to every device.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../../include/bling.h"
#include "bvh_build.h"
#include "dev_scene.h"

namespace bplan {

struct SceneItems {
  std::vector<float4> geo;                    // tri_geo: 3 float4 per triangle (dev_scene.h)
  std::vector<float> pts;                     // 9 floats per triangle, for the shading frames
  std::vector<int32_t> tri_prim, shape_prim;  // triangle / shape -> reference primitive id
  int32_t fractal_prim = -1;
  std::vector<bvh::Box> boxes;                // BVH items in reference order ...
  std::vector<uint32_t> refs;                 // ... and their leaf reference words
  float world_c[3], world_r, kd_lo[3], kd_hi[3];   // the reference kd-tree's worldBounds and their sphere
};

// What bling_debug_scene_info and bling_debug_scene_plan print.
struct PlanSummary {
  uint32_t prims = 0;
  int bvh_depth = 0, bvh_leaves = 0, max_leaf = 0, bvh4_depth = 0;
  uint32_t bvh4_nodes = 0, stack4_need = 0, stack4_lds = 0;
  bool lds_all4 = false;
  size_t lds_trace4 = 0;
  uint32_t pkt_n = 0, bf_prims = 0, features = 0, lds4_shapes = 0, lds4_tris = 0, lds4_nodes = 0, sample_major = 0;
};

// An infinite light's CDFs, each row with its guide table behind it; marg ends in the three Perez denominators.
struct LightTables { std::vector<float> rows, marg; };

struct ScenePlan {
  SceneItems items;                   // geo, pts, tri_prim, shape_prim; boxes and refs are freed (the tree holds them)
  bvh::Result bvh2;
  std::vector<float4> leaf_geo;       // primitive records in leaf order (dev_trace.h LeafRec)
  std::vector<float> nodes4, pkt;     // bvh::collapse4, bvh::threaded
  std::vector<bd::DevShape> shapes;
  std::vector<LightTables> tables;    // one per light; empty unless the light is infinite
  bd::DevScene S{};                   // every field but the device pointers and stack4_lanes
  size_t lds_trace = 0;               // dynamic LDS bytes of the BVH2 traversal kernels (the BVH4's: info)
  bool lds_all = false;               // the whole BVH2, triangle set and leaf refs are LDS-resident
  bool mis_cull_ok = false;           // every shape that carries an area light is that light's own shape
  PlanSummary info;                   // with scene_features() of the description and the BVH4 plan's LDS bytes
};

// The sizes of the two trees and the threaded list: all the plan needs of them.
struct DeriveCounts {
  uint32_t n2 = 0, nrefs = 0;                       // BVH2 nodes, leaf refs
  int bvh_depth = 0, bvh_leaves = 0, max_leaf = 0;  // bvh::Result
  uint32_t n4 = 0;                                  // BVH4 nodes ...
  int bvh4_depth = 0, stack_need = 0;               // ... and bvh::Result4
  uint32_t pkt_entries = 0;                         // entries of the threaded list (0: none was derived)
};

void validate_scene(const bling_scene_desc* d);
SceneItems scene_items(const bling_scene_desc& d);
// consumes the items and the tree: their arrays move into the plan
ScenePlan scene_derive(const bling_scene_desc& d, SceneItems&& items, bvh::Result&& bvh2);
// the part of scene_derive that needs the counts alone: the LDS plans, the packet and brute switches, shape records,
// light tables, the scalar half of DevScene and the summary.  scene_derive ends in it; an upload that derives the
// arrays on the device (bvh_derive.hip) calls it with the counts read back.  bvh2, leaf_geo, nodes4 and pkt stay empty.
ScenePlan scene_plan_counts(const bling_scene_desc& d, SceneItems&& items, const DeriveCounts& k);
// the BVH2 of the items by the host's binned SAH, as every upload that does not use the device builder builds it
bvh::Result host_bvh2(const SceneItems& items);
// the summary as the JSON object of bling_debug_scene_info and bling_debug_scene_plan
std::string summary_json(const PlanSummary& p);

}  // namespace bplan
