// scene_upload.hip -- a scene plan (scene_plan.h) onto the devices of a context: the BVH2 by the builder asked
// for, the plan's arrays into device buffers (or derived there: derive_on_device), the pointer half of DevScene,
// and the entry points around them.
// Every decision about the scene is the plan's; what is settled here needs a device (the shading frames'
// kernel, the device builder, the BVH4 overflow rows sized by the CU count).
#include "core_internal.h"
#include "../common/bvh4.h"

#include <chrono>

using namespace bd;
using namespace bcore;

namespace {

// one thread per triangle: its shading frame (dev_shade.h tri_frame_build)
__global__ void k_tri_frames(const float* __restrict__ pts, const float* __restrict__ uvs, float4* __restrict__ out,
                             uint32_t n) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) tri_frame_build(pts + (size_t)9 * t, uvs + (size_t)6 * t, out + (size_t)4 * t);
}

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// The BVH2 of the items by the builder asked for (BLING_BVH_*), and how it came about.  The device builder
// (bvh_device.hip) stands down for what bling.h lists; the host's binned SAH then builds as it always did.
// With n_kept, a tree the device builder made stays in c->nodes / c->refs (lbvh_build_device): *n_kept receives its
// node count and R holds its depth, leaves and max_leaf alone; *n_kept stays 0 when the host built the tree.
bvh::Result build_bvh2(bling_ctx* c, const bplan::SceneItems& items, uint32_t builder, bling_bvh_build_info* info,
                       uint32_t* n_kept = nullptr) {
  const std::vector<bvh::Box>& boxes = items.boxes;
  *info = bling_bvh_build_info{};
  info->requested = info->used = builder;
  info->items = (uint32_t)boxes.size();
  bvh::Result R;
  if (builder == BLING_BVH_DEVICE) {
    const int cap = c->bvh_depth_cap ? c->bvh_depth_cap : STACK_DEPTH - 1;
    if (items.fractal_prim >= 0) info->fallback = BLING_BVH_FALLBACK_FRACTAL;
    else if (boxes.size() < 3) info->fallback = BLING_BVH_FALLBACK_ITEMS;
    else if (boxes.size() > ((size_t)1 << 24)) info->fallback = BLING_BVH_FALLBACK_REFS;
    else {
      float ms = 0.f;
      int depth = 0;
      HIPCHK(hipSetDevice(c->device));
      if (lbvh_build_device(c, boxes, items.refs, cap, R, &ms, &depth, n_kept)) { info->ms_build = ms; return R; }
      info->fallback = BLING_BVH_FALLBACK_DEPTH;
    }
    info->used = BLING_BVH_HOST;
  }
  const auto t0 = std::chrono::steady_clock::now();
  R = bplan::host_bvh2(items);
  info->ms_build = ms_since(t0);
  return R;
}

// The plan's arrays and the description's records into c's device buffers, and DevScene with their addresses.
// on_device: the triangle records, the BVH2, its refs, the leaf records and the BVH4 are in c's buffers already
// (derive_on_device); the plan holds none of the last four.
void upload_plan(bling_ctx* c, const bling_scene_desc* d, const bplan::ScenePlan& P, bool on_device = false) {
  HIPCHK(hipSetDevice(c->device));
  const uint32_t nt = d->num_triangles;
  DevScene& S = c->S;
  S = P.S;
  if (!on_device) c->tri_geo.upload(P.items.geo.data(), P.items.geo.size());
  {                                   // per-triangle shading frames (dev_shade.h tri_frame_build)
    DBuf<float> dpts, duvs;
    dpts.upload(P.items.pts.data(), P.items.pts.size());
    duvs.upload(d->tri_uvs, (size_t)6 * nt);
    c->tri_frame.alloc((size_t)4 * nt);
    if (nt) {
      k_tri_frames<<<(nt + 255) / 256, 256, 0, c->stream>>>(dpts.p, duvs.p, c->tri_frame.p, nt);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(c->stream));
    }
  }
  c->tri_material.upload(d->tri_material, nt);
  if (d->tri_normals && d->tri_has_normals) {
    c->tri_normals.upload(d->tri_normals, (size_t)9 * nt);
    c->tri_has_n.upload(d->tri_has_normals, nt);
  } else { c->tri_normals.free(); c->tri_has_n.free(); }
  if (!on_device) {
    c->nodes.upload(reinterpret_cast<const float4*>(P.bvh2.nodes.data()), P.bvh2.nodes.size() / 4);
    c->refs.upload(P.bvh2.refs.data(), P.bvh2.refs.size());
    c->leaf_geo.upload(P.leaf_geo.data(), P.leaf_geo.size());
    c->nodes4.upload(reinterpret_cast<const float4*>(P.nodes4.data()), P.nodes4.size() / 4);
  }
  S.stack4_lanes = 0;
  if (S.stack4_need > S.stack4_lds) {
    int cus = 256;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess) cus = 256;
    S.stack4_lanes = (uint32_t)cus * 2048u;           // every resident lane of a persistent grid
    c->stack4_ovf.alloc((size_t)(S.stack4_need - S.stack4_lds) * S.stack4_lanes);
  } else {
    c->stack4_ovf.free();
  }
  c->pkt.upload(reinterpret_cast<const float4*>(P.pkt.data()), P.pkt.size() / 4);
  c->tri_prim.upload(P.items.tri_prim.data(), P.items.tri_prim.size());
  c->shape_prim.upload(P.items.shape_prim.data(), P.items.shape_prim.size());
  c->shapes.upload(P.shapes.data(), P.shapes.size());
  c->materials.upload(d->materials, d->num_materials);
  c->textures.upload(d->textures, d->num_textures);
  c->stex.upload(d->scalar_textures, d->num_scalar_textures);
  // --- lights and texture images: the tables' pointers rewritten to device copies
  c->light_arrays.clear();
  auto up = [&](const float* h, size_t n) -> const float* {
    if (!h || !n) return nullptr;
    c->light_arrays.emplace_back(new DBuf<float>());
    c->light_arrays.back()->upload(h, n);
    return c->light_arrays.back()->p;
  };
  std::vector<bling_light> lights(d->lights, d->lights + d->num_lights);
  for (size_t k = 0; k < lights.size(); ++k) {
    bling_light& l = lights[k];
    if (l.kind != BLING_LIGHT_INFINITE) continue;
    const size_t nu = l.dist_nu, nv = l.dist_nv;
    if (l.env_kind == BLING_ENV_IMAGE) l.env_texels = up(l.env_texels, (size_t)l.env_w * l.env_h * 16);
    l.dist_func = up(l.dist_func, nu * nv);
    l.dist_cdf = up(P.tables[k].rows.data(), P.tables[k].rows.size());
    l.dist_func_int = up(l.dist_func_int, nv);
    l.marg_func = up(l.marg_func, nv);
    l.marg_cdf = up(P.tables[k].marg.data(), P.tables[k].marg.size());
  }
  c->lights.upload(lights.data(), lights.size());
  std::vector<bling_image> images(d->images, d->images + d->num_images);
  for (auto& im : images) im.texels = up(im.texels, (size_t)im.width * im.height * im.channels);
  c->images.upload(images.data(), images.size());
  // --- DevScene's pointers
  S.nodes = as_global(c->nodes.p); S.leaf_refs = as_global(c->refs.p); S.leaf_geo = as_global(c->leaf_geo.p);
  S.nodes4 = as_global(c->nodes4.p); S.stack4_ovf = c->stack4_ovf.p;
  S.pkt = as_global(c->pkt.p);
  S.tri_geo = as_global(c->tri_geo.p); S.tri_frame = as_global(c->tri_frame.p);
  S.tri_normals = as_global(c->tri_normals.p); S.tri_has_n = as_global(c->tri_has_n.p);
  S.tri_material = as_global(c->tri_material.p); S.tri_prim = as_global(c->tri_prim.p);
  S.shapes = as_global(c->shapes.p);
  S.materials = as_global(c->materials.p); S.textures = as_global(c->textures.p); S.stex = as_global(c->stex.p); S.lights = as_global(c->lights.p);
  S.images = as_global(c->images.p);
  c->plan_info = P.info;
  c->features = P.info.features;
  c->lds_trace = P.lds_trace; c->lds_all = P.lds_all;
  c->lds_trace4 = P.info.lds_trace4; c->lds_all4 = P.info.lds_all4;
  c->mis_cull_ok = P.mis_cull_ok;
  c->counters.alloc(1);
  c->dscene.upload(&S, 1);
  c->film_dev.free();
  c->cfg = d->config;
  c->lt = d->light;
  c->mp = d->metropolis;
  c->sppm.free_all();
  c->light.free_all();
  c->mlt.free_all();
  c->merge.free_all();                   // the record budget stays: it belongs to the context
  c->mlt_boot_override.clear();
}

// BLING_UPLOAD_DERIVE_DEVICE: the BVH2 by the builder asked for, left or put on the device; leaf records and BVH4
// derived there (bvh_derive.hip); the counts back; the plan from the counts.  The threaded list alone is made on
// the host, from a BVH2 small enough to have one worth walking (bling.h).
bplan::ScenePlan derive_on_device(bling_ctx* c, const bling_scene_desc* d, bplan::SceneItems&& items, uint32_t builder,
                                  bling_bvh_build_info* info, bling_derive_info* di) {
  HIPCHK(hipSetDevice(c->device));
  uint32_t n_kept = 0;
  bvh::Result R = build_bvh2(c, items, builder, info, &n_kept);
  const auto t_derive = std::chrono::steady_clock::now();
  bplan::DeriveCounts k;
  if (!n_kept && R.nodes.empty()) {                    // nothing to derive from: the host derivation's empty plan
    di->used = BLING_DERIVE_HOST; di->fallback = BLING_DERIVE_FALLBACK_NODES;
    bplan::ScenePlan P = bplan::scene_derive(*d, std::move(items), std::move(R));
    di->ms_plan_host = info->ms_derive = ms_since(t_derive);
    return P;
  }
  if (n_kept) {
    k.n2 = n_kept; k.nrefs = (uint32_t)c->refs.n;
  } else {                                             // a host tree (asked for, or the device builder stood down): up once
    k.n2 = (uint32_t)(R.nodes.size() / 16); k.nrefs = (uint32_t)R.refs.size();
    c->nodes.upload(reinterpret_cast<const float4*>(R.nodes.data()), R.nodes.size() / 4);
    c->refs.upload(R.refs.data(), R.refs.size());
  }
  k.bvh_depth = R.depth; k.bvh_leaves = R.leaves; k.max_leaf = R.max_leaf;
  if (R.depth > STACK_DEPTH - 1) throw std::runtime_error("BVH deeper than the traversal stack");
  c->tri_geo.upload(items.geo.data(), items.geo.size());
  bvh_derive_device(c, d->num_triangles, k, di);
  const auto t_plan = std::chrono::steady_clock::now();
  std::vector<float> pkt;
  if (k.n2 <= bbvh4::kThreadedMaxNodes) {
    bvh::Result small;
    small.nodes.resize((size_t)16 * k.n2);
    HIPCHK(hipMemcpy(small.nodes.data(), c->nodes.p, small.nodes.size() * sizeof(float), hipMemcpyDeviceToHost));
    pkt = bvh::threaded(small);
  }
  k.pkt_entries = (uint32_t)(pkt.size() / 8);
  bplan::ScenePlan P = bplan::scene_plan_counts(*d, std::move(items), k);
  P.pkt = std::move(pkt);
  di->ms_plan_host = ms_since(t_plan);
  info->nodes = k.n2;
  info->depth = (uint32_t)k.bvh_depth; info->leaves = (uint32_t)k.bvh_leaves; info->max_leaf = (uint32_t)k.max_leaf;
  info->ms_derive = ms_since(t_derive);
  return P;
}

// a link of a BVH2 handed to bling_host_bvh4 / bling_host_threaded names a node of the array, no node is named twice
// and none names the root: what is reached from the root is then a tree.  Returns it as a bvh::Result.
bvh::Result checked_bvh2(const float* nodes2, size_t n2) {
  if (!nodes2 || n2 < 1 || n2 > ((size_t)1 << 25)) throw std::invalid_argument("BVH2: no nodes, or more than 2^25");
  std::vector<uint8_t> named(n2, 0);
  for (size_t i = 0; i < n2; ++i)
    for (int cidx = 0; cidx < 2; ++cidx) {
      int32_t link;
      std::memcpy(&link, nodes2 + 16 * i + 12 + cidx, 4);
      if (link < 0) continue;
      if (link == 0 || (size_t)link >= n2 || named[link]) throw std::invalid_argument("BVH2: a link names the root, no node, or a node named before");
      named[link] = 1;
    }
  // depth from the root, breadth-first: the threaded list is made by recursion
  std::vector<int32_t> q{0}, lvl{1};
  for (size_t h = 0; h < q.size(); ++h)
    for (int cidx = 0; cidx < 2; ++cidx) {
      int32_t link;
      std::memcpy(&link, nodes2 + 16 * (size_t)q[h] + 12 + cidx, 4);
      if (link < 0) continue;
      if (lvl[h] >= 64) throw std::invalid_argument("BVH2: deeper than 64 levels");
      q.push_back(link); lvl.push_back(lvl[h] + 1);
    }
  bvh::Result R;
  R.nodes.assign(nodes2, nodes2 + 16 * n2);
  return R;
}

// a text result of the C ABI: NUL-terminated into buf (at most size bytes), the full length into *len
void put_text(const std::string& s, char* buf, size_t size, size_t* len) {
  if (len) *len = s.size();
  if (buf && size) { std::strncpy(buf, s.c_str(), size - 1); buf[size - 1] = '\0'; }
}

}  // namespace

extern "C" {

int bling_scene_upload_with(bling_ctx* c, const bling_scene_desc* d, const bling_upload_params* up) {
  return guarded([&] {
    if (!c || !d || !up) throw std::invalid_argument("null argument");
    if (up->bvh_builder != BLING_BVH_HOST && up->bvh_builder != BLING_BVH_DEVICE) throw std::invalid_argument("unknown BVH builder");
    if (up->flags & ~BLING_UPLOAD_DERIVE_DEVICE) throw std::invalid_argument("unknown upload flags");
    bplan::validate_scene(d);
    // no pass may mix a new scene on one device with an old or half-uploaded one on another: the
    // context and every peer lose their scene first and get it back only once all uploads succeeded
    c->has_scene = false;
    for (auto& q : c->peers) q->has_scene = false;
    // the BVH2 is built once, on the first device, and the plan derived once; every device gets that plan
    bplan::SceneItems items = bplan::scene_items(*d);
    bling_bvh_build_info info{};
    bling_derive_info di{};
    if (up->flags & BLING_UPLOAD_DERIVE_DEVICE) {
      di.requested = BLING_DERIVE_DEVICE;
      if (items.fractal_prim >= 0) di.fallback = BLING_DERIVE_FALLBACK_FRACTAL;
      else if (!c->peers.empty()) di.fallback = BLING_DERIVE_FALLBACK_DEVICES;
      else {
        di.used = BLING_DERIVE_DEVICE;
        const bplan::ScenePlan P = derive_on_device(c, d, std::move(items), up->bvh_builder, &info, &di);
        upload_plan(c, d, P, di.used == BLING_DERIVE_DEVICE);
        c->bvh_info = info;
        c->derive_info = di;
        c->has_scene = true;
        return BLING_OK;
      }
    }
    bvh::Result R = build_bvh2(c, items, up->bvh_builder, &info);
    const auto t_derive = std::chrono::steady_clock::now();
    const bplan::ScenePlan P = bplan::scene_derive(*d, std::move(items), std::move(R));
    info.nodes = (uint32_t)(P.bvh2.nodes.size() / 16);
    info.depth = (uint32_t)P.bvh2.depth; info.leaves = (uint32_t)P.bvh2.leaves; info.max_leaf = (uint32_t)P.bvh2.max_leaf;
    info.ms_derive = ms_since(t_derive);
    di.bvh4_nodes = P.info.bvh4_nodes; di.bvh4_depth = (uint32_t)P.info.bvh4_depth; di.stack_need = P.info.stack4_need;
    di.ms_plan_host = info.ms_derive;
    upload_plan(c, d, P);
    for (auto& q : c->peers) upload_plan(q.get(), d, P);   // replicated scene (8e)
    HIPCHK(hipSetDevice(c->device));
    c->bvh_info = info;
    c->derive_info = di;
    for (auto& q : c->peers) { q->bvh_info = info; q->derive_info = di; q->has_scene = true; }
    c->has_scene = true;
    return BLING_OK;
  });
}

int bling_scene_upload(bling_ctx* c, const bling_scene_desc* d) {
  const bling_upload_params up{BLING_BVH_HOST, 0u};
  return bling_scene_upload_with(c, d, &up);
}

int bling_scene_validate(const bling_scene_desc* d) {
  return guarded([&] {
    bplan::validate_scene(d);
    return BLING_OK;
  });
}

int bling_debug_scene_plan(const bling_scene_desc* d, char* buf, size_t size, size_t* len) {
  return guarded([&] {
    bplan::validate_scene(d);
    bplan::SceneItems items = bplan::scene_items(*d);
    bvh::Result R = bplan::host_bvh2(items);
    put_text(bplan::summary_json(bplan::scene_derive(*d, std::move(items), std::move(R)).info), buf, size, len);
    return BLING_OK;
  });
}

int bling_debug_scene_info(bling_ctx* c, char* buf, size_t size, size_t* len) {
  return guarded([&] {
    if (!c) throw std::invalid_argument("null argument");
    if (!c->has_scene) throw std::invalid_argument("no scene uploaded");
    put_text(bplan::summary_json(c->plan_info), buf, size, len);
    return BLING_OK;
  });
}

int bling_debug_bvh(bling_ctx* c, float* nodes, size_t cap_nodes, uint32_t* refs, size_t cap_refs, size_t* n_nodes, size_t* n_refs) {
  return guarded([&] {
    if (!c || !n_nodes || !n_refs) throw std::invalid_argument("null argument");
    need_scene(c);
    *n_nodes = c->nodes.n / 4;
    *n_refs = c->refs.n;
    if (!nodes && !refs) return BLING_OK;
    if ((nodes && cap_nodes < *n_nodes) || (refs && cap_refs < *n_refs)) throw std::invalid_argument("capacity below the BVH's size");
    HIPCHK(hipSetDevice(c->device));
    if (nodes && c->nodes.n) HIPCHK(hipMemcpy(nodes, c->nodes.p, c->nodes.n * sizeof(float4), hipMemcpyDeviceToHost));
    if (refs && c->refs.n) HIPCHK(hipMemcpy(refs, c->refs.p, c->refs.n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return BLING_OK;
  });
}

int bling_debug_derived(bling_ctx* c, float* nodes4, size_t cap_nodes4, float* leaf_geo, size_t cap_leaf_quads, float* pkt, size_t cap_pkt,
                        size_t* n_nodes4, size_t* n_leaf_quads, size_t* n_pkt) {
  return guarded([&] {
    if (!c || !n_nodes4 || !n_leaf_quads || !n_pkt) throw std::invalid_argument("null argument");
    need_scene(c);
    *n_nodes4 = c->nodes4.n / 7;
    *n_leaf_quads = c->leaf_geo.n;
    *n_pkt = std::min<size_t>(c->S.pkt_n, c->pkt.n / 2);      // the entries walked (two float4 each)
    if (!nodes4 && !leaf_geo && !pkt) return BLING_OK;
    if ((nodes4 && cap_nodes4 < *n_nodes4) || (leaf_geo && cap_leaf_quads < *n_leaf_quads) || (pkt && cap_pkt < *n_pkt))
      throw std::invalid_argument("capacity below the derived arrays' size");
    HIPCHK(hipSetDevice(c->device));
    if (nodes4 && *n_nodes4) HIPCHK(hipMemcpy(nodes4, c->nodes4.p, *n_nodes4 * 7 * sizeof(float4), hipMemcpyDeviceToHost));
    if (leaf_geo && *n_leaf_quads) HIPCHK(hipMemcpy(leaf_geo, c->leaf_geo.p, *n_leaf_quads * sizeof(float4), hipMemcpyDeviceToHost));
    if (pkt && *n_pkt) HIPCHK(hipMemcpy(pkt, c->pkt.p, *n_pkt * 2 * sizeof(float4), hipMemcpyDeviceToHost));
    return BLING_OK;
  });
}

int bling_debug_derive_info(bling_ctx* c, bling_derive_info* out) {
  if (!c || !out) { set_last_error("null argument"); return BLING_EINVAL; }
  if (!c->has_scene) { set_last_error("no scene uploaded"); return BLING_ENOSCENE; }
  *out = c->derive_info;
  return BLING_OK;
}

int bling_host_bvh4(const float* nodes2, size_t n2, float* nodes4_out, size_t cap_nodes4, size_t* n4, int* depth, int* stack_need) {
  return guarded([&] {
    if (!n4 || !depth || !stack_need) throw std::invalid_argument("null argument");
    const bvh::Result4 Q = bvh::collapse4(checked_bvh2(nodes2, n2));
    *n4 = Q.nodes.size() / 28; *depth = Q.depth; *stack_need = Q.stack_need;
    if (!nodes4_out) return BLING_OK;
    if (cap_nodes4 < *n4) throw std::invalid_argument("capacity below the BVH4's size");
    std::memcpy(nodes4_out, Q.nodes.data(), Q.nodes.size() * sizeof(float));
    return BLING_OK;
  });
}

int bling_host_threaded(const float* nodes2, size_t n2, float* entries_out, size_t cap_entries, size_t* n_entries) {
  return guarded([&] {
    if (!n_entries) throw std::invalid_argument("null argument");
    const std::vector<float> e = bvh::threaded(checked_bvh2(nodes2, n2));
    *n_entries = e.size() / 8;
    if (!entries_out) return BLING_OK;
    if (cap_entries < *n_entries) throw std::invalid_argument("capacity below the list's size");
    std::memcpy(entries_out, e.data(), e.size() * sizeof(float));
    return BLING_OK;
  });
}

int bling_debug_bvh_build_info(bling_ctx* c, bling_bvh_build_info* out) {
  if (!c || !out) { set_last_error("null argument"); return BLING_EINVAL; }
  if (!c->has_scene) { set_last_error("no scene uploaded"); return BLING_ENOSCENE; }
  *out = c->bvh_info;
  return BLING_OK;
}

int bling_debug_set_bvh_depth_cap(bling_ctx* c, int cap) {
  if (!c || cap < 0 || cap > STACK_DEPTH - 1) { set_last_error("bad argument"); return BLING_EINVAL; }
  c->bvh_depth_cap = cap;
  return BLING_OK;
}

}  // extern "C"
