// lbvh_host.cpp -- bling_host_lbvh: the device BVH builder's algorithm (common/lbvh.h) on the CPU, one
// item after another.  No context, no GPU; the device tree (core/bvh_device.hip) is pinned to this
// restatement bit for bit, and this one to an independent restatement in the tests.
#include "../../../include/bling_host.h"
#include "../common/lbvh.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

struct Fit { float b[6]; int height; };

struct Tree {
  uint32_t n;
  const float* boxes;
  const uint64_t* keys;
  std::vector<uint32_t> first, last, split;
  std::vector<Fit> fit;                      // per internal node: its box and the levels of nodes below it

  void item_box(uint32_t pos, float* b) const { std::memcpy(b, boxes + 6 * (size_t)(uint32_t)keys[pos], 6 * sizeof(float)); }
  static void grow(float* a, const float* b) {
    for (int k = 0; k < 3; ++k) { a[k] = std::min(a[k], b[k]); a[3 + k] = std::max(a[3 + k], b[3 + k]); }
  }
  bool left_is_item(uint32_t i) const { return first[i] == split[i]; }
  bool right_is_item(uint32_t i) const { return last[i] == split[i] + 1; }

  // bottom-up fit of node i (the hierarchy is at most 62 levels deep: one per key bit that varies)
  void fit_node(uint32_t i) {
    Fit& f = fit[i];
    float r[6];
    int hl = 0, hr = 0;
    if (left_is_item(i)) item_box(split[i], f.b);
    else { fit_node(split[i]); std::memcpy(f.b, fit[split[i]].b, sizeof f.b); hl = fit[split[i]].height; }
    if (right_is_item(i)) item_box(split[i] + 1, r);
    else { fit_node(split[i] + 1); std::memcpy(r, fit[split[i] + 1].b, sizeof r); hr = fit[split[i] + 1].height; }
    grow(f.b, r);
    f.height = blbvh::is_leaf_range(first[i], last[i]) ? 0 : 1 + std::max(hl, hr);
  }
};

}  // namespace

extern "C" int bling_host_lbvh(const float* boxes, const uint32_t* refs, size_t n_items, int depth_cap, float* nodes_out,
                               uint32_t* refs_out, uint64_t* keys_out, bling_lbvh_info* info) {
  if (!boxes || !refs || !nodes_out || !refs_out || !info) return BLING_LBVH_EINVAL;
  if (n_items < 3 || n_items > blbvh::kMaxItems || depth_cap < 0 || depth_cap > blbvh::kDepthCap) return BLING_LBVH_EINVAL;
  const uint32_t n = (uint32_t)n_items;
  const int cap = depth_cap ? depth_cap : blbvh::kDepthCap;
  std::memset(info, 0, sizeof *info);
  info->items = n;

  float cmin[3], cmax[3], scale[3];
  for (int a = 0; a < 3; ++a) {
    cmin[a] = cmax[a] = blbvh::centre(boxes[a], boxes[3 + a]);
    for (uint32_t i = 1; i < n; ++i) {
      const float c = blbvh::centre(boxes[6 * (size_t)i + a], boxes[6 * (size_t)i + 3 + a]);
      cmin[a] = std::min(cmin[a], c);
      cmax[a] = std::max(cmax[a], c);
    }
    scale[a] = blbvh::axis_scale(cmin[a], cmax[a]);
  }
  std::vector<uint64_t> keys(n);
  for (uint32_t i = 0; i < n; ++i) keys[i] = blbvh::make_key(boxes + 6 * (size_t)i, cmin, scale, i);
  std::sort(keys.begin(), keys.end());
  if (keys_out) std::memcpy(keys_out, keys.data(), n * sizeof(uint64_t));
  for (uint32_t k = 0; k < n; ++k) refs_out[k] = refs[(uint32_t)keys[k]];

  Tree T{n, boxes, keys.data(), {}, {}, {}, {}};
  T.first.resize(n - 1); T.last.resize(n - 1); T.split.resize(n - 1); T.fit.resize(n - 1);
  for (uint32_t i = 0; i + 1 < n; ++i) blbvh::node_range(keys.data(), n, i, &T.first[i], &T.last[i], &T.split[i]);
  T.fit_node(0);

  // the surviving nodes' numbers: ascending in i
  std::vector<uint32_t> number(n - 1);
  uint32_t count = 0;
  for (uint32_t i = 0; i + 1 < n; ++i) { number[i] = count; if (!blbvh::is_leaf_range(T.first[i], T.last[i])) ++count; }
  info->nodes = count;
  info->depth = (uint32_t)T.fit[0].height;
  if (T.fit[0].height > cap) return BLING_LBVH_EDEPTH;

  for (uint32_t i = 0; i + 1 < n; ++i) {
    if (blbvh::is_leaf_range(T.first[i], T.last[i])) continue;
    float* nd = nodes_out + 16 * (size_t)number[i];
    for (int c = 0; c < 2; ++c) {
      const bool item = c == 0 ? T.left_is_item(i) : T.right_is_item(i);
      const uint32_t pos = T.split[i] + (uint32_t)c;          // the item's position, or the child node's index
      float b[6];
      int32_t link;
      if (item) {
        T.item_box(pos, b);
        link = blbvh::leaf_code(pos, 1u);
      } else {
        std::memcpy(b, T.fit[pos].b, sizeof b);
        link = blbvh::is_leaf_range(T.first[pos], T.last[pos]) ? blbvh::leaf_code(T.first[pos], 2u) : (int32_t)number[pos];
      }
      if (link < 0) {
        const uint32_t cnt = (uint32_t)~link & 0xFFu;
        info->leaves++;
        info->max_leaf = std::max(info->max_leaf, cnt);
      }
      blbvh::pad_box(b);
      std::memcpy(nd + 6 * c, b, sizeof b);
      std::memcpy(nd + 12 + c, &link, 4);
    }
    nd[14] = nd[15] = 0.f;
  }
  return BLING_LBVH_OK;
}
