// cam_windows.h -- what bling_camera_samples[_device] (include/bling.h) and bling_host_camera_samples
// (include/bling_host.h) check before they write anything, stated once for the device library and the host
// library: the sample extent (sampleExtent, Image.hs:162-168), and a window list against it and its offsets.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../../include/bling_scene.h"

namespace bcam {

struct Extent { int32_t x0, x1, y0, y1; };

// the extent bling_scene_upload gives the device scene (core.hip): (0.5 + width) + fw, rounded twice
inline Extent sample_extent(const bling_scene_desc& d) {
  const float fw = d.filter.width, fh = d.filter.height;
  return Extent{(int32_t)std::floor(0.5f - fw), (int32_t)std::floor(0.5f + (float)d.config.width + fw),
                (int32_t)std::floor(0.5f - fh), (int32_t)std::floor(0.5f + (float)d.config.height + fh)};
}

inline bool empty(const bling_image_window& w) { return w.x1 < w.x0 || w.y1 < w.y0; }

// samples of a window inside the extent: (x1 - x0 + 1) (y1 - y0 + 1) spp, 0 for an empty one
inline uint64_t count(const bling_image_window& w, int spp) {
  if (empty(w)) return 0;
  return (uint64_t)((int64_t)w.x1 - w.x0 + 1) * (uint64_t)((int64_t)w.y1 - w.y0 + 1) * (uint64_t)spp;
}

// true, or false with the reason: a renderer other than the sampler's, spp < 1, a first that does not start
// at 0 or does not match the windows' counts, a non-empty window with a pixel outside the extent
inline bool check(const bling_render_config& cfg, const Extent& e, const bling_image_window* windows,
                  const uint64_t* first, size_t n_windows, std::string* why) {
  if (cfg.renderer != BLING_RENDERER_SAMPLER_PATH) { *why = "camera_samples: the scene's renderer is not the sampler renderer"; return false; }
  if (cfg.spp < 1) { *why = "camera_samples: fewer than one sample per pixel"; return false; }
  if (!first || (n_windows && !windows)) { *why = "camera_samples: null argument"; return false; }
  if (first[0] != 0) { *why = "camera_samples: first does not start at 0"; return false; }
  for (size_t k = 0; k < n_windows; ++k) {
    const bling_image_window& w = windows[k];
    if (!empty(w) && (w.x0 < e.x0 || w.x1 > e.x1 || w.y0 < e.y0 || w.y1 > e.y1)) {
      *why = "camera_samples: window " + std::to_string(k) + " has a pixel outside the sample extent";
      return false;
    }
    if (first[k + 1] < first[k] || first[k + 1] - first[k] != count(w, cfg.spp)) {
      *why = "camera_samples: first[" + std::to_string(k + 1) + "] - first[" + std::to_string(k) +
             "] is not the sample count of window " + std::to_string(k);
      return false;
    }
  }
  return true;
}

}  // namespace bcam
