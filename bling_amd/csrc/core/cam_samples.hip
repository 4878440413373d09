// cam_samples.hip -- the sampler and camera seam (include/bling.h, "the sampler and camera seam"): the samples
// and camera rays of the caller's SampleWindows on device buffers.  Per call: the windows and their offsets are
// checked on the host (common/cam_windows.h, the rules bling_host_camera_samples applies), copied to the device
// once, and k_cam_samples (cam_samples.h) runs over the slots on the context's stream, in launches of at most
// 2^30 slots.  Needs the uploaded scene's DevScene record only: no LDS scene, no path set, no queue.
#include "core_internal.h"
#include "cam_samples.h"
#include "../common/cam_windows.h"

namespace bcore {
namespace {

constexpr uint64_t kCamLaunch = (uint64_t)1 << 30;   // slots per launch: 2^22 blocks of 256

bool cam_overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return a && b && pa < pb + nb && pb < pa + na;
}

// everything the two entry points refuse before they look at the outputs; returns first[n_windows]
uint64_t cam_ready(bling_ctx* c, const bling_image_window* windows, const uint64_t* first, size_t n_windows) {
  if (!c) throw std::invalid_argument("null argument");
  need_scene(c);
  std::string why;
  const bcam::Extent e{c->S.ex0, c->S.ex1, c->S.ey0, c->S.ey1};
  if (!bcam::check(c->cfg, e, windows, first, n_windows, &why)) throw std::invalid_argument(why);
  if (n_windows >= ((size_t)1 << 31)) throw std::invalid_argument("camera_samples: 2^31 windows or more");
  return first[n_windows];
}

void cam_check_outputs(const void* xy, const void* ids, const void* rays, const void* lens, uint64_t n) {
  if ((((uintptr_t)xy | (uintptr_t)ids | (uintptr_t)rays | (uintptr_t)lens) & 3u) != 0)
    throw std::invalid_argument("camera_samples: an output is not aligned to 4 bytes");
  const void* out[4] = {xy, ids, rays, lens};
  const uint64_t bytes[4] = {8 * n, 8 * n, 28 * n, 8 * n};
  for (int a = 0; a < 4; ++a)
    for (int b = a + 1; b < 4; ++b)
      if (cam_overlap(out[a], bytes[a], out[b], bytes[b])) throw std::invalid_argument("camera_samples: two outputs overlap");
}

// n > 0 slots into device buffers (any of them NULL); returns after completion
void cam_run(bling_ctx* c, uint32_t seed, uint32_t pass, const bling_image_window* windows, const uint64_t* first,
             size_t n_windows, uint64_t n, float* xy, uint32_t* ids, float* rays, float* lens, bling_camera_stats* st) {
  HIPCHK(hipSetDevice(c->device));
  CamState& K = c->cam;
  static_assert(sizeof(CamWin) == 2 * sizeof(uint4), "a window record is two uint4");
  std::vector<CamWin> hw(n_windows);
  for (size_t k = 0; k < n_windows; ++k) {
    const bling_image_window& w = windows[k];
    // an empty window owns no slot and is never read; its divisor only has to exist
    const uint32_t width = bcam::empty(w) ? 1u : (uint32_t)((int64_t)w.x1 - w.x0 + 1);
    hw[k] = CamWin{w.x0, w.y0, FastDiv::make(width), {0u, 0u, 0u}};
  }
  if (K.wins.n < 2 * n_windows) K.wins.alloc(2 * n_windows);
  if (K.first.n < n_windows + 1) K.first.alloc(n_windows + 1);
  const hipStream_t s = c->stream;
  HIPCHK(hipMemcpyAsync(K.wins.p, hw.data(), n_windows * sizeof(CamWin), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(K.first.p, first, (n_windows + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
  CamOut out{};
  out.xy = xy; out.ids = ids; out.lens = lens;
  for (int p = 0; p < 7; ++p) out.plane[p] = rays ? rays + (uint64_t)p * n : nullptr;
  out.pairs8 = (((uintptr_t)xy | (uintptr_t)ids | (uintptr_t)lens) & 7u) == 0 ? 1u : 0u;
  const EventPair ev;
  ev.a.record(s);
  if (xy || ids || rays || lens)
    for (uint64_t base = 0; base < n; base += kCamLaunch) {
      const uint32_t m = (uint32_t)std::min(kCamLaunch, n - base);
      k_cam_samples<<<(m + 255u) / 256u, 256, 0, s>>>(c->dscene.p, reinterpret_cast<const CamWin*>(K.wins.p), K.first.p,
                                                       (uint32_t)n_windows, base, m, out, seed, pass);
      HIPCHK(hipGetLastError());
    }
  ev.b.record(s);
  HIPCHK(hipStreamSynchronize(s));
  if (!st) return;
  st->samples = n;
  st->windows = n_windows;
  st->ms_total = ev.elapsed_ms();
}

}  // namespace
}  // namespace bcore

extern "C" {

int bling_camera_samples_device(bling_ctx* c, uint32_t seed, uint32_t pass_index, const bling_image_window* windows,
                                const uint64_t* first, size_t n_windows, void* xy_dev, void* ids_dev, void* rays_soa_dev,
                                void* lens_dev, bling_camera_stats* st) {
  return guarded([&] {
    const uint64_t n = cam_ready(c, windows, first, n_windows);
    if (st) *st = bling_camera_stats{0, n_windows, 0.0};
    if (n == 0) return BLING_OK;
    cam_check_outputs(xy_dev, ids_dev, rays_soa_dev, lens_dev, n);
    cam_run(c, seed, pass_index, windows, first, n_windows, n, static_cast<float*>(xy_dev), static_cast<uint32_t*>(ids_dev),
            static_cast<float*>(rays_soa_dev), static_cast<float*>(lens_dev), st);
    return BLING_OK;
  });
}

int bling_camera_samples(bling_ctx* c, uint32_t seed, uint32_t pass_index, const bling_image_window* windows,
                         const uint64_t* first, size_t n_windows, float* xy, uint32_t* ids, float* rays_soa, float* lens,
                         bling_camera_stats* st) {
  return guarded([&] {
    const uint64_t n = cam_ready(c, windows, first, n_windows);
    if (st) *st = bling_camera_stats{0, n_windows, 0.0};
    if (n == 0) return BLING_OK;
    cam_check_outputs(xy, ids, rays_soa, lens, n);
    HIPCHK(hipSetDevice(c->device));
    CamState& K = c->cam;
    if (xy && K.xy.n < 2 * n) K.xy.alloc(2 * n);
    if (ids && K.ids.n < 2 * n) K.ids.alloc(2 * n);
    if (rays_soa && K.rays.n < 7 * n) K.rays.alloc(7 * n);
    if (lens && K.lens.n < 2 * n) K.lens.alloc(2 * n);
    // the staged planes keep the stride n, whatever the buffer's capacity
    cam_run(c, seed, pass_index, windows, first, n_windows, n, xy ? K.xy.p : nullptr, ids ? K.ids.p : nullptr,
            rays_soa ? K.rays.p : nullptr, lens ? K.lens.p : nullptr, st);
    if (xy) HIPCHK(hipMemcpy(xy, K.xy.p, 2 * n * sizeof(float), hipMemcpyDeviceToHost));
    if (ids) HIPCHK(hipMemcpy(ids, K.ids.p, 2 * n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (rays_soa) HIPCHK(hipMemcpy(rays_soa, K.rays.p, 7 * n * sizeof(float), hipMemcpyDeviceToHost));
    if (lens) HIPCHK(hipMemcpy(lens, K.lens.p, 2 * n * sizeof(float), hipMemcpyDeviceToHost));
    return BLING_OK;
  });
}

}  // extern "C"
