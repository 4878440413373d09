// bling_main.cpp -- command-line front end: the reference's "render one .bling once" harness
// (commented out in src/cmdline/Main.hs:15-42: parseJob >>= render renderer job prog, writing
// pass-NNNNN.png and .hdr at PassDone) over the host loader and the MI355X core.
//
//   bling <scene.bling> [--overrides "image=W,H;..."] [--passes N] [--out prefix] [--device D]
//         [--develop host|device] [--splat atomic|ordered] [--film atomic|ordered] [--bvh host|device] [--derive host|device]
// --develop device makes each written pass's 8-bit and RGBE pixels on the device (bling_film_develop)
// and hands them to the encoders; the default, host, develops with the host library.  Same files.
// --splat ordered (light tracer, Metropolis and SPPM scenes) adds every pixel's splats in the reference's order
// (BLING_SPLAT_ORDERED): the same files on every run; the default, atomic, adds them with float atomics.
// --film ordered (sampler scenes; the environment's BLING_FILM_ORDERED=1 means the same) forms every pass's film in
// the reference's order without float atomics (BLING_PASS_ORDERED_FILM): the same files on every run.  The splat
// renderers refuse it: their switch is --splat.
// --seams (with --film ordered, sampler scenes, not the bidir integrator) renders each pass as a caller of the seams
// would: windows -> bling_camera_samples_device -> bling_surface_li_device -> bling_image_add_windowed_device.  Same files.
//   bling --image-filters [--out DIR] [--size WxH] [--develop host|device] [--device D] [--windows N]
// reproduces the reference's live command line (main = imageFilters, src/cmdline/Examples.hs:10-58) and is the whole
// run: for box, gauss 3 3 2, mitchell 3 3 1/3 1/3, sinc 3 3 3 and triangle 3 3 it writes DIR/filter-show-<name>.png
// (64 x 64, box film, red or green by the sign of evalFilter) and DIR/filter-test-<name>.png (480 x 270 unless --size
// says otherwise, 25 offsets a pixel over the sample extent, |sin (150 r^2)| grey through rgbToSpectrumIllum).  The
// samples are made on the host in row chunks and added on the device in order (bling_image_add_samples_device).
// --windows N adds the test images' samples as a renderer does instead: the sample extent is cut into splitWindow's
// 16 x 16 windows (Sampling.hs:55-58), each window's samples go to its own tile image and the tiles are added in
// window order (bling_image_add_windowed_device, N windows a call); the files are the same for every N > 0.
// With --develop device, or --splat ordered, such a scene's splat image (and an SPPM scene's film) lives on
// the device for the whole run (bling_light_pass_device / bling_mlt_pass_device / bling_sppm_pass_device);
// --develop device then develops it there (bling_film_develop_device) and only the developed pixels come back.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "bling.h"
#include "bling_host.h"

namespace {
// The device buffers of a light tracer / Metropolis run whose splat image stays on the device: the image,
// an empty film and the developed pixels (4 bytes a pixel at most).
struct DeviceFilm {
  void *splat = nullptr, *film = nullptr, *out = nullptr;
  bool alloc(int w, int h) {
    const size_t px = (size_t)w * h;
    if (hipMalloc(&splat, px * 12) != hipSuccess || hipMalloc(&film, px * 16) != hipSuccess || hipMalloc(&out, px * 4) != hipSuccess ||
        hipMemset(splat, 0, px * 12) != hipSuccess || hipMemset(film, 0, px * 16) != hipSuccess) {
      std::fprintf(stderr, "device film: %s\n", hipGetErrorString(hipGetLastError()));
      return false;
    }
    return true;
  }
  ~DeviceFilm() { (void)hipFree(splat); (void)hipFree(film); (void)hipFree(out); }
};

// One written pass of a device splat image: developed on the device, or fetched and developed by the host library.
int write_pass(bling_ctx* ctx, bool on_device, const std::string& name, const float* film, const float* splat, float sw,
               int w, int h, std::vector<float>& rgb);
int write_pass_device_film(bling_ctx* ctx, bool dev_develop, const DeviceFilm& df, const std::string& name, const float* film,
                           float sw, int w, int h, std::vector<float>& rgb) {
  const size_t px = (size_t)w * h;
  if (!dev_develop) {
    std::vector<float> splat(px * 3);
    if (hipMemcpy(splat.data(), df.splat, px * 12, hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "splat image: copy failed\n"); return 1; }
    return write_pass(ctx, false, name, film, splat.data(), sw, w, h, rgb);
  }
  std::vector<unsigned char> px8(px * 3), pxe(px * 4);
  bling_develop_params dp{BLING_DEVELOP_RGB8, sw, {0, w - 1, 0, h - 1}};
  if (bling_film_develop_device(ctx, &dp, df.film, df.splat, df.out) != 0) { std::fprintf(stderr, "%s\n", bling_last_error()); return 1; }
  if (hipMemcpy(px8.data(), df.out, px * 3, hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "developed image: copy failed\n"); return 1; }
  dp.format = BLING_DEVELOP_RGBE;
  if (bling_film_develop_device(ctx, &dp, df.film, df.splat, df.out) != 0) { std::fprintf(stderr, "%s\n", bling_last_error()); return 1; }
  if (hipMemcpy(pxe.data(), df.out, px * 4, hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "developed image: copy failed\n"); return 1; }
  const std::string png = name + ".png", hdr = name + ".hdr";
  if (bling_host_write_png_rgb8(png.c_str(), px8.data(), w, h) != 0 || bling_host_write_hdr_rgbe(hdr.c_str(), pxe.data(), w, h) != 0) {
    std::fprintf(stderr, "%s\n", bling_host_last_error());
    return 1;
  }
  return 0;
}

// One written pass: <name>.png and <name>.hdr.  On the device: RGB8 and RGBE through bling_film_develop
// and the two pixel encoders; on the host: today's path.  splat may be NULL (then sw is unused).
int write_pass(bling_ctx* ctx, bool on_device, const std::string& name, const float* film, const float* splat, float sw,
               int w, int h, std::vector<float>& rgb) {
  const std::string png = name + ".png", hdr = name + ".hdr";
  if (on_device) {
    std::vector<unsigned char> px8((size_t)w * h * 3), pxe((size_t)w * h * 4);
    bling_develop_params dp{BLING_DEVELOP_RGB8, splat ? sw : 0.f, {0, w - 1, 0, h - 1}};
    if (bling_film_develop(ctx, &dp, film, splat, px8.data()) != 0) { std::fprintf(stderr, "%s\n", bling_last_error()); return 1; }
    dp.format = BLING_DEVELOP_RGBE;
    if (bling_film_develop(ctx, &dp, film, splat, pxe.data()) != 0) { std::fprintf(stderr, "%s\n", bling_last_error()); return 1; }
    if (bling_host_write_png_rgb8(png.c_str(), px8.data(), w, h) != 0 || bling_host_write_hdr_rgbe(hdr.c_str(), pxe.data(), w, h) != 0) {
      std::fprintf(stderr, "%s\n", bling_host_last_error());
      return 1;
    }
    return 0;
  }
  int rc;
  if (splat) {
    bling_host_film_splat_to_rgb(film, splat, sw, w, h, rgb.data());
    rc = bling_host_write_png_splat(png.c_str(), film, splat, sw, w, h);
  } else {
    bling_host_film_to_rgb(film, w, h, rgb.data());
    rc = bling_host_write_png(png.c_str(), film, w, h);
  }
  if (rc != 0 || bling_host_write_hdr(hdr.c_str(), rgb.data(), w, h) != 0) {
    std::fprintf(stderr, "%s\n", bling_host_last_error());
    return 1;
  }
  return 0;
}

// execImageT of one of imageFilters' two sample generators over an image on the device, then writePng.
struct FilterImage {
  bling_ctx* ctx;
  bool dev_develop;
  bling_image_desc desc{};
  void *film = nullptr, *xy = nullptr, *spectra = nullptr, *out = nullptr;
  size_t cap = 0;                               // samples xy and spectra hold
  std::vector<float> hxy, hsp;
  std::vector<bling_image_window> wins;           // --windows: the windows gathered so far and their sample offsets
  std::vector<uint64_t> first;
  bling_image_stats total{};
  ~FilterImage() { (void)hipFree(film); (void)hipFree(xy); (void)hipFree(spectra); (void)hipFree(out); }
  bool start(const bling_filter& f, int w, int h) {
    desc.width = w; desc.height = h; desc.filter = f;
    total = bling_image_stats{};
    (void)hipFree(film); (void)hipFree(out);
    film = out = nullptr;
    const size_t px = (size_t)w * h;
    return hipMalloc(&film, px * 16) == hipSuccess && hipMemset(film, 0, px * 16) == hipSuccess && hipMalloc(&out, px * 3) == hipSuccess;
  }
  void sample(float x, float y, const float rgb[3]) {
    hxy.push_back(x); hxy.push_back(y);
    hsp.resize(hsp.size() + 16);
    bling_host_rgb_to_spectrum_illum(rgb, hsp.data() + hsp.size() - 16);
  }
  // --windows: the samples gathered since the last call are those of window w
  void end_window(const bling_image_window& w) {
    if (first.empty()) first.push_back(0);
    wins.push_back(w);
    first.push_back(hxy.size() / 2);
  }
  // addSample' of the samples gathered so far, in order; with windows gathered, tile by tile (addTile)
  bool flush() {
    const size_t n = hxy.size() / 2;
    if (n == 0 && wins.empty()) return true;
    if (n > cap) {
      (void)hipFree(xy); (void)hipFree(spectra);
      xy = spectra = nullptr;
      if (hipMalloc(&xy, n * 8) != hipSuccess || hipMalloc(&spectra, n * 64) != hipSuccess) { cap = 0; return false; }
      cap = n;
    }
    if (hipMemcpy(xy, hxy.data(), n * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(spectra, hsp.data(), n * 64, hipMemcpyHostToDevice) != hipSuccess)
      return false;
    bling_image_stats st;
    const int rc = wins.empty() ? bling_image_add_samples_device(ctx, &desc, BLING_IMAGE_ADD, xy, spectra, n, film, &st)
                                : bling_image_add_windowed_device(ctx, &desc, BLING_IMAGE_ADD, wins.data(), first.data(), wins.size(), xy,
                                                                  spectra, n, film, nullptr, &st);
    if (rc != 0) {
      std::fprintf(stderr, "%s\n", bling_last_error());
      return false;
    }
    wins.clear(); first.clear();
    total.samples += st.samples; total.tile_pairs += st.tile_pairs; total.chunks += st.chunks; total.ms += st.ms;
    total.dropped_spectrum += st.dropped_spectrum; total.dropped_position += st.dropped_position;
    hxy.clear(); hsp.clear();
    return true;
  }
  bool write(const std::string& path) {
    const int w = desc.width, h = desc.height;
    const size_t px = (size_t)w * h;
    int rc;
    if (dev_develop) {
      std::vector<unsigned char> px8(px * 3);
      bling_develop_params dp{BLING_DEVELOP_RGB8, 0.f, {0, w - 1, 0, h - 1}};
      if (bling_image_develop_device(ctx, &desc, &dp, film, nullptr, out) != 0) { std::fprintf(stderr, "%s\n", bling_last_error()); return false; }
      if (hipMemcpy(px8.data(), out, px * 3, hipMemcpyDeviceToHost) != hipSuccess) return false;
      rc = bling_host_write_png_rgb8(path.c_str(), px8.data(), w, h);
    } else {
      std::vector<float> host(px * 4);
      if (hipMemcpy(host.data(), film, px * 16, hipMemcpyDeviceToHost) != hipSuccess) return false;
      rc = bling_host_write_png(path.c_str(), host.data(), w, h);
    }
    if (rc != 0) std::fprintf(stderr, "%s\n", bling_host_last_error());
    return rc == 0;
  }
};

int image_filters(int argc, char** argv) {
  const char* dir = ".";
  int width = 480, height = 270, device = 0, windows = 0;
  bool dev_develop = false;
  for (int i = 2; i + 1 < argc; i += 2) {
    if (!std::strcmp(argv[i], "--out")) dir = argv[i + 1];
    else if (!std::strcmp(argv[i], "--device")) device = std::atoi(argv[i + 1]);
    else if (!std::strcmp(argv[i], "--windows")) {
      if ((windows = std::atoi(argv[i + 1])) < 1) {
        std::fprintf(stderr, "--windows takes a count of at least 1, not %s\n", argv[i + 1]);
        return 2;
      }
    } else if (!std::strcmp(argv[i], "--size")) {
      if (std::sscanf(argv[i + 1], "%dx%d", &width, &height) != 2 || width < 1 || height < 1) {
        std::fprintf(stderr, "--size takes WxH, not %s\n", argv[i + 1]);
        return 2;
      }
    } else if (!std::strcmp(argv[i], "--develop")) {
      if (std::strcmp(argv[i + 1], "host") && std::strcmp(argv[i + 1], "device")) {
        std::fprintf(stderr, "--develop takes host or device, not %s\n", argv[i + 1]);
        return 2;
      }
      dev_develop = !std::strcmp(argv[i + 1], "device");
    } else {
      std::fprintf(stderr, "--image-filters: unknown option %s\n", argv[i]);
      return 2;
    }
  }
  struct Flt { const char* name; int kind; int n; float p[4]; };
  const Flt flts[] = {{"box", BLING_FILTER_BOX, 0, {}},
                      {"gauss", BLING_FILTER_GAUSS, 3, {3.f, 3.f, 2.f}},
                      {"mitchell", BLING_FILTER_MITCHELL, 4, {3.f, 3.f, 1.f / 3.f, 1.f / 3.f}},
                      {"sinc", BLING_FILTER_SINC, 3, {3.f, 3.f, 3.f}},
                      {"triangle", BLING_FILTER_TRIANGLE, 2, {3.f, 3.f}}};
  bling_ctx* ctx = nullptr;
  if (bling_create(&device, 1, &ctx) != 0 || hipSetDevice(device) != hipSuccess) { std::fprintf(stderr, "%s\n", bling_last_error()); return 1; }
  int rc = 0;
  {
    FilterImage img{ctx, dev_develop};
    bling_filter box;
    bling_host_make_filter(BLING_FILTER_BOX, nullptr, 0, &box);
    constexpr int kShow = 64, kRows = 16;       // showSize; sample-extent rows per device call
    const float offs[5] = {0.f, 0.2f, 0.4f, 0.6f, 0.8f};
    for (const Flt& f : flts) {
      std::printf("%s\n", f.name);
      bling_filter flt;
      if (bling_host_make_filter(f.kind, f.p, f.n, &flt) != 0) { std::fprintf(stderr, "%s\n", bling_host_last_error()); rc = 1; break; }
      int32_t e[4];
      // fltShow: the filter's own shape, through a box film
      if (!img.start(box, kShow, kShow)) { std::fprintf(stderr, "device film: allocation failed\n"); rc = 1; break; }
      bling_host_image_extent(&img.desc, e);
      bool ok = true;
      for (int py = e[2]; py <= e[3] && ok; ++py) {
        for (int px = e[0]; px <= e[1]; ++px) {
          const float x = (float)px, y = (float)py;
          const float xs = (x / (float)kShow - 0.5f) * 4.f, ys = (y / (float)kShow - 0.5f) * 4.f;
          const float d = bling_host_eval_filter(f.kind, f.p, xs, ys);
          const float c[3] = {d > 0.f ? d : 0.f, d > 0.f ? 0.f : -d, 0.f};
          img.sample(x, y, c);
        }
        if ((py - e[2]) % kRows == kRows - 1 || py == e[3]) ok = img.flush();
      }
      const std::string base = std::string(dir) + "/filter-";
      if (!ok || !img.write(base + "show-" + f.name + ".png")) { rc = 1; break; }
      // fltTest: a zone plate through the filter
      if (!img.start(flt, width, height)) { std::fprintf(stderr, "device film: allocation failed\n"); rc = 1; break; }
      bling_host_image_extent(&img.desc, e);
      const float sz = (float)std::min(width, height);
      const auto pixel = [&](int px, int py) {
        for (float sx : offs)
          for (float sy : offs) {
            const float x = (float)px + sx, y = (float)py + sy;
            const float dx = x / sz - 0.5f, dy = 1.f - y / sz;
            const float d = std::fabs(std::sin(150.f * (dx * dx + dy * dy)));
            const float c[3] = {d, d, d};
            img.sample(x, y, c);
          }
      };
      if (windows > 0) {
        // splitWindow (Sampling.hs:55-58) over the extent; a window's samples are its pixels', rows first
        int k = 0;
        for (int wy = e[2]; wy <= e[3] && ok; wy += 16)
          for (int wx = e[0]; wx <= e[1] && ok; wx += 16) {
            const bling_image_window w{wx, std::min(wx + 15, e[1]), wy, std::min(wy + 15, e[3])};
            for (int py = w.y0; py <= w.y1; ++py)
              for (int px = w.x0; px <= w.x1; ++px) pixel(px, py);
            img.end_window(w);
            if (++k % windows == 0) ok = img.flush();
          }
        ok = ok && img.flush();
      } else {
        for (int py = e[2]; py <= e[3] && ok; ++py) {
          for (int px = e[0]; px <= e[1]; ++px) pixel(px, py);
          if ((py - e[2]) % kRows == kRows - 1 || py == e[3]) ok = img.flush();
        }
      }
      if (!ok || !img.write(base + "test-" + f.name + ".png")) { rc = 1; break; }
      std::printf("   filter-test-%s: %llu samples, %llu tile pairs, %llu chunks, %.2f ms on the device\n", f.name,
                  (unsigned long long)img.total.samples, (unsigned long long)img.total.tile_pairs, (unsigned long long)img.total.chunks,
                  img.total.ms);
    }
  }
  bling_destroy(ctx);
  return rc;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s scene.bling [--overrides S] [--passes N] [--out prefix] [--device D] [--develop host|device] [--splat atomic|ordered] [--film atomic|ordered] [--seams] [--bvh host|device] [--derive host|device]\n"
                         "       %s --image-filters [--out DIR] [--size WxH] [--develop host|device] [--device D] [--windows N]\n", argv[0], argv[0]);
    return 2;
  }
  if (!std::strcmp(argv[1], "--image-filters")) return image_filters(argc, argv);
  const char* scene = argv[1];
  const char* ov = nullptr;
  const char* out = "pass";
  int passes = 1, device = 0;
  bool dev_develop = false, ordered = false;
  const char* film_env = std::getenv("BLING_FILM_ORDERED");
  bool film_ordered = film_env && film_env[0] == '1';
  bool seams = false;
  uint32_t bvh_builder = BLING_BVH_HOST;
  bool bvh_line = false;
  uint32_t upload_flags = 0u;
  bool derive_line = false;
  for (int i = 2; i < argc; i += 2) {
    if (!std::strcmp(argv[i], "--seams")) { seams = true; --i; continue; }   // the one switch without a value
    if (i + 1 >= argc) break;
    if (!std::strcmp(argv[i], "--overrides")) ov = argv[i + 1];
    else if (!std::strcmp(argv[i], "--passes")) passes = std::atoi(argv[i + 1]);
    else if (!std::strcmp(argv[i], "--out")) out = argv[i + 1];
    else if (!std::strcmp(argv[i], "--device")) device = std::atoi(argv[i + 1]);
    else if (!std::strcmp(argv[i], "--develop")) {
      if (std::strcmp(argv[i + 1], "host") && std::strcmp(argv[i + 1], "device")) {
        std::fprintf(stderr, "--develop takes host or device, not %s\n", argv[i + 1]);
        return 2;
      }
      dev_develop = !std::strcmp(argv[i + 1], "device");
    } else if (!std::strcmp(argv[i], "--splat")) {
      if (std::strcmp(argv[i + 1], "atomic") && std::strcmp(argv[i + 1], "ordered")) {
        std::fprintf(stderr, "--splat takes atomic or ordered, not %s\n", argv[i + 1]);
        return 2;
      }
      ordered = !std::strcmp(argv[i + 1], "ordered");
    } else if (!std::strcmp(argv[i], "--film")) {
      if (std::strcmp(argv[i + 1], "atomic") && std::strcmp(argv[i + 1], "ordered")) {
        std::fprintf(stderr, "--film takes atomic or ordered, not %s\n", argv[i + 1]);
        return 2;
      }
      film_ordered = !std::strcmp(argv[i + 1], "ordered");
    } else if (!std::strcmp(argv[i], "--bvh")) {
      if (std::strcmp(argv[i + 1], "host") && std::strcmp(argv[i + 1], "device")) {
        std::fprintf(stderr, "--bvh takes host or device, not %s\n", argv[i + 1]);
        return 2;
      }
      bvh_builder = !std::strcmp(argv[i + 1], "device") ? BLING_BVH_DEVICE : BLING_BVH_HOST;
      bvh_line = true;
    } else if (!std::strcmp(argv[i], "--derive")) {
      if (std::strcmp(argv[i + 1], "host") && std::strcmp(argv[i + 1], "device")) {
        std::fprintf(stderr, "--derive takes host or device, not %s\n", argv[i + 1]);
        return 2;
      }
      upload_flags = !std::strcmp(argv[i + 1], "device") ? BLING_UPLOAD_DERIVE_DEVICE : 0u;
      derive_line = true;
    }
  }
  bling_host_scene* hs = nullptr;
  if (bling_host_load(scene, ov, &hs) != 0) { std::fprintf(stderr, "%s\n", bling_host_last_error()); return 1; }
  std::printf("Job Stats\n   %s\n", bling_host_summary(hs));
  const bling_scene_desc* d = bling_host_desc(hs);
  bling_ctx* ctx = nullptr;
  const bling_upload_params up{bvh_builder, upload_flags};
  if (bling_create(&device, 1, &ctx) != 0 || bling_scene_upload_with(ctx, d, &up) != 0) {
    std::fprintf(stderr, "%s\n", bling_last_error());
    return 1;
  }
  if (bvh_line) {                      // --bvh: how the BVH2 was built
    bling_bvh_build_info bi;
    if (bling_debug_bvh_build_info(ctx, &bi) != 0) { std::fprintf(stderr, "%s\n", bling_last_error()); return 1; }
    static const char* const why[] = {"", " (fractal scene: host tree)", " (fewer than 3 items: host tree)",
                                      " (deeper than the traversal stack: host tree)", " (too many items: host tree)"};
    std::printf("bvh: builder %s%s, %u items, %u nodes, depth %u, build %.3f ms, derive %.3f ms\n",
                bi.used == BLING_BVH_DEVICE ? "device" : "host", why[bi.fallback <= 4 ? bi.fallback : 0], bi.items, bi.nodes,
                bi.depth, bi.ms_build, bi.ms_derive);
  }
  if (derive_line) {                   // --derive: where the BVH4, the leaf records and the plans were derived
    bling_derive_info di;
    if (bling_debug_derive_info(ctx, &di) != 0) { std::fprintf(stderr, "%s\n", bling_last_error()); return 1; }
    static const char* const why[] = {"", " (fractal scene: host derivation)", " (several devices: host derivation)",
                                      " (no BVH2 nodes: host derivation)"};
    std::printf("derive: %s%s, %u BVH4 nodes, depth %u, stack %u, %u levels, device %.3f ms, host %.3f ms\n",
                di.used == BLING_DERIVE_DEVICE ? "device" : "host", why[di.fallback <= 3 ? di.fallback : 0], di.bvh4_nodes,
                di.bvh4_depth, di.stack_need, di.level_launches, di.ms_derive_device, di.ms_plan_host);
  }
  int w = d->config.width, h = d->config.height;
  std::vector<float> film((size_t)w * h * 4, 0.f), rgb((size_t)w * h * 3);
  const bool splats = d->config.renderer == BLING_RENDERER_LIGHT || d->config.renderer == BLING_RENDERER_METROPOLIS ||
                      d->config.renderer == BLING_RENDERER_SPPM;
  if (seams) {
    const char* why = splats ? "--seams renders a sampler scene through its seams; this scene's renderer splats"
                      : d->config.integrator == BLING_INTEGRATOR_BIDIR
                          ? "--seams: surface_li refuses the bidir integrator (its walk makes the camera ray inside)"
                      : !film_ordered ? "--seams needs --film ordered: the chain of seams is the ordered film"
                                      : nullptr;
    if (why) { std::fprintf(stderr, "%s\n", why); return 2; }
  }
  if (splats && film_ordered) {
    std::fprintf(stderr, "--film ordered is for sampler scenes; this scene's renderer splats: use --splat ordered\n");
    return 2;
  }
  const bool device_film = splats && (dev_develop || ordered);
  const uint32_t splat_flags = ordered ? BLING_SPLAT_ORDERED : 0u;
  DeviceFilm df;
  if (device_film && (hipSetDevice(device) != hipSuccess || !df.alloc(w, h))) return 1;
  if (d->config.renderer == BLING_RENDERER_LIGHT) {
    // instance Renderer LightTracer (Renderer/LightTracer.hs:37-52): the film stays empty, every pass
    // adds its splats, and the image of pass n weighs them with 1 / (n * passPhotons)
    std::vector<float> splat((size_t)w * h * 3, 0.f);
    for (int p = 1; p <= passes; ++p) {
      bling_light_stats st;
      const int rc = device_film ? bling_light_pass_device(ctx, 0x0B11A6u, (uint32_t)p, splat_flags, df.splat, &st)
                                 : bling_light_pass(ctx, 0x0B11A6u, (uint32_t)p, splat.data(), &st);
      if (rc != 0) { std::fprintf(stderr, "%s\n", bling_last_error()); return 1; }
      std::printf("pass %d: %.1f ms, %llu photons, %llu splats, %.1f Mrays/s\n", p, st.ms_total, (unsigned long long)st.photons,
                  (unsigned long long)st.splats, (st.photon_rays + st.shadow_rays) / (st.ms_total * 1e3));
      const float sw = 1.f / (float)((long long)p * d->light.pass_photons);
      char name[512];
      std::snprintf(name, sizeof name, "%s-%05d", out, p);
      std::printf("Writing %s...\n", name);
      if ((device_film ? write_pass_device_film(ctx, dev_develop, df, name, film.data(), sw, w, h, rgb)
                       : write_pass(ctx, dev_develop, name, film.data(), splat.data(), sw, w, h, rgb)) != 0) return 1;
    }
    bling_destroy(ctx);
    bling_host_free(hs);
    return 0;
  }
  if (d->config.renderer == BLING_RENDERER_METROPOLIS) {
    // instance Renderer Metropolis (Renderer/Metropolis.hs:76-120): the film stays empty, every pass adds
    // its splats, and the image of pass p weighs them with bnext / p, bnext = lerp (1 / p) b b' from b = 1
    std::vector<float> splat((size_t)w * h * 3, 0.f);
    float b = 1.f;
    for (int p = 1; p <= passes; ++p) {
      bling_mlt_stats st;
      const int rc = device_film ? bling_mlt_pass_device(ctx, 0x0B11A6u, (uint32_t)p, splat_flags, df.splat, &st)
                                 : bling_mlt_pass(ctx, 0x0B11A6u, (uint32_t)p, splat.data(), &st);
      if (rc != 0) { std::fprintf(stderr, "%s\n", bling_last_error()); return 1; }
      const float t = 1.f / (float)p;
      b = (1.f - t) * b + t * (float)st.b;
      std::printf("pass %d: %.1f ms, %llu mutations (%llu large, %llu accepted), b = %g, %.2f Mmutations/s\n", p, st.ms_total,
                  (unsigned long long)st.mutations, (unsigned long long)st.large_steps, (unsigned long long)st.accepted, b,
                  st.mutations / (st.ms_total * 1e3));
      const float sw = b / (float)p;
      char name[512];
      std::snprintf(name, sizeof name, "%s-%05d", out, p);
      std::printf("Writing %s...\n", name);
      if ((device_film ? write_pass_device_film(ctx, dev_develop, df, name, film.data(), sw, w, h, rgb)
                       : write_pass(ctx, dev_develop, name, film.data(), splat.data(), sw, w, h, rgb)) != 0) return 1;
    }
    bling_destroy(ctx);
    bling_host_free(hs);
    return 0;
  }
  if (d->config.renderer == BLING_RENDERER_SPPM) {
    // instance Renderer SPPM (Renderer/SPPM.hs:466-480): every pass adds its eye samples to the film and its
    // photons' splats to the splat image, and the image of pass k weighs the splats with 1 / (threads k sn^2) (:460)
    std::vector<float> splat((size_t)w * h * 3, 0.f);
    for (int p = 1; p <= passes; ++p) {
      bling_sppm_stats st;
      const int rc = device_film ? bling_sppm_pass_device(ctx, 0x0B11A6u, (uint32_t)p, splat_flags, df.film, df.splat, &st)
                                 : bling_sppm_pass(ctx, 0x0B11A6u, (uint32_t)p, film.data(), splat.data(), &st);
      if (rc != 0) { std::fprintf(stderr, "%s\n", bling_last_error()); return 1; }
      std::printf("pass %d: %.1f ms, %llu hit points, %llu photons, %llu pairs\n", p, st.ms_total, (unsigned long long)st.hitpoints,
                  (unsigned long long)st.photons, (unsigned long long)st.photon_hits);
      const float sw = bling_host_sppm_splat_weight(&d->config, p, nullptr);
      char name[512];
      std::snprintf(name, sizeof name, "%s-%05d", out, p);
      std::printf("Writing %s...\n", name);
      // host develop of device images: the film comes back here, the splat image in write_pass_device_film
      if (device_film && !dev_develop &&
          hipMemcpy(film.data(), df.film, film.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
        std::fprintf(stderr, "film: copy failed\n");
        return 1;
      }
      if ((device_film ? write_pass_device_film(ctx, dev_develop, df, name, film.data(), sw, w, h, rgb)
                       : write_pass(ctx, dev_develop, name, film.data(), splat.data(), sw, w, h, rgb)) != 0) return 1;
    }
    bling_destroy(ctx);
    bling_host_free(hs);
    return 0;
  }
  if (seams) {
    // prender (Rendering.hs:118-134) written by a caller: splitWindow's 16 x 16 windows of the sample extent, their
    // samples and rays from the sampler and camera seam, surfaceLi along them, the windows' tiles onto the film --
    // three device calls a pass; only the windows go up, only the film comes back to be written.
    bling_image_desc idesc{w, h, d->filter};
    int32_t e[4];
    bling_host_image_extent(&idesc, e);
    std::vector<bling_image_window> wins;
    std::vector<uint64_t> first(1, 0);
    for (int wy = e[2]; wy <= e[3]; wy += 16)
      for (int wx = e[0]; wx <= e[1]; wx += 16) {
        const bling_image_window wn{wx, std::min(wx + 15, e[1]), wy, std::min(wy + 15, e[3])};
        wins.push_back(wn);
        first.push_back(first.back() + (uint64_t)(wn.x1 - wn.x0 + 1) * (uint64_t)(wn.y1 - wn.y0 + 1) * (uint64_t)d->config.spp);
      }
    const size_t n = first.back();
    struct Bufs {
      void *xy = nullptr, *ids = nullptr, *rays = nullptr, *L = nullptr, *film = nullptr;
      ~Bufs() { (void)hipFree(xy); (void)hipFree(ids); (void)hipFree(rays); (void)hipFree(L); (void)hipFree(film); }
    } b;
    if (hipSetDevice(device) != hipSuccess || hipMalloc(&b.xy, n * 8) != hipSuccess || hipMalloc(&b.ids, n * 8) != hipSuccess ||
        hipMalloc(&b.rays, n * 28) != hipSuccess || hipMalloc(&b.L, n * 64) != hipSuccess ||
        hipMalloc(&b.film, film.size() * sizeof(float)) != hipSuccess || hipMemset(b.film, 0, film.size() * sizeof(float)) != hipSuccess) {
      std::fprintf(stderr, "--seams: %s\n", hipGetErrorString(hipGetLastError()));
      return 1;
    }
    for (int p = 1; p <= passes; ++p) {
      bling_camera_stats cs;
      bling_li_stats ls;
      bling_image_stats is;
      if (bling_camera_samples_device(ctx, 0x0B11A6u, (uint32_t)p, wins.data(), first.data(), wins.size(), b.xy, b.ids, b.rays, nullptr, &cs) != 0 ||
          bling_surface_li_device(ctx, 0x0B11A6u, (uint32_t)p, b.rays, b.ids, n, b.L, &ls) != 0 ||
          bling_image_add_windowed_device(ctx, &idesc, BLING_IMAGE_ADD, wins.data(), first.data(), wins.size(), b.xy, b.L, n, b.film,
                                          nullptr, &is) != 0) {
        std::fprintf(stderr, "%s\n", bling_last_error());
        return 1;
      }
      const uint64_t rays = ls.rays + ls.rays_continuation + ls.rays_mis + ls.rays_shadow;
      const double ms = cs.ms_total + ls.ms_total + is.ms;
      std::printf("pass %d: %.1f ms (camera %.2f, surface_li %.1f, film %.1f), %llu samples, %.1f Mrays/s\n", p, ms, cs.ms_total,
                  ls.ms_total, is.ms, (unsigned long long)cs.samples, rays / (ms * 1e3));
      if (hipMemcpy(film.data(), b.film, film.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
        std::fprintf(stderr, "film: copy failed\n");
        return 1;
      }
      char name[512];
      std::snprintf(name, sizeof name, "%s-%05d", out, p);
      std::printf("Writing %s...\n", name);
      if (write_pass(ctx, dev_develop, name, film.data(), nullptr, 0.f, w, h, rgb) != 0) return 1;
    }
    bling_destroy(ctx);
    bling_host_free(hs);
    return 0;
  }
  for (int p = 1; p <= passes; ++p) {
    bling_pass_params pp{0x0B11A6u, (uint32_t)p, 0, 1, 1, 0, film_ordered ? BLING_PASS_ORDERED_FILM : 0u};
    bling_stats st;
    if (bling_render_pass(ctx, &pp, film.data(), &st) != 0) { std::fprintf(stderr, "%s\n", bling_last_error()); return 1; }
    uint64_t rays = st.rays_camera + st.rays_continuation + st.rays_mis + st.rays_shadow;
    std::printf("pass %d: %.1f ms, %llu samples, %.1f Mrays/s\n", p, st.ms_total, (unsigned long long)st.camera_samples,
                rays / (st.ms_total * 1e3));
    // progressWriter (IO/Progress.hs:23-36): <out>-NNNNN.png and .hdr after every pass
    char name[512];
    std::snprintf(name, sizeof name, "%s-%05d", out, p);
    std::printf("Writing %s...\n", name);
    if (write_pass(ctx, dev_develop, name, film.data(), nullptr, 0.f, w, h, rgb) != 0) return 1;
  }
  bling_destroy(ctx);
  bling_host_free(hs);
  return 0;
}
