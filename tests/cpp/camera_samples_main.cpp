// camera_samples_main.cpp -- a stand-alone caller of bling_host_camera_samples for sanitizer builds of the host
// library's source (no Python, no GPU):
//   g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -I include \
//       tests/cpp/camera_samples_main.cpp bling_amd/csrc/host/loader.cpp -lz -o camera_samples_main
//   ./camera_samples_main fixtures/scenes/cornell-box.bling
// C1 at 16 x 16: splitWindow's windows, a repeated, a nested and two empty ones; every output, then each alone;
// then the refusals.  Exits 0 when the outputs agree among themselves and every refusal is refused.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "bling_host.h"

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s cornell-box.bling\n", argv[0]); return 2; }
  bling_host_scene* hs = nullptr;
  if (bling_host_load(argv[1], "image=16,16;stratified=2,2;path=15,3;force_path=1", &hs) != 0) {
    std::fprintf(stderr, "%s\n", bling_host_last_error());
    return 1;
  }
  const bling_scene_desc* d = bling_host_desc(hs);
  bling_image_desc id{d->config.width, d->config.height, d->filter};
  int32_t e[4];
  bling_host_image_extent(&id, e);
  std::vector<bling_image_window> w;
  for (int y = e[2]; y <= e[3]; y += 16)
    for (int x = e[0]; x <= e[1]; x += 16) w.push_back({x, std::min(x + 15, e[1]), y, std::min(y + 15, e[3])});
  w.push_back(w[1]);
  w.push_back({e[0] + 2, e[0] + 4, e[2] + 1, e[2] + 1});
  w.push_back({5, 4, 0, 3});
  w.push_back({0, 3, 7, 2});
  std::vector<uint64_t> first(1, 0);
  for (const auto& q : w)
    first.push_back(first.back() + (q.x1 < q.x0 || q.y1 < q.y0 ? 0 : (uint64_t)(q.x1 - q.x0 + 1) * (q.y1 - q.y0 + 1) * d->config.spp));
  const size_t n = first.back();
  std::vector<float> xy(2 * n), rays(7 * n), lens(2 * n), xy2(2 * n), rays2(7 * n), lens2(2 * n);
  std::vector<uint32_t> ids(2 * n), ids2(2 * n);
  int bad = 0;
  bad += bling_host_camera_samples(d, 0x0B11A6u, 0, w.data(), first.data(), w.size(), xy.data(), ids.data(), rays.data(), lens.data()) != 0;
  bad += bling_host_camera_samples(d, 0x0B11A6u, 0, w.data(), first.data(), w.size(), xy2.data(), nullptr, nullptr, nullptr) != 0;
  bad += bling_host_camera_samples(d, 0x0B11A6u, 0, w.data(), first.data(), w.size(), nullptr, ids2.data(), nullptr, nullptr) != 0;
  bad += bling_host_camera_samples(d, 0x0B11A6u, 0, w.data(), first.data(), w.size(), nullptr, nullptr, rays2.data(), nullptr) != 0;
  bad += bling_host_camera_samples(d, 0x0B11A6u, 0, w.data(), first.data(), w.size(), nullptr, nullptr, nullptr, lens2.data()) != 0;
  bad += std::memcmp(xy.data(), xy2.data(), 8 * n) != 0 || std::memcmp(ids.data(), ids2.data(), 8 * n) != 0 ||
         std::memcmp(rays.data(), rays2.data(), 28 * n) != 0 || std::memcmp(lens.data(), lens2.data(), 8 * n) != 0;
  // refusals: outside the extent, a first off by one, overlapping outputs, no windows at all is fine
  bling_image_window out{e[0] - 1, e[0], e[2], e[2]};
  uint64_t f2[2] = {0, 2ull * d->config.spp};
  bad += bling_host_camera_samples(d, 1, 0, &out, f2, 1, xy2.data(), nullptr, nullptr, nullptr) == 0;
  first[1] += 1;
  bad += bling_host_camera_samples(d, 1, 0, w.data(), first.data(), w.size(), xy2.data(), nullptr, nullptr, nullptr) == 0;
  first[1] -= 1;
  bad += bling_host_camera_samples(d, 1, 0, w.data(), first.data(), w.size(), xy2.data(), nullptr, nullptr, xy2.data() + 2) == 0;
  uint64_t zero = 0;
  bad += bling_host_camera_samples(d, 1, 0, nullptr, &zero, 0, nullptr, nullptr, nullptr, nullptr) != 0;
  bad += std::memcmp(xy.data(), xy2.data(), 8 * n) != 0;          // the refused calls wrote nothing
  std::printf("%zu samples of %zu windows, %d failures\n", n, w.size(), bad);
  bling_host_free(hs);
  return bad != 0;
}
