// camera_samples.h -- the sampler and camera seam on the host (bling_host_camera_samples, include/bling_host.h):
// `sample sampler window` (Sampling.hs:101-132) and fireRay (Camera.hs:49-76) for every sample of a list of
// SampleWindows, sequentially, in binary32.  The operations and their order are those of the device's
// camera_sample and fire_ray (core/dev_shade.h:65-105) with xpoint / xvector / normalize /
// concentric_sample_disk of core/dev_common.h, so k_cam_samples (core/cam_samples.h) gives the same bits;
// the counter RNG and sincosf are the shared headers themselves.  Compile with -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../../include/bling_scene.h"
#include "../common/cam_windows.h"
#include "../common/counter_rng.h"
#include "../common/cr_math.h"

namespace bhcam {

constexpr float PI = 3.14159265358979323846f;
constexpr float ALMOST_ONE = 0x1.fffffep-1f;

struct V3 { float x, y, z; };
inline V3 xpoint(const float* m, V3 p) {                             // Transform.hs:247-272
  const float xp = m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3];
  const float yp = m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7];
  const float zp = m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11];
  const float wp = m[12] * p.x + m[13] * p.y + m[14] * p.z + m[15];
  if (wp == 1.f) return {xp, yp, zp};
  return {xp / wp, yp / wp, zp / wp};
}
inline V3 xvector(const float* m, V3 v) {
  return {m[0] * v.x + m[1] * v.y + m[2] * v.z, m[4] * v.x + m[5] * v.y + m[6] * v.z, m[8] * v.x + m[9] * v.y + m[10] * v.z};
}
inline V3 normalize(V3 v) {
  const float sq = v.x * v.x + v.y * v.y + v.z * v.z;
  if (sq != 0.f) { const float il = 1.f / std::sqrt(sq); return {v.x * il, v.y * il, v.z * il}; }
  return {0.f, 1.f, 0.f};
}
inline void concentric_sample_disk(float u1, float u2, float* ox, float* oy) {   // Montecarlo.hs:389-406
  const float sx = u1 * 2.f - 1.f, sy = u2 * 2.f - 1.f;
  if (sx == 0.f && sy == 0.f) { *ox = 0.f; *oy = 0.f; return; }
  float r, th;
  if (sx >= -sy) {
    if (sx > sy) { if (sy > 0.f) { r = sx; th = sy / sx; } else { r = sx; th = 8.f + sy / sx; } }
    else { r = sy; th = 2.f - sx / sy; }
  } else if (sx <= sy) { r = -sx; th = 4.f - sy / (-sx); }
  else { r = -sy; th = 6.f + sx / (-sy); }
  const float theta = th * PI / 4.f;
  const bcr::SinCos sc = bcr::sincosf(theta);
  *ox = r * sc.c;
  *oy = r * sc.s;
}

// the sampler fields bling_scene_upload derives from the render configuration (core.hip)
struct Sampler {
  int32_t sampler, nu, spp;
  float inv_nu, inv_nv;
  explicit Sampler(const bling_render_config& c)
      : sampler(c.sampler), nu(c.nu), spp(c.spp), inv_nu(1.f / (float)c.nu), inv_nv(1.f / (float)c.nv) {}
};

inline float draw01(uint32_t skey, uint32_t dim) { return brng::u01(brng::draw(skey, dim)); }

// camera_sample (dev_shade.h): the pixel offsets (unshuffled stratified2D) and the shuffled lens strata of
// sample n of the pixel whose key is pkey (runSample, Sampling.hs:112-132), or four fresh draws
inline void camera_sample(const Sampler& S, uint32_t pkey, uint32_t n, float* ox, float* oy, float* lu, float* lv) {
  const uint32_t skey = brng::sample_key(pkey, n);
  if (S.sampler == BLING_SAMPLER_STRATIFIED) {
    const float du = S.inv_nu, dv = S.inv_nv;
    const uint32_t nq = n / (uint32_t)S.nu;
    const int u = (int)nq, v = (int)(n - nq * (uint32_t)S.nu);        // quotRem i nu (trap T5)
    const float ju = draw01(skey, brng::DIM_PIX), jv = draw01(skey, brng::DIM_PIX + 1);
    *ox = std::fmin(ALMOST_ONE, ((float)u + ju) * du);
    *oy = std::fmin(ALMOST_ONE, ((float)v + jv) * dv);
    const uint32_t j = brng::permute(n, (uint32_t)S.spp, brng::draw(brng::sample_key(pkey, brng::ALL_SAMPLES), brng::DIM_LENS_PERM));
    const float lj = draw01(skey, brng::DIM_LENS_J), lk = draw01(skey, brng::DIM_LENS_J + 1);
    const uint32_t jq = j / (uint32_t)S.nu;
    const int lu_i = (int)jq, lv_i = (int)(j - jq * (uint32_t)S.nu);
    *lu = std::fmin(ALMOST_ONE, ((float)lu_i + lj) * du);
    *lv = std::fmin(ALMOST_ONE, ((float)lv_i + lk) * dv);
    return;
  }
  *ox = draw01(skey, brng::DIM_RAND_CAM);
  *oy = draw01(skey, brng::DIM_RAND_CAM + 1);
  *lu = draw01(skey, brng::DIM_RAND_CAM + 2);
  *lv = draw01(skey, brng::DIM_RAND_CAM + 3);
}

// fireRay (Camera.hs:49-76): origin and direction; tmin = 0, tmax = infinity
inline void fire_ray(const bling_camera& cam, float ix, float iy, float lu, float lv, V3* o, V3* d) {
  if (cam.kind == BLING_CAM_ENVIRONMENT) {
    const float t = PI * iy / cam.yres, p = 2.f * PI * ix / cam.xres;
    const bcr::SinCos st = bcr::sincosf(t), sp = bcr::sincosf(p);
    *o = xpoint(cam.c2w, V3{0.f, 0.f, 0.f});
    *d = xvector(cam.c2w, V3{st.s * sp.c, st.c, st.s * sp.s});
    return;
  }
  const V3 pc = xpoint(cam.r2c, V3{ix, iy, 0.f});
  V3 ro{0.f, 0.f, 0.f}, rd = normalize(pc);
  if (cam.lens_radius > 0.f) {
    float dx, dy;
    concentric_sample_disk(lu, lv, &dx, &dy);
    const V3 lo{dx * cam.lens_radius, dy * cam.lens_radius, 0.f};
    const float ft = cam.focal_distance / rd.z;
    const V3 pf{ro.x + rd.x * ft, ro.y + rd.y * ft, ro.z + rd.z * ft};
    ro = lo;
    rd = normalize(V3{pf.x - lo.x, pf.y - lo.y, pf.z - lo.z});
  }
  *o = xpoint(cam.c2w, ro);
  *d = xvector(cam.c2w, rd);
}

// Every sample of the (already checked) windows, window after window, y outer, x inner, n innermost
// (coverWindow's order); n_total = first[n_windows] is the stride of the ray planes.  Any output may be NULL.
inline void run(const bling_scene_desc& D, uint32_t seed, uint32_t pass, const bling_image_window* windows,
                const uint64_t* first, size_t n_windows, float* xy, uint32_t* ids, float* rays, float* lens) {
  const Sampler S(D.config);
  const bcam::Extent e = bcam::sample_extent(D);
  const int32_t ext_w = e.x1 - e.x0 + 1;
  const uint64_t n_total = first[n_windows];
  for (size_t k = 0; k < n_windows; ++k) {
    const bling_image_window& w = windows[k];
    if (bcam::empty(w)) continue;
    uint64_t i = first[k];
    for (int32_t iy = w.y0; iy <= w.y1; ++iy)
      for (int32_t ix = w.x0; ix <= w.x1; ++ix) {
        const uint32_t pixel = (uint32_t)((iy - e.y0) * ext_w + (ix - e.x0));
        const uint32_t pkey = brng::pixel_key(seed, pass, pixel);
        for (uint32_t n = 0; n < (uint32_t)S.spp; ++n, ++i) {
          float ox, oy, lu, lv;
          camera_sample(S, pkey, n, &ox, &oy, &lu, &lv);
          const float imx = (float)ix + ox, imy = (float)iy + oy;
          if (xy) { xy[2 * i] = imx; xy[2 * i + 1] = imy; }
          if (ids) { ids[2 * i] = pixel; ids[2 * i + 1] = n; }
          if (lens) { lens[2 * i] = lu; lens[2 * i + 1] = lv; }
          if (rays) {
            V3 o, d;
            fire_ray(D.camera, imx, imy, lu, lv, &o, &d);
            rays[i] = o.x; rays[n_total + i] = o.y; rays[2 * n_total + i] = o.z;
            rays[3 * n_total + i] = d.x; rays[4 * n_total + i] = d.y; rays[5 * n_total + i] = d.z;
            rays[6 * n_total + i] = 0.f;
          }
        }
      }
  }
}

}  // namespace bhcam
