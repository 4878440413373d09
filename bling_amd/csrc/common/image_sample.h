// image_sample.h -- the per-sample arithmetic of the image API (addSample, addUnfilteredSample, splatSample:
// Image.hs:201-299): the drop rules, XYZ of a 16-band spectrum, the clipped pixel range of a sample along one
// axis and the filter table index, and the geometry of a window's tile image (mkImageTile, addTile's guard:
// Image.hs:108-120, 178-199).  Product code shared by the host library's sequential restatements
// (bling_host_image_add_samples, bling_host_image_add_windowed) and the HIP kernels (core/image_ops.hip), so
// that both make the same decisions; every operation is binary32 in the reference's order.  Compile with -ffp-contract=off.
#pragma once
#include <stdint.h>
#include "spectral_data.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BLING_IMG_HD __host__ __device__ inline
#else
#include <cmath>
#define BLING_IMG_HD inline
#endif

namespace bimgs {

// ops of the image calls (BLING_IMAGE_* of include/bling.h)
enum : int { OP_ADD = 0, OP_UNFILTERED = 1, OP_SPLAT = 2 };

constexpr float kMaxPosition = 1048576.f;   // 2^20: beyond it (or non-finite) a position is dropped

BLING_IMG_HD bool finite_f(float v) { return v - v == 0.f; }   // false for NaN and +-Inf
BLING_IMG_HD bool position_ok(float x, float y) {
  return finite_f(x) && finite_f(y) && fabsf(x) <= kMaxPosition && fabsf(y) <= kMaxPosition;
}
BLING_IMG_HD bool spectrum_ok(const float* b) {                 // not sNaN, not sInfinite
  bool ok = true;
  for (int i = 0; i < 16; ++i) ok = ok && finite_f(b[i]);
  return ok;
}
// spectrumToXYZ (Spectrum.hs:349-355): three left folds from 0, each divided by the Y sum
BLING_IMG_HD void to_xyz(const float* b, float* x, float* y, float* z) {
  float ax = 0.f, ay = 0.f, az = 0.f;
  for (int i = 0; i < 16; ++i) {
    ax = ax + BLING_CIE_X_BANDS[i] * b[i];
    ay = ay + BLING_CIE_Y_BANDS[i] * b[i];
    az = az + BLING_CIE_Z_BANDS[i] * b[i];
  }
  *x = ax / BLING_CIE_Y_SUM; *y = ay / BLING_CIE_Y_SUM; *z = az / BLING_CIE_Y_SUM;
}

// addSample's range along one axis of an image of n pixels: lo = max 0 (ceiling (d - fw)), hi = min (n - 1)
// (floor (d + fw)), clamped in binary32 before the conversion so that a huge filter cannot overflow the
// integer; empty when hi < lo.  d = position - 0.5.
BLING_IMG_HD void filter_range(float d, float fw, int n, int* lo, int* hi) {
  const float a = ceilf(d - fw), b = floorf(d + fw);
  *lo = a <= 0.f ? 0 : (a >= (float)n ? n : (int)a);
  *hi = b >= (float)(n - 1) ? n - 1 : (b < 0.f ? -1 : (int)b);
}
// the single pixel of addUnfilteredSample / splatSample along one axis: floor s, or -1 outside [0, n)
BLING_IMG_HD int floor_pixel(float s, int n) {
  const float f = floorf(s);
  return (f >= 0.f && f < (float)n) ? (int)f : -1;
}
// the pixel rectangle a sample reaches (op BLING_IMAGE_*); false when it reaches none
BLING_IMG_HD bool sample_rect(int op, float sx, float sy, float fw, float fh, int w, int h, int* x0, int* x1, int* y0, int* y1) {
  if (op == OP_ADD) {
    filter_range(sx - 0.5f, fw, w, x0, x1);
    filter_range(sy - 0.5f, fh, h, y0, y1);
    return *x0 <= *x1 && *y0 <= *y1;
  }
  *x0 = *x1 = floor_pixel(sx, w);
  *y0 = *y1 = floor_pixel(sy, h);
  return *x0 >= 0 && *y0 >= 0;
}
// mkImageTile (Image.hs:108-120) of a SampleWindow x0..x1, y0..y1: the tile image's offset px = max 0 x0 and
// size w = x1 - px + floor (0.5 + fw), likewise py and h.  False when w or h is below 1 (MV.replicate of a
// negative length) or beyond an int32.
struct Tile { int px, py, w, h; };
BLING_IMG_HD bool make_tile(int x0, int x1, int y0, int y1, float fw, float fh, Tile* t) {
  const float gx = floorf(0.5f + fw), gy = floorf(0.5f + fh);
  if (!(gx < 1073741824.f && gy < 1073741824.f)) return false;
  t->px = x0 > 0 ? x0 : 0;
  t->py = y0 > 0 ? y0 : 0;
  const long long w = (long long)x1 - t->px + (long long)gx, h = (long long)y1 - t->py + (long long)gy;
  if (w < 1 || h < 1 || w > 2147483647ll || h > 2147483647ll) return false;
  t->w = (int)w; t->h = (int)h;
  return true;
}
// the film pixels addTile (Image.hs:178-199) adds the tile to: x + px < width, y + py < height; x1 < x0 or
// y1 < y0 when there are none.  Inclusive.
struct Rect { int x0, y0, x1, y1; };
BLING_IMG_HD Rect tile_cover(const Tile& t, int w, int h) {
  const long long ex = (long long)t.px + t.w, ey = (long long)t.py + t.h;
  return Rect{t.px, t.py, (int)(ex < w ? ex : w) - 1, (int)(ey < h ? ey : h) - 1};
}
BLING_IMG_HD bool rect_empty(const Rect& r) { return r.x1 < r.x0 || r.y1 < r.y0; }
// sample_rect of a sample added to a tile image, for the film pixels the tile is added to (cover): addSample's
// x0 = max ox (ceiling (dx - fw)), x1 = min (ox + w - 1) (floor (dx + fw)), the unfiltered ops' floor sx - ox in
// [0, w), each met with addTile's guard.  False when the sample reaches none of them.
BLING_IMG_HD bool sample_rect_in(int op, float sx, float sy, float fw, float fh, int w, int h, const Rect& cover, int* x0, int* x1,
                                 int* y0, int* y1) {
  if (!sample_rect(op, sx, sy, fw, fh, w, h, x0, x1, y0, y1)) return false;
  if (*x0 < cover.x0) *x0 = cover.x0;
  if (*x1 > cover.x1) *x1 = cover.x1;
  if (*y0 < cover.y0) *y0 = cover.y0;
  if (*y1 > cover.y1) *y1 = cover.y1;
  return *x0 <= *x1 && *y0 <= *y1;
}
// index into one axis of the 16 x 16 filter table: min (floor |(p - d) * inv * 16|) 15
BLING_IMG_HD int table_index(int p, float d, float inv) {
  const float t = fabsf(((float)p - d) * inv * 16.f);
  return t < 15.f ? (int)floorf(t) : 15;     // a NaN (0 * inf of a denormal filter width) takes the last entry
}

}  // namespace bimgs
