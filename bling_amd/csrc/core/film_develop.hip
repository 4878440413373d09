// film_develop.hip -- develops a device film into a display image on the device: getPixel + xyzToRgb
// (Image.hs:302-315, Spectrum.hs:162-168) as linear RGB, rgbPixels' 8-bit bytes (Image.hs:317-331) and
// writeRgbe's RGBE bytes (IO/Bitmap.hs:36-41).  It restates the host library's three loops
// (host/loader.cpp bling_host_film_splat_to_rgb, bling_host_rgb_pixels_splat, bling_host_write_hdr)
// operation for operation, so its output equals theirs bit for bit; the unit is compiled with
// -ffp-contract=off like every other one, and float division is the correctly rounded one.
//
// One thread per pixel of the (clipped) window, plain stores: 16 B of film and, with a splat buffer,
// 12 B more read per pixel, 3 / 4 / 12 B written.  At 1024^2 the launch costs about as much as the
// traffic, so nothing is packed.
#include "core_internal.h"

namespace bcore {
namespace {

// the host's std::max(a, b): a < b ? b : a (NaN in b is dropped, NaN in a is kept)
__device__ inline float std_max(float a, float b) { return a < b ? b : a; }

// (unsigned char)(x) of the host's x86 build: truncate to int32, keep the low 8 bits (256 wraps to 0).
// Every x here lies in [0, 256] except the NaN an +Inf channel makes, which is written as 0.
__device__ inline uint32_t low_byte(float x) { return x == x ? (uint32_t)(int)x & 0xFFu : 0u; }

template <int FMT>
__global__ void __launch_bounds__(256) k_film_develop(const float* __restrict__ film, const float* __restrict__ splat,
                                                      float sw, const float* __restrict__ tab, int w, int x0, int y0,
                                                      int ww, uint32_t n, int out_aligned4, void* __restrict__ out) {
  // rgbPixels' thresholds (common/gamma_table.h): 255 ascending floats and a NaN that no value reaches
  __shared__ float t[256];
  if (FMT == BLING_DEVELOP_RGB8) {
    t[threadIdx.x] = tab[threadIdx.x];
    __syncthreads();
  }
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const size_t p = (size_t)(y0 + (int)(i / (uint32_t)ww)) * (size_t)w + (size_t)(x0 + (int)(i % (uint32_t)ww));

  // bling_host_film_splat_to_rgb
  const float W = film[4 * p], X = film[4 * p + 1], Y = film[4 * p + 2], Z = film[4 * p + 3];
  const float sr = splat ? splat[3 * p] : 0.f, sg = splat ? splat[3 * p + 1] : 0.f, sb = splat ? splat[3 * p + 2] : 0.f;
  float x, y, z;
  if (W == 0.f) { x = sw * sr; y = sw * sg; z = sw * sb; }
  else { const float iw = 1.f / W; x = sw * sr + X * iw; y = sw * sg + Y * iw; z = sw * sb + Z * iw; }
  const float c[3] = {3.240479f * x - 1.537150f * y - 0.498535f * z,
                      (-0.969256f) * x + 1.875991f * y + 0.041556f * z,
                      0.055648f * x - 0.204043f * y + 1.057311f * z};

  if (FMT == BLING_DEVELOP_RGB_F32) {
    float* o = static_cast<float*>(out) + 3 * p;
    o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
  } else if (FMT == BLING_DEVELOP_RGB8) {
    // the byte is the number of thresholds <= v (NaN, finite negatives and +-0 pass none, +Inf all): a branch-free binary search of 8 steps over the 256
    // entries (the search never reads past t[255]: pos + step <= 256 before every probe)
    unsigned char* o = static_cast<unsigned char*>(out) + 3 * p;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      // powf (-Inf) (1 / 2.2) is +Inf: the host's byte of -Inf is 255, the one negative that is not 0
      const float v = c[k] == -INFINITY ? INFINITY : c[k];
      uint32_t pos = 0;
#pragma unroll
      for (uint32_t step = 128; step >= 1; step >>= 1) pos += t[pos + step - 1] <= v ? step : 0u;
      o[k] = (unsigned char)pos;
    }
  } else {
    // bling_host_write_hdr's loop.  m >= 1e-32f is never subnormal, so frexp is two bit fields; an
    // +Inf m (outside the contract) takes fraction 0.5 and exponent 129: sc = 0 and the bytes are
    // 0 for every channel and 1 for the exponent.
    const float r = std_max(0.f, c[0]), g = std_max(0.f, c[1]), b = std_max(0.f, c[2]);
    const float m = std_max(r, std_max(g, b));
    uint32_t e = 0;
    if (m >= 1e-32f) {
      const uint32_t mb = __float_as_uint(m);
      const int ex = (int)((mb >> 23) & 0xFFu) - 126;
      const float fr = __uint_as_float((mb & 0x007FFFFFu) | 0x3F000000u);
      const float sc = fr * 256.f / m;
      e = low_byte(r * sc) | low_byte(g * sc) << 8 | low_byte(b * sc) << 16 | ((uint32_t)(ex + 128) & 0xFFu) << 24;
    }
    if (out_aligned4) {
      static_cast<uint32_t*>(out)[p] = e;
    } else {
      unsigned char* o = static_cast<unsigned char*>(out) + 4 * p;
      o[0] = (unsigned char)e; o[1] = (unsigned char)(e >> 8); o[2] = (unsigned char)(e >> 16); o[3] = (unsigned char)(e >> 24);
    }
  }
}

}  // namespace

size_t develop_pixel_bytes(int format) {
  return format == BLING_DEVELOP_RGB_F32 ? 12 : format == BLING_DEVELOP_RGB8 ? 3 : 4;
}

namespace {
bool clip_window(int w, int h, const int32_t* win, int* x0, int* x1, int* y0, int* y1) {
  *x0 = std::max(win[0], 0); *x1 = std::min(win[1], w - 1);
  *y0 = std::max(win[2], 0); *y1 = std::min(win[3], h - 1);
  return *x0 <= *x1 && *y0 <= *y1;
}
}  // namespace

bool develop_clip(const bling_ctx* c, const int32_t* win, int* x0, int* x1, int* y0, int* y1) {
  return clip_window(c->S.width, c->S.height, win, x0, x1, y0, y1);
}

void develop_table(bling_ctx* c) {
  float t[256];
  bgamma::thresholds(t);
  t[255] = std::nanf("");
  c->gamma_tab.upload(t, 256);
}

// one launch on the context's stream; the caller synchronises
void develop_launch(bling_ctx* c, const bling_develop_params* dp, const float* film, const float* splat, void* out) {
  develop_launch(c, dp, c->S.width, c->S.height, film, splat, out);
}

void develop_launch(bling_ctx* c, const bling_develop_params* dp, int w, int h, const float* film, const float* splat, void* out) {
  int x0, x1, y0, y1;
  if (!clip_window(w, h, dp->window, &x0, &x1, &y0, &y1)) return;   // a window outside the image writes nothing
  const int ww = x1 - x0 + 1;
  const uint64_t n64 = (uint64_t)ww * (uint64_t)(y1 - y0 + 1);
  if (n64 > 0xFFFFFF00ull) throw std::invalid_argument("develop: window too large");
  const uint32_t n = (uint32_t)n64, blocks = (n + 255u) / 256u;
  const int a4 = ((uintptr_t)out & 3u) == 0;
  const float sw = dp->splat_weight, *tab = c->gamma_tab.p;
  hipStream_t s = c->stream;
  switch (dp->format) {
    case BLING_DEVELOP_RGB_F32: k_film_develop<BLING_DEVELOP_RGB_F32><<<blocks, 256, 0, s>>>(film, splat, sw, tab, w, x0, y0, ww, n, a4, out); break;
    case BLING_DEVELOP_RGB8: k_film_develop<BLING_DEVELOP_RGB8><<<blocks, 256, 0, s>>>(film, splat, sw, tab, w, x0, y0, ww, n, a4, out); break;
    default: k_film_develop<BLING_DEVELOP_RGBE><<<blocks, 256, 0, s>>>(film, splat, sw, tab, w, x0, y0, ww, n, a4, out); break;
  }
  HIPCHK(hipGetLastError());
}

}  // namespace bcore
