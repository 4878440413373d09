// gamma_table.h -- rgbPixels' float -> 8-bit step (Image.hs:317-331) as a table of 255 thresholds.
//
// The host's byte of a linear channel v is nearbyint(hmin(1, hmax(0, powf(v, 1/2.2f))) * 255).  The
// device has no powf that agrees with glibc's in every last ulp (cr_math.h), so it does not evaluate
// the expression: it counts the thresholds t[k] <= v, where t[k] is the smallest binary32 whose host
// byte is at least k + 1.  The table is made by the host expression itself, bisecting over the bit
// patterns of [+0, 1]; it reproduces the expression for every v as long as the expression is monotone
// in v (tools/gamma_monotone.cpp walks every binary32 of [0, 1]).  NaN, finite
// negatives and +-0 count no threshold (byte 0, as GHC's max gives), +Inf and everything >= 1 count all
// 255.  One value is not a count: powf(-Inf, 1/2.2f) is +Inf, so the host's byte of -Inf is 255, and a
// lookup takes -Inf as +Inf.
//
// Host code only: the loader and the core's host side both include it, so both build the same table.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

namespace bgamma {

// the byte of bling_host_rgb_pixels[_splat] for one linear channel value
inline unsigned char host_byte(float v) {
  const float xg = 1.f / 2.2f;                                    // gamma x = let x' = 1 / x
  auto hmax = [](float a, float b) { return a <= b ? b : a; };    // GHC Ord Float max / min
  auto hmin = [](float a, float b) { return a <= b ? a : b; };
  float g = std::pow(v, xg);                                      // r ** x' (powf)
  float c = hmin(1.f, hmax(0.f, g)) * 255.f;
  return (unsigned char)(int)std::nearbyint(c);                   // round: half to even
}

inline float from_bits(uint32_t b) { float f; std::memcpy(&f, &b, sizeof f); return f; }

// out255[k] = the smallest binary32 v with host_byte(v) >= k + 1, k = 0 .. 254
inline void thresholds(float* out255) {
  for (int k = 0; k < 255; ++k) {
    uint32_t lo = 0x00000000u, hi = 0x3F800000u;   // host_byte(+0) = 0 < k + 1 <= 255 = host_byte(1)
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if ((int)host_byte(from_bits(mid)) >= k + 1) hi = mid; else lo = mid;
    }
    out255[k] = from_bits(hi);
  }
}

}  // namespace bgamma
