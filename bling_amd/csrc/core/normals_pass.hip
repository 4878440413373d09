// normals_pass.hip -- host driver of one wave of the normal-map integrator (normals.h): the scene's
// planned closest-hit launch over the camera rays k_raygen left in the wave, then k_shade_nm.
//
// The kernels are instantiated per feature profile (core_internal.h kProfiles), as the Path kernels
// are: profiles 0-2 compile here with the driver, profiles 3-4 in normals_pass_b.hip and profile 5
// in normals_pass_c.hip, which include this file with BLING_NM_UNIT set to 1 / 2, so the build runs
// the three side by side.  The closest-hit kernels are the Path pipeline's own templates
// (wavefront.h), instantiated without the traversal counters.
#ifndef BLING_NM_UNIT
#define BLING_NM_UNIT 0
#endif
#if !defined(BCR_HUGE_ARGS) && BLING_NM_UNIT != 2
#define BCR_HUGE_ARGS 0   // profiles 0-4: no computed textures, sin / cos arguments are angles (cr_math.h)
#endif
#include "core_internal.h"
#include "normals.h"

namespace bcore {

// The plan TraceLaunch (core_wave.h) picks for the scene -- exhaustive, wave-coherent packets, BVH4
// all-LDS or LDS prefix with global fallback, the fractal march -- for the closest-hit queue alone.
template <uint32_t F, bool ALLL>
int normals_wave_t(bling_ctx* c, WaveState W, uint32_t n, WaveTiming* tm) {
  hipStream_t s = c->stream;
  const DevScene* d = c->dscene.p;
  Counters* C = c->counters.p;
  int launches = 0;
  tm->timed(WaveTiming::Closest, s, [&] {     // tm is never NULL here: normals_wave_prof substitutes an empty one
    if constexpr (!(F & FT_FRACTAL)) {
      if (c->S.bf_tris + c->S.bf_shapes > 0) {
        const unsigned g = persistent_grid(k_trace_closest_bf<F, false>, 0, n);
        k_trace_closest_bf<F, false><<<g, 256, 0, s>>>(d, W, C);
        ++launches;
        return;
      }
      if (c->S.pkt_n > 0) {
        const size_t lds = sizeof(DevShape) * c->S.lds4_shapes;             // packet_lds
        const unsigned g = persistent_grid(k_trace_closest_pkt<F, false>, lds, n);
        k_trace_closest_pkt<F, false><<<g, 256, lds, s>>>(d, W, C);
        ++launches;
        return;
      }
    }
    if constexpr ((F & FT_FRACTAL) != 0) {
      // Mandelbulb scenes: the march of the queue precedes its traversal (wavefront.h k_march_jobs);
      // Julia scenes and deep iteration counts march inside the traversal
      const bool premarch = W.march_t != nullptr && c->S.fractal.kind == BLING_FRACTAL_MANDELBULB && c->S.fractal.iterations < 32767;
      if (premarch) {
        const unsigned gm = persistent_grid(k_march_jobs<F, false, false>, 0, n);
        k_march_jobs<F, false, false><<<gm, 256, 0, s>>>(d, W, C);
        ++launches;
      } else {
        W.march_t = nullptr;
      }
    } else {
      W.march_t = nullptr;
    }
    const size_t lds = use_bvh4<F>() ? c->lds_trace4 : c->lds_trace;
    const unsigned g = persistent_grid(k_trace_closest<F, false, ALLL>, lds, n);
    if constexpr (use_bvh4<F>()) {
      if ((size_t)g * 256 > c->S.stack4_lanes && c->S.stack4_need > c->S.stack4_lds)
        throw std::runtime_error("BVH4 stack overflow rows sized for fewer lanes than the traversal grid");
    }
    k_trace_closest<F, false, ALLL><<<g, 256, lds, s>>>(d, W, C);
    ++launches;
  });
  tm->timed(WaveTiming::Shade, s, [&] { k_shade_nm<F><<<grid_for(n), 256, 0, s>>>(d, W, n, C); });
  return launches + 1;
}

template <uint32_t F>
int normals_wave_prof(bling_ctx* c, const WaveState& W, uint32_t n, WaveTiming* tm) {
  WaveTiming none;
  const bool all = use_bvh4<F>() ? c->lds_all4 : c->lds_all;
  return all ? normals_wave_t<F, true>(c, W, n, tm ? tm : &none) : normals_wave_t<F, false>(c, W, n, tm ? tm : &none);
}

#define BLING_NM_ARGS bling_ctx*, const WaveState&, uint32_t, WaveTiming*
#if BLING_NM_UNIT == 1
template int normals_wave_prof<kProfiles[3]>(BLING_NM_ARGS);
template int normals_wave_prof<kProfiles[4]>(BLING_NM_ARGS);
#elif BLING_NM_UNIT == 2
template int normals_wave_prof<kProfiles[5]>(BLING_NM_ARGS);
#else
extern template int normals_wave_prof<kProfiles[3]>(BLING_NM_ARGS);
extern template int normals_wave_prof<kProfiles[4]>(BLING_NM_ARGS);
extern template int normals_wave_prof<kProfiles[5]>(BLING_NM_ARGS);

int normals_wave(bling_ctx* c, const WaveState& W, uint32_t n, WaveTiming* tm) {
  if (n == 0) return 0;
  int launches = 0;
  with_profile(c->features, [&](auto prof) { launches = normals_wave_prof<decltype(prof)::value>(c, W, n, tm); });
  return launches;
}
#endif

}  // namespace bcore
