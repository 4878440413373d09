// coverage.h -- what a restatement's light paths met, test infrastructure only (included by
// lighttracer_ref.cpp and bidir_ref.cpp after the oracle's translation unit, and through the latter
// by mlt_ref.cpp).  tests/test_adjoint_scenes.py holds every generated scene of
// tests/adjoint_scenes.py to a floor on the counter it is about, so that a device test on that scene
// cannot pass without the adjoint branch having run.  The counters change nothing the restatements
// compute; the slots' order is tests/cov_ref.py's COV_NAMES.
#pragma once

enum {
  COV_VERTS,          // light-path vertices: sampleAdjBsdf calls
  COV_SHADING,        // ... whose shading normal is not the geometric normal (|sideTest| scales f)
  COV_BUMP,           // ... on a bump-mapped material
  COV_LAMB,           // the BxDF sampleAdjBsdf chose, by kind: cosSample (Diffuse.hs:14-22)
  COV_OREN,           // Oren-Nayar's s True (Diffuse.hs:44-49)
  COV_LAMB_BTDF,      // the two through brdfToBtdf (Reflection.hs:188-195)
  COV_OREN_BTDF,
  COV_MICRO_DIEL,     // mkMicrofacet s True (Microfacet.hs:42-54) with frDielectric
  COV_MICRO_COND,     // ... with frConductor
  COV_SREFL,          // specRefl
  COV_SREFL_COND,     // specRefl with frConductor (shinyMetal's second lobe)
  COV_STRANS,         // sampleSpecTrans True
  COV_FBLEND_ISO,     // mkFresnelBlend s True (Microfacet.hs:88-101), equal exponents
  COV_FBLEND_ANISO,   // ... unequal exponents
  COV_FBLEND_DEPTH,   // ... with an absorbing depth > 0
  COV_FRACTAL,        // vertices on a fractal primitive (the distance-estimator march found them)
  COV_ENV_RAYS,       // light rays emitted by an infinite light with an image map
  COV_N
};

struct Cov {
  uint64_t c[COV_N] = {};
  void add(const Cov& o) { for (int i = 0; i < COV_N; ++i) c[i] += o.c[i]; }
};

// one sampleAdjBsdf bsdf wi uc _ at hit h: the component index is sampleBsdf''s sNum over bxdfAll
inline void cov_vertex(Cov& C, const Scene& Sc, const Hit& h, const Bsdf& bs, float uc) {
  C.c[COV_VERTS]++;
  const V ns = bs.cs.n;
  if (ns.x != bs.ng.x || ns.y != bs.ng.y || ns.z != bs.ng.z) C.c[COV_SHADING]++;
  const Prim& pr = Sc.prims[h.prim];                                // hit_bsdf's material
  const int mat = pr.kind == 0 ? Sc.d->tri_material[pr.index] : pr.kind == 1 ? Sc.d->shapes[pr.index].material : Sc.d->fractal.material;
  if (Sc.d->materials[mat].stex[3] >= 0) C.c[COV_BUMP]++;
  if (pr.kind != 0 && pr.kind != 1) C.c[COV_FRACTAL]++;
  if (bs.n == 0) return;
  const int i = std::max(0, std::min(bs.n - 1, (int)std::floor(uc * (float)bs.n)));
  const BxDF& b = bs.b[i];
  switch (b.kind) {
    case K_LAMB: C.c[b.btdf ? COV_LAMB_BTDF : COV_LAMB]++; break;
    case K_OREN: C.c[b.btdf ? COV_OREN_BTDF : COV_OREN]++; break;
    case K_MICRO: C.c[b.fr.kind == FR_COND ? COV_MICRO_COND : COV_MICRO_DIEL]++; break;
    case K_SREFL: C.c[COV_SREFL]++; if (b.fr.kind == FR_COND) C.c[COV_SREFL_COND]++; break;
    case K_STRANS: C.c[COV_STRANS]++; break;
    case K_FBLEND:
      C.c[b.e == b.ey ? COV_FBLEND_ISO : COV_FBLEND_ANISO]++;
      if (b.depth > 0.f) C.c[COV_FBLEND_DEPTH]++;
      break;
    default: break;
  }
}

// one sampleLightRay: ul picks the light as sample_light_ray does
inline void cov_light_ray(Cov& C, const Scene& Sc, float ul) {
  const int n = (int)Sc.d->num_lights;
  if (n == 0) return;
  const bling_light& L = Sc.d->lights[n == 1 ? 0 : std::min((int)std::floor(ul * (float)n), n - 1)];
  const bool delta_or_area = L.kind == BLING_LIGHT_POINT || L.kind == BLING_LIGHT_DIRECTIONAL || L.kind == BLING_LIGHT_AREA;
  if (!delta_or_area && L.env_kind == BLING_ENV_IMAGE) C.c[COV_ENV_RAYS]++;
}
