// bidir.h -- the bidirectional path integrator (Integrator/BidirPath.hs) on the device, a surface
// integrator of the sampler renderer beside Path and DirectLighting.  One wave of camera samples:
//   k_bd_walk      one lane per camera sample: the camera ray, the light subpath (lightPath, :167-173),
//                  the eye subpath (eyePath, :161-164) -- nextVertex (:175-213) with sampleAdjBsdf /
//                  sampleBsdf -- and at every eye vertex the unweighted one-light estimate
//                  (estimateDirect, :142-154) and the le term (:79-82); one record per vertex
//   k_bd_connect   one lane per (sample, light vertex s): connect (:114-140) against every eye vertex
//                  t in order, the inner sum of :90-92
//   k_bd_finish    one lane per sample: countSpec's weights (:103-112), ld + le (+ l) (:70-96), the
//                  sample's result where Path's shade_end writes it (the film kernels run unchanged)
// A vertex record keeps the segment's ray and hit record, the sampled wo, the lobe type and alpha; the
// BSDF is rebuilt from them with the hit_geometry + make_bsdf calls that made it, so computed textures
// (FT_PROCTEX) are served.  Citations are BidirPath.hs:line; the reference's oddities are traps
// T25-T31 of DESIGN.md and are reproduced.  The LDS scene set-up and the per-thread trace are sppm.h's.
#pragma once
#include "light_tracer.h"

namespace bd {

constexpr int BD_MAX_DEPTH = 16;          // both specular masks fit 16 bits; nspec's index stays below 32

// Vertex records, structure of arrays: vertex slot v of sample i at v * cap + i; the eye vertex t has
// slot t, the light vertex s slot md + s.  Every index is bounded by 2 md and the wave's samples (<= cap).
struct BdBufs {
  float4* vorg;      // the segment's ray: o.xyz, tmin
  float4* vdir;      // d.xyz, the sampled lobe's type bits
  float4* vhit;      // its closest hit: t, ref, b1, b2
  float4* vwo;       // the sampled wo.xyz
  float4* valpha;    // [2 md][cap][4] alpha
  float4* ld;        // [md][cap][4] estimateDirect of eye vertex i (lHere * alpha, unweighted)
  float4* conn;      // [md][cap][4] the inner sum of light vertex s
  float4* le;        // [cap][4] the le term
  uint4* info;       // eye length, light length, eye specular mask, light specular mask
  float4* terms;     // bling_debug_bidir_terms: [n][3][4] ld, le, l; nullptr = off
  uint32_t cap;
  int md;
};

DEV size_t bd_at(const BdBufs& B, int slot, uint32_t sid) { return (size_t)slot * B.cap + sid; }
DEV void bd_store_sp(float4* dst, size_t i, const Sp& s) {
  float4* p = dst + 4 * i;
#pragma unroll
  for (int q = 0; q < 4; ++q) p[q] = make_float4(s.v[4 * q], s.v[4 * q + 1], s.v[4 * q + 2], s.v[4 * q + 3]);
}
DEV Sp bd_load_sp(const float4* src, size_t i) {
  const float4* p = src + 4 * i;
  Sp s;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 v = p[q];
    s.v[4 * q] = v.x; s.v[4 * q + 1] = v.y; s.v[4 * q + 2] = v.z; s.v[4 * q + 3] = v.w;
  }
  return s;
}

// countSpec (:103-112): nspec[k], the pairs (i, j) with i + j + 2 = k, i < ne, j < nl whose eye vertex
// i or light vertex j is specular, from the two masks: bit i of rl is light bit k - 2 - i.
DEV float bd_nspec(int k, int ne, int nl, uint32_t em, uint32_t lm) {
  const int m = k - 2;
  const int lo = max(0, m - nl + 1), hi = min(ne - 1, m);
  if (m < 0 || m > 30 || hi < lo) return 0.f;
  const uint32_t rl = __brev(lm) >> (31 - m);
  const uint32_t valid = ((2u << hi) - 1u) & ~((1u << lo) - 1u);
  return (float)__popc((em | rl) & valid);
}

struct BdRays { unsigned long long cam, cont, mis, shadow, verts, dropped; };

// sampleOneLight (Scene.hs:61-118) of an eye vertex with estimateDirect's dimensions (:144-147): the
// light sample and its any-hit shadow ray, the BSDF-MIS sample and its closest-hit ray, the power
// heuristic -- the oracle's order, resolve_L's operations (wavefront.h).
template <uint32_t F, class K = SampleKey>
DEV Sp bd_direct(const DevScene& S, const LdsScene& L, const K& k, const Bsdf& bsdf, V3 wo, float eps, int i,
                 BdRays& R) {
  const int lc = S.num_lights;
  Sp ld = sconst(0.f);
  if (lc == 0) return ld;
  const V3 p = bsdf.p;
  const float lNumU = rnd1(S, k, 1 + 12 * i);
  const int ln = lc == 1 ? 0 : min((int)floorf(lNumU * (float)lc), lc - 1);
  const bling_light& Lt = light_rec<F>(S, ln);
  TraceCount tc{0u, 0u, 0u, 0u};
  Sp ls = sconst(0.f), bs = sconst(0.f);
  {                                                                  // sampleLightMis (Scene.hs:61-69)
    float ld1, ld2; rnd2(S, k, 2 + 9 * i, &ld1, &ld2);
    const LightSample smp = light_sample<F>(S, Lt, p, bsdf.cs.n, eps, ld1, ld2);
    if (!(smp.pdf == 0.f) && !is_black(smp.li)) {
      float dps[2] = {__builtin_nanf(""), __builtin_nanf("")};
      const Sp f = eval_bsdf<F>(bsdf, wo, smp.wi, dps);
      if (!is_black(f)) {
        ++R.shadow;
        HitRec hs;
        if (!trace<true, F>(S, L, smp.ray, hs, tc)) {
          const float w = smp.delta ? 1.f : power_heuristic(smp.pdf, bsdf_pdf<F>(bsdf, wo, smp.wi, dps));
          ls = sscale(f * smp.li, w / smp.pdf);
        }
      }
    }
  }
  {                                                                  // sampleBsdfMis (Scene.hs:71-82)
    const float lBc = rnd1(S, k, 2 + 12 * i);
    float lb1, lb2; rnd2(S, k, 3 + 9 * i, &lb1, &lb2);
    Sp bf; V3 bwi; int bfl;
    const float bpdf = sample_bsdf<F>(bsdf, wo, lBc, lb1, lb2, bf, bwi, bfl);
    if (!(bpdf == 0.f) && !is_black(bf)) {
      ++R.mis;
      const Ray mr{p, bwi, eps, INFINITY};
      HitRec hm;
      if (trace<false, F>(S, L, mr, hm, tc)) {
        if ((hm.ref >> 30) == REF_SHAPE) {
          const DevShape& hs = gen(S.shapes[hm.ref & 0x3FFFFFFFu]);
          if (hs.light == ln) {                                      // l' == l (Light.hs:48-50)
            const float w = power_heuristic(bpdf, light_pdf<F>(S, Lt, p, bwi));
            const DG dg = shape_dg<F>(hs, mr, hm.t);
            const Sp le = dot(dg.n, -bwi) > 0.f ? sload(gen(S.lights[ln]).radiance) : sconst(0.f);   // intLe (-wi)
            bs = sscale(bf * le, w);
          }
        }
      } else {
        const float w = power_heuristic(bpdf, light_pdf<F>(S, Lt, p, bwi));
        bs = sscale(bf * light_le<F>(Lt, bwi), w);
      }
    }
  }
  ld = ls + bs;
  if (lc > 1) ld = sscale(ld, (float)lc);
  return ld;
}

// Both subpaths of a sample, the light subpath first: nextVertex (:175-213), the recursion as a loop
// whose one segment query serves every vertex of both walks (one traversal body in the kernel).  The
// first clause matches the intersection before the depth guard, so the segment after vertex md - 1 is
// traced too (trap T31); a vertex whose sample is black or has pdf 0 is kept and ends its walk.  The
// roulette draws are compared against rrProb = 1 and not drawn.
// K is the sample source: rnd1(S, k, dim) / rnd2(S, k, dim, &a, &b) give the sample's values -- the
// counter sampler's SampleKey (dev_shade.h), or the Metropolis renderer's primary sample (mlt.h PssKey).
template <uint32_t F, class K = SampleKey>
DEV void bd_walks(const DevScene& S, const LdsScene& L, const BdBufs& B, uint32_t sid, const K& k,
                  const Ray& lray, V3 lwi, const Sp& lalpha, const Ray& cam, int& ne, int& nl, uint32_t& emask,
                  uint32_t& lmask, Sp& le, BdRays& R) {
  const int md = B.md;
  bool adj = true;
  Ray ray = lray;
  V3 wi = lwi;
  Sp alpha = lalpha;
  int depth = 0;
  uint32_t mask = 0u;
  bool prev_spec = true;                                             // :75: the first vertex counts
  ne = nl = 0; emask = lmask = 0u;
  TraceCount tc{0u, 0u, 0u, 0u};
  ++R.cont;                                                          // the light ray
#pragma unroll 1
  for (;;) {
    HitRec h;
    bool end = !trace<false, F>(S, L, ray, h, tc) || depth == md;    // :187, :189
    if (!end) {
      const float4 hv = make_float4(h.t, __uint_as_float(h.ref), h.b1, h.b2);
      DG dgg, dgs;
      float eps;
      int mat, hit_light;
      hit_geometry<F>(S, ray, hv, dgg, dgs, eps, mat, hit_light);
      float ttmp[bsdf_tmp_floats<F>()];
      const Bsdf bsdf = make_bsdf<F>(S, mat, dgg, dgs, ttmp);
      const float ubc = rnd1(S, k, (adj ? 4 : 3) + 12 * depth);       // :162, :173
      float u1, u2; rnd2(S, k, (adj ? 5 : 4) + 9 * depth, &u1, &u2);
      Sp bf; V3 wo; int fl;
      float spdf;
      if (adj) spdf = sample_bsdf<F, true>(bsdf, wi, ubc, u1, u2, bf, wo, fl);   // sampleAdjBsdf
      else spdf = sample_bsdf<F, false>(bsdf, wi, ubc, u1, u2, bf, wo, fl);
      const size_t at = bd_at(B, (adj ? md : 0) + depth, sid);
      B.vorg[at] = make_float4(ray.o.x, ray.o.y, ray.o.z, ray.tmin);
      B.vdir[at] = make_float4(ray.d.x, ray.d.y, ray.d.z, __uint_as_float((uint32_t)fl));
      B.vhit[at] = hv;
      B.vwo[at] = make_float4(wo.x, wo.y, wo.z, 0.f);
      bd_store_sp(B.valpha, at, alpha);
      const bool spec = (fl & F_SPEC) == F_SPEC;
      if (spec) mask |= 1u << depth;
      if (!adj) {
        if (prev_spec) {                                             // alpha * intLe int wo (:81, trap T27)
          const Sp e = (hit_light >= 0 && dot(dgg.n, wo) > 0.f) ? sload(gen(S.lights[hit_light]).radiance) : sconst(0.f);
          le = le + alpha * e;
        }
        prev_spec = spec;
        const Sp d = bd_direct<F, K>(S, L, k, bsdf, wi, eps, depth, R) * alpha;   // estimateDirect (:142-154)
        bd_store_sp(B.ld, bd_at(B, depth, sid), d);
      }
      ++depth; ++R.verts;
      if (is_black(bf) || spdf == 0.f) end = true;                   // :207-208: no next segment
      else {
        alpha = bf * alpha;                                          // :199-201: pathScale = f, rrProb = 1 (trap T26)
        ray = Ray{bsdf.p, wo, eps, INFINITY};
        wi = -wo;
        ++R.cont;
      }
    }
    if (end) {
      if (!adj) { ne = depth; emask = mask; break; }
      nl = depth; lmask = mask;                                      // eyePath (:161-164)
      adj = false;
      ray = cam; wi = -cam.d; alpha = sconst(1.f);
      depth = 0; mask = 0u; prev_spec = true;
      ++R.cam;
    }
  }
}

DEV void bd_flush(Counters* C, const BdRays& R) {
  const unsigned long long a = wave_sum_u64(R.cam), b = wave_sum_u64(R.cont), m = wave_sum_u64(R.mis),
                           s = wave_sum_u64(R.shadow), v = wave_sum_u64(R.verts), d = wave_sum_u64(R.dropped);
  if ((threadIdx.x & 63) == 0) {
    if (a) atomicAdd(&C->cam, a);
    if (b) atomicAdd(&C->cont, b);
    if (m) atomicAdd(&C->mis, m);
    if (s) atomicAdd(&C->shadow, s);
    if (v) atomicAdd(&C->vertices, v);
    if (d) atomicAdd(&C->dropped, d);
  }
}

// lightPath's first segment (:167-173): sampleLightRay (Scene.hs:121-135) of the sample's one light
template <uint32_t F, class K = SampleKey>
DEV void bd_light_start(const DevScene& S, const K& k, Ray& lray, V3& lwi, Sp& lalpha) {
  const float ul = rnd1(S, k, 0);
  float uo1, uo2, ud1, ud2;
  rnd2(S, k, 0, &uo1, &uo2);
  rnd2(S, k, 1, &ud1, &ud2);
  float pdf = 0.f;
  Sp li = sconst(0.f);
  Ray ray{mk(0.f, 0.f, 0.f), mk(0.f, 1.f, 0.f), 0.f, 0.f};
  V3 nl3 = mk(0.f, 1.f, 0.f);
  if (S.num_lights > 0) {
    const int lc = S.num_lights;
    const int ln = lc == 1 ? 0 : min((int)floorf(ul * (float)lc), lc - 1);
    pdf = light_ray<F>(S, gen(S.lights[ln]), uo1, uo2, ud1, ud2, li, ray, nl3);
    if (lc > 1) pdf = pdf / (float)lc;
  }
  const V3 wo = -ray.d;                                              // not normalised, pdf not tested (trap T25)
  li = sscale(li, fabsf(dot(nl3, wo)) / pdf);
  lray = ray; lwi = wo; lalpha = li;
}

// The camera samples of a wave: tile mode (tiles != nullptr: grid (blocks, tile), k_raygen's sample
// order) or list mode (list of n (x, y, n) samples, bling_sample_li).
template <uint32_t F>
static __global__ __launch_bounds__(256) void k_bd_walk(const DevScene* __restrict__ Sptr, WaveState W, BdBufs B,
                                                 const TileDesc* __restrict__ tiles, const int32_t* __restrict__ list,
                                                 uint32_t n_list, uint32_t seed, uint32_t pass, Counters* __restrict__ C) {
  extern __shared__ float4 smem[];
  const DevScene& S = *Sptr;
  const LdsScene L = lds_setup(S, smem);
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  BdRays R{0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
  bool live = false;
  uint32_t sid = 0u, n = 0u;
  int ix = 0, iy = 0;
  if (tiles) {
    const TileDesc td = tiles[blockIdx.y];
    if (j < td.count) {
      const int tw = td.x1 - td.x0 + 1;
      uint32_t pt;
      if (S.sample_major) {
        const uint32_t npix = (uint32_t)(tw * (td.y1 - td.y0 + 1));
        n = j / npix; pt = j - n * npix;
      } else {
        pt = S.fd_spp.div(j); n = j - pt * (uint32_t)S.spp;
      }
      ix = td.x0 + (int)(pt % (uint32_t)tw); iy = td.y0 + (int)(pt / (uint32_t)tw);
      sid = td.offset + j;
      live = true;
    }
  } else if (j < n_list) {
    ix = list[3 * j]; iy = list[3 * j + 1]; n = (uint32_t)list[3 * j + 2];
    sid = j;
    live = true;
  }
  if (live && sid < B.cap) {
    const uint32_t pixel = (uint32_t)((iy - S.ey0) * S.ext_w + (ix - S.ex0));
    const SampleKey k = sample_key(seed, pass, pixel, n);
    float ox, oy, lu, lv;
    camera_sample(S, k, &ox, &oy, &lu, &lv);
    const float imx = (float)ix + ox, imy = (float)iy + oy;
    const Ray cam = fire_ray(S.camera, imx, imy, lu, lv);
    W.img[sid] = make_float2(imx, imy);
    uint32_t emask, lmask;
    int ne, nl;
    Sp le = sconst(0.f), lalpha;
    Ray lray;
    V3 lwi;
    bd_light_start<F>(S, k, lray, lwi, lalpha);
    bd_walks<F>(S, L, B, sid, k, lray, lwi, lalpha, cam, ne, nl, emask, lmask, le, R);
    bd_store_sp(B.le, sid, le);
    B.info[sid] = make_uint4((uint32_t)ne, (uint32_t)nl, emask, lmask);
  }
  bd_flush(C, R);
}

// The BSDF of a stored vertex, as the walk built it
template <uint32_t F>
DEV Bsdf bd_vertex_bsdf(const DevScene& S, const BdBufs& B, size_t at, float* ttmp, float& eps) {
  const float4 o = B.vorg[at], d = B.vdir[at];
  const Ray ray{mk(o.x, o.y, o.z), mk(d.x, d.y, d.z), o.w, INFINITY};
  DG dgg, dgs;
  int mat, hit_light;
  hit_geometry<F>(S, ray, B.vhit[at], dgg, dgs, eps, mat, hit_light);
  return make_bsdf<F>(S, mat, dgg, dgs, ttmp);
}

// connect (:114-140) as called at :90-92 with ((vl, s), (ve, t)): the light vertex takes the
// pattern's eye role (evalBsdf False, its eps at the ray's start), the eye vertex the light role
// (evalBsdf True) (trap T28); both are evaluated towards their sampled wo (trap T29).  Lane = s * n + i.
template <uint32_t F>
static __global__ __launch_bounds__(256) void k_bd_connect(const DevScene* __restrict__ Sptr, BdBufs B, uint32_t n,
                                                    Counters* __restrict__ C) {
  extern __shared__ float4 smem[];
  const DevScene& S = *Sptr;
  const LdsScene L = lds_setup(S, smem);
  const unsigned long long gid = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  BdRays R{0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
  const int s = (int)(gid / n);
  const uint32_t sid = (uint32_t)(gid - (unsigned long long)s * n);
  if (s < B.md && sid < B.cap) {
    const uint4 info = B.info[sid];
    const int ne = (int)info.x, nl = (int)info.y;
    const uint32_t em = info.z, lm = info.w;
    if (s < nl) {
      Sp inner = sconst(0.f);
      if (!((lm >> s) & 1u)) {                                       // :118 (every term of a specular s is black)
        const size_t la = bd_at(B, B.md + s, sid);
        float tmp_a[bsdf_tmp_floats<F>()];
        float eps_a;
        const Bsdf ba = bd_vertex_bsdf<F>(S, B, la, tmp_a, eps_a);
        const float4 wa4 = B.vwo[la];
        const V3 wo_a = mk(wa4.x, wa4.y, wa4.z);
        const Sp alpha_a = bd_load_sp(B.valpha, la);
        TraceCount tc{0u, 0u, 0u, 0u};
#pragma unroll 1
        for (int t = 0; t < ne; ++t) {
          Sp c = sconst(0.f);
          if (!((em >> t) & 1u)) {                                   // :119
            const size_t ea = bd_at(B, t, sid);
            float tmp_b[bsdf_tmp_floats<F>()];
            float eps_b;
            const Bsdf bb = bd_vertex_bsdf<F>(S, B, ea, tmp_b, eps_b);
            const V3 pe = ba.p, pl = bb.p;
            const V3 dv = pl - pe;
            const float l2 = sqlen(dv);
            const float wl = l2 != 0.f ? sqrtf(l2) : 0.f;            // normLen (Math.hs:356-363)
            const V3 w = l2 != 0.f ? vs(dv, 1.f / wl) : dv;
            const Sp fe = eval_bsdf<F>(ba, wo_a, w);                 // :130
            if (!is_black(fe)) {                                     // :120
              const float4 wb4 = B.vwo[ea];
              const Sp fl = eval_bsdf_adj<F>(bb, mk(wb4.x, wb4.y, wb4.z), -w);   // :134
              if (!is_black(fl)) {
                ++R.shadow;
                HitRec hs;
                if (!trace<true, F>(S, L, Ray{pe, w, eps_a, wl - eps_b}, hs, tc)) {   // :121, :136
                  const int kk = s + t + 2;
                  const float pathWt = 1.f / ((float)kk - bd_nspec(kk, ne, nl, em, lm));   // :124
                  const float g = 1.f / sqlen(pl - pe);              // :125
                  c = sscale(alpha_a * fe * bd_load_sp(B.valpha, ea) * fl, g * pathWt);   // :122
                }
              }
            }
          }
          inner = inner + c;
        }
      }
      bd_store_sp(B.conn, bd_at(B, s, sid), inner);
    }
  }
  bd_flush(C, R);
}

// contrib (:50-96): ld, the eye vertices' estimates weighted by 1 / (1 + i - nspec[i + 1]) and summed
// from 0 in order; + le; + l, the light vertices' inner sums from 0 in order, unless a path is empty.
static __global__ __launch_bounds__(256) void k_bd_finish(WaveState W, BdBufs B, uint32_t n, Counters* __restrict__ C) {
  const uint32_t sid = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long dropped = 0ull;
  if (sid < n && sid < B.cap) {
    const uint4 info = B.info[sid];
    const int ne = min((int)info.x, B.md), nl = min((int)info.y, B.md);
    Sp ld = sconst(0.f), l = sconst(0.f);
    for (int i = 0; i < ne; ++i)
      ld = ld + sscale(bd_load_sp(B.ld, bd_at(B, i, sid)), 1.f / (1.f + (float)i - bd_nspec(i + 1, ne, nl, info.z, info.w)));
    const Sp le = bd_load_sp(B.le, sid);
    if (ne > 0)
      for (int s = 0; s < nl; ++s) l = l + bd_load_sp(B.conn, bd_at(B, s, sid));
    if (B.terms) {
      bd_store_sp(B.terms, (size_t)3 * sid, ld);
      bd_store_sp(B.terms, (size_t)3 * sid + 1, le);
      bd_store_sp(B.terms, (size_t)3 * sid + 2, l);
    }
    const Sp Lr = (ne == 0 || nl == 0) ? ld + le : ld + le + l;
    finalize(W, sid, Lr, dropped);
  }
  flush_dropped(C, dropped);
}

}  // namespace bd
