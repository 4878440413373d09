// scene_plan.cpp -- the host-only stages of scene_plan.h.  No HIP runtime call: the device types and the
// kernels' LDS size formulas (dev_trace.h) are all it takes from the device headers.
#include "core_internal.h"

#include <cmath>
#include <cstdlib>

using namespace bd;
using namespace bcore;

namespace bplan {
namespace {

// largest threaded BVH (child boxes) walked by the wave-coherent kernels.  A/B on MI355X
// (DESIGN.md 3): sun-sky (8 entries) closest-hit -11 %; cornell-box (30) +28 %, so it stays per-lane
constexpr uint32_t kPacketMaxEntries = 16;
// primitives up to which the traversal kernels test every primitive instead of walking a tree:
// sun-sky's 4 shapes, closest-hit 108 -> 93 ms per C4 pass; cornell's 31 primitives measured even
// (closest 28.9 -> 28.4 ms, any-hit 8.6 -> 9.4: profiles/r05_ab_session.txt r05h-l), so they walk
// the BVH4
constexpr uint32_t kBruteMax = 16;
static_assert(2 * kPacketMaxEntries <= 64, "the packet kernels hold the entry list in one VGPR float4 per lane");
// scenes with at most this many analytic shapes keep their shape records in the BVH4 kernels' LDS
constexpr uint32_t kLdsShapesMax = 8;

// LDS plan of the traversal kernels: keep a block at <= 30 KiB so five 256-thread blocks fit a CU's
// 160 KiB.  The stack takes depth x 1 KiB; small scenes then go to LDS whole, larger ones keep the
// breadth-first node prefix (the top levels every ray visits).
void plan_lds(DevScene& S, uint32_t nodes, uint32_t tris, uint32_t refs, uint32_t depth) {
  constexpr size_t kBudget = 30 * 1024;
  S.stack_depth = depth;
  const size_t stack = (size_t)4 * TRACE_BLOCK * depth;
  const size_t avail = kBudget > stack ? kBudget - stack : 0;
  const size_t ref_b = (size_t)16 * ((refs + 3) / 4);
  if ((size_t)64 * nodes + lds_tri_bytes(tris) + ref_b <= avail) {
    S.lds_nodes = nodes; S.lds_tris = tris; S.lds_refs = refs;
    return;
  }
  S.lds_tris = 0;
  S.lds_refs = ref_b <= avail / 4 ? refs : 0;
  const size_t left = avail - (S.lds_refs ? ref_b : 0);
  S.lds_nodes = (uint32_t)std::min<size_t>(nodes, left / 64);
}

// LDS plan of the BVH4 (Traversal4): a 26-KiB block budget, so six 256-thread blocks share a CU's
// 160 KiB -- the meshes-profile kernel's 78 VGPRs allow six waves per SIMD, and occupancy beats a
// longer node prefix (A/B on C3, profiles/r02_ab_lds4_budget_s5.txt: 20 / 26 / 30 / 40 / 53 KiB ->
// 5 002 / 5 046 / 4 822 / 4 518 / 3 009 Mrays/s).  When the tree,
// triangles, refs and the whole stack bound fit, everything goes to LDS (lds_all4).  Otherwise
// stack4_lds rows of the stack stay in LDS (12: flat from 8 to 20 rows on C3), the
// rest spill to global rows, and the breadth-first node prefix (and the refs, if small) take what is
// left (112 bytes a node).
void plan_lds4(DevScene& S, uint32_t nodes, uint32_t tris, uint32_t refs, uint32_t need, uint32_t shapes) {
  constexpr size_t kBudget = (size_t)26 * 1024;
  const size_t ref_b = (size_t)16 * ((refs + 3) / 4);
  S.stack4_need = need;
  // shape records (176 B each) go to LDS whole when the scene has a few: cornell's light quad
  const uint32_t sh = shapes <= kLdsShapesMax ? shapes : 0u;
  S.lds4_shapes = sh;
  // all in LDS: decided with the size the all-LDS kernels launch with (their leaf-order layout and
  // its two spare stack rows), so an lds_all4 block never exceeds the budget
  if (lds_bytes4_leaf(nodes, refs, need, sh) <= kBudget) {
    S.lds4_nodes = nodes; S.lds4_tris = tris; S.lds4_refs = refs; S.stack4_lds = need;
    return;
  }
  const uint32_t rows = std::max(1u, std::min(12u, need));
  S.stack4_lds = rows;
  const size_t stack = (size_t)4 * TRACE_BLOCK * rows + sizeof(DevShape) * sh;
  const size_t avail = kBudget > stack ? kBudget - stack : 0;
  S.lds4_tris = 0;
  S.lds4_refs = ref_b <= avail / 4 ? refs : 0;
  const size_t left = avail - (S.lds4_refs ? ref_b : 0);
  S.lds4_nodes = (uint32_t)std::min<size_t>(nodes, left / 112);
}

// A CDF of `rows` rows of n entries with a guide table behind it (the device layout of dev_shade.h
// sample_c1d): g[k] = the first index whose CDF value is >= k / kCdfGuide (k = 0 .. kCdfGuide),
// so a search for u starts in [g[floor(u kCdfGuide)], g[floor(u kCdfGuide) + 1]] instead of the
// whole row (the sun-sky map's 641-entry rows: 10 dependent loads -> 1 to 3).
std::vector<float> with_guide(const float* cdf, size_t n, size_t rows) {
  std::vector<float> out(cdf, cdf + n * rows);
  for (size_t r = 0; r < rows; ++r) {
    const float* row = cdf + r * n;
    size_t i = 0;
    for (int k = 0; k <= kCdfGuide; ++k) {
      const float t = (float)k / (float)kCdfGuide;
      while (i < n && !(row[i] >= t)) ++i;
      uint32_t gi = (uint32_t)i;
      float f;
      std::memcpy(&f, &gi, 4);
      out.push_back(f);
    }
  }
  return out;
}

// The render configuration's half of DevScene: sampler, depths, the integrator's sample dimensions, the
// exact divisions, the film extent and the filter.
void plan_config(DevScene& S, const bling_scene_desc& d) {
  S.camera = d.camera;
  std::memcpy(S.lt_w2r, d.light.w2r, sizeof S.lt_w2r);
  S.lt_pixel_area = d.light.pixel_area;
  std::memcpy(S.filter_table, d.filter.table, sizeof S.filter_table);
  S.filter_w = d.filter.width; S.filter_h = d.filter.height;
  const bling_render_config& cfg = d.config;
  S.sampler = cfg.sampler; S.nu = cfg.nu; S.nv = cfg.nv; S.spp = cfg.spp;
  S.max_depth = cfg.max_depth; S.sample_depth = cfg.sample_depth;
  S.integrator = cfg.integrator;
  if (cfg.renderer == BLING_RENDERER_METROPOLIS) {                   // mkBidirPathIntegrator md md (Metropolis.hs:46-49)
    S.integrator = BLING_INTEGRATOR_BIDIR;
    S.max_depth = S.sample_depth = d.metropolis.max_depth;
  }
  if (S.integrator == BLING_INTEGRATOR_DIRECT) S.n1d = S.n2d = 2 * cfg.max_depth;   // DirectLighting.hs:17-18
  else if (S.integrator == BLING_INTEGRATOR_BIDIR) { S.n1d = 12 * S.sample_depth + 1; S.n2d = 9 * S.sample_depth + 2; }   // BidirPath.hs:44-48
  else if (S.integrator == BLING_INTEGRATOR_NORMALS) { S.n1d = S.n2d = 0; S.max_depth = S.sample_depth = 0; }   // SurfaceIntegrator li 0 0 (Debug.hs:26)
  else { S.n1d = 4 * cfg.sample_depth; S.n2d = 3 * cfg.sample_depth; }              // Path.hs:26-28
  if (cfg.spp > (1 << 24)) throw std::runtime_error("more than 2^24 samples per pixel (the sampler's permutation, counter_rng.h)");
  S.fd_spp = FastDiv::make((uint32_t)std::max(1, cfg.spp));
  S.fd_nu = FastDiv::make((uint32_t)std::max(1, cfg.nu));
  {
    uint32_t w = (uint32_t)std::max(1, cfg.spp) - 1u;                 // brng::permute's mask
    w |= w >> 1; w |= w >> 2; w |= w >> 4; w |= w >> 8; w |= w >> 16;
    S.perm_mask_spp = w;
  }
  S.inv_spp = 1.f / (float)cfg.spp; S.inv_nu = 1.f / (float)cfg.nu; S.inv_nv = 1.f / (float)cfg.nv;
  S.width = cfg.width; S.height = cfg.height;
  float fw = d.filter.width, fh = d.filter.height;
  S.ex0 = (int)floorf(0.5f - fw); S.ex1 = (int)floorf(0.5f + (float)cfg.width + fw);      // Image.hs:162-168
  S.ey0 = (int)floorf(0.5f - fh); S.ey1 = (int)floorf(0.5f + (float)cfg.height + fh);
  S.ext_w = S.ex1 - S.ex0 + 1;
  if ((int)std::ceil(fw) + 17 > FILM_TILE_MAX || (int)std::ceil(fh) + 17 > FILM_TILE_MAX)
    throw std::runtime_error("filter wider than the LDS film tile supports");
}

}  // namespace

// Everything the later stages and the kernels assume of a scene description, checked on the host before
// any device work (bling_scene_validate runs it without a device): render config, texture graphs
// (computed textures at the top, their children stored), host-folded material spectra, light
// count, images and the textures and environment maps that index them.
void validate_scene(const bling_scene_desc* d) {
  if (!d) throw std::invalid_argument("null argument");
  if (d->config.width <= 0 || d->config.height <= 0) throw std::invalid_argument("bad render config");
  if (d->config.renderer == BLING_RENDERER_SPPM) {
    // eye trees are walked depth-first with one parked sibling per level (k_sppm_eye)
    if (d->config.max_depth < 1 || d->config.max_depth > SPPM_MAX_DEPTH)
      throw std::invalid_argument("sppm maxDepth outside [1, " + std::to_string(SPPM_MAX_DEPTH) + "]");
    if (d->config.sppm_photons < 1 || d->config.sppm_threads < 1) throw std::invalid_argument("bad sppm photon count");
  } else if (d->config.renderer == BLING_RENDERER_LIGHT) {
    if (d->light.pass_photons < 1) throw std::invalid_argument("light tracer passPhotons < 1");
  } else if (d->config.renderer == BLING_RENDERER_METROPOLIS) {
    const bling_metropolis& m = d->metropolis;
    // the chain's integrator is the bidirectional one with maxDepth = sampleDepth (Metropolis.hs:46-49)
    if (m.max_depth < 1 || m.max_depth > BD_MAX_DEPTH)
      throw std::invalid_argument("metropolis maxDepth outside [1, " + std::to_string(BD_MAX_DEPTH) + "]");
    if (m.bootstrap < 1) throw std::invalid_argument("metropolis bootstrap < 1");
    const float mut = mlt_mutations(m, d->config.width, d->config.height);
    if (!(mut >= 1.f)) throw std::invalid_argument("metropolis mpp gives no mutation (floor (mpp * nPixels) < 1)");
    if (!(mut < 2147483648.f)) throw std::invalid_argument("metropolis mpp gives 2^31 mutations or more");
    if (m.chains < 1) throw std::invalid_argument("metropolis chains < 1");
    if ((uint32_t)m.chains > MLT_MAX_CHAINS) throw std::invalid_argument("metropolis chains > 2^20");
  } else if (d->config.spp <= 0) {
    throw std::invalid_argument("bad render config");
  } else if (d->config.integrator == BLING_INTEGRATOR_DIRECT) {
    // the tree is walked depth-first with one parked sibling per level (k_shade_dl): bound it
    if (d->config.max_depth < 1 || d->config.max_depth > kMaxDlDepth)
      throw std::invalid_argument("directLighting maxDepth outside [1, " + std::to_string(kMaxDlDepth) + "]");
  } else if (d->config.integrator == BLING_INTEGRATOR_BIDIR) {
    // both subpaths' specular masks are 16-bit words, the vertex buffers 2 maxDepth records (bidir.h)
    if (d->config.max_depth < 1 || d->config.max_depth > BD_MAX_DEPTH)
      throw std::invalid_argument("bidir maxDepth outside [1, " + std::to_string(BD_MAX_DEPTH) + "]");
    if (d->config.sample_depth < 0) throw std::invalid_argument("bidir sampleDepth < 0");
  } else if (d->config.integrator != BLING_INTEGRATOR_PATH && d->config.integrator != BLING_INTEGRATOR_NORMALS) {
    throw std::invalid_argument("unknown surface integrator");
  }
  for (uint32_t k = 0; k < d->num_textures; ++k) {     // computed textures: children the device resolves
    const bling_texture& t = d->textures[k];
    auto simple = [&](int32_t ti) {
      return ti >= 0 && (uint32_t)ti < d->num_textures && d->textures[ti].kind <= BLING_TEX_GRAPHPAPER;
    };
    auto stex_ok = [&](int32_t si) { return si >= 0 && (uint32_t)si < d->num_scalar_textures; };
    bool ok = true;
    if (t.kind == BLING_TEX_BLEND) ok = simple(t.tex1) && simple(t.tex2) && stex_ok(t.stex);
    else if (t.kind == BLING_TEX_CHECKER) ok = simple(t.tex1) && simple(t.tex2);
    else if (t.kind == BLING_TEX_GRADIENT) {
      ok = t.tex2 >= 1 && t.tex1 >= 0 && (uint64_t)t.tex1 + (uint64_t)t.tex2 <= d->num_textures && stex_ok(t.stex);
      for (int32_t s = 0; ok && s < t.tex2; ++s) ok = d->textures[t.tex1 + s].kind == BLING_TEX_CONST;
    } else if (t.kind == BLING_TEX_GRAPHPAPER) ok = simple(t.tex1) && simple(t.tex2);
    else ok = t.kind == BLING_TEX_CONST || t.kind == BLING_TEX_IMAGE;   // the image index is checked below
    if (!ok) throw std::invalid_argument("texture " + std::to_string(k) + ": malformed or nested computed texture");
  }
  for (uint32_t k = 0; k < d->num_scalar_textures; ++k) {
    const bling_scalar_texture& t = d->scalar_textures[k];
    bool ok = t.kind >= BLING_STEX_CONST && t.kind <= BLING_STEX_IMAGE;
    if (t.kind == BLING_STEX_SCALE) ok = t.child >= 0 && (uint32_t)t.child < d->num_scalar_textures;
    if (t.kind == BLING_STEX_CRYSTAL)
      ok = t.octaves >= 1 && t.child >= 0 && (uint64_t)t.child + (uint64_t)t.octaves <= d->num_scalar_textures;
    if (!ok) throw std::invalid_argument("scalar texture " + std::to_string(k) + ": malformed");
  }
  for (uint32_t k = 0; k < d->num_materials; ++k) {
    // the encoding of bling_scene.h ("materials"): every texture a kind reads is in range; a scalar
    // slot's stex is a scalar texture or -1; a transformed spectrum slot is either folded (a constant
    // record make_bsdf reads directly) or raw (any texture eval_spectrum serves at the top of a slot,
    // which the texture loop above established for every record)
    const bling_material& m = d->materials[k];
    const std::string who = "material " + std::to_string(k);
    int nt = 0, ns = 1;                                   // textures read, scalar slots with an stex
    bool raw[4] = {true, true, true, true};               // untransformed slots take any texture
    auto flag = [&](int j) {
      if (m.stex[j] != -1 && m.stex[j] != BLING_SLOT_RAW) throw std::invalid_argument(who + ": bad raw-slot flag in stex[" + std::to_string(j) + "]");
      return m.stex[j] == BLING_SLOT_RAW;
    };
    switch (m.kind) {
      case BLING_MAT_BLACKBODY: ns = 0; break;
      case BLING_MAT_MATTE: nt = 1; break;
      case BLING_MAT_PLASTIC: case BLING_MAT_GLASS: case BLING_MAT_METAL: nt = 2; break;
      case BLING_MAT_MIRROR: nt = 1; ns = 0; break;
      case BLING_MAT_TRANSMATTE: nt = 2; raw[0] = raw[1] = flag(1); break;
      case BLING_MAT_SHINYMETAL:
        nt = 4; raw[0] = raw[1] = flag(1); raw[2] = raw[3] = flag(2);
        if ((raw[0] && m.tex[0] != m.tex[1]) || (raw[2] && m.tex[2] != m.tex[3]))
          throw std::invalid_argument(who + ": a raw shinyMetal spectrum must sit in both of its slots");
        break;
      case BLING_MAT_SUBSTRATE: nt = 3; ns = 3; break;    // raw or folded by the texture's kind
      default: throw std::invalid_argument(who + ": unknown kind");
    }
    for (int j = 0; j < nt; ++j) {
      const int32_t ti = m.tex[j];
      if (ti < 0 || (uint32_t)ti >= d->num_textures)
        throw std::invalid_argument(who + ": texture " + std::to_string(j) + " out of range");
      if (!raw[j] && d->textures[ti].kind != BLING_TEX_CONST)
        throw std::invalid_argument(who + ": texture " + std::to_string(j) + " is marked folded but is no constant spectrum");
    }
    for (int j = 0; j < 4; ++j) {
      if (!(j < ns || j == 3)) continue;                  // stex[3]: bump
      if (m.stex[j] < -1 || (m.stex[j] >= 0 && (uint32_t)m.stex[j] >= d->num_scalar_textures))
        throw std::invalid_argument(who + ": scalar texture " + std::to_string(j) + " out of range");
    }
  }
  // the path state packs a light index (and a hit light + 1) into 8 bits each (wavefront.h vf_*)
  if (d->num_lights > 254) throw std::invalid_argument("more than 254 lights");
  for (uint32_t k = 0; k < d->num_lights; ++k) {
    const bling_light& l = d->lights[k];
    if (l.kind == BLING_LIGHT_INFINITE && l.env_kind == BLING_ENV_IMAGE && (l.env_w <= 0 || l.env_h <= 0 || !l.env_texels))
      throw std::invalid_argument("infinite light: empty image map");
  }
  for (uint32_t k = 0; k < d->num_images; ++k) {
    const bling_image& im = d->images[k];
    if (im.width <= 0 || im.height <= 0 || !im.texels || (im.channels != 1 && im.channels != 16))
      throw std::invalid_argument("texture image: bad size, channels or texels");
  }
  for (uint32_t k = 0; k < d->num_textures; ++k) {
    const bling_texture& t = d->textures[k];
    if (t.kind == BLING_TEX_IMAGE && (t.tex1 < 0 || (uint32_t)t.tex1 >= d->num_images || d->images[t.tex1].channels != 16))
      throw std::invalid_argument("image texture " + std::to_string(k) + ": no spectral image");
  }
  for (uint32_t k = 0; k < d->num_scalar_textures; ++k) {
    const bling_scalar_texture& t = d->scalar_textures[k];
    if (t.kind == BLING_STEX_IMAGE && (t.child < 0 || (uint32_t)t.child >= d->num_images || d->images[t.child].channels != 1))
      throw std::invalid_argument("scalar image texture " + std::to_string(k) + ": no greyscale image");
  }
}

SceneItems scene_items(const bling_scene_desc& d) {
  SceneItems I;
  const uint32_t nt = d.num_triangles, ns = d.num_shapes;
  // --- triangles: MT record (v0, e1 = p2 - p1, e2 = p3 - p1) and shading data
  std::vector<float4>& geo = I.geo;
  std::vector<float>& pts = I.pts;
  geo.resize((size_t)3 * nt);
  pts.resize((size_t)9 * nt);
  for (uint32_t t = 0; t < nt; ++t) {
    const uint32_t* ix = d.tri_indices + 3 * t;
    float p[3][3];
    for (int k = 0; k < 3; ++k)
      for (int a = 0; a < 3; ++a) { p[k][a] = d.vertices[3 * ix[k] + a]; pts[9 * t + 3 * k + a] = p[k][a]; }
    float e1[3], e2[3];
    for (int a = 0; a < 3; ++a) { e1[a] = p[1][a] - p[0][a]; e2[a] = p[2][a] - p[0][a]; }
    geo[3 * t + 0] = make_float4(p[0][0], p[0][1], p[0][2], e1[0]);
    geo[3 * t + 1] = make_float4(e1[1], e1[2], e2[0], e2[1]);
    geo[3 * t + 2] = make_float4(e2[2], 0.f, 0.f, 0.f);
  }
  // --- primitive list (reference order) -> BVH items
  I.tri_prim.assign(nt, -1);
  I.shape_prim.assign(ns, -1);
  for (uint32_t i = 0; i < d.num_prims; ++i) {
    int kind = d.prim_kind[i], idx = d.prim_index[i];
    bvh::Box b;
    for (int a = 0; a < 3; ++a) { b.lo[a] = INFINITY; b.hi[a] = -INFINITY; }
    if (kind == 0) {
      I.tri_prim[idx] = (int32_t)i;
      for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a) { float v = pts[9 * idx + 3 * k + a]; b.lo[a] = std::min(b.lo[a], v); b.hi[a] = std::max(b.hi[a], v); }
      I.refs.push_back((REF_TRI << 30) | (uint32_t)idx);
    } else if (kind == 1) {
      I.shape_prim[idx] = (int32_t)i;
      const bling_shape& s = d.shapes[idx];
      float mn[3], mx[3];
      const float* P = s.params;                                   // objectBounds (Shape.hs:299-311)
      if (s.kind == BLING_SHAPE_QUAD) { mn[0] = -P[0]; mn[1] = -P[1]; mn[2] = 0.f; mx[0] = P[0]; mx[1] = P[1]; mx[2] = 0.f; }
      else if (s.kind == BLING_SHAPE_DISK) { mn[0] = -P[1]; mn[1] = -P[1]; mn[2] = P[0]; mx[0] = P[1]; mx[1] = P[1]; mx[2] = P[0]; }
      else if (s.kind == BLING_SHAPE_CYLINDER) { mn[0] = -P[0]; mn[1] = -P[0]; mn[2] = P[1]; mx[0] = P[0]; mx[1] = P[0]; mx[2] = P[2]; }
      else if (s.kind == BLING_SHAPE_BOX) { for (int a = 0; a < 3; ++a) { mn[a] = P[a]; mx[a] = P[3 + a]; } }
      else { for (int a = 0; a < 3; ++a) { mn[a] = -P[0]; mx[a] = P[0]; } }
      for (int cidx = 0; cidx < 8; ++cidx) {
        float q[3] = {(cidx & 4) ? mx[0] : mn[0], (cidx & 2) ? mx[1] : mn[1], (cidx & 1) ? mx[2] : mn[2]};
        const float* m = s.o2w;
        float w = m[12] * q[0] + m[13] * q[1] + m[14] * q[2] + m[15];
        for (int a = 0; a < 3; ++a) {
          float v = m[4 * a] * q[0] + m[4 * a + 1] * q[1] + m[4 * a + 2] * q[2] + m[4 * a + 3];
          if (w != 1.f) v /= w;
          b.lo[a] = std::min(b.lo[a], v); b.hi[a] = std::max(b.hi[a], v);
        }
      }
      I.refs.push_back((REF_SHAPE << 30) | (uint32_t)idx);
    } else {
      I.fractal_prim = (int32_t)i;
      const float fr = d.fractal.kind == BLING_FRACTAL_JULIA ? 1.7321f : 1.4143f;   // entry spheres r^2 = 3 / 2
      for (int a = 0; a < 3; ++a) { b.lo[a] = -fr; b.hi[a] = fr; }
      I.refs.push_back((REF_FRACTAL << 30));
    }
    I.boxes.push_back(b);
  }
  // worldBounds of the reference's kd-tree (union of the primitive bounds; the fractals' are
  // mkMandelBulb's +-2.5 and the Julia radius sqrt 3, not the tighter BVH entry spheres)
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t i = 0; i < d.num_prims; ++i) {
    bvh::Box b = I.boxes[i];
    if (d.prim_kind[i] == 2) {
      const float fr = d.fractal.kind == BLING_FRACTAL_JULIA ? sqrtf(3.f) : 2.5f;
      for (int a = 0; a < 3; ++a) { b.lo[a] = -fr; b.hi[a] = fr; }
    }
    for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], b.lo[a]); hi[a] = std::max(hi[a], b.hi[a]); }
  }
  float dd[3];
  for (int a = 0; a < 3; ++a) { I.world_c[a] = lo[a] + (hi[a] - lo[a]) * 0.5f; dd[a] = hi[a] - I.world_c[a]; }
  I.world_r = sqrtf(dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2]);
  for (int a = 0; a < 3; ++a) { I.kd_lo[a] = lo[a]; I.kd_hi[a] = hi[a]; }
  return I;
}

// Leaves of at most two primitives: the all-LDS BVH4 kernel tests two primitives per step, so a
// leaf costs one step (A/B, profiles/r02_ab_bvh_leaf_s5.txt: C2 closest-hit 37.4 -> 31.5 ms per
// pass against leaves of up to 4; C3, C4 and C5 within noise).
bvh::Result host_bvh2(const SceneItems& items) { return bvh::build(items.boxes, items.refs, 2); }

ScenePlan scene_derive(const bling_scene_desc& d, SceneItems&& items, bvh::Result&& bvh2) {
  const bvh::Result& R = bvh2;
  const uint32_t nrefs = (uint32_t)R.refs.size();
  // the primitives' records in leaf order, the ref in each, one zero record behind them (the layout:
  // dev_trace.h LeafRec, common/bvh4.h leaf_quad).  The BVH4 kernels with a global fallback test a leaf primitive
  // with one dependent load instead of two; the all-LDS kernels copy the records into LDS as they are.
  std::vector<float4> lg(leaf_geo_quads(nrefs), make_float4(0.f, 0.f, 0.f, 0.f));
  for (size_t j = 0; j < nrefs; ++j) {
    const uint32_t ref = R.refs[j], idx = ref & 0x3FFFFFFFu;
    if ((ref >> 30) == REF_TRI) { lg[3 * j] = items.geo[3 * idx]; lg[3 * j + 1] = items.geo[3 * idx + 1]; }
    float rf;
    std::memcpy(&rf, &ref, sizeof rf);
    lg[3 * j + 2] = make_float4((ref >> 30) == REF_TRI ? items.geo[3 * idx + 2].x : 0.f, rf, 0.f, 0.f);
  }
  if (lg.size() != (size_t)3 * (nrefs + 1)) throw std::runtime_error("leaf_geo: not 3 x (refs + 1) records");
  if (R.depth > STACK_DEPTH - 1) throw std::runtime_error("BVH deeper than the traversal stack");
  // the 4-wide tree for the queue traversal kernels of non-fractal profiles (Traversal4), and the threaded list
  // of the wave-coherent walk (packet_walk, dev_trace.h)
  bvh::Result4 Q = bvh::collapse4(R);
  std::vector<float> pkt = bvh::threaded(R);
  DeriveCounts k;
  k.n2 = (uint32_t)(R.nodes.size() / 16); k.nrefs = nrefs;
  k.bvh_depth = R.depth; k.bvh_leaves = R.leaves; k.max_leaf = R.max_leaf;
  k.n4 = (uint32_t)(Q.nodes.size() / 28); k.bvh4_depth = Q.depth; k.stack_need = Q.stack_need;
  k.pkt_entries = (uint32_t)(pkt.size() / 8);
  ScenePlan P = scene_plan_counts(d, std::move(items), k);
  P.bvh2 = std::move(bvh2);
  P.leaf_geo = std::move(lg);
  P.nodes4 = std::move(Q.nodes);
  P.pkt = std::move(pkt);
  return P;
}

ScenePlan scene_plan_counts(const bling_scene_desc& d, SceneItems&& items, const DeriveCounts& k) {
  ScenePlan P;
  P.items = std::move(items);
  const SceneItems& I = P.items;
  std::vector<bvh::Box>().swap(P.items.boxes);   // the tree is built: its items are not kept for the uploads
  std::vector<uint32_t>().swap(P.items.refs);
  const uint32_t nt = d.num_triangles, ns = d.num_shapes, nrefs = k.nrefs, n2 = k.n2;
  const bool fractal = I.fractal_prim >= 0;
  DevScene& S = P.S;
  PlanSummary& info = P.info;
  std::memcpy(S.world_c, I.world_c, sizeof S.world_c);
  S.world_r = I.world_r;
  std::memcpy(S.kd_lo, I.kd_lo, sizeof S.kd_lo);
  std::memcpy(S.kd_hi, I.kd_hi, sizeof S.kd_hi);
  info.prims = d.num_prims;
  info.bvh_depth = k.bvh_depth; info.bvh_leaves = k.bvh_leaves; info.max_leaf = k.max_leaf;
  if (k.bvh_depth > STACK_DEPTH - 1) throw std::runtime_error("BVH deeper than the traversal stack");
  info.features = bfeat::scene_features(&d);
  static_assert(FT_PROCTEX == bfeat::PROCTEX && FT_BUMP == bfeat::BUMP && FT_MATTE == bfeat::MATTE &&
                FT_MULTI_LIGHT == bfeat::MULTI_LIGHT, "feature bits");
  S.num_nodes = n2;
  plan_lds(S, n2, nt, nrefs, (uint32_t)k.bvh_depth + 1);
  P.lds_trace = lds_bytes(S.lds_nodes, S.lds_tris, S.lds_refs, S.stack_depth);
  P.lds_all = S.lds_nodes == n2 && S.lds_tris == nt && S.lds_refs == nrefs;
  {
    const uint32_t n4 = k.n4;
    plan_lds4(S, n4, nt, nrefs, (uint32_t)std::max(1, k.stack_need), ns);
    info.lds_all4 = S.lds4_nodes == n4 && S.lds4_tris == nt && S.lds4_refs == nrefs &&
                    S.stack4_lds == S.stack4_need && S.lds4_shapes == ns;
    // the all-LDS kernels lay the primitives out in leaf order (dev_trace.h lds_setup<..., LEAF>)
    info.lds_trace4 = info.lds_all4 ? lds_bytes4_leaf(S.lds4_nodes, S.lds4_refs, S.stack4_lds, S.lds4_shapes)
                                    : lds_bytes4(S.lds4_nodes, S.lds4_tris, S.lds4_refs, S.stack4_lds, S.lds4_shapes);
    info.bvh4_depth = k.bvh4_depth;
    S.num_nodes4 = n4;
  }
  {
    // small scenes walk the threaded BVH wave-coherently (packet_walk, dev_trace.h): at most
    // kPacketMaxEntries child boxes, no fractal
    const uint32_t ne = k.pkt_entries;
    const bool on = !fractal && ne > 0 && ne <= kPacketMaxEntries;
    S.pkt_n = on ? ne : 0u;
    S.pkt_refs = nrefs;
    S.sample_major = on ? 1u : 0u;       // k_raygen's slot order: see there
  }
  {
    // scenes of at most kBruteMax primitives test all of them per ray (brute_walk, dev_trace.h) instead
    // of walking a tree; BLING_BRUTE=<n> sets the limit (0: never), for A/B measurements
    const char* env = std::getenv("BLING_BRUTE");
    const uint32_t lim = env ? (uint32_t)std::strtoul(env, nullptr, 10) : kBruteMax;
    const bool on = !fractal && nt + ns > 0 && nt + ns <= lim && nrefs == (size_t)nt + ns;
    S.bf_tris = on ? nt : 0u;
    S.bf_shapes = on ? ns : 0u;
  }
  // --- shapes
  P.shapes.resize(ns);
  for (uint32_t k = 0; k < ns; ++k) {
    const bling_shape& s = d.shapes[k];
    DevShape& o = P.shapes[k];
    o.kind = s.kind; o.material = s.material; o.light = s.light; o.prim = I.shape_prim[k];
    std::memcpy(o.params, s.params, sizeof o.params);
    std::memcpy(o.w2o, s.w2o, 64);
    std::memcpy(o.o2w, s.o2w, 64);
  }
  // The MIS cull (wavefront.h mis_cull_test) tests the sampled area light's own shape only: it holds
  // when no other shape carries that light.  The loader pairs them one to one; a hand-made
  // description that does not renders without the cull.
  P.mis_cull_ok = true;
  for (uint32_t k = 0; k < ns; ++k) {
    const int l = d.shapes[k].light;
    if (l >= 0 && !((uint32_t)l < d.num_lights && d.lights[l].kind == BLING_LIGHT_AREA && d.lights[l].shape == (int)k))
      P.mis_cull_ok = false;
  }
  // --- infinite lights: each CDF travels with its guide table; the marginal buffer also carries the
  // sky's Perez denominators (host libm, as the oracle evaluates them)
  P.tables.resize(d.num_lights);
  for (uint32_t k = 0; k < d.num_lights; ++k) {
    const bling_light& l = d.lights[k];
    if (l.kind != BLING_LIGHT_INFINITE) continue;
    const size_t nu = l.dist_nu, nv = l.dist_nv;
    P.tables[k].rows = with_guide(l.dist_cdf, nu + 1, nv);
    std::vector<float>& marg = P.tables[k].marg = with_guide(l.marg_cdf, nv + 1, 1);
    float den[3] = {0.f, 0.f, 0.f};
    if (l.env_kind == BLING_ENV_SUNSKY) {
      const float* ps[3] = {l.perez_x, l.perez_y, l.perez_Y};
      const float st = l.sun_theta, cst = bcr::cosf(st);
      for (int j = 0; j < 3; ++j) {                  // perez's denominator (SunSky.hs:81-86)
        const float* q = ps[j];
        den[j] = (1.f + q[0] * bcr::expf(q[1])) * (1.f + q[2] * bcr::expf(q[3] * st)) + q[4] * cst * cst;
      }
    }
    marg.insert(marg.end(), den, den + 3);
  }
  // --- DevScene: everything but the device pointers
  S.fractal = d.fractal; S.fractal_prim = I.fractal_prim;
  {
    long long pw = 1;                     // order ^ k is a Haskell Int: 8^14 needs 64 bits
    for (int k = 0; k < 32; ++k) { S.fractal_pw[k] = (float)pw; pw *= (long long)d.fractal.order; }
    if (d.fractal.present && (d.fractal.iterations < 0 || d.fractal.iterations > 32))
      throw std::runtime_error("fractal iterations outside [0, 32]");
  }
  S.num_lights = (int32_t)d.num_lights;
  plan_config(S, d);
  info.bvh4_nodes = S.num_nodes4; info.stack4_need = S.stack4_need; info.stack4_lds = S.stack4_lds;
  info.pkt_n = S.pkt_n; info.bf_prims = S.bf_tris + S.bf_shapes; info.sample_major = S.sample_major;
  info.lds4_shapes = S.lds4_shapes; info.lds4_tris = S.lds4_tris; info.lds4_nodes = S.lds4_nodes;
  return P;
}

std::string summary_json(const PlanSummary& p) {
  char tmp[1024];
  const int n = std::snprintf(tmp, sizeof tmp,
      "{\"prims\": %u, \"bvh_depth\": %d, \"bvh_leaves\": %d, \"bvh4_nodes\": %u, \"bvh4_depth\": %d, "
      "\"stack4_need\": %u, \"lds_all4\": %d, \"lds_trace4\": %zu, \"pkt_n\": %u, \"bf_prims\": %u, "
      "\"features\": %u, \"stack4_lds\": %u, \"lds4_shapes\": %u, \"lds4_tris\": %u, "
      "\"lds4_nodes\": %u, \"max_leaf\": %d, \"sample_major\": %u}",
      p.prims, p.bvh_depth, p.bvh_leaves, p.bvh4_nodes, p.bvh4_depth, p.stack4_need, p.lds_all4 ? 1 : 0,
      p.lds_trace4, p.pkt_n, p.bf_prims, p.features, p.stack4_lds,
      p.lds4_shapes, p.lds4_tris, p.lds4_nodes, p.max_leaf, p.sample_major);
  if (n < 0 || (size_t)n >= sizeof tmp) throw std::runtime_error("format error");
  return std::string(tmp, (size_t)n);
}

}  // namespace bplan
