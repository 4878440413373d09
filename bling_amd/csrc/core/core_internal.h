// core_internal.h -- host-side state of the MI355X core shared by its translation units:
// the context (bling_ctx), device buffers, kernel feature profiles and the per-profile entry points
// that the profile units (prof_*.hip) instantiate.  Splitting the kernel instantiations by profile
// lets the build compile them in parallel.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/bling.h"
#include "../common/scene_features.h"
#include "../common/gamma_table.h"
#include "bvh_build.h"
#include "scene_plan.h"
#include "wavefront.h"
#include "sppm.h"
#include "light_tracer.h"
#include "bidir.h"
#include "mlt.h"
#include "splat_merge.h"

namespace bcore {
using namespace bd;

struct HipError : std::runtime_error { using std::runtime_error::runtime_error; };
// An entry point's refusal under a BLING_E* code of its own (guarded returns it; any other exception is BLING_EINVAL)
struct Refusal : std::runtime_error {
  int code;
  Refusal(int code, const std::string& msg) : std::runtime_error(msg), code(code) {}
};

#define HIPCHK(x)                                                                        \
  do {                                                                                   \
    hipError_t e_ = (x);                                                                 \
    if (e_ != hipSuccess) throw HipError(std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

// ------------------------------------------------------------------ device buffers
template <class T>
struct DBuf {
  T* p = nullptr;
  size_t n = 0;
  DBuf() = default;
  DBuf(const DBuf&) = delete;              // owns device memory: never copied
  DBuf& operator=(const DBuf&) = delete;
  void alloc(size_t count) {
    free();
    if (count == 0) return;
    HIPCHK(hipMalloc(&p, count * sizeof(T)));
    n = count;
  }
  void upload(const T* h, size_t count) {
    alloc(count);
    if (count) HIPCHK(hipMemcpy(p, h, count * sizeof(T), hipMemcpyHostToDevice));
  }
  void free() { if (p) { (void)hipFree(p); p = nullptr; n = 0; } }
  ~DBuf() { free(); }
};

// A HIP event, destroyed on every way out of its scope (a HIPCHK that throws included); moved, never copied.
struct Event {
  hipEvent_t e = nullptr;
  explicit Event(bool timing = true) { HIPCHK(timing ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming)); }
  Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
  ~Event() { if (e) (void)hipEventDestroy(e); }
  operator hipEvent_t() const { return e; }
  void record(hipStream_t s) const { HIPCHK(hipEventRecord(e, s)); }
};
inline float elapsed_ms(const Event& from, const Event& to) { float ms = 0.f; HIPCHK(hipEventElapsedTime(&ms, from, to)); return ms; }
struct EventPair {     // the two events around something timed
  Event a, b;
  float elapsed_ms() const { return bcore::elapsed_ms(a, b); }
};

// device bytes per path in flight, for sizing waves: per path set the SoA streams of wavefront.h
// PathSet (org, dir, hit, meta, mdir, fac, sh_o, sh_d: 16 B each; mhit 8 B; fm, occ, rtex 4 B each),
// T and L (64 B each) and, for the non-factored profiles, Tn, lsc and bsc (64 B each); two sets for the Path
// pipeline, plus result, img, six queue words and the queue flag
constexpr uint64_t kSetBytes = 8 * 16 + 8 + 3 * 4 + 64 + 64;
constexpr uint64_t kSetSpectraBytes = 3 * 64;
constexpr uint64_t kLeanSetBytes = 4 * 16;   // the normal-map integrator's set: org, dir, hit, meta
constexpr uint64_t kPathFixedBytes = 16 + 8 + 6 * 4 + 1 + 4 + 2 * 4;   // ... + the k_march results (2 words)
// DirectLighting adds the continuation origin, the sibling mask and one parked ray (org, dir,
// weight) per level below maxDepth
constexpr uint64_t kDlSlotBytes = 16 + 16 + 64;
constexpr int kMaxDlDepth = 16;
// The bidirectional integrator keeps no path set; per sample it stores 2 maxDepth vertex records (ray,
// direction, hit, wo: 16 B each; alpha 64 B), maxDepth direct and maxDepth connection spectra, the le
// term and the lengths / masks (bidir.h BdBufs)
constexpr uint64_t kBdVertexBytes = 4 * 16 + 64;
inline uint64_t bd_sample_bytes(int md) { return (uint64_t)md * (2 * kBdVertexBytes + 2 * 64) + 64 + 16; }

// SPPM renderer state (sppm.h): hit points, hash grid and the per-pixel statistics that persist
// across passes (reset by a scene upload or bling_sppm_reset)
struct SppmState {
  bool ready = false;
  uint32_t hp_cap = 0, items_cap = 0, n_stats = 0, nth = 0, n_tiles = 0, n_ext = 0;
  DBuf<float4> hp_pos, hp_hit, hp_o, hp_d, hp_f, result;
  DBuf<Bsdf> hp_bsdf;
  DBuf<float2> img;
  DBuf<uint32_t> hp_count, cnt, bstart, bcur, items;
  DBuf<float> r2, nacc, splat, film, kd_mr, kd_c;
  DBuf<unsigned long long> hp_key;
  DBuf<SppmGrid> grid;
  DBuf<unsigned long long> ctr;
  DBuf<TileDesc> tiles;
  // ordered mode (BLING_SPLAT_ORDERED): the tile images of the eye film, one sampler's splat image, one
  // launch's counts, counters, records and record count
  DBuf<float4> timg;
  DBuf<float> thread_img;
  DBuf<uint32_t> cnt_tmp, rec_count;
  DBuf<unsigned long long> rctr;
  DBuf<uint4> rec;
  void free_all() {
    timg.free(); thread_img.free(); cnt_tmp.free(); rec_count.free(); rctr.free(); rec.free();
    for (auto* b : {&hp_pos, &hp_hit, &hp_o, &hp_d, &hp_f, &result}) b->free();
    img.free(); hp_bsdf.free();
    for (auto* b : {&hp_count, &cnt, &bstart, &bcur, &items}) b->free();
    for (auto* b : {&r2, &nacc, &splat, &film, &kd_mr, &kd_c}) b->free();
    hp_key.free(); grid.free(); ctr.free(); tiles.free();
    ready = false; hp_cap = items_cap = 0;
  }
};

// Bidirectional integrator state (bidir.h): the vertex buffers of one wave, sized for the largest wave a
// bidir scene of this context asked for (not for the path capacity an earlier scene left behind)
struct BidirState {
  DBuf<float4> vorg, vdir, vhit, vwo, valpha, ld, conn, le;
  DBuf<uint4> info;
  uint32_t cap = 0;
  int md = 0;
  void alloc(uint32_t n, int depth) {
    cap = n; md = depth;
    const size_t v = (size_t)2 * depth * n, e = (size_t)depth * n;
    for (auto* b : {&vorg, &vdir, &vhit, &vwo}) b->alloc(v);
    valpha.alloc(4 * v); ld.alloc(4 * e); conn.alloc(4 * e); le.alloc((size_t)4 * n); info.alloc(n);
  }
  void free_all() {
    for (auto* b : {&vorg, &vdir, &vhit, &vwo, &valpha, &ld, &conn, &le}) b->free();
    info.free(); cap = 0; md = 0;
  }
};

// Light tracer state (light_tracer.h): the splat image, counters and the record buffer of record mode
struct LightState {
  DBuf<float> splat;
  DBuf<unsigned long long> ctr;
  DBuf<uint4> rec;
  DBuf<uint32_t> rec_count;
  void free_all() { splat.free(); ctr.free(); rec.free(); rec_count.free(); }
};

// Metropolis renderer state (mlt.h): the chains' primary samples, their current contribution, the
// bootstrap contributions and the record buffer of record mode; the splat image is the light tracer's
struct MltState {
  DBuf<float> cur, prop, cur_l, boot_i;
  DBuf<float4> lfull;
  DBuf<uint32_t> flags, start;
  DBuf<unsigned long long> ctr;
  DBuf<uint4> rec;
  void free_all() {
    for (auto* b : {&cur, &prop, &cur_l, &boot_i}) b->free();
    lfull.free(); flags.free(); start.free(); ctr.free(); rec.free();
  }
};

// Ordered splat merge state (splat_merge.h): the per-pixel counts, segment starts, the scan's block sums,
// the list of long segments, the segments' keys and values, the record buffer the ordered Metropolis pass
// and bling_debug_splat_merge fill, and the record budget (0: the default, from the device's memory)
struct MergeState {
  DBuf<uint32_t> cnt, start, sums, longs, rec_count;
  DBuf<unsigned long long> key;
  DBuf<float4> val;
  DBuf<uint4> rec;
  size_t budget = 0, default_budget = 0;
  double ms_kernel = 0., ms_merge = 0.;   // the last ordered pass: its photon / chain launches, its merges
  void free_all() {
    for (auto* b : {&cnt, &start, &sums, &longs, &rec_count}) b->free();
    key.free(); val.free(); rec.free();
  }
};

// Image API state (image_ops.hip): per-sample results (X, Y, Z, valid) of one chunk, the per-tile counts,
// segment starts, the scan's block sums and the (tile, sample) pair buffer, the drop / pair counters, the
// host variant's staging buffers, and the pair budget (0: the default).  The windowed calls add each sample's
// window, the windows' sample offsets and cover rectangles, the carry image of a window cut by a chunk's end,
// and the host variant's second staged image.
struct ImageState {
  DBuf<float4> res;
  DBuf<uint32_t> cnt, start, sums, pairs;
  DBuf<unsigned long long> ctr;
  DBuf<float> xy, spectra, target;
  DBuf<uint32_t> win;
  DBuf<unsigned long long> first;
  DBuf<int4> cover;
  DBuf<float> carry, target2;
  size_t budget = 0;
};

// The integrator seam for a caller's rays (li_rays.hip): a wave's 16-band records, its dropped flags, the
// dropped counter, the host variant's staging buffers, and the debug chunk (0: the default).
struct LiState {
  DBuf<float4> lfull;
  DBuf<uint8_t> drop;
  DBuf<unsigned long long> ctr;
  DBuf<float> rays, L;
  DBuf<uint32_t> ids;
  size_t chunk = 0;
};

// The sampler and camera seam (cam_samples.hip): the call's window records (32 B each, cam_samples.h CamWin)
// and offsets on the device, and the host variant's staging buffers.
struct CamState {
  DBuf<uint4> wins;
  DBuf<unsigned long long> first;
  DBuf<float> xy, rays, lens;
  DBuf<uint32_t> ids;
};

}  // namespace bcore

struct bling_ctx;
namespace bcore {
// core.hip: the thread's bling_last_error text, for entry points defined in other units
void set_last_error(const std::string& msg);
// runs an entry point's body: no C++ exception crosses the ABI, the error text is kept for bling_last_error
template <class F>
int guarded(F f) {
  try {
    return f();
  } catch (const Refusal& e) {
    set_last_error(e.what());
    return e.code;
  } catch (const HipError& e) {
    set_last_error(e.what());
    return BLING_EHIP;
  } catch (const std::bad_alloc&) {
    set_last_error("out of memory");
    return BLING_ENOMEM;
  } catch (const std::exception& e) {
    set_last_error(e.what());
    return BLING_EINVAL;
  }
}
// splat_merge.hip: start[0 .. n] = the exclusive prefix of cnt[0 .. n) (start[n] the total), enqueued on s;
// sums holds (n + 1023) / 1024 + 1 words of scratch
void sm_scan(hipStream_t s, const uint32_t* cnt, uint32_t n, uint32_t* sums, uint32_t* start);
// splat_merge.hip: the record budget of this context's ordered passes; the ordered merge of n records
// (layout SM_LAYOUT_*) into the device image img (W * H * 3), enqueued on the context's stream
size_t splat_budget(bling_ctx* c);
void splat_merge(bling_ctx* c, const uint4* recs, size_t n, int layout, float* img);
// film_develop.hip: bytes per pixel of a BLING_DEVELOP_* format; the window clipped to the uploaded
// scene's image (false: empty); the threshold table's upload; one develop launch on the context's stream
size_t develop_pixel_bytes(int format);
bool develop_clip(const bling_ctx* c, const int32_t* window, int* x0, int* x1, int* y0, int* y1);
void develop_table(bling_ctx* c);
void develop_launch(bling_ctx* c, const bling_develop_params* dp, const float* film, const float* splat, void* out);
// the same for an image of w x h pixels that is not the uploaded scene's (bling_image_develop_device)
void develop_launch(bling_ctx* c, const bling_develop_params* dp, int w, int h, const float* film, const float* splat, void* out);
// bvh_device.hip: the linear BVH of common/lbvh.h over the items (3 <= n <= 2^24), built on the context's device
// and read back into R once.  false, with R untouched, when the tree is deeper than depth_cap (*depth holds
// its depth).  *ms: HIP events around the kernels.  With n_kept, the tree stays on the device instead: the nodes go
// to c->nodes and the refs to c->refs, *n_kept receives the node count, and R holds depth, leaves and max_leaf alone.
bool lbvh_build_device(bling_ctx* c, const std::vector<bvh::Box>& boxes, const std::vector<uint32_t>& refs, int depth_cap,
                       bvh::Result& R, float* ms, int* depth, uint32_t* n_kept = nullptr);
// bvh_derive.hip: the leaf records (c->leaf_geo) and the BVH4 (c->nodes4) of the BVH2 in c->nodes / c->refs over the
// n_tris triangle records of c->tri_geo, on the context's device (common/bvh4.h).  k.n2 and k.nrefs go in; k.n4,
// k.bvh4_depth and k.stack_need come out, and info's bvh4_*, stack_need, level_launches and ms_derive_device.
void bvh_derive_device(bling_ctx* c, uint32_t n_tris, bplan::DeriveCounts& k, bling_derive_info* info);
}  // namespace bcore

// the context lives in the global namespace (include/bling.h declares `struct bling_ctx`)
using namespace bd;
using namespace bcore;

struct bling_ctx {
  using WaveState = bd::WaveState;
  int device = 0;
  hipStream_t stream = nullptr;
  // a pipelined pass (core.hip render): one stream per half-wave, the event they start after and the
  // events the film waits on; created by the first such pass
  hipStream_t half_stream[2] = {nullptr, nullptr};
  hipEvent_t half_fork = nullptr, half_done[2] = {nullptr, nullptr};
  // the shade grid of a half-wave: four blocks per CU, the blocks k_shade keeps resident (one round of
  // blocks, not grid_for's two).  Measured on C2 with the half traversal grids, pass ms pipelined /
  // single in one process: 1 block per CU 70.1 / 65.8, 2: 61.6 / 64.4, 3: 61.5 / 65.7, 4: 60.7 / 65.4,
  // grid_for's 8: 60.8 / 65.7 (profiles/r09_c2_pipeline_ab.jsonl)
  unsigned half_shade_blocks = 4 * 256;
  int pipeline_mode = -1;       // bling_debug_set_pipeline: -1 the profile's default, 0 never, 1 wherever legal
  int last_pass_waves = 0;      // waves of the last render pass on this device; -2: two half-waves in flight together
  uint32_t last_n[2] = {0, 0}, last_off[2] = {0, 0};   // the samples of its last wave (or two half-waves) in result
  bool has_scene = false;
  DevScene S{};
  // scene memory
  DBuf<float4> nodes, tri_geo, pkt;   // BVH2 nodes, triangle records, threaded entry list
  DBuf<float4> leaf_geo;              // primitive records in leaf order, each with its ref (dev_trace.h LeafRec)
  DBuf<uint32_t> refs;
  DBuf<float> tri_normals;
  DBuf<float4> tri_frame;
  DBuf<uint8_t> tri_has_n;
  DBuf<int32_t> tri_material, tri_prim, shape_prim;
  DBuf<DevShape> shapes;
  DBuf<bling_material> materials;
  DBuf<bling_texture> textures;
  DBuf<bling_scalar_texture> stex;
  DBuf<bling_light> lights;
  DBuf<bling_image> images;
  std::vector<std::unique_ptr<DBuf<float>>> light_arrays;   // Dist2D tables, env maps, texture images
  // path state (WaveState): two sets of per-slot records (PathSet), by-sample arrays, queues
  uint32_t cap = 0;
  struct SetBufs {
    DBuf<float4> org, dir, hit, mdir, fac, sh_o, sh_d, T, Tn, L, lsc, bsc;
    DBuf<uint4> meta;
    DBuf<float2> mhit;
    DBuf<float> fm;
    DBuf<uint32_t> occ, rtex;
    // lean: the records the camera rays, one closest-hit launch and the film need (org, dir, hit,
    // meta) and nothing else -- the normal-map integrator's set (normals.h)
    void alloc(uint32_t n, bool spectra, bool lean = false) {
      if (lean) {
        free();
        for (auto* b : {&org, &dir, &hit}) b->alloc(n);
        meta.alloc(n);
        return;
      }
      for (auto* b : {&org, &dir, &hit, &mdir, &fac, &sh_o, &sh_d}) b->alloc(n);
      meta.alloc(n); mhit.alloc(n); fm.alloc(n); occ.alloc(n); rtex.alloc(n);
      T.alloc((size_t)4 * n); L.alloc((size_t)4 * n);
      if (spectra) { Tn.alloc((size_t)4 * n); lsc.alloc((size_t)4 * n); bsc.alloc((size_t)4 * n); }
      else { Tn.free(); lsc.free(); bsc.free(); }
    }
    void free() {
      for (auto* b : {&org, &dir, &hit, &mdir, &fac, &sh_o, &sh_d, &T, &Tn, &L, &lsc, &bsc}) b->free();
      meta.free(); mhit.free(); fm.free(); occ.free(); rtex.free();
    }
    PathSet view() const {
      return PathSet{org.p, dir.p, hit.p, meta.p, mdir.p, mhit.p, fm.p, occ.p, fac.p, rtex.p, sh_o.p, sh_d.p,
                     T.p, Tn.p, L.p, lsc.p, bsc.p};
    }
  } set[2];
  bool sets_spectra = false, sets_two = false, sets_lean = false;   // layout of the allocated sets
  DBuf<float4> corg, dl_org, dl_dir, dl_T;          // DirectLighting only
  DBuf<uint32_t> dl_mask;
  int dl_levels = 0;                                // slots allocated per path (0 = Path)
  DBuf<float4> result;
  DBuf<float2> img;
  DBuf<uint32_t> qmem, qcount, blk;
  DBuf<float> march;                                 // k_march results, one per closest / any queue entry
  DBuf<uint8_t> qflag;
  DBuf<TileDesc> tiles_dev;
  DBuf<Counters> counters;
  uint64_t mis_culled = 0;      // Counters::mis_culled of the last pass (bling_debug_mis_culled)
  // every shape that carries an area light is that light's own shape (wavefront.h mis_cull_test)
  bool mis_cull_ok = false;
  bool mis_cull_off = false;    // bling_debug_set_mis_cull(ctx, 0): bling_sample_li walks every MIS ray too
  uint64_t stream_bytes[2 * BLING_N_STREAMS] = {};   // Counters::sb of the last pass (BLING_STREAM_STATS)
  DBuf<DevScene> dscene;      // the DevScene record in device memory (kernels take a pointer)
  DBuf<float> film_dev;
  // bling_film_develop (film_develop.hip): rgbPixels' threshold table, uploaded with the context, and
  // the host variant's staging buffers for the splat image and the developed image (the film stages
  // through film_dev)
  DBuf<float> gamma_tab, develop_splat;
  DBuf<uint8_t> develop_out;
  // trace scratch
  DBuf<float> tr_rays, tr_t, tr_bary;
  DBuf<uint32_t> tr_prim;
  // the uploaded scene's plan (scene_plan.h), as scene_upload.hip left it: the summary, and the fields the
  // launches read
  bplan::PlanSummary plan_info;      // bling_debug_scene_info
  bling_bvh_build_info bvh_info{};   // how the uploaded BVH2 was built (bling_debug_bvh_build_info)
  int bvh_depth_cap = 0;             // bling_debug_set_bvh_depth_cap: 0 = STACK_DEPTH - 1
  bling_derive_info derive_info{};   // where what follows the BVH2 was derived (bling_debug_derive_info)
  uint32_t features = FT_ALL;   // scene_features() of the uploaded scene
  size_t lds_trace = 0;         // dynamic LDS bytes of the traversal kernels
  bool lds_all = false;         // the whole BVH, triangle set and leaf refs are LDS-resident
  size_t lds_trace4 = 0;        // the same for the BVH4 plan (queue traversal kernels, dev_trace.h Traversal4)
  bool lds_all4 = false;
  DBuf<float4> nodes4;          // BVH4 nodes
  DBuf<int32_t> stack4_ovf;     // BVH4 stack rows beyond the LDS ones
  bling_render_config cfg{};    // the uploaded scene's renderer configuration
  SppmState sppm;
  LightState light;
  BidirState bidir;
  bling_light_tracer lt{};      // the uploaded scene's light tracer block (photons per pass)
  MltState mlt;
  bling_metropolis mp{};        // the uploaded scene's Metropolis block
  std::vector<float> mlt_boot_override;   // bling_debug_mlt_set_boot: I values that replace the evaluated ones
  // Multi-device fan-out (bling_create with n_devices > 1): one context per further device; every
  // device renders its share as tile images, the peers push theirs over xGMI into stage, and the
  // primary adds them all (Rendering.hs:118).
  std::vector<std::unique_ptr<bling_ctx>> peers;
  DBuf<float> pass_tiles;          // this device's tile images of the pass (BLING_PASS_TILE_IMAGES)
  DBuf<TileSrc> tile_src;          // the merge's per-tile sources (k_add_tiles)
  DBuf<const float4*> rank_bufs;   // the ordered merge's per-rank tile-image buffers (k_film_add_ordered)
  std::vector<std::unique_ptr<DBuf<float>>> stage;  // primary: landing buffer of peer j's tile images
  MergeState merge;                // the ordered splat merge (splat_merge.h)
  ImageState image;                // the image API (image_ops.hip)
  LiState li;                      // the integrator seam for a caller's rays (li_rays.hip)
  CamState cam;                    // the sampler and camera seam (cam_samples.hip)

  ~bling_ctx() {
    peers.clear();                          // each peer frees its memory on its own device
    (void)hipSetDevice(device);
    for (int h = 0; h < 2; ++h) {
      if (half_stream[h]) (void)hipStreamDestroy(half_stream[h]);
      if (half_done[h]) (void)hipEventDestroy(half_done[h]);
    }
    if (half_fork) (void)hipEventDestroy(half_fork);
    if (stream) (void)hipStreamDestroy(stream);
  }

  int want_dl_levels() const { return S.integrator == BLING_INTEGRATOR_DIRECT ? S.max_depth : 0; }
  // the uploaded scene's kernel profile keeps the three non-factored spectra per slot (wavefront.h
  // factored()); DirectLighting runs in place on one set
  bool want_spectra() const;
  bool want_two_sets() const { return S.integrator == BLING_INTEGRATOR_PATH; }
  int want_bd_depth() const { return S.integrator == BLING_INTEGRATOR_BIDIR ? S.max_depth : 0; }
  bool want_lean() const { return S.integrator == BLING_INTEGRATOR_NORMALS; }
  uint64_t path_bytes() const {
    const uint64_t set_b = want_lean() ? kLeanSetBytes : kSetBytes + (want_spectra() ? kSetSpectraBytes : 0);
    return (want_two_sets() ? 2 : 1) * set_b + kPathFixedBytes + (want_dl_levels() ? 20 + kDlSlotBytes * want_dl_levels() : 0) +
           (want_bd_depth() ? bd_sample_bytes(want_bd_depth()) : 0);
  }

  void ensure_paths(uint32_t n) {
    const int lv = want_dl_levels();
    const bool sp = want_spectra(), two = want_two_sets();
    // the bidir vertex buffers follow the waves asked for, not cap, which never shrinks: after a large
    // Path pass a bidir scene would otherwise allocate its 384 maxDepth + 80 bytes for every old slot
    if (const int bdm = want_bd_depth()) {
      const uint32_t need = (n + 255u) & ~255u;
      if (bidir.md != bdm || bidir.cap < need) bidir.alloc(need, bdm);
    } else if (bidir.cap) {
      bidir.free_all();
    }
    const bool lean = want_lean();
    const bool relayout = lv != dl_levels || sp != sets_spectra || two != sets_two || lean != sets_lean;
    if (n <= cap && !relayout) return;
    cap = std::max(cap, (n + 255u) & ~255u);
    dl_levels = lv; sets_spectra = sp; sets_two = two; sets_lean = lean;
    set[0].alloc(cap, sp, lean);
    if (two) set[1].alloc(cap, sp); else set[1].free();
    if (lv) {
      corg.alloc(cap); dl_mask.alloc(cap);
      dl_org.alloc((size_t)lv * cap); dl_dir.alloc((size_t)lv * cap); dl_T.alloc((size_t)4 * lv * cap);
    } else {
      for (auto* b : {&corg, &dl_org, &dl_dir, &dl_T}) b->free();
      dl_mask.free();
    }
    result.alloc(cap); img.alloc(cap);
    qmem.alloc((size_t)6 * cap);     // SHADE0, SHADE1, CLOSEST (2 cap), ANY, RESOLVE
    march.alloc((size_t)2 * cap);    // reused: closest-queue results, then any-queue results
    qcount.alloc(2 * kQcountStride);   // per half-wave: the Q_N queue lengths and the culled MIS count (QC_MISCULL)
    qflag.alloc(cap);
    blk.alloc((size_t)5 * (cap / COMPACT_CHUNK + 4) + 4);   // per half-wave: [nb][4], totals [4], culled [nb]
  }
  static constexpr uint32_t kQcountStride = 8;
  static_assert(kQcountStride >= QC_N, "a half-wave's counters");
  void ensure_half_streams() {
    for (int h = 0; h < 2; ++h) {
      if (!half_stream[h]) HIPCHK(hipStreamCreateWithFlags(&half_stream[h], hipStreamNonBlocking));
      if (!half_done[h]) HIPCHK(hipEventCreateWithFlags(&half_done[h], hipEventDisableTiming));
    }
    if (!half_fork) {
      HIPCHK(hipEventCreateWithFlags(&half_fork, hipEventDisableTiming));
      int cus = 0;
      if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
        half_shade_blocks = 4u * (unsigned)cus;
    }
  }
  WaveState state() {
    WaveState W{};
    W.cur = set[0].view();
    W.nxt = sets_two ? set[1].view() : W.cur;
    W.corg = dl_levels ? corg.p : nullptr;
    W.img = img.p; W.result = result.p;
    W.Lfull = nullptr; W.dbg = nullptr;
    W.march_t = march.p;             // run_wave_t keeps it for Mandelbulb scenes only (k_march)
    W.dl_org = dl_levels ? dl_org.p : nullptr; W.dl_dir = dl_levels ? dl_dir.p : nullptr;
    W.dl_T = dl_levels ? dl_T.p : nullptr; W.dl_mask = dl_levels ? dl_mask.p : nullptr;
    W.queue[Q_SHADE0] = qmem.p;
    W.queue[Q_SHADE1] = qmem.p + cap;
    W.queue[Q_CLOSEST] = qmem.p + 2 * (size_t)cap;
    W.queue[Q_ANY] = qmem.p + 4 * (size_t)cap;
    W.queue[Q_RESOLVE] = qmem.p + 5 * (size_t)cap;
    W.qcount = qcount.p;
    W.qflag = qflag.p;
    W.blk = blk.p;
    W.sb = counters.p ? counters.p->sb : nullptr;
    W.cap = cap;
    W.mis_cull = (mis_cull_ok && !mis_cull_off) ? 1u : 0u;   // bling_render_pass* clears it on BLING_PASS_NO_MIS_CULL
    return W;
  }
  // Half-wave h of a pipelined pass (Path only): the first cap_a slots of every buffer are half 0's,
  // the rest half 1's, so the two hold what one wave holds.  cap_a is a multiple of 256: every half's
  // arrays keep the alignment their 16-byte accesses need (flag words, compaction rows).
  WaveState state_half(int h, uint32_t cap_a) {
    WaveState W = state();
    const size_t o = h ? cap_a : 0;
    const uint32_t ch = h ? cap - cap_a : cap_a;
    for (PathSet* P : {&W.cur, &W.nxt}) {
      P->org += o; P->dir += o; P->hit += o; P->meta += o; P->mdir += o; P->mhit += o; P->fm += o; P->occ += o;
      P->fac += o; P->rtex += o; P->sh_o += o; P->sh_d += o;
      P->T += 4 * o; P->L += 4 * o;
      if (P->Tn) { P->Tn += 4 * o; P->lsc += 4 * o; P->bsc += 4 * o; }
    }
    W.img += o; W.result += o;
    W.march_t += 2 * o;
    uint32_t* q = qmem.p + 6 * o;
    W.queue[Q_SHADE0] = q;
    W.queue[Q_SHADE1] = q + ch;
    W.queue[Q_CLOSEST] = q + 2 * (size_t)ch;
    W.queue[Q_ANY] = q + 4 * (size_t)ch;
    W.queue[Q_RESOLVE] = q + 5 * (size_t)ch;
    W.qcount += h * kQcountStride;
    W.qflag += o;
    if (h) W.blk += ((size_t)5 * (cap_a / COMPACT_CHUNK + 2) + 3) & ~(size_t)3;
    W.cap = ch;
    return W;
  }
};

namespace bcore {

// what every entry point that needs the uploaded scene checks first
inline void need_scene(const bling_ctx* c) {
  if (!c->has_scene) throw Refusal(BLING_ENOSCENE, "no scene uploaded");
}

// Host staging of a caller's image of n elements around a pass: the caller's values (host == nullptr: zeros)
// into buf, and back into host when there is one
template <class T>
void stage_in(DBuf<T>& buf, const T* host, size_t n) {
  if (buf.n != n) buf.alloc(n);
  if (host) HIPCHK(hipMemcpy(buf.p, host, n * sizeof(T), hipMemcpyHostToDevice));
  else HIPCHK(hipMemset(buf.p, 0, n * sizeof(T)));
}
template <class T>
void stage_out(T* host, const DBuf<T>& buf, size_t n) {
  if (host) HIPCHK(hipMemcpy(host, buf.p, n * sizeof(T), hipMemcpyDeviceToHost));
}

// Kernel profiles: feature sets the kernels are compiled for.  A scene runs on the first profile
// that covers its features (scene_features.h); the last one covers everything.
// The cornell and sun-sky profiles serve one-light scenes only (dev_scene.h one_light): their light
// record -- for the sun-sky profile the sky model's constants -- is read with scalar loads (sun-sky
// one-light: C4 9 170 -> 9 789 Mrays/s, shade 873 -> 806 ms per pass, profiles/r06_ab_session.txt
// r06s2w); the others serve any number.
constexpr uint32_t kProfiles[] = {
    FT_MATTE | FT_AREA | FT_TRIS,                                                         // cornell
    FT_MATTE | FT_PLASTIC | FT_AREA | FT_ENV_CONST | FT_TRIS | FT_TRI_NORMALS | FT_MULTI_LIGHT,   // meshes
    FT_MATTE | FT_PLASTIC | FT_GLASS | FT_METAL | FT_MIRROR | FT_GRAPHPAPER | FT_AREA | FT_ENV_CONST |
        FT_ENV_SKY | FT_SPHERE,                                                           // analytic shapes (sun-sky)
    FT_MATTE | FT_GRAPHPAPER | FT_AREA | FT_ENV_CONST | FT_ENV_SKY | FT_FRACTAL | FT_MULTI_LIGHT,   // mandelbulb
    FT_ALL & ~(FT_FRACTAL | FT_PROCTEX),                                                  // surfaces
    FT_ALL,
};

// SPPM keeps each hit point's BSDF record between its eye and photon passes; computed spectra
// (FT_PROCTEX) live only while one thread shades, so SPPM runs without them (bling_sppm_pass
// refuses such scenes).  Photons leave area, infinite, point and directional lights (sppm.h light_ray).
constexpr uint32_t kSppmAll = FT_ALL & ~FT_PROCTEX;

template <size_t I = 0, class Fn>
void with_profile(uint32_t need, Fn&& fn) {
  constexpr uint32_t P = kProfiles[I];
  if constexpr (I + 1 < sizeof(kProfiles) / sizeof(kProfiles[0])) {
    if ((need & ~P) != 0u) return with_profile<I + 1>(need, fn);
  }
  fn(std::integral_constant<uint32_t, P>{});
}

inline uint32_t profile_of(uint32_t need) {
  uint32_t p = 0;
  with_profile(need, [&](auto prof) { p = decltype(prof)::value; });
  return p;
}

// The launches bidir_wave is made of, for the Metropolis driver (mlt_pass.hip): the vertex buffers of a
// wave of n samples, and connect + finish of a walked wave.
BdBufs bidir_bufs(bling_ctx* c, uint32_t n, float* terms);
void bidir_connect_finish(bling_ctx* c, const WaveState& W, const BdBufs& B, uint32_t n);
// What a Metropolis pass returns beside the splat image (mlt_pass.hip): b', the chains' start samples
// (bootstrap sample indices) and, in record mode, the records sorted by (chain, mutation).
struct MltOut {
  float b = 0.f;
  std::vector<uint32_t> start;
  std::vector<bling_mlt_record> rec;
};
// One pass of the Metropolis renderer; splat: the device image it accumulates into (nullptr = none), with
// float atomics or, ordered, through splat records and one splat_merge; records of chains
// rec_first .. rec_first + rec_chains - 1 (0 = off).  Throws std::invalid_argument where the reference
// would stop with an error (bootstrap selection on an unwritten slot) and, ordered, when the pass's 2 M
// possible splat records exceed the record budget (before any launch).
void mlt_pass_run(bling_ctx* c, uint32_t seed, uint32_t pass, float* splat, bool ordered, uint32_t rec_first, uint32_t rec_chains,
                  bling_mlt_stats* st, MltOut* out);
// The host bookkeeping of bootstrap (mlt_pass.hip): b' and the chains' start samples from the I values.
float mlt_boot_select(const float* I, uint32_t nboot, uint32_t seed, uint32_t pass, uint32_t chains, uint32_t* start);
// Bootstrap samples evaluated per wave when there are more of them than chains; it bounds the vertex
// buffers a large `bootstrap` asks for (bd_sample_bytes per sample: 100 MB at maxDepth 16)
constexpr uint32_t kMltBootChunk = 16384u;
// M = floor (mpp * nPixels) (Metropolis.hs:86) as a float; NaN or < 1 is refused by validation
inline float mlt_mutations(const bling_metropolis& m, int w, int h) { return floorf(m.mpp * (float)(w * h)); }

}  // namespace bcore

inline bool bling_ctx::want_spectra() const {
  bool full = true;
  bcore::with_profile(features, [&](auto prof) { full = !bd::factored<decltype(prof)::value>(); });
  if (S.integrator == BLING_INTEGRATOR_BIDIR) return false;   // its kernels keep no path set (bidir.h)
  if (S.integrator == BLING_INTEGRATOR_NORMALS) return false; // one closest hit per sample, no spectra (normals.h)
  return full || S.integrator == BLING_INTEGRATOR_DIRECT;
}

namespace bcore {

// Drive one wave of n freshly generated paths to completion (Path.hs:41-87 for every path).
// Queue lengths stay on the device: every launch is a grid-stride loop that reads the live count
// itself, so the host never synchronises inside the loop.
// One half-wave of a pipelined pass: its state, paths and stream, and its tiles (n_tiles entries of
// the pass's tile table on the device, the largest of max_tile samples) for the camera rays.
struct HalfWave {
  WaveState W;
  uint32_t n;
  hipStream_t s;
  const TileDesc* td;
  unsigned n_tiles;
  uint32_t max_tile;
};

// The event pairs of a timed pass (BLING_PASS_KERNEL_TIMING), owned: the wave drivers wrap their closest-hit
// and shading launches in timed() (a pair on s around what fn enqueues), render() harvests after each wave's sync.
struct WaveTiming {
  enum Kind { Closest, Shade };      // each k_trace_closest launch; each (fused resolve +) shade launch
  bool on = false;
  std::vector<EventPair> pairs[2];
  template <class Fn>
  void timed(Kind k, hipStream_t s, Fn&& fn) {
    if (!on) return fn();
    EventPair p;
    p.a.record(s); fn(); p.b.record(s);
    pairs[k].push_back(std::move(p));
  }
  // adds every pair's elapsed time and count to the pass's sums; the launches must have finished
  void harvest(double& ms_closest, uint64_t& n_closest, double& ms_shade, uint64_t& n_shade) {
    for (const EventPair& p : pairs[Closest]) { ms_closest += p.elapsed_ms(); ++n_closest; }
    for (const EventPair& p : pairs[Shade]) { ms_shade += p.elapsed_ms(); ++n_shade; }
    pairs[Closest].clear(); pairs[Shade].clear();
  }
};

inline unsigned grid_for(uint32_t items) {
  constexpr uint32_t kMaxBlocks = 256 * 8;       // 8 blocks of 256 per CU, grid-stride beyond
  return std::max(1u, std::min((items + 255u) / 256u, kMaxBlocks));
}

// Grid of a persistent (grid-stride, lane-refill) kernel: exactly the blocks that are co-resident
// on the device, so no second partial round of blocks idles most CUs at the tail.
// div = 2: half of them, for a half-wave of a pipelined pass that shares the device with the other's.
template <class K>
unsigned persistent_grid(K kernel, size_t lds, uint32_t items, unsigned div = 1) {
  int dev = 0, cus = 0, per_cu = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    cus = 256;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, lds) != hipSuccess || per_cu < 1) per_cu = 1;
  const uint32_t cap = std::max(1u, (uint32_t)(cus * per_cu) / std::max(1u, div));
  return std::max(1u, std::min((items + 255u) / 256u, cap));
}

// Per-profile entry points, explicitly instantiated by prof_<k>.hip (one unit per kProfiles entry;
// the largest profiles compile their shading kernels in prof_<k>a / b (/ c).hip beside it, so
// the build runs them in parallel) and sppm_pass.hip.
template <uint32_t F>
int run_wave_prof(bling_ctx* c, const WaveState& W, uint32_t n, uint32_t seed, uint32_t pass, bool stats, WaveTiming* tm);
// The same for a pipelined pass (core_wave.h run_wave_pair_t): the two half-waves h[0], h[1], from
// their camera rays on.
template <uint32_t F>
int run_wave_pair_prof(bling_ctx* c, const HalfWave* h, uint32_t seed, uint32_t pass, bool stats, WaveTiming* tm);
template <uint32_t F>
void launch_trace_prof(bling_ctx* c, const float* rays, uint32_t n, int any_hit, float* t, uint32_t* prim, float* bary);
template <uint32_t F>
void sppm_pass_t(bling_ctx* c, uint32_t seed, uint32_t pass, float* film, float* splat, uint32_t flags, bling_sppm_stats* st);
// The splat records of photons first .. first + count - 1 of sampler k (sppm_pass.hip), after an eye pass and
// hash of its own for the context's current radii; neither image nor the pixel statistics are touched.
// Returns the records claimed (which may exceed rec_cap); the first min(claimed, rec_cap) are in c->sppm.rec.
template <uint32_t F>
uint32_t sppm_records_t(bling_ctx* c, uint32_t seed, uint32_t pass, uint32_t k, uint32_t first, uint32_t count, uint32_t rec_cap);
// sn of the photon samplers (SPPM.hs:441-453, 474); throws where a pass would hold too many photons
uint32_t sppm_sn(const bling_ctx* c);
void sppm_init(bling_ctx* c);
// One light tracer launch (light_pass.hip): photons first .. first + count - 1 of the pass into the
// device image splat (nullptr = none) and / or the context's record buffer of rec_cap records (0 = off);
// returns the records claimed, which may exceed rec_cap.
template <uint32_t F>
uint32_t light_pass_t(bling_ctx* c, uint32_t seed, uint32_t pass, uint32_t first, uint32_t count, float* splat,
                      uint32_t rec_cap, bling_light_stats* st);
// One wave of the bidirectional integrator (bidir_pass.hip): the n camera samples of the tile table
// (tiles != nullptr, the largest tile of max_tile samples) or of the device list of (x, y, n) triples,
// walked, connected and finished into W.img / W.result (and W.Lfull); terms != nullptr: 3 x 16 floats
// per sample (ld, le, l).  The kernels exist for the cornell profile and for every feature (computed
// textures included: a vertex's BSDF is rebuilt where it is used).  Returns the launches.
int bidir_wave(bling_ctx* c, const WaveState& W, const TileDesc* tiles, unsigned n_tiles, uint32_t max_tile,
               const int32_t* list, uint32_t n, uint32_t seed, uint32_t pass, float* terms);
// One wave of the normal-map integrator (normals_pass.hip): the n camera samples k_raygen / k_raygen_list
// left in W (slot = sample id, the closest queue holding them all), traced with the scene's planned
// closest-hit launch and shaded by k_shade_nm into W.result (and W.Lfull).  tm (may be NULL): event
// pairs around the two launches of a timed pass.  Returns the launches.
int normals_wave(bling_ctx* c, const WaveState& W, uint32_t n, WaveTiming* tm);

}  // namespace bcore
