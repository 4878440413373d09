/*
 * bling.h -- C ABI of the MI355X-native intersection + path-integration core (libbling_hip.so).
 *
 * This is the drop-in seam for bling's per-sample hot path.  The reference has no FFI; its plug-in
 * point is the Renderer class, `render :: a -> RenderJob -> ProgressReporter -> IO ()`
 * (src/lib/Graphics/Bling/Rendering.hs:77-78), whose sampler renderer `prender`
 * (Rendering.hs:111-150) drives Sampling.runSample -> Camera.fireRay -> Integrator.Path.nextVertex
 * (Integrator/Path.hs:41-87) -> Scene.scIntersect/occluded (Scene.hs:45-51) -> KdTree traversal
 * (Primitive/KdTree.hs:210-246) -> Shape/Triangle intersect.  Each entry point below names the
 * reference interface it replaces.  Conventions:
 *   - return 0 on success, a negative BLING_E* code on failure; no C++ exception crosses the ABI;
 *   - host buffers are caller-owned and copied; device memory is owned by the context unless an
 *     entry point says it takes a device pointer;
 *   - a context is used by one host thread at a time; every call blocks until its result is ready.
 */
#ifndef BLING_H
#define BLING_H

#include <stddef.h>
#include <stdint.h>
#include "bling_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BLING_OK           0
#define BLING_EINVAL      -1   /* bad argument                                  */
#define BLING_ENODEV      -2   /* no usable HIP device                          */
#define BLING_EHIP        -3   /* a HIP runtime call failed                     */
#define BLING_ENOSCENE    -4   /* no scene uploaded                             */
#define BLING_EUNSUPPORTED -5  /* scene feature not implemented on the device   */
#define BLING_ENOMEM      -6

#define BLING_MISS 0xFFFFFFFFu

typedef struct bling_ctx bling_ctx;

/* One render pass = every camera sample of the sample extent once (Rendering.hs:127-140).
 * Samples are keyed by (seed, pass_index, pixel, sample, dimension) through the counter RNG that
 * replaces the per-tile MWC streams of Random.hs:56-62 / Rendering.hs:128. */
typedef struct bling_pass_params {
    uint32_t seed;
    uint32_t pass_index;
    int32_t  shard_rank;       /* of the tiles the stride keeps, the m-th (m = k / tile_stride) */
    int32_t  shard_world;      /* is rendered iff m % shard_world == shard_rank; 1 = all of them */
    int32_t  tile_stride;      /* >1: keep only tiles k with k % tile_stride == 0 (sub-sample)  */
    int32_t  chunk_paths;      /* paths in flight per wave (0 = default)                       */
    uint32_t flags;            /* BLING_PASS_* bits                                            */
    void*    tiles_device;     /* BLING_PASS_TILE_IMAGES: device buffer of the pass's tile images */
    uint64_t tiles_capacity;   /* floats tiles_device holds (and, for bling_film_add_*, each rank's
                                  buffer): the core refuses (BLING_EINVAL) a layout that needs more,
                                  so a buffer sized for another shard / stride is never overrun */
} bling_pass_params;

#define BLING_PASS_TRAVERSAL_STATS 1u  /* count node fetches / triangle / shape tests (slower)   */
#define BLING_PASS_KERNEL_TIMING   2u  /* HIP events around every closest-hit launch (roofline)  */
/* Tile images instead of a film (the multi-rank merge): the pass writes each of its
 * tiles' mkImageTile images (Image.hs:108-120) -- slot k = the k-th tile the shard / stride select,
 * in splitWindow order, slot_w x slot_h x 4 floats, zero padded, every slot written whole -- into
 * tiles_device on device_ids[0]; the film argument is ignored (may be NULL).  Single-device
 * contexts only.  bling_pass_tile_layout gives the slot count, size and origins; a rank gathers the
 * others' slots and adds them with bling_film_add_tiles (addTile, Image.hs:178-199). */
#define BLING_PASS_TILE_IMAGES     4u
/* bling_render only: RegionStarted / SamplesAdded reports per sample window before each PassDone */
#define BLING_PASS_REGION_EVENTS   8u
/* Walk every BSDF-MIS ray.  By default a vertex whose sampled light is an area light answers its MIS
 * query itself when the light's own shape rejects the ray (its candidate is then exactly zero,
 * DESIGN.md section 3): same film, same counts, a shorter closest-hit queue.  The switch is for A/B
 * measurements and the tests.  BLING_DEBUG_VERTEX builds never cull (they record every vertex's MIS
 * hit distance, record 29), with or without this bit. */
#define BLING_PASS_NO_MIS_CULL     16u
/* Render the pass as one wave on one stream.  By default a pass whose paths fit one wave and that has
 * at least two tiles runs, for the scene profiles where that measured faster, as
 * two half-waves cut at a tile boundary, each on its own stream, so that one half's shading and the
 * other's traversal share the device.  Every sample's arithmetic is the same either way; only the
 * order of the film's float additions differs.  The switch is for A/B measurements and the tests. */
#define BLING_PASS_NO_PIPELINE     32u
/* The film of the `sampler` renderer in the reference's order, without a float atomic: the same bits on
 * every run, however the pass is cut into waves, and equal to the CPU restatement's.  Every tile's
 * mkImageTile image (Image.hs:108-120) is formed per pixel and channel from +0 by adding the tile's
 * contributing samples one at a time in (iy, ix, n) order -- a = a + w for W, a = a + (v * w) for X, Y, Z,
 * the product rounded first -- whatever the slot order of the pass (addSample, Image.hs:250-299); the film
 * then becomes film = film + tile_k per channel for every selected tile whose image covers the pixel, in
 * ascending tile index, zero values included (addTile, Image.hs:178-199).  The incoming film is the first
 * operand, so accumulated passes stay ordered.  Honoured by bling_render_pass, bling_render_pass_device,
 * bling_render (with BLING_PASS_REGION_EVENTS every SamplesAdded film is ordered too), a
 * BLING_PASS_TILE_IMAGES pass (the slots hold the ordered tile images), bling_film_add_tiles (that
 * shard's tiles in tile order) and bling_film_add_shards (the union of all ranks' tiles in global tile
 * order: the film of a gathered multi-rank pass equals the single-rank ordered film bit for bit).
 * The pass keeps all its tile images until the last wave: n_tiles * slot_w * slot_h * 16 bytes of device
 * memory (bling_pass_tile_layout; the caller's buffer with BLING_PASS_TILE_IMAGES).  Single-device
 * contexts only: a context of several devices refuses the flag with BLING_EINVAL.  The splat renderers
 * have their own switch (BLING_SPLAT_ORDERED). */
#define BLING_PASS_ORDERED_FILM    64u

typedef struct bling_stats {
    uint64_t camera_samples;   /* paths started                                               */
    uint64_t rays_camera;      /* closest-hit queries of camera rays                          */
    uint64_t rays_continuation;/* closest-hit queries of BSDF-sampled continuation rays        */
    uint64_t rays_mis;         /* closest-hit queries of BSDF-sampled MIS rays (Scene.hs:71-82)  */
    uint64_t rays_shadow;      /* any-hit queries of light-sample shadow rays (Scene.hs:45-47)  */
    uint64_t dropped_samples;  /* NaN / Inf samples skipped by addSample (Image.hs:253-256)     */
    uint64_t tiles;            /* tiles rendered by this call                                  */
    double   ms_total;         /* device wall time of the pass (HIP events)                    */
    double   ms_bounce;        /* path-vertex pipeline time (HIP events on the core's stream)   */
    double   ms_film;          /* film splat + merge                                           */
    uint64_t bounce_launches;  /* number of path-vertex pipeline launches                      */
    uint64_t path_vertices;    /* alive paths entering a bounce launch, summed                 */
    uint64_t node_visits;      /* BVH2 nodes fetched (64 B each)                               */
    uint64_t tri_tests;        /* triangle tests (48 B records)                                */
    uint64_t shape_tests;      /* instanced shape / fractal tests                              */
    /* ms_closest and ms_shade are sums over launches of each launch's own elapsed time.  In a
       pipelined pass (see BLING_PASS_NO_PIPELINE) the two half-waves' launches overlap, so the sums
       count shared time twice and no longer add up to ms_bounce; ms_total is the yardstick.  In such
       a pass ms_bounce runs from the halves' start to the end of the later one, which includes the
       first half's film (it runs beside the second half's last launches), and ms_film is the second
       half's film alone. */
    double   ms_closest;       /* BLING_PASS_KERNEL_TIMING: summed k_trace_closest launch times */
    uint64_t closest_launches; /* BLING_PASS_KERNEL_TIMING: k_trace_closest launches timed      */
    uint64_t march_ticks;      /* BLING_PASS_TRAVERSAL_STATS: Mandelbulb march iterations (one
                                  bulbPower each, Fractal.hs:90-137)                            */
    /* BLING_PASS_TRAVERSAL_STATS, closest-hit queries only (the four counts above include the
       shadow rays' any-hit traversals): the work basis of the closest-hit kernel's roofline */
    uint64_t closest_node_visits, closest_tri_tests, closest_shape_tests, closest_march_ticks;
    double   ms_shade;         /* BLING_PASS_KERNEL_TIMING: summed launch times of the shading
                                  kernel: depth 0 and the fused resolve + shade launches      */
    uint64_t shade_launches;   /* BLING_PASS_KERNEL_TIMING: shade launches timed                */
} bling_stats;

/* Replaces: the process-wide GHC RTS + spark pool (bling.cabal:98-103, Rendering.hs:118).
 * device_ids: n_devices HIP device ordinals (NULL / 0 = device 0).  With n_devices > 1 the context
 * fans every bling_render_pass[_device] out over all of them: the scene is
 * replicated at upload, each device renders an interleaved share of the pass's tiles concurrently
 * as tile images (BLING_PASS_TILE_IMAGES), every peer pushes its images over xGMI onto
 * device_ids[0] (concurrent copies, one per peer stream), and they are added there (addTile) once
 * every device has succeeded, before the call returns.  bling_trace, bling_sample_li and the SPPM
 * calls run on device_ids[0] only (the light tracer refuses such a context).  One process per GPU
 * (torch.distributed / RCCL) instead passes one id per process and uses the shard fields.  A device id listed twice is BLING_EINVAL (unless
 * the environment sets BLING_ALLOW_REPEATED_DEVICES=1, a test hook that runs the fan-out with two
 * contexts on one GPU). */
int bling_create(const int* device_ids, int n_devices, bling_ctx** out);

/* Replaces: Scene.mkScene -> KdTree.mkKdTree (Scene.hs:37-43, KdTree.hs:107-139).  Builds a binned
 * SAH BVH2 on the host, flattens triangles/shapes/materials/lights to SoA and uploads them. */
int bling_scene_upload(bling_ctx* ctx, const bling_scene_desc* desc);

/* The same upload with a choice of BVH builder.  BLING_BVH_HOST is bling_scene_upload: the binned SAH on one
 * host thread.  BLING_BVH_DEVICE builds a linear BVH on device_ids[0] (csrc/common/lbvh.h: Morton keys, an LDS
 * radix sort, the common-prefix hierarchy, bottom-up bounds, leaves of one or two items) in the very node and
 * leaf format of the host tree; the BVH2 and its refs come back to the host once, and the BVH4, the threaded
 * list, the LDS plans and the leaf records are derived from it as from the host tree.  The tree depends on the
 * items only: the same bits on every run, equal to bling_host_lbvh (bling_host.h).  Peers of a multi-device
 * context receive the arrays built on the first device.
 * The device builder stands down -- the upload succeeds with the host tree, and bling_debug_bvh_build_info
 * names the reason -- for a fractal scene, for fewer than three items, for a tree deeper than the traversal
 * stack allows (31) and for more than 2^24 items.  A bvh_builder other than the two is BLING_EINVAL.
 *
 * flags: 0, or BLING_UPLOAD_DERIVE_DEVICE; any other bit is BLING_EINVAL.  With the bit, what follows the BVH2 is
 * derived on device_ids[0] (csrc/common/bvh4.h, csrc/core/bvh_derive.hip): the leaf records by a gather, the BVH4
 * level by level.  Each array is bit for bit the host derivation's of the same BVH2.  A host-built tree is
 * uploaded once and a device-built one never leaves the device: only counts come back, and the LDS plans are
 * settled from them on the host.  The threaded list is the one exception: it is walked only when it has at most
 * 16 entries, so a BVH2 of more than 16 nodes gets none (pkt_n = 0, as on the host path), and a smaller one (at
 * most 1 KiB) is read back and threaded on the host.
 * The device derivation stands down -- the upload succeeds with the host derivation, and
 * bling_debug_derive_info names the reason -- for a fractal scene, for a context of several devices (the peers
 * receive the host's plan) and for a BVH2 without nodes. */
#define BLING_BVH_HOST   0u
#define BLING_BVH_DEVICE 1u
#define BLING_UPLOAD_DERIVE_DEVICE 1u
typedef struct bling_upload_params {
  uint32_t bvh_builder;     /* BLING_BVH_* */
  uint32_t flags;           /* 0 or BLING_UPLOAD_DERIVE_DEVICE */
} bling_upload_params;
int bling_scene_upload_with(bling_ctx* ctx, const bling_scene_desc* desc, const bling_upload_params* params);

/* The checks bling_scene_upload makes of a scene description before any device work (render
 * config, texture graphs, host-folded material spectra, lights, images), without a context or a
 * device: the parser's error path (parseJob, IO/RenderJob.hs:31-34, and the `fail` paths of
 * IO/ParserCore.hs:147-186, fail at parse time) for a description built
 * elsewhere.  BLING_OK or BLING_EINVAL with bling_last_error() set. */
int bling_scene_validate(const bling_scene_desc* desc);

/* Replaces: prender's onePass (Rendering.hs:127-140) for the `sampler` renderer with its `path`
 * (Integrator/Path.hs), `directLighting` (Integrator/DirectLighting.hs), `bidir`
 * (Integrator/BidirPath.hs) or `debug normals` (Integrator/Debug.hs:25-34) surface integrator, selected
 * by desc->config.integrator at upload
 * (directLighting and bidir maxDepth must lie in [1, 16]; else BLING_EINVAL with the reason).  A normal-map
 * pass traces the camera rays once and adds rgbToSpectrumRefl ((1 + n) / 2) of the hit's shading normal
 * (black on a miss, no environment term); BLING_PASS_TRAVERSAL_STATS leaves its traversal counters at 0.  A bidir
 * pass keeps 2 maxDepth vertex records per sample in flight and is cut into more waves accordingly;
 * its ray counts are mapped as bling_sample_li describes.
 * film_out: host buffer of width*height*4 floats (W, X, Y, Z per pixel, Image.hs:64-71),
 * ACCUMULATED into (pass several passes to get the progressive sum); may be NULL.  On a multi-device
 * context the film holds the sum over all devices; stats sum the counts (times: the slowest device,
 * ms_total = host wall time of the whole fan-out including the film merge). */
int bling_render_pass(bling_ctx* ctx, const bling_pass_params* p, float* film_out,
                      bling_stats* stats);

/* Replaces: prender's whole progressive loop with its ProgressReporter (Rendering.hs:60-78, 111-140):
 * passes p->pass_index, p->pass_index + 1, ... each accumulated into film_out (host, width*height*4,
 * as bling_render_pass; may be NULL), and after each one report(user, &ev) with ev.kind =
 * BLING_PROGRESS_PASS_DONE, the pass number, the accumulated film (finalImg) and splat weight 1
 * (`PassDone pass img' 1`); the loop stops when report returns 0 (`if cont then onePass (pass + 1)`).
 * With BLING_PASS_REGION_EVENTS in p->flags, each PassDone is preceded by prender's per-tile
 * reports (`RegionStarted w`, then `SamplesAdded w img'`, Rendering.hs:130-134) for every sample
 * window of the pass in tile order; their return values are ignored, as the reference ignores them.
 * The device renders the pass as a whole into its tile images; with a host film on a single-device
 * context they come back to the host and are added one window after another (addTile in the
 * reference's window order), so every SamplesAdded carries the film up to and including its window,
 * as the reference's does.  On a multi-device context (or with film_out NULL) the reports follow the
 * pass and carry the film after the whole pass.  stats (may be NULL)
 * sums the counts of every pass and takes the times' sum.  report must not be NULL (the reference
 * always has a reporter). */
typedef struct bling_progress {
    int32_t      kind;         /* BLING_PROGRESS_* (the constructors of Progress, Rendering.hs:60-73) */
    int32_t      pass;         /* progPassNum (every kind: the pass the event belongs to)        */
    const float* film;         /* finalImg / SamplesAdded's image: film_out after this pass, or (single
                                  device) up to this window; NULL if film_out is NULL or for
                                  RegionStarted                                                   */
    float        splat_weight; /* splatWeight (1)                                                */
    const struct bling_stats* pass_stats;   /* PassDone: this pass's counters and times (not the running
                                               sum); NULL otherwise                                */
    int32_t      region[4];    /* RegionStarted / SamplesAdded: the SampleWindow x0, x1, y0, y1 (inclusive) */
} bling_progress;
#define BLING_PROGRESS_STARTED        0
#define BLING_PROGRESS_SAMPLES_ADDED  1
#define BLING_PROGRESS_REGION_STARTED 2
#define BLING_PROGRESS_PASS_DONE      3
typedef int (*bling_progress_fn)(void* user, const bling_progress* ev);
int bling_render(bling_ctx* ctx, const bling_pass_params* p, float* film_out, bling_progress_fn report, void* user,
                 bling_stats* stats);

/* Same as bling_render_pass, but accumulates into a DEVICE film buffer (width*height*4 floats on
 * device_ids[0]) that the caller owns -- e.g. a tensor later reduced over RCCL. */
int bling_render_pass_device(bling_ctx* ctx, const bling_pass_params* p, void* film_device,
                             bling_stats* stats);

/* The tile-image layout of a pass (BLING_PASS_TILE_IMAGES) with p's shard and stride: *n_tiles
 * slots of *slot_w x *slot_h x 4 floats (15 + floor(0.5 + filter width) square for the square
 * filters); origins_out (2 ints per slot: the tile image's film x, y) may be NULL. */
int bling_pass_tile_layout(bling_ctx* ctx, const bling_pass_params* p, int32_t* origins_out, size_t* n_tiles,
                           int32_t* slot_w, int32_t* slot_h);

/* addTile (Image.hs:178-199) of the tile images of p's shard / stride (tiles_device, written by a
 * BLING_PASS_TILE_IMAGES pass of that shard, possibly on another rank) into film_device (width *
 * height * 4 floats), both device buffers on device_ids[0]. */
int bling_film_add_tiles(bling_ctx* ctx, const bling_pass_params* p, const void* tiles_device, void* film_device);

/* The same for every rank of a multi-rank pass at once (the merge after the gather): tiles_devices
 * holds p->shard_world device pointers, rank r's tile images (shard (r, shard_world), p's stride);
 * one launch adds them all into film_device. */
int bling_film_add_shards(bling_ctx* ctx, const bling_pass_params* p, const void* const* tiles_devices,
                          void* film_device);

/* Replaces: getPixel + xyzToRgb (Image.hs:302-315), rgbPixels (Image.hs:317-331) and the pixel loop of
 * writeRgbe (IO/Bitmap.hs:36-41) -- the develop step of progressWriter's PassDone and of the GUI's
 * SamplesAdded -- for a film that lives on the device.  film: width*height*4 floats (W, X, Y, Z);
 * splat: width*height*3 floats (XYZ) or NULL (= all zero); the pixel's XYZ is splat_weight * splat
 * (+ film XYZ / W where W != 0).  Width and height are the uploaded scene's.  out is a whole-image
 * buffer in one of three formats, row-major from the top:
 *   BLING_DEVELOP_RGB_F32  width*height*3 floats, bit for bit bling_host_film_splat_to_rgb (a NaN is
 *                          a NaN, of whatever payload);
 *   BLING_DEVELOP_RGB8     width*height*3 bytes, byte for byte bling_host_rgb_pixels_splat: gamma 2.2,
 *                          clamp, round half to even, looked up in the host library's table of 255
 *                          thresholds (bling_host_gamma_thresholds) rather than computed with a device
 *                          pow; NaN, finite negatives and +-0 give 0, +Inf gives 255 and so does
 *                          -Inf (powf (-Inf) (1 / 2.2) is +Inf), which the lookup takes as +Inf;
 *   BLING_DEVELOP_RGBE     width*height*4 bytes, the bytes bling_host_write_hdr puts after its header
 *                          for that RGB image (a mantissa that rounds to 256 and the exponent byte of
 *                          m >= 2^127 wrap to 0, as the host's do).  A pixel with a +Inf channel is
 *                          outside that contract (the host's frexp exponent is unspecified there):
 *                          the device writes 0, 0, 0, 1.
 * window = x0, x1, y0, y1, inclusive, clipped to the image (as rgbPixels filters coverWindow): only its
 * pixels are written and the rest of out stays as it was, so one buffer serves as a preview updated
 * per SamplesAdded window; a window wholly outside the image (or x1 < x0, y1 < y0) writes nothing.
 * Errors: BLING_ENOSCENE without a scene; BLING_EINVAL for a format other than the three, a NULL
 * params / film / out, or an out that overlaps film or splat.  On a multi-device context the call runs
 * on device_ids[0], where every film merge lands.  Both calls run on the context's stream and return
 * after completion.
 * bling_film_develop_device: film, splat and out are device buffers on device_ids[0], e.g. the film
 * of bling_render_pass_device; nothing crosses to the host.
 * bling_film_develop: film, splat and out are host buffers; film and splat are staged through device
 * buffers the context owns (allocated once, reused) and only the developed rows come back: 3 or 4
 * bytes per pixel for the byte formats instead of the film's 16. */
#define BLING_DEVELOP_RGB_F32 0
#define BLING_DEVELOP_RGB8    1
#define BLING_DEVELOP_RGBE    2
typedef struct bling_develop_params {
    int32_t format;            /* BLING_DEVELOP_*                                               */
    float   splat_weight;
    int32_t window[4];         /* x0, x1, y0, y1, inclusive                                     */
} bling_develop_params;
int bling_film_develop_device(bling_ctx* ctx, const bling_develop_params* p, const void* film_dev,
                              const void* splat_dev, void* out_dev);
int bling_film_develop(bling_ctx* ctx, const bling_develop_params* p, const float* film_host,
                       const float* splat_host, void* out_host);

/* Replaces: Scene.scIntersect / Scene.occluded for a batch (Scene.hs:45-51 -> KdTree.hs:236-246).
 * rays_soa: 8 planes of n floats (ox, oy, oz, dx, dy, dz, tmin, tmax).
 * closest (any_hit=0): t_out[n], prim_out[n] (index into desc->prim_kind order, BLING_MISS on
 * miss), bary_out[2n] (triangle b1,b2 / shape u,v); any_hit=1: prim_out[i] = 1 if occluded else 0
 * (t_out, bary_out may be NULL).  Host buffers. */
int bling_trace(bling_ctx* ctx, const float* rays_soa, size_t n, int any_hit,
                float* t_out, uint32_t* prim_out, float* bary_out);

/* Device-pointer variant of bling_trace for benchmarks (no host copies); timing via ms_out. */
int bling_trace_device(bling_ctx* ctx, const void* rays_soa_dev, size_t n, int any_hit,
                       void* t_dev, void* prim_dev, void* bary_dev, int repeats, double* ms_out);

/* Parity hook: radiance of individual camera samples, the uploaded scene's surface integrator
 * (Path.li, Integrator/Path.hs:38-39; DirectLighting; BidirPath's contrib, BidirPath.hs:50-96) for
 * sample n of extent pixel (x, y) after Camera.fireRay.  samples: 3 ints (x, y, n) per sample;
 * L_out: 16 floats per sample (the spectrum before addSample's NaN filter); img_out: 2 floats per
 * sample (imageX, imageY), may be NULL.  Host buffers.  stats (may be NULL) receives the ray counts;
 * for the bidirectional integrator: rays_camera = camera samples traced, rays_continuation = the
 * closest-hit queries of both subpaths' segments (the light ray included), rays_mis = estimateDirect's
 * BSDF-MIS rays, rays_shadow = its shadow rays plus the connections' occluded queries,
 * path_vertices = the vertices of both subpaths; for the normal-map integrator: rays_camera = the
 * samples, path_vertices = the samples whose camera ray hit, every other ray count 0. */
int bling_sample_li(bling_ctx* ctx, uint32_t seed, uint32_t pass_index, const int32_t* samples, size_t n,
                    float* L_out, float* img_out, bling_stats* stats);

/* Parity hook of the bidirectional integrator (BLING_INTEGRATOR_BIDIR scenes, else BLING_EINVAL): the
 * terms of contrib (BidirPath.hs:70-96) for the same samples as bling_sample_li.  terms_out: 3 x 16
 * floats per sample -- ld (the weighted direct terms), le, l (the connections; zero where a subpath is
 * empty, the case in which contrib leaves it out); lens_out: 4 ints per sample -- eye subpath
 * length, light subpath length, and the two masks whose bit i says that vertex i's sampled lobe was
 * specular.  A parity mismatch so names its term. */
int bling_debug_bidir_terms(bling_ctx* ctx, uint32_t seed, uint32_t pass_index, const int32_t* samples, size_t n,
                            float* terms_out, int32_t* lens_out);

/* Debug hook (parity diagnosis): bling_sample_li plus one record of BLING_DV_FIELDS floats per path
 * vertex (vertex d of sample k at vtx_out[(k * BLING_DV_DEPTHS + d) * BLING_DV_FIELDS]; NaN where a
 * vertex or field was not reached).  The oracle's oracle_sample_li_vertices writes the same fields,
 * so the first field where the two differ names the first operation that diverges.  Only a build
 * with BLING_DEBUG_VERTEX (`make variant V=dbg DEFS=-DBLING_DEBUG_VERTEX=1`) records; the product
 * library returns BLING_EUNSUPPORTED.  Path integrator only.  Fields, in the vertex's order:
 *   0-2 ray origin, 3-5 ray direction, 6 hit t (Path.hs:41, scIntersect)
 *   7-9 shading point p, 10-12 geometric normal, 13 ray epsilon (mkIntersection, DG)
 *   14-16 light-sample wi, 17 its pdf (Light.sample, Scene.hs:61-69)
 *   18-20 BSDF-MIS wi, 21 its pdf (sampleBsdf, Scene.hs:71-82)
 *   22-24 continuation wi, 25 its pdf (Path.hs:74-79)
 *   26 Russian-roulette pc, 27 its uniform (Path.hs:68-72)
 *   28 shadow ray occluded (1 / 0), 29 BSDF-MIS ray hit t (inf = miss)
 *   30 sum of the vertex's 16-band radiance term, 31 sum of L after the vertex (Path.hs:73-79) */
#define BLING_DV_DEPTHS 16
#define BLING_DV_FIELDS 32
int bling_sample_li_vertices(bling_ctx* ctx, uint32_t seed, uint32_t pass_index, const int32_t* samples, size_t n,
                             float* L_out, float* vtx_out);

/* ---- SPPM renderer (Renderer/SPPM.hs), the second consumer of the trace core ---- */
typedef struct bling_sppm_stats {
    uint64_t hitpoints;        /* hit points recorded by the eye pass (mkHitPoints)              */
    uint64_t photons;          /* photons emitted: sppm_threads * sn^2 (SPPM.hs:449, 474)         */
    uint64_t photon_rays;      /* closest-hit queries of photon segments (followPhoton)           */
    uint64_t photon_hits;      /* (photon hit, hit point) pairs within the hit point's radius      */
    uint64_t cam_rays;         /* closest-hit queries of eye rays (traceCam)                      */
    uint64_t dropped;          /* NaN / Inf eye samples and splats skipped                        */
    double   ms_total, ms_eye, ms_hash, ms_photon;   /* device time (HIP events)                  */
} bling_sppm_stats;

/* Replaces: SPPM's onePass (Renderer/SPPM.hs:424-460) for a scene whose renderer block is
 * `sppm photonCount maxDepth radius [alpha]` (maxDepth in [1, 16]): one random camera sample per
 * sample-extent pixel builds the hit points (their Ls is addSample'd into film_out, W*H*4), then
 * sppm_threads * sn^2 photons splat into splat_out (W*H*3 XYZ, splatSample); both host buffers are
 * ACCUMULATED into and may be NULL.  The per-pixel radius statistics (psR2, psN) live in the
 * context and carry over to the next pass; pass_index numbers passes from 1 like onePass.  The
 * reference's image of pass k is getPixel with splat weight 1 / (threads * k * sn^2) (:460). */
int bling_sppm_pass(bling_ctx* ctx, uint32_t seed, uint32_t pass_index, float* film_out, float* splat_out,
                    bling_sppm_stats* stats);

/* bling_sppm_pass with both images in caller-owned device buffers: film_device
 * holds W*H*4 floats (W, X, Y, Z) and splat_device W*H*3 floats (XYZ), both on device_ids[0] (e.g. torch
 * tensors' data_ptr()); they are ACCUMULATED into and never copied to the host, and feed
 * bling_film_develop_device directly.  Either may be NULL: that image is then not produced.  The pixel
 * statistics stay in the context.  The call runs on the context's stream and returns after completion.
 *   flags == 0: bling_sppm_pass's kernels and float atomics -- the same arithmetic, counters and statistics,
 *     images that differ from its only in the order of their binary32 sums -- without the host staging.
 *   BLING_SPLAT_ORDERED (below): no float atomic anywhere in the pass; both images are formed in the
 *     reference's order (SPPM.hs:133-164, 424-460) and are the same on every run, whatever the launch
 *     geometry, chunking or timing.
 *     Film: each 16 x 16 extent tile's image starts at zero and receives the addSample of its pixels' eye
 *     samples in (iy, ix) order; the tile images are then added into the film in tile order, film = film + tile
 *     per channel.
 *     Splats: each of the sppm_threads samplers k builds its own image from zero, adding its splats one at a
 *     time by (photon n, then the order in which the photon's walk meets (vertex, hit point) pairs: depth,
 *     then treeLookup's order); the samplers' images are then added in k order, splat = splat + image_k.  A
 *     two-level sum: a flat fold over all the splats of a pixel gives other bits.
 *     The statistics, the pixel statistics and the hit points equal the atomic mode's exactly.
 *     A sampler's splats go through the record buffer of the ordered light tracer (its budget,
 *     bling_debug_set_splat_budget): ascending photon ranges are merged one after another, a range whose
 *     records exceed the budget is halved and run again (its rays, pairs and per-pixel counts are taken over
 *     only once it fits), and a single photon that alone exceeds it is BLING_EINVAL (the film, the splats of
 *     the samplers before it and the pixel statistics of no pass are then in an unspecified state: call
 *     bling_sppm_reset).
 * Errors: those of bling_sppm_pass; BLING_EINVAL for unknown flag bits and for a context of several devices. */
int bling_sppm_pass_device(bling_ctx* ctx, uint32_t seed, uint32_t pass_index, uint32_t flags, void* film_device,
                           void* splat_device, bling_sppm_stats* stats);

/* Parity hook: the splats of photons first_photon .. first_photon + n_photons - 1 of sampler `thread` of
 * that pass, one record per splat, sorted by (photon, seq); seq is the running index of the photon's
 * (vertex, hit point) pairs, counting every pair (also those whose splat falls outside the image or is
 * dropped), depth the vertex (0 = first hit).  The call performs an eye pass and builds the hash ITSELF,
 * for the context's CURRENT radii: to see a pass's records, call it before that pass (a pass updates the
 * radii).  Nothing is accumulated into any image and the pixel statistics are not updated; the hit points
 * and buckets of the diagnostics below become this call's.  *n receives the number of records; a capacity
 * smaller than *n is BLING_EINVAL (with *n set): never a silent truncation. */
typedef struct bling_sppm_record {
    uint32_t thread, photon, seq, depth;
    int32_t  sx, sy;           /* pixel (floor of the hit point's raster position)                */
    float    x, y, z;          /* the XYZ the splat adds                                          */
    uint32_t pad;
} bling_sppm_record;
int bling_debug_sppm_records(bling_ctx* ctx, uint32_t seed, uint32_t pass_index, uint32_t thread, uint32_t first_photon,
                             uint32_t n_photons, bling_sppm_record* records, size_t cap, size_t* n);

/* The per-pixel statistics (PixelStats psR2 / psN, SPPM.hs:245-257) over the sample extent, in
 * sIdx order (windowPixels entries, written to *n_pixels); r2_out / n_out may be NULL. */
int bling_sppm_pixel_stats(bling_ctx* ctx, float* r2_out, float* n_out, size_t* n_pixels);

/* Restarts the SPPM statistics (every radius back to the scene's initial radius). */
int bling_sppm_reset(bling_ctx* ctx);

/* Diagnostics: the hit points of the last SPPM pass, in the device's (arbitrary) order -- shading
 * point and radius^2 (4 floats each) and the key pixel << 24 | eye-tree node id that orders the
 * kd-trees' ties.  *n receives the count; at most cap are copied (either array may be NULL). */
int bling_debug_sppm_hitpoints(bling_ctx* ctx, float* pos_r2, uint64_t* keys, size_t cap, size_t* n);
/* Diagnostics: the last SPPM pass's hash buckets as its kd-trees laid them out (k_sppm_kd): bucket
 * offsets (*nb = buckets + 1), hit point indices per bucket in kd order, and per entry the node's
 * mr at pivot positions (*ni entries).  Arrays are copied only when their capacity suffices. */
int bling_debug_sppm_buckets(bling_ctx* ctx, uint32_t* bstart, uint32_t* items, float* mr, size_t cap_b,
                             size_t cap_i, size_t* nb, size_t* ni);

/* ---- light tracer (Renderer/LightTracer.hs), the third consumer of the trace core ---- */
typedef struct bling_light_stats {
    uint64_t photons;          /* photons emitted: passPhotons                                   */
    uint64_t photon_rays;      /* closest-hit queries of photon segments (oneRay / nextVertex)    */
    uint64_t shadow_rays;      /* any-hit queries of camera connections (connectCam's occluded)   */
    uint64_t splats;           /* connections handed to splatSample inside the image, finite      */
    uint64_t dropped;          /* NaN / Inf connections inside the image, skipped (Image.hs:201-221) */
    double   ms_total;         /* device time of the pass (HIP events)                           */
} bling_light_stats;

/* Replaces: one pass of `instance Renderer LightTracer` (Renderer/LightTracer.hs:37-52) for a scene
 * whose renderer block is `light passPhotons N`: N photons leave the lights (oneRay, :54-66), and
 * every vertex of a photon's walk (nextVertex, :84-109; no depth limit, Russian roulette with 0.8
 * beyond depth 3) is connected to the pinhole of the perspective camera (connectCam, :68-82;
 * sampleCam, Camera.hs:90-100) and splatted (splatSample) into splat_inout: W*H*3 XYZ, host,
 * ACCUMULATED into, may be NULL.  pass_index numbers passes from 1.  The reference's image after
 * pass k is getPixel of an empty film with splat weight sw = 1 / (k * passPhotons) (:50).
 * As in the reference, a vertex behind the camera is projected and splatted all the same, the lens
 * radius is ignored, and the emitter itself and specular chains seen from the eye never appear
 * (traps).  Errors: BLING_ENOSCENE without a scene; BLING_EINVAL when the scene's
 * renderer is not the light tracer or the context holds several devices; BLING_EUNSUPPORTED for an
 * environment camera (sampleCam is `error` there) and for computed textures (as bling_sppm_pass). */
int bling_light_pass(bling_ctx* ctx, uint32_t seed, uint32_t pass_index, float* splat_inout,
                     bling_light_stats* stats);

/* Parity hook: the splats of photons first_photon .. first_photon + n_photons - 1 of that pass, one
 * record per splat, sorted by (photon, depth); nothing is accumulated.  The film's float atomics
 * make its sums order-dependent; the records are what parity is pinned on.  *n receives the number
 * of records the photons produced; at most cap are written.  A capacity smaller than *n is
 * BLING_EINVAL (with *n set, so the caller can size the buffer): never a silent truncation. */
typedef struct bling_light_record {
    uint32_t photon, depth;    /* photon index of the pass, vertex depth (0 = first hit)          */
    int32_t  sx, sy;           /* pixel (floor of the raster position)                            */
    float    x, y, z;          /* the XYZ the splat adds                                          */
    uint32_t pad;
} bling_light_record;
int bling_debug_light_records(bling_ctx* ctx, uint32_t seed, uint32_t pass_index, uint32_t first_photon,
                              uint32_t n_photons, bling_light_record* records, size_t cap, size_t* n);

/* ---- Metropolis renderer (Renderer/Metropolis.hs) over the bidirectional integrator ---- */
typedef struct bling_mlt_stats {
    double   b;                /* this pass's b' = sum I / bootstrap (a binary32 value)           */
    uint64_t mutations;        /* M = floor (mpp * nPixels), over all chains                      */
    uint64_t large_steps;      /* mutations whose large-step draw was < plarge                    */
    uint64_t accepted;
    uint64_t splats;           /* splats inside the image, finite                                 */
    uint64_t dropped;          /* NaN / Inf splats inside the image, skipped (Image.hs:201-221)   */
    uint64_t rays_camera, rays_continuation, rays_mis, rays_shadow, path_vertices;   /* as bling_stats,
                                  over the bootstrap samples, the chains' first evaluation and the
                                  mutations                                                        */
    double   ms_total;         /* device time of the pass (HIP events)                           */
} bling_mlt_stats;

/* Replaces: one pass of `instance Renderer Metropolis` (Renderer/Metropolis.hs:76-120) for a scene
 * whose renderer block is `metropolis maxDepth N mpp F bootstrap N plarge F directSamples 0`:
 * the bootstrap (:142-169), then M = floor (mpp * nPixels) mutations over `chains` independent chains
 * (chain c does M div C, plus one if c < M mod C; chains = 1 is the reference's one chain), each
 * splatting the current and the proposed sample (:96-104) into splat_inout: W*H*3 XYZ, host,
 * ACCUMULATED into, may be NULL.  pass_index numbers passes from 1.  The reference's image after pass
 * p is getPixel of an empty film with splat weight bnext / p, bnext = lerp (1 / p) b b' from b = 1
 * (:115-117); stats->b is this pass's b'.  Errors: BLING_ENOSCENE without a scene; BLING_EINVAL when
 * the scene's renderer is not this one, the context holds several devices, or the bootstrap selection
 * lands where the reference stops with an error (a slot a NaN bootstrap sample left unwritten). */
int bling_mlt_pass(bling_ctx* ctx, uint32_t seed, uint32_t pass_index, float* splat_inout, bling_mlt_stats* stats);

/* Parity hook: one record per (chain, mutation) of chains first_chain .. first_chain + n_chains - 1 of
 * that pass, sorted by that pair; nothing is accumulated.  starts (may be NULL) receives n_chains
 * bootstrap sample indices, the chains' start samples; *b (may be NULL) the pass's b'.  *n receives the
 * number of records; a capacity smaller than *n is BLING_EINVAL (with *n set). */
typedef struct bling_mlt_record {
    uint32_t chain, mutation;
    float    x, y;             /* the proposal's imageX, imageY                                   */
    float    i_prop, a;        /* evalI of the proposal, min 1 (iProp / iCurr) (NaN where GHC's is) */
    uint32_t flags;            /* bit 0: large step, bit 1: accepted                              */
    uint32_t pad;
} bling_mlt_record;
int bling_debug_mlt_records(bling_ctx* ctx, uint32_t seed, uint32_t pass_index, uint32_t first_chain, uint32_t n_chains,
                            bling_mlt_record* records, size_t cap, size_t* n, uint32_t* starts, float* b);

/* Probe of the pass's host bookkeeping (bootstrap, Metropolis.hs:150-167), without a context or a device:
 * from n bootstrap contributions I it forms *b = sum I / n (a NaN counts 0) and every chain's start sample
 * (starts: `chains` bootstrap sample indices), with the pass's own keys.  BLING_EINVAL, with the reason,
 * where a chain's selection reads a slot that a NaN sample left unwritten. */
int bling_debug_mlt_boot(const float* I, uint32_t n, uint32_t seed, uint32_t pass_index, uint32_t chains, float* b,
                         uint32_t* starts);
/* Test hook: the following bling_mlt_pass / bling_debug_mlt_records calls of this context take these n
 * values for the bootstrap contributions when n equals the scene's bootstrap (the samples are still
 * evaluated); n = 0 or a scene upload ends it. */
int bling_debug_mlt_set_boot(bling_ctx* ctx, const float* I, uint32_t n);

/* ---- splat images on the device, and ordered splat films ----
 * bling_light_pass_device / bling_mlt_pass_device are bling_light_pass / bling_mlt_pass with the splat
 * image in a caller-owned device buffer: splat_device holds W*H*3 floats (XYZ) on device_ids[0] (e.g. a
 * torch tensor's data_ptr()), is ACCUMULATED into and never copied to the host; it must not be NULL and
 * feeds bling_film_develop_device directly as splat_dev.  The calls run on the context's stream and return
 * after completion; the context's own splat image is not touched.
 *   flags == 0: the splats are added with float atomics, as in the host-buffer calls: the same arithmetic,
 *     counters and records, and an image that differs from theirs only in the order of its binary32 sums.
 *   BLING_SPLAT_ORDERED: every pixel's new value is its old value plus that pixel's splats of this pass,
 *     added one at a time in binary32 in the reference's order -- the light tracer's by (photon, depth)
 *     (replicateM_ ppp oneRay into one image, LightTracer.hs:41-50), Metropolis' by (chain, mutation, the
 *     current sample before the proposal) (Metropolis.hs:96-104).  No float atomic is used.  The image is
 *     the same on every run, whatever the launch geometry, chunking or timing, and equals the CPU
 *     restatements' binary32 images bit for bit; the stats equal the atomic mode's.
 *     The splats go through a record buffer of at most `budget` records (default: a sixteenth of the
 *     device's memory at 56 bytes a record, between 2^16 and 2^27 records).  The light tracer merges
 *     ascending photon ranges one after another and halves a range whose records exceed the budget; a single
 *     photon that alone exceeds it is BLING_EINVAL (the image then holds the ranges before it).  Metropolis
 *     merges once a pass: 2 M records (M = mutations) beyond the budget are refused with BLING_EINVAL
 *     before any launch, the image untouched.
 * Errors: those of bling_light_pass / bling_mlt_pass, and BLING_EINVAL for unknown flag bits or a NULL
 * splat_device.  SPPM's film and splat image are served by bling_sppm_pass_device (above), whose ordered
 * sum has two levels. */
#define BLING_SPLAT_ORDERED 1u
int bling_light_pass_device(bling_ctx* ctx, uint32_t seed, uint32_t pass_index, uint32_t flags, void* splat_device,
                            bling_light_stats* stats);
int bling_mlt_pass_device(bling_ctx* ctx, uint32_t seed, uint32_t pass_index, uint32_t flags, void* splat_device,
                          bling_mlt_stats* stats);

/* Test hook: the ordered merge alone.  n host records in any order are merged into splat_device (W*H*3
 * floats on device_ids[0]): for every pixel with records, img = (((img + r0) + r1) + ...) per channel in
 * binary32, its records in ascending key order; other pixels stay as they are.  Records with equal keys
 * merge in any order among themselves.  Needs an uploaded scene for W and H only; BLING_EINVAL for a pixel
 * index beyond W*H. */
typedef struct bling_splat_rec {
    uint32_t pixel;            /* y * W + x                                                       */
    uint32_t pad;
    uint64_t key;              /* the order within the pixel                                      */
    float    x, y, z;          /* the XYZ the splat adds                                          */
    uint32_t pad2;
} bling_splat_rec;
int bling_debug_splat_merge(bling_ctx* ctx, const bling_splat_rec* recs, size_t n, void* splat_device);
/* Test hook: the record budget of this context's ordered passes; 0 restores the default. */
int bling_debug_set_splat_budget(bling_ctx* ctx, size_t max_records);
/* Diagnostics: device time of the context's last ordered pass, split into its photon / chain launches and
 * its merges (their sum is the pass's ms_total). */
int bling_debug_splat_times(bling_ctx* ctx, double* ms_kernel, double* ms_merge);

/* ---- the image API on the device: caller samples onto a film, in order ----
 * Replaces: the image monad of Image.hs -- addSample', addUnfilteredSample', splatSample and execImageT
 * (Image.hs:201-299, 333-370) -- for samples the CALLER computed: what the reference's live command line
 * does (imageFilters, src/cmdline/Examples.hs) and what a host-side Renderer instance uses to put its own
 * samples on a device film.  These calls need NO uploaded scene and leave an uploaded one untouched (SPPM,
 * light tracer and Metropolis state included); width, height and filter come from the desc.  They run on
 * device_ids[0], on the context's stream, and return after completion.
 *   xy: 2 floats per sample (imageX, imageY); spectra: 16 floats per sample; n samples.
 *   target: width*height*4 floats (W, X, Y, Z) for BLING_IMAGE_ADD and BLING_IMAGE_ADD_UNFILTERED,
 *   width*height*3 floats (XYZ) for BLING_IMAGE_SPLAT; ACCUMULATED into.
 * The order promise: the target after the call is, bit for bit in binary32, what the reference's one thread
 * makes of it by applying the op to samples 0 .. n-1 in that order, the incoming target value being the first
 * operand: per pixel and channel a = a + w for W and a = a + (v * w) for X, Y, Z with the product rounded
 * first (a = a + 1, a = a + v for the two unfiltered ops), the contributing samples in ascending index.
 * XYZ comes from the 16 bands as the film kernels form it (three sequential binary32 sums divided by
 * BLING_CIE_Y_SUM); trap T12 (ifh = 1 / fw) is kept.  Hence two calls with lists A then B give the same bits
 * as one call with A followed by B, and the same list gives the same bytes on every run.  No float atomic is
 * used anywhere: integer atomics count and claim slots, and nothing depends on their order.
 * The drop rules, the same in bling_host_image_add_samples (bling_host.h):
 *   - a sample whose x or y is NaN, infinite or exceeds 2^20 in magnitude is dropped and counted in
 *     dropped_position (the reference's ceiling / floor of such a position are meaningless);
 *   - of the others, a sample with a NaN or infinite band is dropped and counted in dropped_spectrum
 *     (Image.hs:204-208, 225-229, 253-256), whether or not it would have landed inside the image;
 *   - a sample that reaches no pixel of the image adds nothing and is counted nowhere.
 * The (16 x 16 destination tile, sample) pairs go through a pair buffer of at most 64 MiB (4 bytes a pair;
 * bling_debug_set_image_budget sets another bound, in pairs): a longer list is cut into chunks of consecutive
 * samples applied one after another, which the composition rule makes legal; stats->chunks is their number
 * and stats->tile_pairs the pairs written.  stats (may be NULL): ms is the device time of the call (HIP events).
 * Errors: BLING_EINVAL for a NULL ctx / desc / xy / spectra / target (xy and spectra may be NULL when n == 0),
 * an unknown op, width or height < 1 (or width * height > 2^28), a filter width or height that is NaN,
 * infinite or <= 0, or a target that overlaps xy or spectra.  n == 0 leaves the target as it was.
 * bling_image_add_samples_device: xy, spectra and target are device buffers on device_ids[0] (e.g. torch
 *   tensors' data_ptr()); nothing crosses to the host.
 * bling_image_add_samples: the three are host buffers, staged through device buffers the context owns.
 * bling_image_develop_device: bling_film_develop_device with the width and height of the desc instead of an
 *   uploaded scene's: the same three formats, window rule and overlap check; no scene needed. */
/* bling_image_desc, bling_image_stats, bling_image_window and the BLING_IMAGE_* ops: bling_scene.h, shared with the
 * host library */
int bling_image_add_samples_device(bling_ctx* ctx, const bling_image_desc* desc, int op, const void* xy_dev,
                                   const void* spectra_dev, size_t n, void* target_dev, bling_image_stats* stats);
int bling_image_add_samples(bling_ctx* ctx, const bling_image_desc* desc, int op, const float* xy, const float* spectra,
                            size_t n, float* target_host, bling_image_stats* stats);
int bling_image_develop_device(bling_ctx* ctx, const bling_image_desc* desc, const bling_develop_params* p,
                               const void* film_dev, const void* splat_dev, void* out_dev);
/* ---- the image API on tiles: a renderer's windows onto the film, in order ----
 * Replaces: mkImageTile, addTile and scaleSplats of Image.hs (:108-120, :178-199, :93-106) as every renderer of
 * the reference uses them: prender (Rendering.hs:118-134) and SPPM's eye pass (SPPM.hs:148-163) make one
 * mkImageTile image per SampleWindow, add that window's samples to it and then addTile the tiles onto the image
 * in window order.  A host-side Renderer that computes its own samples in parallel windows reproduces the
 * reference's film through these calls.  Like the calls above they need no scene and leave one untouched.
 *   windows: n_windows SampleWindows (host array, ends inclusive); first: n_windows + 1 ascending sample
 *   offsets (host array) from 0 to n -- window k owns samples first[k] .. first[k+1]-1; xy, spectra: as above.
 *   film: width*height*4 floats, splat: width*height*3 floats.  Either may be NULL, except the one the op
 *   writes; a NULL image is not touched at all.
 * The promise: film and splat after the call equal, bit for bit, bling_host_image_add_windowed (bling_host.h)
 * of the same arguments, and are the same bytes on every run; no float atomic is used.  For k = 0, 1, ... in
 * order: a zeroed tile image (offset px = max 0 x0, py = max 0 y0, size w = x1 - px + floor (0.5 + fw), h
 * likewise -- a tile does not extend to the left of or above its window) receives the op of the window's
 * samples in ascending index, clipped to the tile (addSample: x0 = max px (ceiling (dx - fw)), x1 = min (px + w
 * - 1) (floor (dx + fw)); the unfiltered ops: floor sx - px in [0, w)); then every tile pixel inside the image
 * does old + tile on the three splat and the four film channels.  So a pixel's value is ((old + T_0) + T_1) + ...
 * over the windows whose tile covers it, T_k summed from +0 -- not the flat list's sample-by-sample sum, and not
 * its pixels either.  This holds for any windows: overlapping, nested, repeated, partly or wholly outside the
 * image, or empty (first[k] == first[k+1]).  Calls compose: windows 0 .. k in one call and k+1 .. in the next
 * give the bits of one call.
 * Trap T36: addTile adds a tile's zeros too, so a film or splat value of -0.0 under any window's tile becomes
 * +0.0 even if no sample reached it; a pixel under no tile keeps its bits.
 * The drop rules and counters are those above: a dropped sample is counted whether or not it lies in its tile; a
 * sample outside its own window's tile is clipped, not counted.  Chunks (the pair budget above) end at window
 * boundaries; a window longer than the budget is cut inside and its partial tile image carried to the next
 * chunk, so a window's sum is never split into two film additions.
 * Errors (BLING_EINVAL, nothing written): those above; a NULL windows / first; a first that does not start at
 * 0, ascend, and end at n; a window whose tile has w < 1 or h < 1 (the reference's MV.replicate of a negative
 * length; also beyond 2^31 - 1); film overlapping splat, or either overlapping xy or spectra.
 * bling_image_add_windowed_device: xy, spectra, film and splat are device buffers on device_ids[0].
 * bling_image_add_windowed: the four are host buffers, staged through device buffers the context owns.
 * bling_image_scale_splats_device: scaleSplats -- every pixel's three splat values become v * s, one binary32
 *   product each, s = factors_dev[i] (width*height floats on the device) or scalar when factors_dev is NULL.
 * splitMImage (Image.hs:84-91) is a zeroed image of the same shape: hipMemset of a buffer, or
 *   torch.zeros_like, serves it; there is no entry point. */
int bling_image_add_windowed_device(bling_ctx* ctx, const bling_image_desc* desc, int op, const bling_image_window* windows,
                                    const uint64_t* first, size_t n_windows, const void* xy_dev, const void* spectra_dev, size_t n,
                                    void* film_dev, void* splat_dev, bling_image_stats* stats);
int bling_image_add_windowed(bling_ctx* ctx, const bling_image_desc* desc, int op, const bling_image_window* windows,
                             const uint64_t* first, size_t n_windows, const float* xy, const float* spectra, size_t n,
                             float* film_host, float* splat_host, bling_image_stats* stats);
int bling_image_scale_splats_device(bling_ctx* ctx, const bling_image_desc* desc, void* splat_dev, const void* factors_dev,
                                    float scalar);
/* Test hook: the pair budget of this context's image calls, in pairs; 0 restores the default (64 MiB). */
int bling_debug_set_image_budget(bling_ctx* ctx, size_t max_tile_pairs);

/* ---- the integrator seam: surfaceLi for the caller's rays, on device buffers ----
 * Replaces: SurfaceIntegrator.surfaceLi :: Scene -> Ray -> Sampled s Spectrum (Integrator.hs:32-36) as every
 * renderer of the reference calls it, with a ray it made itself.  bling_sample_li always fires the uploaded
 * scene's own camera; these calls take the rays from the caller -- its own camera model, or any rays along which
 * it wants radiance -- and return the spectra in the layout bling_image_add_samples_device and
 * bling_image_add_windowed_device take as `spectra`, so that caller's rays -> surfaceLi -> addSample / addTile ->
 * develop runs on the device end to end.
 *   rays_soa: 7 planes of n floats: ox, oy, oz, dx, dy, dz, tmin.  tmax is +infinity, as fireRay's
 *     (Camera.hs:49-76).  The direction is used as given: the caller normalises, as fireRay does.
 *   ids: 2 uint32 per ray, (pixel, n): the ray's random stream is that of sample n of stream `pixel` of the pass,
 *     sample_key(seed, pass_index, pixel, n).  The camera's dimensions are simply not drawn; the path's
 *     dimensions keep the indices they have after a camera sample.  The built-in camera's stream for sample n of
 *     extent pixel (ix, iy) is pixel = (iy - ey0) * ext_w + (ix - ex0), with (ex0, ey0) the sample extent's
 *     first pixel and ext_w its width: a ray equal to that camera ray, with those ids, gives bling_sample_li's
 *     spectrum bit for bit.  Any pixel value is a valid stream; n must be below the scene's spp.
 *   L: n x 16 floats, row-major, ray k at 16 k: the spectrum before addSample's NaN filter, as bling_sample_li
 *     gives it.
 * The radiance is that of the integrator desc->config.integrator selected at upload: `path`, `directLighting` or
 * `debug normals`.  A ray's 16 floats depend on its seven floats, its ids, the seed and the pass only: not on n,
 * on its position in the batch, on what else is in the batch, or on how the call is cut into waves.
 * Dropped rays: a ray with a NaN or infinite float (tmin = +infinity excepted: a valid ray that misses
 * everything), with an all-zero direction, or with n >= spp is not traced.  It writes sixteen +0.0, counts in
 * stats->dropped and changes nothing for any other ray.
 * The call cuts itself into waves of at most the context's path capacity (at least 2^22 rays;
 * bling_debug_set_li_chunk sets another bound): any n is served, stats->waves is their number.
 * Errors: BLING_EINVAL for a NULL ctx; BLING_ENOSCENE without a scene; BLING_EINVAL when the scene's renderer
 * is not `sampler`; BLING_EUNSUPPORTED for the `bidir` integrator (its walk kernels make their camera ray
 * inside); then n == 0 is BLING_OK; BLING_EINVAL for a NULL rays_soa / ids / L, or an L that overlaps either
 * input.  Not served: a finite tmax.  stats may be NULL.
 * bling_surface_li_device: the three buffers are device buffers on device_ids[0] (e.g. torch tensors'
 *   data_ptr()); nothing is staged through the host.  The call runs on the context's stream and returns after
 *   completion; a multi-device context runs it on device_ids[0], as bling_sample_li.
 * bling_surface_li: the three are host buffers, staged through device buffers the context owns. */
typedef struct bling_li_stats {
    uint64_t rays;              /* rays handed in                                                   */
    uint64_t dropped;           /* rays not traced (see above); their L is +0                       */
    uint64_t rays_continuation, rays_mis, rays_shadow, path_vertices;   /* as bling_stats; a dropped
                                   ray is no vertex                                                 */
    uint64_t waves;             /* chunks the call was cut into                                     */
    double   ms_total;          /* device time of the call (HIP events)                             */
} bling_li_stats;
int bling_surface_li_device(bling_ctx* ctx, uint32_t seed, uint32_t pass_index, const void* rays_soa_dev,
                            const void* ids_dev, size_t n, void* L_dev, bling_li_stats* stats);
int bling_surface_li(bling_ctx* ctx, uint32_t seed, uint32_t pass_index, const float* rays_soa, const uint32_t* ids,
                     size_t n, float* L_out, bling_li_stats* stats);
/* Test hook: the rays per wave of this context's bling_surface_li* calls; 0 restores the default. */
int bling_debug_set_li_chunk(bling_ctx* ctx, size_t max_rays);

/* ---- the sampler and camera seam: a window's samples and rays, on device buffers ----
 * Replaces: the first third of prender's per-window work (Rendering.hs:118-134): `sample sampler window`
 * (Sampling.hs:101-132) walking the window's pixels, and fireRay cam (Camera.hs:49-76) of every sample -- for a
 * caller that keeps its own loop and wants the built-in sampler's and camera's samples but its own treatment of
 * them.  The outputs are what the other seams take: windows -> bling_camera_samples_device ->
 * bling_surface_li_device -> bling_image_add_windowed_device -> develop is a sampler-renderer pass whose film
 * equals the ordered film of bling_render_pass bit for bit, and the host sends only the windows.
 *   windows: n_windows SampleWindows (host array, ends inclusive, as the image calls take it); x1 < x0 or
 *     y1 < y0 is an empty window.
 *   first: n_windows + 1 ascending sample offsets (host array) from 0, the image calls' convention: window k owns
 *     slots first[k] .. first[k+1]-1, its pixels y outer, x inner, n = 0 .. spp-1 innermost (coverWindow's
 *     order); first[k+1] - first[k] must equal (x1-x0+1) (y1-y0+1) spp, 0 for an empty window.
 *     n = first[n_windows].
 *   xy_dev: 2 n floats, imageX, imageY: the xy of bling_image_add_*_device.
 *   ids_dev: 2 n uint32, (pixel, n) with pixel = (iy - ey0) * ext_w + (ix - ex0): the ids of
 *     bling_surface_li_device.
 *   rays_soa_dev: 7 planes of n floats, ox oy oz dx dy dz tmin of fireRay, tmin = 0: its rays_soa.
 *   lens_dev: 2 n floats, the lens sample (lu, lv), for a caller that applies its own lens.
 *   Each of the four may be NULL and is then not produced; the others' bits do not depend on that.
 * A window's block depends on the window, the seed, the pass and the uploaded scene only: not on the other
 * windows, their order, or how the call is cut (two calls over halves of the list, into offset pointers, give
 * the bits of one).  Windows may overlap, nest, repeat or be empty.  Every integrator of the sampler renderer
 * is served, `bidir` included: the camera sample does not depend on the integrator.  The outputs equal
 * bling_host_camera_samples (bling_host.h) of the same description bit for bit.  No path state of the context
 * is touched.  Any n is served with 64-bit slot arithmetic; a call of more than 2^30 samples is cut into
 * launches.
 * Errors: BLING_EINVAL for a NULL ctx; BLING_ENOSCENE without a scene; then BLING_EINVAL, with nothing written,
 * for a scene whose renderer is not `sampler`, a NULL first (or windows, when n_windows > 0), a first that does
 * not start at 0 or does not match the windows' counts, a non-empty window with a pixel outside the scene's
 * sample extent (the stream id is defined inside the extent only), an output that is not aligned to 4 bytes or
 * that overlaps another.  n = 0 succeeds.  stats may be NULL.
 * bling_camera_samples_device: the four outputs are device buffers on device_ids[0] (e.g. torch tensors'
 *   data_ptr()).  The call runs on the context's stream and returns after completion; a multi-device context
 *   runs it on device_ids[0], as bling_surface_li_device.
 * bling_camera_samples: the four are host buffers, staged through device buffers the context owns. */
typedef struct bling_camera_stats {
    uint64_t samples;           /* n                                                                */
    uint64_t windows;           /* n_windows                                                        */
    double   ms_total;          /* device time of the call (one pair of HIP events)                 */
} bling_camera_stats;
int bling_camera_samples_device(bling_ctx* ctx, uint32_t seed, uint32_t pass_index, const bling_image_window* windows,
                                const uint64_t* first, size_t n_windows, void* xy_dev, void* ids_dev, void* rays_soa_dev,
                                void* lens_dev, bling_camera_stats* stats);
int bling_camera_samples(bling_ctx* ctx, uint32_t seed, uint32_t pass_index, const bling_image_window* windows,
                         const uint64_t* first, size_t n_windows, float* xy, uint32_t* ids, float* rays_soa, float* lens,
                         bling_camera_stats* stats);

/* Diagnostics (no reference counterpart): the path-state bytes the shading kernel k_shade moved in
 * the context's last bling_render_pass*, per stream and direction -- out[2 k] read, out[2 k + 1]
 * written, stream k in the order BLING_STREAM_NAMES lists -- counted where the algorithm needs
 * them (a record the path uses), for the roofline's algorithmic bytes (DESIGN.md "Roofline").
 * Counted only by a BLING_STREAM_STATS build (make variant V=streams DEFS=-DBLING_STREAM_STATS=1);
 * other builds return BLING_EUNSUPPORTED.  *n_streams receives the stream count; out may be NULL. */
#define BLING_STREAM_NAMES "queue,hit,meta,org,dir,mdir,mhit,fm,occ,fac,rtex,T,L,Tn,lsc,bsc,sh_o,sh_d,result,qflag"
#define BLING_N_STREAMS 20
int bling_debug_stream_bytes(bling_ctx* ctx, uint64_t* out, size_t n, size_t* n_streams);

/* Diagnostics (no reference counterpart): of the rays_mis of the context's last bling_render_pass*,
 * the queries the shading kernels answered themselves (the MIS cull, BLING_PASS_NO_MIS_CULL); the
 * closest-hit kernel walked rays_camera + rays_continuation + rays_mis - *out queries. */
int bling_debug_mis_culled(bling_ctx* ctx, uint64_t* out);
/* on = 0: every later call on the context (bling_sample_li, which takes no pass flags, included)
 * walks all its MIS rays, as BLING_PASS_NO_MIS_CULL does for one pass; on = 1 (the default) restores
 * the cull.  Per-sample radiance is summed by no atomics, so it can be compared bit for bit. */
int bling_debug_set_mis_cull(bling_ctx* ctx, int on);

/* Diagnostics: which passes of the context run pipelined (BLING_PASS_NO_PIPELINE still wins): -1 the
 * scene profile's default, 0 none, 1 every pass for which it is legal (Path integrator, one wave, at
 * least two tiles, the traversal stack in LDS). */
int bling_debug_set_pipeline(bling_ctx* ctx, int mode);
/* Diagnostics: the per-sample results (X, Y, Z, 1, or zeros for a dropped sample: what addSample
 * receives) of the context's last bling_render_pass*, in the pass's tile order, and how it ran:
 * *waves = the number of waves run one after another, or -2 for two half-waves in flight together.
 * Only a pass of one wave or of two half-waves keeps them all (else BLING_EINVAL).  No float
 * atomics sum them, so two passes can be compared bit for bit.  *n receives the sample count; out
 * (4 floats per sample, cap samples; may be NULL) is written when cap suffices. */
int bling_debug_pass_results(bling_ctx* ctx, float* out, size_t cap, size_t* n, int* waves);
/* Diagnostics: one order-preserving compaction (the k_compact_* launches between two path vertices)
 * of n shade-queue entries with the given flag bytes (QF_* bits: 1 resolve, 2 shadow ray, 4 MIS ray,
 * 8 continuation, 16 culled MIS query) and input queue words, launched over capacity >= n entries.
 * queues_out: 6 * capacity words -- the two shade queues (capacity each), the closest-hit queue
 * (2 * capacity), the any-hit queue and the resolve list; qcount_out: their five lengths and the
 * culled count.  fused: as the Path integrator compacts (entries) or as DirectLighting (sample ids). */
int bling_debug_compact(bling_ctx* ctx, const uint8_t* flags, const uint32_t* queue_in, size_t n, size_t capacity,
                        int fused, uint32_t* queues_out, uint32_t* qcount_out);

/* The uploaded scene's acceleration / kernel plan as one JSON object (BVH2 and BVH4 depth and
 * sizes, the BVH4 stack bound, the LDS plans, the packet walk, the in-line shadow test), written
 * NUL-terminated into buf (at most size bytes); *len (may be NULL) receives the full length.
 * Diagnostics for bench.py and the tests; no reference counterpart. */
int bling_debug_scene_info(bling_ctx* ctx, char* buf, size_t size, size_t* len);
/* The same JSON object for a description that is not uploaded: the plan bling_scene_upload would settle
 * (its host builder), from the description alone -- no context and no device, like bling_scene_validate,
 * whose refusals it shares (BLING_EINVAL with the reason). */
int bling_debug_scene_plan(const bling_scene_desc* desc, char* buf, size_t size, size_t* len);

/* The host's derivation of the BVH4 and of the threaded list from a BVH2 (n2 nodes of 16 floats, as
 * bling_debug_bvh and bling_host_lbvh return them), without a context or a device: the specification the device
 * derivation is pinned to (csrc/common/bvh4.h).  A link must name a node of the array, and no node may be named
 * twice or name the root: BLING_EINVAL otherwise.
 *   bling_host_bvh4: nodes4_out (may be NULL) has room for cap_nodes4 nodes of 28 floats; *n4 always receives
 *     the node count (at most n2), *depth and *stack_need the BVH4's depth and stack bound; the nodes are written
 *     only when cap_nodes4 suffices (BLING_EINVAL otherwise, with nothing written).
 *   bling_host_threaded: the same for the entry list, 8 words an entry, at most 2 n2 entries. */
int bling_host_bvh4(const float* nodes2, size_t n2, float* nodes4_out, size_t cap_nodes4, size_t* n4, int* depth, int* stack_need);
int bling_host_threaded(const float* nodes2, size_t n2, float* entries_out, size_t cap_entries, size_t* n_entries);

/* Diagnostics: the uploaded scene's BVH2 as the kernels walk it, whichever builder made it, read back from
 * device_ids[0]: 16 floats per node (two child boxes, two links, two zero words) and the leaf refs.  *n_nodes
 * and *n_refs always receive the sizes; nodes and refs (either may be NULL) are written only when both
 * capacities (in nodes and in refs) suffice -- BLING_EINVAL otherwise, with nothing written. */
int bling_debug_bvh(bling_ctx* ctx, float* nodes, size_t cap_nodes, uint32_t* refs, size_t cap_refs, size_t* n_nodes,
                    size_t* n_refs);

/* Diagnostics: how the uploaded scene's BVH2 was built. */
#define BLING_BVH_FALLBACK_NONE    0u
#define BLING_BVH_FALLBACK_FRACTAL 1u   /* a fractal scene: its leaf order is the host tree's */
#define BLING_BVH_FALLBACK_ITEMS   2u   /* fewer than three items */
#define BLING_BVH_FALLBACK_DEPTH   3u   /* the linear BVH is deeper than the traversal stack allows */
#define BLING_BVH_FALLBACK_REFS    4u   /* more items than a leaf code can address */
typedef struct bling_bvh_build_info {
  uint32_t requested, used;       /* BLING_BVH_* */
  uint32_t fallback;              /* BLING_BVH_FALLBACK_*: why used differs from requested */
  uint32_t items, nodes, depth, leaves, max_leaf;
  double ms_build;                /* device builder: HIP events around its kernels; host builder: wall time */
  double ms_derive;               /* host wall time of what is derived from the BVH2: BVH4, threaded list, plans, leaf records;
                                   * host work alone (it used to span the upload of the tree's five arrays too) */
} bling_bvh_build_info;
int bling_debug_bvh_build_info(bling_ctx* ctx, bling_bvh_build_info* out);
/* Test hook: the depth above which the device builder stands down, 1 .. 31; 0 restores 31. */
int bling_debug_set_bvh_depth_cap(bling_ctx* ctx, int cap);

/* Diagnostics: what the uploaded scene's kernels walk besides the BVH2, whichever path derived it, read back
 * from device_ids[0]: the BVH4 (28 floats a node), the leaf records (float4s: three per leaf ref and one zero
 * record of three behind them) and the threaded list as it is walked (8 words an entry: the scene plan's pkt_n
 * entries, none when the list is too long to be walked).  *n_nodes4, *n_leaf_quads and *n_pkt always receive
 * the sizes (nodes, float4s, entries); the arrays (any may be NULL) are written only when every capacity given
 * with a non-NULL array suffices -- BLING_EINVAL otherwise, with nothing written. */
int bling_debug_derived(bling_ctx* ctx, float* nodes4, size_t cap_nodes4, float* leaf_geo, size_t cap_leaf_quads, float* pkt,
                        size_t cap_pkt, size_t* n_nodes4, size_t* n_leaf_quads, size_t* n_pkt);

/* Diagnostics: where the uploaded scene's BVH4, leaf records and plans were derived. */
#define BLING_DERIVE_HOST   0u
#define BLING_DERIVE_DEVICE 1u
#define BLING_DERIVE_FALLBACK_NONE     0u
#define BLING_DERIVE_FALLBACK_FRACTAL  1u   /* a fractal scene: its profiles walk the BVH2 in the host path's leaf order */
#define BLING_DERIVE_FALLBACK_DEVICES  2u   /* a context of several devices: the peers receive the host's plan */
#define BLING_DERIVE_FALLBACK_NODES    3u   /* a BVH2 without nodes */
typedef struct bling_derive_info {
  uint32_t requested, used;       /* BLING_DERIVE_* */
  uint32_t fallback;              /* BLING_DERIVE_FALLBACK_*: why used differs from requested */
  uint32_t bvh4_nodes, bvh4_depth, stack_need;
  uint32_t level_launches;        /* device: BVH4 levels, each one open / scan / link round; host: 0 */
  uint32_t reserved;
  double ms_derive_device;        /* device: HIP events around the derive kernels (the per-level count read-backs included) */
  double ms_plan_host;            /* host wall time of the host's share: the whole derivation, or the plan from the counts */
} bling_derive_info;
int bling_debug_derive_info(bling_ctx* ctx, bling_derive_info* out);

/* Frees every device resource of the context. */
void bling_destroy(bling_ctx* ctx);

/* Thread-local description of the last error on this thread. */
const char* bling_last_error(void);

/* Build identification (arch, compile flags) for reports. */
const char* bling_version(void);

#ifdef __cplusplus
}
#endif
#endif /* BLING_H */
