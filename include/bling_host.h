/*
 * bling_host.h -- host side of the boundary: the `.bling` scene loader and film output.
 *
 * In the reference this is Haskell and stays unchanged (north_star: "unchanged: parser,
 * Material/Texture, Film/tonemap"): parseJob (IO/RenderJob.hs:31-34) and the PState parsers in
 * IO/ *.hs, plus getPixel/xyzToRgb (Image.hs:302-315) and the HDR writer (IO/Bitmap.hs:36-41).
 * GHC is absent from this image, so this C++ library restates them for the config subset and
 * produces the flattened bling_scene_desc that bling_scene_upload() (bling.h) consumes.
 */
#ifndef BLING_HOST_H
#define BLING_HOST_H

#include <stddef.h>
#include "bling_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bling_host_scene bling_host_scene;

/* Parse a .bling file (parseJob, IO/RenderJob.hs:31-65).
 * overrides: NULL or "key=value;..." applied at parse time, e.g.
 *   "image=1024,1024;stratified=8,8;path=15,3"   (imageSize is patched IN PLACE, trap T2)
 *   "random=512"  "filter=triangle,2,2"  "force_path=1" (trap T1: the last renderer wins)
 * Returns 0 or a negative error (message via bling_host_last_error). */
int bling_host_load(const char* path, const char* overrides, bling_host_scene** out);

const bling_scene_desc* bling_host_desc(const bling_host_scene* s);

/* Renderer configuration and filter extent of the parsed job (for drivers). */
void bling_host_config(const bling_host_scene* s, bling_render_config* out);
void bling_host_filter_size(const bling_host_scene* s, float* wh);
/* The light tracer block: photons per pass, and the camera's world-to-raster matrix and pixel area. */
void bling_host_light(const bling_host_scene* s, bling_light_tracer* out);
void bling_host_metropolis(const bling_host_scene* s, bling_metropolis* out);
/* The 16x16 filter table (mkTableFilter, Image.hs:48-61) and the scene's prim/shape/light counts
 * (out[0..5] = triangles, shapes, fractal present, prims, lights, feature bits) for tests/tools. */
void bling_host_filter_table(const bling_host_scene* s, float* out256);
void bling_host_counts(const bling_host_scene* s, uint32_t* out6);

/* Human-readable summary of the parsed scene (prettyPrint Scene, Scene.hs:28-35). */
const char* bling_host_summary(const bling_host_scene* s);

/* SPPM's splat weight of pass k (k >= 1): 1 / (threads * k * sn^2), sn = ceil (sqrt (photons / threads))
 * in binary32 (Renderer/SPPM.hs:449, 460, 474) -- what getPixel applies to the photon image after pass k.
 * *sn_out (may be NULL) receives sn.  0 for a scene whose renderer is not sppm or k < 1. */
float bling_host_sppm_splat_weight(const bling_render_config* cfg, int pass, int* sn_out);

void bling_host_free(bling_host_scene* s);

const char* bling_host_last_error(void);

/* Film -> RGB (getPixel: XYZ/W + splat, then xyzToRgb; Image.hs:302-315, Spectrum.hs:162-168).
 * film: w*h*4 (W,X,Y,Z); rgb_out: w*h*3. */
void bling_host_film_to_rgb(const float* film, int w, int h, float* rgb_out);

/* Radiance HDR (.hdr, RGBE) writer for the RGB image (writeRgbe, IO/Bitmap.hs:36-41). */
int bling_host_write_hdr(const char* path, const float* rgb, int w, int h);

/* rgbPixels (Image.hs:317-331) of the whole film: getPixel with splat weight 1 and an empty splat
 * buffer, gamma 2.2 (Float `**` = powf of 1/2.2), clamp to [0,1] with Haskell min/max NaN rules,
 * * 255 and Haskell `round` (half to even).  out_rgb8: w*h*3 bytes, row-major from the top. */
void bling_host_rgb_pixels(const float* film, int w, int h, unsigned char* out_rgb8);

/* 8-bit RGB PNG of rgbPixels (writePng, IO/Bitmap.hs:40-41 / Progress.hs:29).  The reference's
 * own float -> 8-bit step lives in JuicyPixels (absent here), so the pixels are the
 * reference's rgbPixels mapping; the zlib stream uses stored (uncompressed) deflate blocks. */
int bling_host_write_png(const char* path, const float* film, int w, int h);

/* getPixel with a splat buffer (w*h*3 XYZ, may be NULL) and splat weight sw (Image.hs:301-314):
 * XYZ = sw * splat (+ film XYZ / W when W != 0), then xyzToRgb.  SPPM's pass-k image uses
 * sw = 1 / (threads * k * sn^2) (Renderer/SPPM.hs:460). */
void bling_host_film_splat_to_rgb(const float* film, const float* splat, float sw, int w, int h, float* rgb_out);
void bling_host_rgb_pixels_splat(const float* film, const float* splat, float sw, int w, int h,
                                 unsigned char* out_rgb8);
int bling_host_write_png_splat(const char* path, const float* film, const float* splat, float sw, int w, int h);

/* The float -> 8-bit step of rgbPixels as a table: out255[k], k = 0 .. 254, is the smallest binary32 v
 * whose byte nearbyint(min(1, max(0, powf(v, 1/2.2f))) * 255) is at least k + 1, found by bisecting
 * over float bit patterns with that very expression.  The byte of any v is then the count of
 * out255[k] <= v (NaN, finite negatives and +-0 count none; +Inf counts all), except that -Inf, whose
 * powf is +Inf, has the byte 255 and is looked up as +Inf.  bling_film_develop (bling.h)
 * looks its RGB8 bytes up in this table, built by the same routine, instead of calling a device pow. */
void bling_host_gamma_thresholds(float* out255);

/* The encoders of the two writers above for pixels that are already developed, e.g. by
 * bling_film_develop: rgb8 is w*h*3 bytes (BLING_DEVELOP_RGB8), rgbe w*h*4 bytes (BLING_DEVELOP_RGBE),
 * row-major from the top.  bling_host_write_png[_splat] and bling_host_write_hdr go through them, so
 * the same pixels give the same file. */
int bling_host_write_png_rgb8(const char* path, const unsigned char* rgb8, int w, int h);
int bling_host_write_hdr_rgbe(const char* path, const unsigned char* rgbe, int w, int h);

/* ---- the host side of the image API (bling_image_*, bling.h) ----
 * bling_host_make_filter: the bling_filter (size and 16 x 16 table, mkTableFilter) of a pixel filter given as
 * the `filter` line of a scene file gives it: kind BLING_FILTER_* and its n parameters -- box none, gauss
 * w h alpha, sinc w h tau, mitchell w h B C, triangle w h.  0, or -1 for an unknown kind or a wrong n.
 * bling_host_eval_filter: evalFilter (Filter.hs:68-96) of that filter at (x, y); 0 for an unknown kind. */
int   bling_host_make_filter(int kind, const float* params, int n, bling_filter* out);
float bling_host_eval_filter(int kind, const float* params, float x, float y);
/* sampleExtent (Image.hs:162-168) of the image: out4 = x0, x1, y0, y1, inclusive. */
void  bling_host_image_extent(const bling_image_desc* desc, int32_t out4[4]);
/* The sequential binary32 restatement of addSample, addUnfilteredSample and splatSample (Image.hs:201-299):
 * op BLING_IMAGE_* applied to samples 0 .. n-1 in that order, accumulated into target (width*height*4 floats,
 * or *3 for BLING_IMAGE_SPLAT).  xy: 2 floats a sample, spectra: 16.  Compiled without multiply-add
 * contraction, as the oracle is; bling_image_add_samples[_device] gives the same bits.  The drop rules are
 * those of bling.h: a sample whose x or y is NaN, infinite or beyond 2^20 in magnitude is dropped, and so is
 * one with a NaN or infinite band.  0, or -1 for a NULL argument, an unknown op, width or height < 1, or a
 * filter size that is not finite and positive. */
int   bling_host_image_add_samples(const bling_image_desc* desc, int op, const float* xy, const float* spectra, size_t n,
                                   float* target);
/* mkImageTile (Image.hs:108-120) of a SampleWindow over the image: the tile image's offset, size and
 * sampleExtent (Image.hs:162-168 with the offset), literally: px = max 0 x0, w = x1 - px + floor (0.5 + fw) -- a
 * tile does not extend to the left of or above its window.  0, or -1 for a NULL argument or a tile with w < 1 or
 * h < 1 (the reference's MV.replicate of a negative length). */
int   bling_host_image_tile(const bling_image_desc* desc, const bling_image_window* window, bling_image_tile* out);
/* The sequential binary32 restatement of a renderer's use of its film (prender, Rendering.hs:118-134): for
 * window k = 0 .. n_windows-1 in order, a zeroed mkImageTile image of windows[k] receives op of samples
 * first[k] .. first[k+1]-1 in ascending index with the tile's offset (addSample's x0 = max ox (ceiling (dx - fw)),
 * x1 = min (ox + w - 1) (floor (dx + fw)); the unfiltered ops' floor sx - ox in [0, w)), and addTile
 * (Image.hs:178-199) then adds the tile onto film AND splat: old + tile for every tile pixel inside the image,
 * the tile's zeros too (trap T36: a -0.0 under a tile becomes +0.0).  first: n_windows + 1 ascending offsets
 * from 0 to n.  film (width*height*4) or splat (width*height*3) may be NULL, except the one the op writes; a
 * NULL image is not touched by addTile either.  stats (may be NULL): samples and the two drop counters of
 * bling.h's rules.  bling_image_add_windowed[_device] gives the same bits.  0, or -1 for a NULL argument, an
 * unknown op, a bad size or filter size, a first that does not ascend from 0 to n, or a window whose tile has
 * w < 1 or h < 1; the images are then untouched. */
int   bling_host_image_add_windowed(const bling_image_desc* desc, int op, const bling_image_window* windows, const uint64_t* first,
                                    size_t n_windows, const float* xy, const float* spectra, size_t n, float* film, float* splat,
                                    bling_image_stats* stats);
/* scaleSplats (Image.hs:93-106): every pixel's three splat values become v * s, one binary32 product each,
 * s = factors[i] of pixel i, or scalar when factors is NULL.  splitMImage (Image.hs:84-91) is a zeroed image of
 * the same shape and needs no call. */
int   bling_host_image_scale_splats(const bling_image_desc* desc, float* splat, const float* factors, float scalar);
/* ---- the host side of the sampler and camera seam (bling_camera_samples*, bling.h) ----
 * The samples and camera rays of SampleWindows, on the CPU: `sample sampler window` (Sampling.hs:101-132, the
 * counter RNG of DESIGN.md in place of MWC) walks a window's pixels y outer, x inner, n = 0 .. spp-1 innermost
 * (coverWindow's order), and every sample fires fireRay (Camera.hs:49-76) of the description's camera.  It needs
 * no context and no GPU: the sequential yardstick of bling_camera_samples_device, whose outputs equal these bit
 * for bit, and the path for a host without a device.  Binary32 in the operation order of the device's
 * camera_sample / fire_ray, compiled without multiply-add contraction.
 *   windows: n_windows SampleWindows, ends inclusive; x1 < x0 or y1 < y0 is an empty window.
 *   first: n_windows + 1 ascending offsets from 0; first[k+1] - first[k] must be (x1-x0+1) (y1-y0+1) spp of
 *     window k (0 for an empty one).  n = first[n_windows].
 *   xy: 2 n floats (imageX, imageY); ids: 2 n uint32 (pixel, n), pixel = (iy - ey0) * ext_w + (ix - ex0) over
 *     the sample extent; rays_soa: 7 planes of n floats, ox oy oz dx dy dz tmin (tmin = 0); lens: 2 n floats,
 *     the lens sample (lu, lv).  Any of the four may be NULL.
 * A window's block depends on the window, the seed, the pass and the description only.  0, or -1 with nothing
 * written: a NULL desc or first, a renderer block that is not the sampler renderer's, a first that does not match
 * the counts, a non-empty window with a pixel outside the sample extent, two outputs that overlap. */
int   bling_host_camera_samples(const bling_scene_desc* desc, uint32_t seed, uint32_t pass_index,
                                const bling_image_window* windows, const uint64_t* first, size_t n_windows, float* xy,
                                uint32_t* ids, float* rays_soa, float* lens);
/* rgbToSpectrumIllum (Spectrum.hs:146-159 over the illuminant bases), as the loader applies it to image maps. */
void  bling_host_rgb_to_spectrum_illum(const float rgb[3], float out16[16]);

/* ---- the host side of the device BVH builder (bling_scene_upload_with, BLING_BVH_DEVICE; bling.h) ----
 * The linear BVH of csrc/common/lbvh.h on the CPU, with no context and no GPU: Morton keys over the boxes'
 * centres (key = 30-bit code << 32 | item index), ascending order, the common-prefix hierarchy, leaves of one or
 * two items, surviving nodes numbered ascending with the root as node 0.  The device builder's tree equals this
 * one bit for bit.
 *   boxes: n items, 6 floats each (lo.xyz, hi.xyz); refs: their n leaf reference words.  3 <= n <= 2^24.
 *   depth_cap: the deepest tree returned, 1 .. 31; 0 = 31.
 *   nodes_out: room for 16 (n - 1) floats; info->nodes nodes of 16 floats are written (two child boxes, two
 *     links, two zero words: the BVH2 node the kernels walk).  refs_out: n words, the refs in sorted order.
 *     keys_out (may be NULL): the n sorted keys.
 * BLING_LBVH_OK; BLING_LBVH_EINVAL for a NULL argument, an n or a depth_cap out of range; BLING_LBVH_EDEPTH for
 * a tree deeper than the cap: info->depth holds its depth, refs_out and keys_out are written, nodes_out is not. */
#define BLING_LBVH_OK      0
#define BLING_LBVH_EINVAL -1
#define BLING_LBVH_EDEPTH -2
typedef struct bling_lbvh_info {
  uint32_t items, nodes, depth, leaves, max_leaf;
} bling_lbvh_info;
int   bling_host_lbvh(const float* boxes, const uint32_t* refs, size_t n, int depth_cap, float* nodes_out, uint32_t* refs_out,
                      uint64_t* keys_out, bling_lbvh_info* info);

#ifdef __cplusplus
}
#endif
#endif
