"""ctypes bindings for the two product shared libraries.

* ``libbling_host.so``  -- the `.bling` loader + film output (include/bling_host.h)
* ``libbling_hip.so``   -- the MI355X core (include/bling.h)

Both are built in-tree by ``make`` (see ``__graft_entry__.build``).  Nothing here falls back to a
CPU implementation: if the HIP library cannot be loaded, :func:`hip` raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIBDIR = os.path.join(_HERE, "_lib")

c_f32p = C.POINTER(C.c_float)
c_u32p = C.POINTER(C.c_uint32)


PASS_TRAVERSAL_STATS = 1   # BLING_PASS_TRAVERSAL_STATS
PASS_KERNEL_TIMING = 2     # BLING_PASS_KERNEL_TIMING
PASS_TILE_IMAGES = 4       # BLING_PASS_TILE_IMAGES
PASS_REGION_EVENTS = 8     # BLING_PASS_REGION_EVENTS (bling_render only)
PASS_NO_MIS_CULL = 16      # BLING_PASS_NO_MIS_CULL
PASS_NO_PIPELINE = 32      # BLING_PASS_NO_PIPELINE
PASS_ORDERED_FILM = 64     # BLING_PASS_ORDERED_FILM


class PassParams(C.Structure):
    """bling_pass_params (include/bling.h)."""
    _fields_ = [("seed", C.c_uint32), ("pass_index", C.c_uint32), ("shard_rank", C.c_int32),
                ("shard_world", C.c_int32), ("tile_stride", C.c_int32), ("chunk_paths", C.c_int32),
                ("flags", C.c_uint32), ("tiles_device", C.c_void_p), ("tiles_capacity", C.c_uint64)]


class Stats(C.Structure):
    """bling_stats (include/bling.h)."""
    _fields_ = [("camera_samples", C.c_uint64), ("rays_camera", C.c_uint64),
                ("rays_continuation", C.c_uint64), ("rays_mis", C.c_uint64),
                ("rays_shadow", C.c_uint64), ("dropped_samples", C.c_uint64),
                ("tiles", C.c_uint64), ("ms_total", C.c_double), ("ms_bounce", C.c_double),
                ("ms_film", C.c_double), ("bounce_launches", C.c_uint64), ("path_vertices", C.c_uint64),
                ("node_visits", C.c_uint64), ("tri_tests", C.c_uint64), ("shape_tests", C.c_uint64),
                ("ms_closest", C.c_double), ("closest_launches", C.c_uint64), ("march_ticks", C.c_uint64),
                ("closest_node_visits", C.c_uint64), ("closest_tri_tests", C.c_uint64),
                ("closest_shape_tests", C.c_uint64), ("closest_march_ticks", C.c_uint64),
                ("ms_shade", C.c_double), ("shade_launches", C.c_uint64)]

    def rays(self) -> int:
        return int(self.rays_camera + self.rays_continuation + self.rays_mis + self.rays_shadow)

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class ImageWindow(C.Structure):
    """bling_image_window (include/bling_scene.h): a SampleWindow, ends inclusive."""
    _fields_ = [("x0", C.c_int32), ("x1", C.c_int32), ("y0", C.c_int32), ("y1", C.c_int32)]


class ImageTile(C.Structure):
    """bling_image_tile (include/bling_scene.h): mkImageTile's offset and size, and the tile's sampleExtent."""
    _fields_ = [("px", C.c_int32), ("py", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("extent", C.c_int32 * 4)]


class SppmStats(C.Structure):
    """bling_sppm_stats (include/bling.h)."""
    _fields_ = [("hitpoints", C.c_uint64), ("photons", C.c_uint64), ("photon_rays", C.c_uint64),
                ("photon_hits", C.c_uint64), ("cam_rays", C.c_uint64), ("dropped", C.c_uint64),
                ("ms_total", C.c_double), ("ms_eye", C.c_double), ("ms_hash", C.c_double),
                ("ms_photon", C.c_double)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class LightStats(C.Structure):
    """bling_light_stats (include/bling.h)."""
    _fields_ = [("photons", C.c_uint64), ("photon_rays", C.c_uint64), ("shadow_rays", C.c_uint64),
                ("splats", C.c_uint64), ("dropped", C.c_uint64), ("ms_total", C.c_double)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class SppmRecord(C.Structure):
    """bling_sppm_record (include/bling.h)."""
    _fields_ = [("thread", C.c_uint32), ("photon", C.c_uint32), ("seq", C.c_uint32), ("depth", C.c_uint32),
                ("sx", C.c_int32), ("sy", C.c_int32), ("x", C.c_float), ("y", C.c_float), ("z", C.c_float),
                ("pad", C.c_uint32)]


class LightRecord(C.Structure):
    """bling_light_record (include/bling.h): one splat of the light tracer's record mode, 32 bytes."""
    _fields_ = [("photon", C.c_uint32), ("depth", C.c_uint32), ("sx", C.c_int32), ("sy", C.c_int32),
                ("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("pad", C.c_uint32)]


class LightTracer(C.Structure):
    """bling_light_tracer (include/bling_scene.h): the trailing member of bling_scene_desc."""
    _fields_ = [("pass_photons", C.c_int32), ("pixel_area", C.c_float), ("w2r", C.c_float * 16)]


class Metropolis(C.Structure):
    """bling_metropolis (include/bling_scene.h): appended to bling_scene_desc after the light tracer block."""
    _fields_ = [("max_depth", C.c_int32), ("mpp", C.c_float), ("bootstrap", C.c_int32), ("plarge", C.c_float),
                ("chains", C.c_int32)]


class MltStats(C.Structure):
    """bling_mlt_stats (include/bling.h)."""
    _fields_ = [("b", C.c_double), ("mutations", C.c_uint64), ("large_steps", C.c_uint64), ("accepted", C.c_uint64),
                ("splats", C.c_uint64), ("dropped", C.c_uint64), ("rays_camera", C.c_uint64),
                ("rays_continuation", C.c_uint64), ("rays_mis", C.c_uint64), ("rays_shadow", C.c_uint64),
                ("path_vertices", C.c_uint64), ("ms_total", C.c_double)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class MltRecord(C.Structure):
    """bling_mlt_record (include/bling.h): one (chain, mutation) of the Metropolis renderer's record mode, 32 bytes."""
    _fields_ = [("chain", C.c_uint32), ("mutation", C.c_uint32), ("x", C.c_float), ("y", C.c_float),
                ("i_prop", C.c_float), ("a", C.c_float), ("flags", C.c_uint32), ("pad", C.c_uint32)]


DEVELOP_RGB_F32, DEVELOP_RGB8, DEVELOP_RGBE = 0, 1, 2   # BLING_DEVELOP_*
SPLAT_ORDERED = 1          # BLING_SPLAT_ORDERED


class DevelopParams(C.Structure):
    """bling_develop_params (include/bling.h); window = x0, x1, y0, y1, inclusive."""
    _fields_ = [("format", C.c_int32), ("splat_weight", C.c_float), ("window", C.c_int32 * 4)]


FILTER_KINDS = {"box": 0, "gauss": 1, "sinc": 2, "mitchell": 3, "triangle": 4}   # BLING_FILTER_*
IMAGE_OPS = {"add": 0, "add_unfiltered": 1, "splat": 2}                            # BLING_IMAGE_*


class Filter(C.Structure):
    """bling_filter (include/bling_scene.h)."""
    _fields_ = [("kind", C.c_int32), ("width", C.c_float), ("height", C.c_float), ("table", C.c_float * 256)]


class ImageDesc(C.Structure):
    """bling_image_desc (include/bling_scene.h)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("filter", Filter)]


class ImageStats(C.Structure):
    """bling_image_stats (include/bling_scene.h)."""
    _fields_ = [("samples", C.c_uint64), ("dropped_spectrum", C.c_uint64), ("dropped_position", C.c_uint64),
                ("tile_pairs", C.c_uint64), ("chunks", C.c_uint64), ("ms", C.c_double)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class LiStats(C.Structure):
    """bling_li_stats (include/bling.h)."""
    _fields_ = [("rays", C.c_uint64), ("dropped", C.c_uint64), ("rays_continuation", C.c_uint64), ("rays_mis", C.c_uint64),
                ("rays_shadow", C.c_uint64), ("path_vertices", C.c_uint64), ("waves", C.c_uint64), ("ms_total", C.c_double)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class CameraStats(C.Structure):
    """bling_camera_stats (include/bling.h)."""
    _fields_ = [("samples", C.c_uint64), ("windows", C.c_uint64), ("ms_total", C.c_double)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


BVH_BUILDERS = {"host": 0, "device": 1}                                          # BLING_BVH_*
BVH_FALLBACKS = ["none", "fractal", "items", "depth", "refs"]                    # BLING_BVH_FALLBACK_*


DERIVE_PATHS = {"host": 0, "device": 1}                                          # BLING_DERIVE_*; the device bit of flags
DERIVE_FALLBACKS = ["none", "fractal", "devices", "nodes"]                       # BLING_DERIVE_FALLBACK_*


class DeriveInfo(C.Structure):
    """bling_derive_info (include/bling.h)."""
    _fields_ = [("requested", C.c_uint32), ("used", C.c_uint32), ("fallback", C.c_uint32), ("bvh4_nodes", C.c_uint32),
                ("bvh4_depth", C.c_uint32), ("stack_need", C.c_uint32), ("level_launches", C.c_uint32), ("reserved", C.c_uint32),
                ("ms_derive_device", C.c_double), ("ms_plan_host", C.c_double)]


class UploadParams(C.Structure):
    """bling_upload_params (include/bling.h)."""
    _fields_ = [("bvh_builder", C.c_uint32), ("flags", C.c_uint32)]


class BvhBuildInfo(C.Structure):
    """bling_bvh_build_info (include/bling.h)."""
    _fields_ = [("requested", C.c_uint32), ("used", C.c_uint32), ("fallback", C.c_uint32), ("items", C.c_uint32),
                ("nodes", C.c_uint32), ("depth", C.c_uint32), ("leaves", C.c_uint32), ("max_leaf", C.c_uint32),
                ("ms_build", C.c_double), ("ms_derive", C.c_double)]


class LbvhInfo(C.Structure):
    """bling_lbvh_info (include/bling_host.h)."""
    _fields_ = [("items", C.c_uint32), ("nodes", C.c_uint32), ("depth", C.c_uint32), ("leaves", C.c_uint32),
                ("max_leaf", C.c_uint32)]


class RenderConfig(C.Structure):
    _fields_ = [("renderer", C.c_int32), ("sampler", C.c_int32), ("nu", C.c_int32), ("nv", C.c_int32),
                ("spp", C.c_int32), ("max_depth", C.c_int32), ("sample_depth", C.c_int32),
                ("width", C.c_int32), ("height", C.c_int32), ("integrator", C.c_int32),
                ("sppm_photons", C.c_int32), ("sppm_radius", C.c_float), ("sppm_alpha", C.c_float),
                ("sppm_threads", C.c_int32)]


_host = None
_hip = None


def host() -> C.CDLL:
    global _host
    if _host is None:
        lib = C.CDLL(os.path.join(LIBDIR, "libbling_host.so"))
        lib.bling_host_load.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]
        lib.bling_host_load.restype = C.c_int
        lib.bling_host_desc.argtypes = [C.c_void_p]
        lib.bling_host_desc.restype = C.c_void_p
        if hasattr(lib, "bling_host_sppm_splat_weight"):
            lib.bling_host_sppm_splat_weight.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
            lib.bling_host_sppm_splat_weight.restype = C.c_float
        lib.bling_host_summary.argtypes = [C.c_void_p]
        lib.bling_host_summary.restype = C.c_char_p
        lib.bling_host_free.argtypes = [C.c_void_p]
        lib.bling_host_config.argtypes = [C.c_void_p, C.POINTER(RenderConfig)]
        lib.bling_host_filter_size.argtypes = [C.c_void_p, c_f32p]
        lib.bling_host_filter_table.argtypes = [C.c_void_p, c_f32p]
        lib.bling_host_counts.argtypes = [C.c_void_p, c_u32p]
        lib.bling_host_last_error.restype = C.c_char_p
        lib.bling_host_film_to_rgb.argtypes = [c_f32p, C.c_int, C.c_int, c_f32p]
        lib.bling_host_film_splat_to_rgb.argtypes = [c_f32p, c_f32p, C.c_float, C.c_int, C.c_int, c_f32p]
        lib.bling_host_light.argtypes = [C.c_void_p, C.POINTER(LightTracer)]
        lib.bling_host_metropolis.argtypes = [C.c_void_p, C.POINTER(Metropolis)]
        lib.bling_host_write_hdr.argtypes = [C.c_char_p, c_f32p, C.c_int, C.c_int]
        lib.bling_host_write_hdr.restype = C.c_int
        lib.bling_host_rgb_pixels.argtypes = [c_f32p, C.c_int, C.c_int, C.POINTER(C.c_uint8)]
        lib.bling_host_write_png.argtypes = [C.c_char_p, c_f32p, C.c_int, C.c_int]
        lib.bling_host_write_png.restype = C.c_int
        c_u8p = C.POINTER(C.c_uint8)
        lib.bling_host_rgb_pixels_splat.argtypes = [c_f32p, c_f32p, C.c_float, C.c_int, C.c_int, c_u8p]
        lib.bling_host_write_png_splat.argtypes = [C.c_char_p, c_f32p, c_f32p, C.c_float, C.c_int, C.c_int]
        lib.bling_host_write_png_splat.restype = C.c_int
        lib.bling_host_gamma_thresholds.argtypes = [c_f32p]
        lib.bling_host_gamma_thresholds.restype = None
        lib.bling_host_write_png_rgb8.argtypes = [C.c_char_p, c_u8p, C.c_int, C.c_int]
        lib.bling_host_write_png_rgb8.restype = C.c_int
        lib.bling_host_write_hdr_rgbe.argtypes = [C.c_char_p, c_u8p, C.c_int, C.c_int]
        lib.bling_host_write_hdr_rgbe.restype = C.c_int
        lib.bling_host_make_filter.argtypes = [C.c_int, c_f32p, C.c_int, C.POINTER(Filter)]
        lib.bling_host_make_filter.restype = C.c_int
        lib.bling_host_eval_filter.argtypes = [C.c_int, c_f32p, C.c_float, C.c_float]
        lib.bling_host_eval_filter.restype = C.c_float
        lib.bling_host_image_extent.argtypes = [C.POINTER(ImageDesc), C.POINTER(C.c_int32)]
        lib.bling_host_image_extent.restype = None
        lib.bling_host_image_add_samples.argtypes = [C.POINTER(ImageDesc), C.c_int, c_f32p, c_f32p, C.c_size_t, c_f32p]
        lib.bling_host_image_add_samples.restype = C.c_int
        lib.bling_host_image_tile.argtypes = [C.POINTER(ImageDesc), C.POINTER(ImageWindow), C.POINTER(ImageTile)]
        lib.bling_host_image_tile.restype = C.c_int
        lib.bling_host_image_add_windowed.argtypes = [C.POINTER(ImageDesc), C.c_int, C.POINTER(ImageWindow), C.POINTER(C.c_uint64),
                                                      C.c_size_t, c_f32p, c_f32p, C.c_size_t, c_f32p, c_f32p, C.POINTER(ImageStats)]
        lib.bling_host_image_add_windowed.restype = C.c_int
        lib.bling_host_image_scale_splats.argtypes = [C.POINTER(ImageDesc), c_f32p, c_f32p, C.c_float]
        lib.bling_host_image_scale_splats.restype = C.c_int
        lib.bling_host_camera_samples.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(ImageWindow), C.POINTER(C.c_uint64),
                                                  C.c_size_t, c_f32p, c_u32p, c_f32p, c_f32p]
        lib.bling_host_camera_samples.restype = C.c_int
        lib.bling_host_rgb_to_spectrum_illum.argtypes = [c_f32p, c_f32p]
        lib.bling_host_rgb_to_spectrum_illum.restype = None
        lib.bling_host_lbvh.argtypes = [c_f32p, c_u32p, C.c_size_t, C.c_int, c_f32p, c_u32p, C.POINTER(C.c_uint64),
                                        C.POINTER(LbvhInfo)]
        lib.bling_host_lbvh.restype = C.c_int
        _host = lib
    return _host


HIP_SYMBOLS = ["bling_create", "bling_scene_upload", "bling_scene_validate", "bling_render_pass", "bling_render_pass_device",
               "bling_trace", "bling_trace_device", "bling_sample_li", "bling_sample_li_vertices", "bling_pass_tile_layout",
               "bling_film_add_tiles", "bling_film_add_shards", "bling_sppm_pass", "bling_sppm_pixel_stats", "bling_sppm_reset",
               "bling_render", "bling_debug_stream_bytes", "bling_debug_scene_info", "bling_debug_mis_culled", "bling_debug_set_mis_cull", "bling_debug_set_pipeline", "bling_debug_pass_results", "bling_debug_compact", "bling_debug_sppm_hitpoints", "bling_debug_sppm_buckets",
               "bling_film_develop", "bling_film_develop_device", "bling_light_pass", "bling_debug_light_records", "bling_mlt_pass", "bling_debug_mlt_records", "bling_debug_mlt_boot", "bling_debug_mlt_set_boot", "bling_light_pass_device", "bling_mlt_pass_device", "bling_debug_splat_merge", "bling_debug_set_splat_budget", "bling_debug_splat_times", "bling_sppm_pass_device", "bling_debug_sppm_records", "bling_debug_bidir_terms",
               "bling_image_add_samples_device", "bling_image_add_samples", "bling_image_develop_device", "bling_debug_set_image_budget",
               "bling_image_add_windowed_device", "bling_image_add_windowed", "bling_image_scale_splats_device",
               "bling_surface_li_device", "bling_surface_li", "bling_debug_set_li_chunk",
               "bling_camera_samples_device", "bling_camera_samples",
               "bling_scene_upload_with", "bling_debug_bvh", "bling_debug_bvh_build_info", "bling_debug_set_bvh_depth_cap",
               "bling_debug_scene_plan", "bling_debug_derived", "bling_debug_derive_info", "bling_host_bvh4", "bling_host_threaded",
               "bling_destroy", "bling_last_error", "bling_version"]


class Progress(C.Structure):
    """bling_progress (include/bling.h): one report of bling_render (PassDone, or with
    PASS_REGION_EVENTS the per-window RegionStarted / SamplesAdded)."""
    _fields_ = [("kind", C.c_int32), ("pass_", C.c_int32), ("film", C.POINTER(C.c_float)), ("splat_weight", C.c_float),
                ("pass_stats", C.POINTER(Stats)), ("region", C.c_int32 * 4)]


PROGRESS_STARTED, PROGRESS_SAMPLES_ADDED, PROGRESS_REGION_STARTED, PROGRESS_PASS_DONE = 0, 1, 2, 3
ProgressFn = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(Progress))
STREAM_NAMES = "queue,hit,meta,org,dir,mdir,mhit,fm,occ,fac,rtex,T,L,Tn,lsc,bsc,sh_o,sh_d,result,qflag".split(",")


def hip() -> C.CDLL:
    """Load libbling_hip.so (raises OSError if it was not built -- no silent fallback)."""
    global _hip
    if _hip is None:
        # BLING_HIP_VARIANT=<v> loads the experiment build libbling_hip_<v>.so (make variant V=<v>)
        var = os.environ.get("BLING_HIP_VARIANT", "")
        path = os.path.join(LIBDIR, f"libbling_hip_{var}.so" if var else "libbling_hip.so")
        if not os.path.exists(path):
            raise OSError(f"{path} missing: run `make` (the HIP core has no CPU fallback)")
        lib = C.CDLL(path)
        lib.bling_create.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]
        lib.bling_create.restype = C.c_int
        lib.bling_scene_upload.argtypes = [C.c_void_p, C.c_void_p]
        lib.bling_scene_upload.restype = C.c_int
        if hasattr(lib, "bling_scene_validate"):      # older experiment builds (BLING_HIP_VARIANT) lack it
            lib.bling_scene_validate.argtypes = [C.c_void_p]
            lib.bling_scene_validate.restype = C.c_int
        lib.bling_render_pass.argtypes = [C.c_void_p, C.POINTER(PassParams), c_f32p, C.POINTER(Stats)]
        lib.bling_render_pass.restype = C.c_int
        lib.bling_render_pass_device.argtypes = [C.c_void_p, C.POINTER(PassParams), C.c_void_p, C.POINTER(Stats)]
        lib.bling_render_pass_device.restype = C.c_int
        lib.bling_pass_tile_layout.argtypes = [C.c_void_p, C.POINTER(PassParams), C.POINTER(C.c_int32),
                                               C.POINTER(C.c_size_t), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        lib.bling_pass_tile_layout.restype = C.c_int
        lib.bling_film_add_tiles.argtypes = [C.c_void_p, C.POINTER(PassParams), C.c_void_p, C.c_void_p]
        lib.bling_film_add_tiles.restype = C.c_int
        lib.bling_film_add_shards.argtypes = [C.c_void_p, C.POINTER(PassParams), C.POINTER(C.c_void_p), C.c_void_p]
        lib.bling_film_add_shards.restype = C.c_int
        lib.bling_trace.argtypes = [C.c_void_p, c_f32p, C.c_size_t, C.c_int, c_f32p, c_u32p, c_f32p]
        lib.bling_trace.restype = C.c_int
        lib.bling_trace_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_int, C.POINTER(C.c_double)]
        lib.bling_trace_device.restype = C.c_int
        lib.bling_sppm_pass.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, c_f32p, c_f32p, C.POINTER(SppmStats)]
        lib.bling_sppm_pass.restype = C.c_int
        lib.bling_sppm_pixel_stats.argtypes = [C.c_void_p, c_f32p, c_f32p, C.POINTER(C.c_size_t)]
        lib.bling_sppm_pixel_stats.restype = C.c_int
        lib.bling_sppm_reset.argtypes = [C.c_void_p]
        lib.bling_sppm_reset.restype = C.c_int
        if hasattr(lib, "bling_render"):              # older experiment builds lack the pass loop
            lib.bling_render.argtypes = [C.c_void_p, C.POINTER(PassParams), c_f32p, ProgressFn, C.c_void_p,
                                         C.POINTER(Stats)]
            lib.bling_render.restype = C.c_int
        lib.bling_debug_sppm_hitpoints.argtypes = [C.c_void_p, c_f32p, C.POINTER(C.c_uint64), C.c_size_t,
                                                   C.POINTER(C.c_size_t)]
        lib.bling_debug_sppm_hitpoints.restype = C.c_int
        lib.bling_debug_sppm_buckets.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), c_f32p,
                                                 C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        lib.bling_debug_sppm_buckets.restype = C.c_int
        lib.bling_light_pass.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, c_f32p, C.POINTER(LightStats)]
        lib.bling_light_pass.restype = C.c_int
        lib.bling_debug_light_records.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                  C.POINTER(LightRecord), C.c_size_t, C.POINTER(C.c_size_t)]
        lib.bling_debug_light_records.restype = C.c_int
        if hasattr(lib, "bling_mlt_pass"):            # older experiment builds lack the Metropolis renderer
            lib.bling_mlt_pass.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, c_f32p, C.POINTER(MltStats)]
            lib.bling_mlt_pass.restype = C.c_int
            lib.bling_debug_mlt_records.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                    C.POINTER(MltRecord), C.c_size_t, C.POINTER(C.c_size_t), c_u32p, c_f32p]
            lib.bling_debug_mlt_records.restype = C.c_int
            lib.bling_debug_mlt_boot.argtypes = [c_f32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, c_f32p, c_u32p]
            lib.bling_debug_mlt_boot.restype = C.c_int
            lib.bling_debug_mlt_set_boot.argtypes = [C.c_void_p, c_f32p, C.c_uint32]
            lib.bling_debug_mlt_set_boot.restype = C.c_int
        if hasattr(lib, "bling_light_pass_device"):   # older experiment builds lack the device splat images
            lib.bling_light_pass_device.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                                    C.POINTER(LightStats)]
            lib.bling_light_pass_device.restype = C.c_int
            lib.bling_mlt_pass_device.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                                  C.POINTER(MltStats)]
            lib.bling_mlt_pass_device.restype = C.c_int
            lib.bling_debug_splat_merge.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
            lib.bling_debug_splat_merge.restype = C.c_int
            lib.bling_debug_set_splat_budget.argtypes = [C.c_void_p, C.c_size_t]
            lib.bling_debug_set_splat_budget.restype = C.c_int
            lib.bling_debug_splat_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
            lib.bling_debug_splat_times.restype = C.c_int
        if hasattr(lib, "bling_sppm_pass_device"):    # older experiment builds lack SPPM's device images
            lib.bling_sppm_pass_device.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                                   C.POINTER(SppmStats)]
            lib.bling_sppm_pass_device.restype = C.c_int
            lib.bling_debug_sppm_records.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                     C.POINTER(SppmRecord), C.c_size_t, C.POINTER(C.c_size_t)]
            lib.bling_debug_sppm_records.restype = C.c_int
        if hasattr(lib, "bling_debug_bidir_terms"):   # older experiment builds lack it
            lib.bling_debug_bidir_terms.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.c_size_t,
                                                    c_f32p, C.POINTER(C.c_int32)]
            lib.bling_debug_bidir_terms.restype = C.c_int
        if hasattr(lib, "bling_film_develop"):        # older experiment builds lack the develop entry points
            lib.bling_film_develop_device.argtypes = [C.c_void_p, C.POINTER(DevelopParams), C.c_void_p, C.c_void_p, C.c_void_p]
            lib.bling_film_develop_device.restype = C.c_int
            lib.bling_film_develop.argtypes = [C.c_void_p, C.POINTER(DevelopParams), c_f32p, c_f32p, C.c_void_p]
            lib.bling_film_develop.restype = C.c_int
        lib.bling_image_add_samples_device.argtypes = [C.c_void_p, C.POINTER(ImageDesc), C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                                       C.c_void_p, C.POINTER(ImageStats)]
        lib.bling_image_add_samples_device.restype = C.c_int
        lib.bling_image_add_samples.argtypes = [C.c_void_p, C.POINTER(ImageDesc), C.c_int, c_f32p, c_f32p, C.c_size_t, c_f32p,
                                                C.POINTER(ImageStats)]
        lib.bling_image_add_samples.restype = C.c_int
        lib.bling_image_develop_device.argtypes = [C.c_void_p, C.POINTER(ImageDesc), C.POINTER(DevelopParams), C.c_void_p, C.c_void_p,
                                                   C.c_void_p]
        lib.bling_image_develop_device.restype = C.c_int
        lib.bling_image_add_windowed_device.argtypes = [C.c_void_p, C.POINTER(ImageDesc), C.c_int, C.POINTER(ImageWindow),
                                                        C.POINTER(C.c_uint64), C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                                        C.c_void_p, C.c_void_p, C.POINTER(ImageStats)]
        lib.bling_image_add_windowed_device.restype = C.c_int
        lib.bling_image_add_windowed.argtypes = [C.c_void_p, C.POINTER(ImageDesc), C.c_int, C.POINTER(ImageWindow),
                                                 C.POINTER(C.c_uint64), C.c_size_t, c_f32p, c_f32p, C.c_size_t, c_f32p, c_f32p,
                                                 C.POINTER(ImageStats)]
        lib.bling_image_add_windowed.restype = C.c_int
        lib.bling_image_scale_splats_device.argtypes = [C.c_void_p, C.POINTER(ImageDesc), C.c_void_p, C.c_void_p, C.c_float]
        lib.bling_image_scale_splats_device.restype = C.c_int
        lib.bling_debug_set_image_budget.argtypes = [C.c_void_p, C.c_size_t]
        lib.bling_debug_set_image_budget.restype = C.c_int
        if hasattr(lib, "bling_surface_li_device"):   # older experiment builds lack the integrator seam
            lib.bling_surface_li_device.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t,
                                                    C.c_void_p, C.POINTER(LiStats)]
            lib.bling_surface_li_device.restype = C.c_int
            lib.bling_surface_li.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, c_f32p, c_u32p, C.c_size_t, c_f32p,
                                             C.POINTER(LiStats)]
            lib.bling_surface_li.restype = C.c_int
            lib.bling_debug_set_li_chunk.argtypes = [C.c_void_p, C.c_size_t]
            lib.bling_debug_set_li_chunk.restype = C.c_int
        if hasattr(lib, "bling_camera_samples_device"):   # older experiment builds lack the sampler and camera seam
            lib.bling_camera_samples_device.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(ImageWindow),
                                                        C.POINTER(C.c_uint64), C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_void_p, C.POINTER(CameraStats)]
            lib.bling_camera_samples_device.restype = C.c_int
            lib.bling_camera_samples.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(ImageWindow), C.POINTER(C.c_uint64),
                                                 C.c_size_t, c_f32p, c_u32p, c_f32p, c_f32p, C.POINTER(CameraStats)]
            lib.bling_camera_samples.restype = C.c_int
        lib.bling_debug_scene_info.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
        lib.bling_debug_scene_info.restype = C.c_int
        lib.bling_debug_scene_plan.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
        lib.bling_debug_scene_plan.restype = C.c_int
        if hasattr(lib, "bling_debug_mis_culled"):    # older experiment builds lack it
            lib.bling_debug_mis_culled.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
            lib.bling_debug_mis_culled.restype = C.c_int
            lib.bling_debug_set_mis_cull.argtypes = [C.c_void_p, C.c_int]
            lib.bling_debug_set_mis_cull.restype = C.c_int
        if hasattr(lib, "bling_debug_set_pipeline"):  # older experiment builds lack them
            lib.bling_debug_set_pipeline.argtypes = [C.c_void_p, C.c_int]
            lib.bling_debug_set_pipeline.restype = C.c_int
            lib.bling_debug_pass_results.argtypes = [C.c_void_p, c_f32p, C.c_size_t, C.POINTER(C.c_size_t),
                                                     C.POINTER(C.c_int)]
            lib.bling_debug_pass_results.restype = C.c_int
            lib.bling_debug_compact.argtypes = [C.c_void_p, C.POINTER(C.c_uint8), c_u32p, C.c_size_t, C.c_size_t, C.c_int,
                                                c_u32p, c_u32p]
            lib.bling_debug_compact.restype = C.c_int
        if hasattr(lib, "bling_debug_stream_bytes"):
            lib.bling_debug_stream_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t,
                                                     C.POINTER(C.c_size_t)]
            lib.bling_debug_stream_bytes.restype = C.c_int
        if hasattr(lib, "bling_scene_upload_with"):   # older experiment builds lack the device BVH builder
            lib.bling_scene_upload_with.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(UploadParams)]
            lib.bling_scene_upload_with.restype = C.c_int
            lib.bling_debug_bvh.argtypes = [C.c_void_p, c_f32p, C.c_size_t, c_u32p, C.c_size_t, C.POINTER(C.c_size_t),
                                            C.POINTER(C.c_size_t)]
            lib.bling_debug_bvh.restype = C.c_int
            lib.bling_debug_bvh_build_info.argtypes = [C.c_void_p, C.POINTER(BvhBuildInfo)]
            lib.bling_debug_bvh_build_info.restype = C.c_int
            lib.bling_debug_set_bvh_depth_cap.argtypes = [C.c_void_p, C.c_int]
            lib.bling_debug_set_bvh_depth_cap.restype = C.c_int
        if hasattr(lib, "bling_debug_derived"):       # older experiment builds lack the device derivation
            c_szp = C.POINTER(C.c_size_t)
            lib.bling_debug_derived.argtypes = [C.c_void_p, c_f32p, C.c_size_t, c_f32p, C.c_size_t, c_f32p, C.c_size_t, c_szp, c_szp, c_szp]
            lib.bling_debug_derived.restype = C.c_int
            lib.bling_debug_derive_info.argtypes = [C.c_void_p, C.POINTER(DeriveInfo)]
            lib.bling_debug_derive_info.restype = C.c_int
            lib.bling_host_bvh4.argtypes = [c_f32p, C.c_size_t, c_f32p, C.c_size_t, c_szp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
            lib.bling_host_bvh4.restype = C.c_int
            lib.bling_host_threaded.argtypes = [c_f32p, C.c_size_t, c_f32p, C.c_size_t, c_szp]
            lib.bling_host_threaded.restype = C.c_int
        lib.bling_destroy.argtypes = [C.c_void_p]
        lib.bling_last_error.restype = C.c_char_p
        lib.bling_version.restype = C.c_char_p
        _hip = lib
    return _hip


def f32ptr(a):
    return a.ctypes.data_as(c_f32p)


def u32ptr(a):
    return a.ctypes.data_as(c_u32p)
