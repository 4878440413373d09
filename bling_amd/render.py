"""Host-side mirror of the reference's renderer interface over the MI355X core (libbling_hip.so).

Reference interface (src/lib/Graphics/Bling/Rendering.hs):
  * ``class Renderer a where render :: a -> RenderJob -> ProgressReporter -> IO ()``   (:77-78)
  * ``SamplerRenderer`` / ``prender``: progressive passes, each pass = every tile once (:252-296)
  * ``Progress`` events ``Started``/``RegionStarted``/``SamplesAdded``/``PassDone`` (:60-73); the
    reporter returns False to stop after a pass (:136-137)
Here the per-pass work is one ``bling_render_pass`` call (the whole tile list on the GPU), so the
progress stream is ``Started`` then one ``PassDone`` per pass.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _ffi
from .scene import Job

DEFAULT_SEED = 0x0B11A6   # master seed of the benchmark


# numpy view of bling_light_record (include/bling.h)
SPPM_RECORD = np.dtype([("thread", "<u4"), ("photon", "<u4"), ("seq", "<u4"), ("depth", "<u4"), ("sx", "<i4"), ("sy", "<i4"),
                        ("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("pad", "<u4")])
LIGHT_RECORD = np.dtype([("photon", "<u4"), ("depth", "<u4"), ("sx", "<i4"), ("sy", "<i4"),
                         ("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("pad", "<u4")])

# numpy view of bling_splat_rec (include/bling.h)
SPLAT_REC = np.dtype([("pixel", "<u4"), ("pad", "<u4"), ("key", "<u8"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"),
                      ("pad2", "<u4")])

# numpy view of bling_mlt_record (include/bling.h)
MLT_RECORD = np.dtype([("chain", "<u4"), ("mutation", "<u4"), ("x", "<f4"), ("y", "<f4"), ("i_prop", "<f4"),
                       ("a", "<f4"), ("flags", "<u4"), ("pad", "<u4")])


class BlingError(RuntimeError):
    def __init__(self, rc: int, msg: str):
        super().__init__(f"bling error {rc}: {msg}")
        self.rc = rc


def _check(rc: int):
    if rc != 0:
        raise BlingError(rc, _ffi.hip().bling_last_error().decode())


def mlt_boot(values, seed, pass_index, chains):
    """bling_debug_mlt_boot: (b', start samples) of hand-given bootstrap contributions; no device needed."""
    v = np.ascontiguousarray(values, np.float32)
    b = np.zeros(1, np.float32)
    starts = np.zeros(chains, np.uint32)
    _check(_ffi.hip().bling_debug_mlt_boot(_ffi.f32ptr(v), len(v), seed, pass_index, chains, _ffi.f32ptr(b), _ffi.u32ptr(starts)))
    return np.float32(b[0]), starts


CAMERA_OUTPUTS = ("xy", "ids", "rays", "lens")


def camera_windows(windows, spp, counts_or_first=None):
    """The ctypes window array, the n_windows + 1 ascending uint64 offsets and the number of windows of a list of
    SampleWindows (x0, x1, y0, y1), ends inclusive.  counts_or_first: the windows' sample counts or the offsets;
    None derives them from the windows and spp -- (x1-x0+1) (y1-y0+1) spp, 0 for an empty window."""
    wl = [tuple(int(v) for v in w) for w in windows]
    if any(len(w) != 4 for w in wl):
        raise ValueError("a window is (x0, x1, y0, y1)")
    if counts_or_first is None:
        c = np.asarray([max(0, x1 - x0 + 1) * max(0, y1 - y0 + 1) * int(spp) for x0, x1, y0, y1 in wl], np.int64)
    else:
        c = np.asarray(counts_or_first, np.int64).reshape(-1)
    if len(c) == len(wl):
        first = np.concatenate([np.zeros(1, np.int64), np.cumsum(c)])
    elif len(c) == len(wl) + 1:
        first = c
    else:
        raise ValueError(f"{len(wl)} windows need {len(wl)} counts or {len(wl) + 1} offsets, not {len(c)}")
    arr = (_ffi.ImageWindow * max(1, len(wl)))(*(_ffi.ImageWindow(*w) for w in wl))
    return arr, np.ascontiguousarray(first.astype(np.uint64)), len(wl)


def host_camera_samples(job: Job, windows, seed=DEFAULT_SEED, pass_index=0, counts_or_first=None, outputs=CAMERA_OUTPUTS,
                        into=None):
    """bling_host_camera_samples: the samples and camera rays of the SampleWindows on the CPU, through
    libbling_host -- no context, no GPU.  Returns (xy (n, 2) float32, ids (n, 2) uint32, rays (7, n) float32,
    lens (n, 2) float32) as numpy arrays; one not named in outputs is None.  into: a dict of preallocated arrays
    to write into instead.  ValueError where the library refuses (nothing is written then)."""
    arr, first, nw = camera_windows(windows, job.spp, counts_or_first)
    n = int(first[-1])
    shapes = {"xy": ((n, 2), np.float32), "ids": ((n, 2), np.uint32), "rays": ((7, n), np.float32), "lens": ((n, 2), np.float32)}
    bufs = {}
    for k in CAMERA_OUTPUTS:
        if k not in outputs:
            bufs[k] = None
        elif into is not None and k in into:
            bufs[k] = into[k]
        else:
            bufs[k] = np.zeros(*shapes[k])
    ptr = {k: (None if b is None else C.c_void_p(b.ctypes.data)) for k, b in bufs.items()}
    lib = _ffi.host()
    rc = lib.bling_host_camera_samples(C.c_void_p(job.desc), seed, pass_index, arr, first.ctypes.data_as(C.POINTER(C.c_uint64)), nw,
                                       C.cast(ptr["xy"], _ffi.c_f32p), C.cast(ptr["ids"], _ffi.c_u32p),
                                       C.cast(ptr["rays"], _ffi.c_f32p), C.cast(ptr["lens"], _ffi.c_f32p))
    if rc != 0:
        raise ValueError(lib.bling_host_last_error().decode())
    return bufs["xy"], bufs["ids"], bufs["rays"], bufs["lens"]


class Context:
    """One bling_ctx (bling_create / bling_destroy) on one HIP device, or on several: a list of
    device ids makes every render pass fan out over all of them inside the library (include/bling.h,
    bling_create), with the summed film on the first device."""

    def __init__(self, device: int | list[int] = 0):
        lib = _ffi.hip()
        h = C.c_void_p()
        ids = [device] if isinstance(device, int) else list(device)
        dev = (C.c_int * len(ids))(*ids)
        _check(lib.bling_create(dev, len(ids), C.byref(h)))
        self._h = h
        self.device = ids[0]
        self.devices = ids
        self.job: Job | None = None

    def upload(self, job: Job, bvh: str | int | None = None, derive: str | None = None):
        """bling_scene_upload (replaces Scene.mkScene -> mkKdTree).  bvh: "host" (the default: the binned SAH
        on the host) or "device" (the linear BVH built on the device, bling_scene_upload_with); an integer is
        passed on as the BLING_BVH_* value it is.  derive: "host" (the default) or "device": the BVH4 and the leaf
        records derived from the BVH2 on the device (BLING_UPLOAD_DERIVE_DEVICE)."""
        if bvh is None and derive is None:
            _check(_ffi.hip().bling_scene_upload(self._h, C.c_void_p(job.desc)))
        else:
            if isinstance(bvh, str) and bvh not in _ffi.BVH_BUILDERS:
                raise ValueError(f"bvh is 'host' or 'device', not {bvh!r}")
            if derive is not None and derive not in _ffi.DERIVE_PATHS:
                raise ValueError(f"derive is 'host' or 'device', not {derive!r}")
            flags = _ffi.DERIVE_PATHS[derive] if derive is not None else 0
            builder = 0 if bvh is None else _ffi.BVH_BUILDERS[bvh] if isinstance(bvh, str) else int(bvh)
            up = _ffi.UploadParams(builder, flags)
            _check(_ffi.hip().bling_scene_upload_with(self._h, C.c_void_p(job.desc), C.byref(up)))
        self.job = job

    def derived(self) -> dict:
        """bling_debug_derived: what the kernels walk besides the BVH2, read back from the device, whichever path
        derived it: {"nodes4": (n, 28) float32, "leaf_geo": (m, 4) float32, "pkt": (e, 8) float32} (pkt: the
        entries the packet kernels walk; none when the list is too long).  Links are int32 bit patterns."""
        n4, nl, ne = C.c_size_t(), C.c_size_t(), C.c_size_t()
        lib = _ffi.hip()
        _check(lib.bling_debug_derived(self._h, None, 0, None, 0, None, 0, C.byref(n4), C.byref(nl), C.byref(ne)))
        out = {"nodes4": np.zeros((int(n4.value), 28), np.float32), "leaf_geo": np.zeros((int(nl.value), 4), np.float32),
               "pkt": np.zeros((int(ne.value), 8), np.float32)}
        _check(lib.bling_debug_derived(self._h, _ffi.f32ptr(out["nodes4"]), n4.value, _ffi.f32ptr(out["leaf_geo"]), nl.value,
                                       _ffi.f32ptr(out["pkt"]), ne.value, C.byref(n4), C.byref(nl), C.byref(ne)))
        return out

    def derive_info(self) -> dict:
        """bling_debug_derive_info: where the BVH4, leaf records and plans were derived: requested / used ("host" /
        "device"), fallback ("none", "fractal", "devices", "nodes"), bvh4_nodes, bvh4_depth, stack_need,
        level_launches, ms_derive_device, ms_plan_host."""
        di = _ffi.DeriveInfo()
        _check(_ffi.hip().bling_debug_derive_info(self._h, C.byref(di)))
        names = {v: k for k, v in _ffi.DERIVE_PATHS.items()}
        out = {k: getattr(di, k) for k, _ in di._fields_ if k != "reserved"}
        out["requested"], out["used"] = names[di.requested], names[di.used]
        out["fallback"] = _ffi.DERIVE_FALLBACKS[di.fallback]
        return out

    def bvh(self):
        """bling_debug_bvh: the uploaded BVH2 as (nodes (n, 16) float32, refs (m,) uint32), whichever builder
        made it.  The links (words 12 and 13 of a node) are int32 bit patterns: nodes.view(np.int32)."""
        nn, nr = C.c_size_t(), C.c_size_t()
        _check(_ffi.hip().bling_debug_bvh(self._h, None, 0, None, 0, C.byref(nn), C.byref(nr)))
        nodes = np.zeros((int(nn.value), 16), np.float32)
        refs = np.zeros(int(nr.value), np.uint32)
        _check(_ffi.hip().bling_debug_bvh(self._h, _ffi.f32ptr(nodes), nodes.shape[0], _ffi.u32ptr(refs), len(refs),
                                          C.byref(nn), C.byref(nr)))
        return nodes, refs

    def bvh_build_info(self) -> dict:
        """bling_debug_bvh_build_info: the builder asked for and used ("host" / "device"), the fallback reason
        ("none", "fractal", "items", "depth", "refs"), items, nodes, depth, leaves, max_leaf, ms_build, ms_derive."""
        bi = _ffi.BvhBuildInfo()
        _check(_ffi.hip().bling_debug_bvh_build_info(self._h, C.byref(bi)))
        names = {v: k for k, v in _ffi.BVH_BUILDERS.items()}
        out = {k: getattr(bi, k) for k, _ in bi._fields_}
        out["requested"], out["used"] = names[bi.requested], names[bi.used]
        out["fallback"] = _ffi.BVH_FALLBACKS[bi.fallback]
        return out

    def set_bvh_depth_cap(self, cap=0):
        """bling_debug_set_bvh_depth_cap: the depth above which the device builder stands down (0: 31)."""
        _check(_ffi.hip().bling_debug_set_bvh_depth_cap(self._h, int(cap)))

    def render_pass(self, seed=DEFAULT_SEED, pass_index=0, shard=(0, 1), tile_stride=1, chunk_paths=0,
                    film: np.ndarray | None = None, flags=0, ordered=False):
        """One pass into a host film (accumulated). Returns (film, Stats).  ordered=True forms the film in
        the reference's order without float atomics (BLING_PASS_ORDERED_FILM): the same bits on every run,
        however the pass is cut, equal to the CPU restatement's film."""
        job = self.job
        if film is None:
            film = np.zeros(job.width * job.height * 4, np.float32)
        pp = _ffi.PassParams(seed, pass_index, shard[0], shard[1], tile_stride, chunk_paths, flags | self._ordered(ordered))
        st = _ffi.Stats()
        _check(_ffi.hip().bling_render_pass(self._h, C.byref(pp), _ffi.f32ptr(film), C.byref(st)))
        return film, st

    @staticmethod
    def _ordered(ordered):
        return _ffi.PASS_ORDERED_FILM if ordered else 0

    def render_loop(self, report, seed=DEFAULT_SEED, first_pass=1, film: np.ndarray | None = None, shard=(0, 1),
                    tile_stride=1, regions=None, ordered=False):
        """bling_render: passes first_pass, first_pass + 1, ... into a host film until report(pass,
        film, stats) returns False (prender's onePass loop with its ProgressReporter,
        Rendering.hs:127-140); stats is that pass's own bling_stats as a dict.  With regions (a
        callable), every pass first reports prender's per-window events as regions(kind, pass,
        (x0, x1, y0, y1), film) with kind "region_started" (film None) or "samples_added"
        (BLING_PASS_REGION_EVENTS).  ordered=True: every pass's film, and with regions every
        samples_added film, is the ordered one (BLING_PASS_ORDERED_FILM).  Returns (film, Stats summed
        over the passes)."""
        job = self.job
        if film is None:
            film = np.zeros(job.width * job.height * 4, np.float32)
        flags = (_ffi.PASS_REGION_EVENTS if regions is not None else 0) | self._ordered(ordered)
        pp = _ffi.PassParams(seed, first_pass, shard[0], shard[1], tile_stride, 0, flags)
        st = _ffi.Stats()
        err = []
        kinds = {_ffi.PROGRESS_REGION_STARTED: "region_started", _ffi.PROGRESS_SAMPLES_ADDED: "samples_added"}

        def cb(_user, ev):
            try:
                e = ev.contents
                if e.kind in kinds:
                    regions(kinds[e.kind], int(e.pass_), tuple(int(v) for v in e.region),
                            film if e.kind == _ffi.PROGRESS_SAMPLES_ADDED else None)
                    return 1
                assert e.kind == _ffi.PROGRESS_PASS_DONE
                one = e.pass_stats.contents.as_dict() if e.pass_stats else {}
                return 1 if report(int(e.pass_), film, one) else 0
            except Exception as ex:          # never unwind through the C frame
                err.append(ex)
                return 0
        fn = _ffi.ProgressFn(cb)
        _check(_ffi.hip().bling_render(self._h, C.byref(pp), _ffi.f32ptr(film), fn, None, C.byref(st)))
        if err:
            raise err[0]
        return film, st

    def scene_info(self) -> dict:
        """bling_debug_scene_info: the uploaded scene's acceleration / kernel plan."""
        import json
        buf = C.create_string_buffer(1024)
        _check(_ffi.hip().bling_debug_scene_info(self._h, buf, len(buf), None))
        return json.loads(buf.value.decode())

    def mis_culled(self) -> int:
        """bling_debug_mis_culled: the last pass's BSDF-MIS queries that were answered without a walk."""
        n = C.c_uint64()
        _check(_ffi.hip().bling_debug_mis_culled(self._h, C.byref(n)))
        return int(n.value)

    def set_mis_cull(self, on: bool):
        """bling_debug_set_mis_cull: switch the MIS cull for every later call (sample_li included)."""
        _check(_ffi.hip().bling_debug_set_mis_cull(self._h, 1 if on else 0))

    def set_pipeline(self, mode: int):
        """bling_debug_set_pipeline: -1 the scene profile's default, 0 never, 1 wherever a pass can run
        as two half-waves on two streams (the pass flag PASS_NO_PIPELINE still wins)."""
        _check(_ffi.hip().bling_debug_set_pipeline(self._h, int(mode)))

    def pass_results(self):
        """bling_debug_pass_results: the last pass's per-sample results, [n, 4] (X, Y, Z, 1 or zeros) in
        tile order, and how it ran: the number of waves, or -2 for two half-waves in flight together."""
        n, waves = C.c_size_t(), C.c_int()
        _check(_ffi.hip().bling_debug_pass_results(self._h, None, 0, C.byref(n), C.byref(waves)))
        out = np.zeros((int(n.value), 4), np.float32)
        _check(_ffi.hip().bling_debug_pass_results(self._h, _ffi.f32ptr(out), out.shape[0], C.byref(n), C.byref(waves)))
        return out, int(waves.value)

    def compact(self, flags: np.ndarray, queue_in: np.ndarray, capacity: int | None = None, fused: bool = True):
        """bling_debug_compact: one compaction of the flag bytes over the input queue.  Returns
        ({"shade0", "shade1", "closest", "any", "resolve"} -> the raw queue arrays, qcount[6])."""
        flags = np.ascontiguousarray(flags, np.uint8)
        queue_in = np.ascontiguousarray(queue_in, np.uint32)
        n = int(flags.size)
        cap = int(capacity if capacity is not None else max(n, 1))
        fl = flags if n else np.zeros(1, np.uint8)
        qi = queue_in if n else np.zeros(1, np.uint32)
        out = np.zeros(6 * cap, np.uint32)
        qc = np.zeros(6, np.uint32)
        _check(_ffi.hip().bling_debug_compact(self._h, fl.ctypes.data_as(C.POINTER(C.c_uint8)), qi.ctypes.data_as(_ffi.c_u32p),
                                              n, cap, 1 if fused else 0, out.ctypes.data_as(_ffi.c_u32p),
                                              qc.ctypes.data_as(_ffi.c_u32p)))
        q = {"shade0": out[:cap], "shade1": out[cap:2 * cap], "closest": out[2 * cap:4 * cap], "any": out[4 * cap:5 * cap],
             "resolve": out[5 * cap:]}
        return q, qc

    def stream_bytes(self) -> dict:
        """bling_debug_stream_bytes: k_shade's path-state bytes of the last pass per stream,
        {name: (read, written)} (BLING_STREAM_STATS builds only)."""
        n = C.c_size_t()
        out = (C.c_uint64 * (2 * len(_ffi.STREAM_NAMES)))()
        _check(_ffi.hip().bling_debug_stream_bytes(self._h, out, len(out), C.byref(n)))
        return {k: (int(out[2 * i]), int(out[2 * i + 1])) for i, k in enumerate(_ffi.STREAM_NAMES)}

    def render_pass_device(self, film_ptr: int, seed=DEFAULT_SEED, pass_index=0, shard=(0, 1), tile_stride=1,
                           chunk_paths=0, flags=0, ordered=False):
        """One pass accumulated into a device film (e.g. ``torch_tensor.data_ptr()``); ordered as
        render_pass's."""
        pp = _ffi.PassParams(seed, pass_index, shard[0], shard[1], tile_stride, chunk_paths, flags | self._ordered(ordered))
        st = _ffi.Stats()
        _check(_ffi.hip().bling_render_pass_device(self._h, C.byref(pp), C.c_void_p(film_ptr), C.byref(st)))
        return st

    def tile_layout(self, shard=(0, 1), tile_stride=1):
        """bling_pass_tile_layout: (origins (n, 2) int32, slot_w, slot_h) of a tile-image pass."""
        pp = _ffi.PassParams(0, 0, shard[0], shard[1], tile_stride, 0, 0, None)
        n, sw, sh = C.c_size_t(), C.c_int32(), C.c_int32()
        _check(_ffi.hip().bling_pass_tile_layout(self._h, C.byref(pp), None, C.byref(n), C.byref(sw), C.byref(sh)))
        org = np.zeros((n.value, 2), np.int32)
        if n.value:
            _check(_ffi.hip().bling_pass_tile_layout(self._h, C.byref(pp), org.ctypes.data_as(C.POINTER(C.c_int32)),
                                                     C.byref(n), C.byref(sw), C.byref(sh)))
        return org, sw.value, sh.value

    @staticmethod
    def _tiles_buf(buf, capacity):
        """(device pointer, floats it holds) of a tile-image buffer.  A tensor-like buffer (anything
        with data_ptr() and numel(), e.g. a torch tensor) carries its own size (capacity, if given,
        may only lower it); a raw integer pointer must come with its capacity -- the core refuses a
        layout that needs more floats than that (include/bling.h bling_pass_params.tiles_capacity)."""
        if hasattr(buf, "data_ptr") and hasattr(buf, "numel"):
            # the capacity is counted in float32 slots: refuse any other element type (a float16
            # tensor's numel would claim twice the bytes it holds) and host tensors
            dt = getattr(buf, "dtype", None)
            if dt is not None and str(dt) not in ("torch.float32", "float32"):
                raise ValueError(f"tile-image buffer must be float32, got {dt}")
            if hasattr(buf, "is_cuda") and not buf.is_cuda:
                raise ValueError("tile-image buffer must be a device tensor")
            n = int(buf.numel())
            return int(buf.data_ptr()), n if capacity is None else min(n, int(capacity))
        if capacity is None:
            raise ValueError("tiles_capacity is required with a raw device pointer (pass the tensor to size it)")
        return int(buf), int(capacity)

    def render_pass_tiles(self, tiles, seed=DEFAULT_SEED, pass_index=0, shard=(0, 1), tile_stride=1,
                          chunk_paths=0, flags=0, tiles_capacity=None, ordered=False):
        """One pass written as tile images into a device buffer (BLING_PASS_TILE_IMAGES, layout
        tile_layout) instead of a film -- the per-rank half of the multi-GPU merge.  tiles: a device
        tensor, or a raw pointer with tiles_capacity (floats).  ordered=True: the slots hold the ordered
        tile images (BLING_PASS_ORDERED_FILM)."""
        ptr, cap = self._tiles_buf(tiles, tiles_capacity)
        pp = _ffi.PassParams(seed, pass_index, shard[0], shard[1], tile_stride, chunk_paths,
                             flags | _ffi.PASS_TILE_IMAGES | self._ordered(ordered), C.c_void_p(ptr), cap)
        st = _ffi.Stats()
        _check(_ffi.hip().bling_render_pass_device(self._h, C.byref(pp), None, C.byref(st)))
        return st

    def film_add_tiles(self, tiles, film_ptr: int, shard=(0, 1), tile_stride=1, tiles_capacity=None, ordered=False):
        """bling_film_add_tiles: addTile of one shard's tile images into a device film; ordered=True adds
        them per pixel in tile order, without atomics."""
        ptr, cap = self._tiles_buf(tiles, tiles_capacity)
        pp = _ffi.PassParams(0, 0, shard[0], shard[1], tile_stride, 0, self._ordered(ordered), None, cap)
        _check(_ffi.hip().bling_film_add_tiles(self._h, C.byref(pp), C.c_void_p(ptr), C.c_void_p(film_ptr)))

    def film_add_shards(self, tiles_list, film_ptr: int, tile_stride=1, tiles_capacity=None, ordered=False):
        """bling_film_add_shards: every rank's tile images (rank r's buffer tiles_list[r]) into a
        device film in one launch -- rank 0's merge after the gather.  The capacity checked against
        each rank's layout is the smallest buffer's (tensors), or tiles_capacity (raw pointers).
        ordered=True adds the union of all ranks' tiles per pixel in global tile order: with ordered tile
        images the film equals the single-rank ordered film bit for bit."""
        world = len(tiles_list)
        bufs = [self._tiles_buf(b, tiles_capacity) for b in tiles_list]
        pp = _ffi.PassParams(0, 0, 0, world, tile_stride, 0, self._ordered(ordered), None, min(c for _, c in bufs))
        arr = (C.c_void_p * world)(*[C.c_void_p(p) for p, _ in bufs])
        _check(_ffi.hip().bling_film_add_shards(self._h, C.byref(pp), arr, C.c_void_p(film_ptr)))

    # fmt -> (BLING_DEVELOP_*, element type, elements per pixel)
    _DEVELOP = {"rgb_f32": (_ffi.DEVELOP_RGB_F32, "float32", 3), "rgb8": (_ffi.DEVELOP_RGB8, "uint8", 3),
                "rgbe": (_ffi.DEVELOP_RGBE, "uint8", 4)}

    @staticmethod
    def _develop_tensor(buf, what, dtype, numel):
        """Device pointer of a tensor-like buffer (data_ptr() and numel(), as _tiles_buf) after checking
        its element type, its size and that it lives on a device."""
        if not (hasattr(buf, "data_ptr") and hasattr(buf, "numel")):
            raise ValueError(f"develop: {what} must be a device tensor")
        dt = getattr(buf, "dtype", None)
        if dt is not None and str(dt) not in ("torch." + dtype, dtype):
            raise ValueError(f"develop: {what} must be {dtype}, got {dt}")
        if hasattr(buf, "is_cuda") and not buf.is_cuda:
            raise ValueError(f"develop: {what} must be a device tensor")
        if hasattr(buf, "is_contiguous") and not buf.is_contiguous():
            raise ValueError(f"develop: {what} must be contiguous")
        if int(buf.numel()) != numel:
            raise ValueError(f"develop: {what} has {int(buf.numel())} elements, expected {numel}")
        return int(buf.data_ptr())

    def develop(self, film, splat=None, splat_weight=0.0, fmt="rgb8", window=None, out=None):
        """bling_film_develop[_device]: the film (W, X, Y, Z; w * h * 4) and an optional splat image
        (X, Y, Z; w * h * 3) with its weight as a display image, made on the device: fmt "rgb_f32"
        (linear RGB, float32 h x w x 3: getPixel + xyzToRgb), "rgb8" (rgbPixels' bytes, uint8 h x w x 3)
        or "rgbe" (writeRgbe's bytes, uint8 h x w x 4), each equal to the host library's.  window =
        (x0, x1, y0, y1), inclusive and clipped to the image, develops those pixels only and leaves the
        rest of out as it was; None is the whole image.
        A numpy film takes the host variant: film and splat are staged to the device, and only the
        image comes back; returns a numpy array (out, if given: a C-contiguous array of the image's
        element type and size).  A tensor-like film (data_ptr() and numel(), e.g. a torch tensor on
        this context's first device) takes the device variant: splat, if given, and out (required)
        are device tensors too, out is written in place and returned.  The call runs on the
        context's own stream: work of another stream on these tensors must have finished."""
        if fmt not in self._DEVELOP:
            raise ValueError(f"develop: unknown format {fmt!r} (rgb_f32, rgb8, rgbe)")
        code, dtype, per = self._DEVELOP[fmt]
        if self.job is None:
            raise BlingError(-4, "no scene uploaded")   # BLING_ENOSCENE: the image size is the scene's
        w, h = self.job.width, self.job.height
        win =(0, w - 1, 0, h - 1) if window is None else tuple(int(v) for v in window)
        if len(win) != 4:
            raise ValueError("develop: window is (x0, x1, y0, y1)")
        dp = _ffi.DevelopParams(code, float(np.float32(splat_weight)), (C.c_int32 * 4)(*win))
        lib = _ffi.hip()
        if isinstance(film, np.ndarray):
            f = np.ascontiguousarray(film, np.float32).reshape(-1)
            s = None if splat is None else np.ascontiguousarray(splat, np.float32).reshape(-1)
            if self.job is not None and (f.size != w * h * 4 or (s is not None and s.size != w * h * 3)):
                raise ValueError(f"develop: film / splat sizes do not match the {w} x {h} image")
            if out is None:
                out = np.zeros((h, w, per), dtype)
            elif not (isinstance(out, np.ndarray) and out.dtype == np.dtype(dtype) and out.size == w * h * per
                      and out.flags.c_contiguous):
                raise ValueError(f"develop: out must be a C-contiguous {dtype} array of {w * h * per} elements")
            _check(lib.bling_film_develop(self._h, C.byref(dp), _ffi.f32ptr(f), None if s is None else _ffi.f32ptr(s),
                                          C.c_void_p(out.ctypes.data)))
            return out
        fp = self._develop_tensor(film, "film", "float32", w * h * 4)
        sp = None if splat is None else self._develop_tensor(splat, "splat", "float32", w * h * 3)
        if out is None:
            raise ValueError("develop: a device film needs out, a device tensor to write into")
        op = self._develop_tensor(out, "out", dtype, w * h * per)
        _check(lib.bling_film_develop_device(self._h, C.byref(dp), C.c_void_p(fp), C.c_void_p(sp), C.c_void_p(op)))
        return out

    def trace(self, rays_soa: np.ndarray, any_hit: bool = False):
        """Scene.scIntersect / Scene.occluded for a batch of rays (8 x n SoA)."""
        rays_soa = np.ascontiguousarray(rays_soa, np.float32)
        n = rays_soa.shape[1]
        t = np.zeros(n, np.float32)
        prim = np.zeros(n, np.uint32)
        bary = np.zeros(2 * n, np.float32)
        _check(_ffi.hip().bling_trace(self._h, _ffi.f32ptr(rays_soa), n, 1 if any_hit else 0, _ffi.f32ptr(t),
                                      _ffi.u32ptr(prim), _ffi.f32ptr(bary)))
        return t, prim, bary.reshape(n, 2)

    def sample_li(self, samples: np.ndarray, seed=DEFAULT_SEED, pass_index=0):
        """Per-sample Path.li on the device; samples = int32 (k, 3) of (x, y, n)."""
        samples = np.ascontiguousarray(samples, np.int32)
        n = samples.shape[0]
        L = np.zeros((n, 16), np.float32)
        img = np.zeros((n, 2), np.float32)
        st = _ffi.Stats()
        lib = _ffi.hip()
        lib.bling_sample_li.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.c_size_t,
                                        _ffi.c_f32p, _ffi.c_f32p, C.POINTER(_ffi.Stats)]
        _check(lib.bling_sample_li(self._h, seed, pass_index, samples.ctypes.data_as(C.POINTER(C.c_int32)), n,
                                   _ffi.f32ptr(L), _ffi.f32ptr(img), C.byref(st)))
        return L, img, st

    def surface_li(self, rays, ids, seed=DEFAULT_SEED, pass_index=0, out=None):
        """bling_surface_li_device: the uploaded scene's integrator (path, directLighting or debug normals) along
        the caller's rays, without a host copy.  rays: a float32 tensor (7, n) on this context's first device --
        the planes ox, oy, oz, dx, dy, dz, tmin; tmax is infinite and the direction is used as given.  ids: an
        int32 or uint32 tensor (n, 2) of (pixel, n): the ray draws from the stream of sample n of stream `pixel`
        (the built-in camera's, for extent pixel (ix, iy): pixel = (iy - ey0) * ext_w + (ix - ex0)).  Returns
        (L, LiStats): L a float32 device tensor (n, 16) -- out, if given -- in the layout Image.add_samples and
        Image.add_windowed take as spectra.  A ray with a NaN or infinite float (tmin = +inf excepted), a zero
        direction or n >= spp is dropped: zeros, counted in LiStats.dropped.  The call runs on the context's own
        stream and returns after completion: work of another stream on the tensors must have finished."""
        import torch
        dev = f"cuda:{self.device}"
        id_types = (torch.int32,) + ((torch.uint32,) if hasattr(torch, "uint32") else ())
        for t, what, types in ((rays, "rays", (torch.float32,)), (ids, "ids", id_types)):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == self.device and t.dtype in types
                    and t.is_contiguous()):
                raise ValueError(f"surface_li: {what} must be a contiguous {' or '.join(str(d) for d in types)} tensor on {dev}")
        if rays.dim() != 2 or rays.shape[0] != 7:
            raise ValueError(f"surface_li: rays must be (7, n), got {tuple(rays.shape)}")
        n = int(rays.shape[1])
        if ids.dim() != 2 or tuple(ids.shape) != (n, 2):
            raise ValueError(f"surface_li: ids must be ({n}, 2), got {tuple(ids.shape)}")
        if out is None:
            out = torch.empty((n, 16), dtype=torch.float32, device=dev)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.device.index == self.device and out.dtype == torch.float32
                  and out.is_contiguous() and out.numel() == n * 16):
            raise ValueError(f"surface_li: out must be a contiguous float32 tensor of {n * 16} elements on {dev}")
        torch.cuda.synchronize(self.device)
        st = _ffi.LiStats()
        _check(_ffi.hip().bling_surface_li_device(self._h, seed, pass_index, C.c_void_p(rays.data_ptr() if n else None),
                                                  C.c_void_p(ids.data_ptr() if n else None), n,
                                                  C.c_void_p(out.data_ptr() if n else None), C.byref(st)))
        return out, st

    def host_surface_li(self, rays: np.ndarray, ids: np.ndarray, seed=DEFAULT_SEED, pass_index=0):
        """bling_surface_li: surface_li for numpy arrays -- rays float32 (7, n), ids (n, 2) of (pixel, n) --
        staged through device buffers the context owns.  Returns (L (n, 16) float32, LiStats)."""
        rays = np.ascontiguousarray(rays, np.float32)
        if rays.ndim != 2 or rays.shape[0] != 7:
            raise ValueError(f"host_surface_li: rays must be (7, n), got {rays.shape}")
        n = rays.shape[1]
        ids = np.ascontiguousarray(np.asarray(ids).astype(np.uint32, copy=False)).reshape(-1, 2)
        if len(ids) != n:
            raise ValueError(f"host_surface_li: {n} rays but {len(ids)} id pairs")
        L = np.zeros((n, 16), np.float32)
        st = _ffi.LiStats()
        _check(_ffi.hip().bling_surface_li(self._h, seed, pass_index, _ffi.f32ptr(rays) if n else None,
                                           _ffi.u32ptr(ids) if n else None, n, _ffi.f32ptr(L) if n else None, C.byref(st)))
        return L, st

    def camera_samples(self, windows, seed=DEFAULT_SEED, pass_index=0, counts_or_first=None, out=None):
        """bling_camera_samples_device: the uploaded scene's sampler and camera over the SampleWindows
        (x0, x1, y0, y1), ends inclusive -- window k's pixels y outer, x inner, n innermost in slots
        first[k] .. first[k+1]-1.  counts_or_first: the windows' sample counts or the n_windows + 1 offsets; None
        derives them from the windows and the job's spp.  Returns (xy, ids, rays, lens, CameraStats) as torch
        tensors on this context's first device: xy (n, 2) float32 as Image.add_windowed takes it, ids (n, 2) int32
        and rays (7, n) float32 as surface_li takes them, lens (n, 2) float32.  out: a dict naming some of "xy",
        "ids", "rays", "lens" -- a tensor to write into, or False to leave that output out (it is returned as
        None); outputs not named are allocated.  Only the windows and offsets go from the host to the device.
        The call runs on the context's own stream and returns after completion."""
        import torch
        if self.job is None:
            raise BlingError(-4, "no scene uploaded")
        dev = f"cuda:{self.device}"
        arr, first, nw = camera_windows(windows, self.job.spp, counts_or_first)
        n = int(first[-1])
        shapes = {"xy": ((n, 2), torch.float32), "ids": ((n, 2), torch.int32), "rays": ((7, n), torch.float32),
                  "lens": ((n, 2), torch.float32)}
        out = dict(out or {})
        if set(out) - set(CAMERA_OUTPUTS):
            raise ValueError(f"camera_samples: out names {sorted(set(out) - set(CAMERA_OUTPUTS))}, not among {CAMERA_OUTPUTS}")
        bufs = {}
        for k, (shape, dt) in shapes.items():
            t = out.get(k)
            if t is False:
                bufs[k] = None
            elif t is None:
                bufs[k] = torch.empty(shape, dtype=dt, device=dev)
            else:
                types = (dt, torch.uint32) if k == "ids" and hasattr(torch, "uint32") else (dt,)
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == self.device and t.dtype in types
                        and t.is_contiguous() and t.numel() == shape[0] * shape[1]):
                    raise ValueError(f"camera_samples: out[{k!r}] must be a contiguous {dt} tensor of {shape[0] * shape[1]} elements on {dev}")
                bufs[k] = t
        torch.cuda.synchronize(self.device)
        st = _ffi.CameraStats()
        ptr = [C.c_void_p(bufs[k].data_ptr() if bufs[k] is not None and n else None) for k in CAMERA_OUTPUTS]
        _check(_ffi.hip().bling_camera_samples_device(self._h, seed, pass_index, arr, first.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                      nw, *ptr, C.byref(st)))
        return bufs["xy"], bufs["ids"], bufs["rays"], bufs["lens"], st

    def host_camera_samples(self, windows, seed=DEFAULT_SEED, pass_index=0, counts_or_first=None, outputs=CAMERA_OUTPUTS):
        """bling_host_camera_samples of the uploaded job: camera_samples on the CPU through libbling_host, as numpy
        arrays (xy, ids, rays, lens); see the module's host_camera_samples, which needs no context."""
        if self.job is None:
            raise BlingError(-4, "no scene uploaded")
        return host_camera_samples(self.job, windows, seed, pass_index, counts_or_first, outputs)

    def render_pass_by_seams(self, image, windows, seed=DEFAULT_SEED, pass_index=0):
        """One sampler-renderer pass as three device calls: camera_samples -> surface_li -> image.add_windowed
        (a bling_amd.image.Image that shares this context).  With splitWindow's windows of the extent the film
        equals render_pass(ordered=True)'s bit for bit.  Returns (CameraStats, LiStats, ImageStats)."""
        if self.job is None:
            raise BlingError(-4, "no scene uploaded")
        _, first, _ = camera_windows(windows, self.job.spp)
        xy, ids, rays, _, cst = self.camera_samples(windows, seed, pass_index, first, out={"lens": False})
        L, lst = self.surface_li(rays, ids, seed, pass_index)
        ist = image.add_windowed(windows, first, xy, L, "add")
        return cst, lst, ist

    def set_li_chunk(self, max_rays=0):
        """bling_debug_set_li_chunk: the rays per wave of surface_li / host_surface_li (0: the default)."""
        _check(_ffi.hip().bling_debug_set_li_chunk(self._h, int(max_rays)))

    def bidir_terms(self, samples: np.ndarray, seed=DEFAULT_SEED, pass_index=0):
        """bling_debug_bidir_terms: (terms (k, 3, 16) = ld, le, l of BidirPath's contrib, lens (k, 4) =
        eye length, light length, eye and light specular masks) of the (x, y, n) samples."""
        samples = np.ascontiguousarray(samples, np.int32)
        n = samples.shape[0]
        terms = np.zeros((n, 3, 16), np.float32)
        lens = np.zeros((n, 4), np.int32)
        lib = _ffi.hip()
        _check(lib.bling_debug_bidir_terms(self._h, seed, pass_index, samples.ctypes.data_as(C.POINTER(C.c_int32)), n,
                                           _ffi.f32ptr(terms), lens.ctypes.data_as(C.POINTER(C.c_int32))))
        return terms, lens

    def sample_li_vertices(self, samples: np.ndarray, seed=DEFAULT_SEED, pass_index=0):
        """sample_li plus the per-vertex debug records (include/bling.h BLING_DV_*): (L (k, 16),
        vtx (k, 16, 32)).  Needs the BLING_DEBUG_VERTEX build (BLING_HIP_VARIANT=dbg); the product
        library raises BlingError(BLING_EUNSUPPORTED)."""
        samples = np.ascontiguousarray(samples, np.int32)
        n = samples.shape[0]
        L = np.zeros((n, 16), np.float32)
        vtx = np.zeros((n, 16, 32), np.float32)
        lib = _ffi.hip()
        lib.bling_sample_li_vertices.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.c_size_t,
                                                 _ffi.c_f32p, _ffi.c_f32p]
        _check(lib.bling_sample_li_vertices(self._h, seed, pass_index, samples.ctypes.data_as(C.POINTER(C.c_int32)), n,
                                            _ffi.f32ptr(L), _ffi.f32ptr(vtx)))
        return L, vtx

    def sppm_pass(self, seed=DEFAULT_SEED, pass_index=1, film: np.ndarray | None = None,
                  splat: np.ndarray | None = None):
        """One SPPM onePass (Renderer/SPPM.hs:424-460) into host film (W,X,Y,Z) and splat (X,Y,Z)
        buffers, both accumulated.  Returns (film, splat, SppmStats)."""
        job = self.job
        if film is None:
            film = np.zeros(job.width * job.height * 4, np.float32)
        if splat is None:
            splat = np.zeros(job.width * job.height * 3, np.float32)
        st = _ffi.SppmStats()
        _check(_ffi.hip().bling_sppm_pass(self._h, seed, pass_index, _ffi.f32ptr(film), _ffi.f32ptr(splat),
                                          C.byref(st)))
        return film, splat, st

    def sppm_pixel_stats(self):
        """(psR2, psN) over the sample extent in sIdx order."""
        n = C.c_size_t()
        _check(_ffi.hip().bling_sppm_pixel_stats(self._h, None, None, C.byref(n)))
        r2 = np.zeros(n.value, np.float32)
        nn = np.zeros(n.value, np.float32)
        _check(_ffi.hip().bling_sppm_pixel_stats(self._h, _ffi.f32ptr(r2), _ffi.f32ptr(nn), C.byref(n)))
        return r2, nn

    def sppm_hitpoints(self):
        """bling_debug_sppm_hitpoints: (pos_r2 (n, 4) float32, keys (n,) uint64) of the last SPPM pass."""
        n = C.c_size_t()
        _check(_ffi.hip().bling_debug_sppm_hitpoints(self._h, None, None, 0, C.byref(n)))
        pos = np.zeros((n.value, 4), np.float32)
        keys = np.zeros(n.value, np.uint64)
        _check(_ffi.hip().bling_debug_sppm_hitpoints(self._h, _ffi.f32ptr(pos.reshape(-1)),
                                                     keys.ctypes.data_as(C.POINTER(C.c_uint64)), n.value, C.byref(n)))
        return pos, keys

    def sppm_buckets(self):
        """bling_debug_sppm_buckets: (bstart, items, mr) of the last SPPM pass's kd-tree buckets."""
        nb, ni = C.c_size_t(), C.c_size_t()
        _check(_ffi.hip().bling_debug_sppm_buckets(self._h, None, None, None, 0, 0, C.byref(nb), C.byref(ni)))
        bs = np.zeros(nb.value, np.uint32); it = np.zeros(ni.value, np.uint32); mr = np.zeros(ni.value, np.float32)
        u32 = C.POINTER(C.c_uint32)
        _check(_ffi.hip().bling_debug_sppm_buckets(self._h, bs.ctypes.data_as(u32), it.ctypes.data_as(u32), _ffi.f32ptr(mr),
                                                   nb.value, ni.value, C.byref(nb), C.byref(ni)))
        return bs, it, mr

    def sppm_reset(self):
        _check(_ffi.hip().bling_sppm_reset(self._h))

    def light_pass(self, seed=DEFAULT_SEED, pass_index=1, splat: np.ndarray | None = None):
        """One light tracer pass (Renderer/LightTracer.hs:41-52) into a host splat image (X,Y,Z),
        accumulated.  Returns (splat, LightStats)."""
        job = self.job
        if splat is None:
            splat = np.zeros(job.width * job.height * 3, np.float32)
        st = _ffi.LightStats()
        _check(_ffi.hip().bling_light_pass(self._h, seed, pass_index, _ffi.f32ptr(splat), C.byref(st)))
        return splat, st

    def light_records(self, seed=DEFAULT_SEED, pass_index=1, first_photon=0, n_photons=None, cap=None):
        """bling_debug_light_records: the splats of a range of the pass's photons as a structured
        array (photon, depth, sx, sy, x, y, z, pad), sorted by (photon, depth).  Without cap the
        buffer is sized by a first counting call; a given cap that is too small raises."""
        if n_photons is None:
            n_photons = self.job.light.pass_photons - first_photon
        lib = _ffi.hip()
        n = C.c_size_t()
        if cap is None:
            rc = lib.bling_debug_light_records(self._h, seed, pass_index, first_photon, n_photons, None, 0, C.byref(n))
            if rc != 0 and n.value == 0:
                _check(rc)
            cap = n.value
        rec = np.zeros(cap, LIGHT_RECORD)
        _check(lib.bling_debug_light_records(self._h, seed, pass_index, first_photon, n_photons,
                                             rec.ctypes.data_as(C.POINTER(_ffi.LightRecord)), cap, C.byref(n)))
        return rec[:n.value]

    def mlt_pass(self, seed=DEFAULT_SEED, pass_index=1, splat: np.ndarray | None = None):
        """One pass of the Metropolis renderer (Renderer/Metropolis.hs:76-120) into a host splat image
        (X,Y,Z), accumulated.  Returns (splat, MltStats); MltStats.b is the pass's b'."""
        job = self.job
        if splat is None:
            splat = np.zeros(job.width * job.height * 3, np.float32)
        st = _ffi.MltStats()
        _check(_ffi.hip().bling_mlt_pass(self._h, seed, pass_index, _ffi.f32ptr(splat), C.byref(st)))
        return splat, st

    def mlt_records(self, seed=DEFAULT_SEED, pass_index=1, first_chain=0, n_chains=None, cap=None):
        """bling_debug_mlt_records: (records sorted by (chain, mutation), the chains' start samples, b').
        Without cap the buffer is sized by a first counting call; a given cap that is too small raises."""
        if n_chains is None:
            n_chains = self.job.metropolis.chains - first_chain
        lib = _ffi.hip()
        n = C.c_size_t()
        if cap is None:
            rc = lib.bling_debug_mlt_records(self._h, seed, pass_index, first_chain, n_chains, None, 0, C.byref(n), None, None)
            if rc != 0 and n.value == 0:
                _check(rc)
            cap = n.value
        rec = np.zeros(cap, MLT_RECORD)
        starts = np.zeros(n_chains, np.uint32)
        b = np.zeros(1, np.float32)
        _check(lib.bling_debug_mlt_records(self._h, seed, pass_index, first_chain, n_chains,
                                           rec.ctypes.data_as(C.POINTER(_ffi.MltRecord)), cap, C.byref(n),
                                           _ffi.u32ptr(starts), _ffi.f32ptr(b)))
        return rec[:n.value], starts, np.float32(b[0])

    def _splat_tensor(self, splat):
        """Device pointer of a splat image tensor (float32, w * h * 3, contiguous, on a device), checked as
        develop checks its buffers; BlingError(-4) without a scene, as the size is the scene's."""
        if self.job is None:
            raise BlingError(-4, "no scene uploaded")
        return self._develop_tensor(splat, "splat", "float32", self.job.width * self.job.height * 3)

    def light_pass_device(self, splat, seed=DEFAULT_SEED, pass_index=1, ordered=False, flags=None):
        """bling_light_pass_device: one light tracer pass accumulated into a device splat image (a float32
        tensor of w * h * 3 elements on this context's first device), which never visits the host.
        ordered=True adds every pixel's splats one at a time in (photon, depth) order (BLING_SPLAT_ORDERED):
        the same bits on every run, equal to the CPU restatement's image.  Returns LightStats."""
        ptr = self._splat_tensor(splat)
        st = _ffi.LightStats()
        fl = (_ffi.SPLAT_ORDERED if ordered else 0) if flags is None else int(flags)
        _check(_ffi.hip().bling_light_pass_device(self._h, seed, pass_index, fl, C.c_void_p(ptr), C.byref(st)))
        return st

    def mlt_pass_device(self, splat, seed=DEFAULT_SEED, pass_index=1, ordered=False, flags=None):
        """bling_mlt_pass_device: one Metropolis pass accumulated into a device splat image, as
        light_pass_device; ordered=True adds in (chain, mutation, current before proposal) order.
        Returns MltStats."""
        ptr = self._splat_tensor(splat)
        st = _ffi.MltStats()
        fl = (_ffi.SPLAT_ORDERED if ordered else 0) if flags is None else int(flags)
        _check(_ffi.hip().bling_mlt_pass_device(self._h, seed, pass_index, fl, C.c_void_p(ptr), C.byref(st)))
        return st

    def sppm_pass_device(self, film, splat, seed=DEFAULT_SEED, pass_index=1, ordered=False, flags=None):
        """bling_sppm_pass_device: one SPPM pass accumulated into a device film (float32, w * h * 4: W, X, Y, Z)
        and a device splat image (float32, w * h * 3), which never visit the host; either may be None and is then
        not produced.  ordered=True forms both in the reference's order without float atomics
        (BLING_SPLAT_ORDERED): the same bits on every run.  Returns SppmStats."""
        if self.job is None:
            raise BlingError(-4, "no scene uploaded")
        fptr = None if film is None else self._develop_tensor(film, "film", "float32", self.job.width * self.job.height * 4)
        sptr = None if splat is None else self._splat_tensor(splat)
        st = _ffi.SppmStats()
        fl = (_ffi.SPLAT_ORDERED if ordered else 0) if flags is None else int(flags)
        _check(_ffi.hip().bling_sppm_pass_device(self._h, seed, pass_index, fl, C.c_void_p(fptr), C.c_void_p(sptr), C.byref(st)))
        return st

    def sppm_records(self, seed=DEFAULT_SEED, pass_index=1, thread=0, first_photon=0, n_photons=None, cap=None):
        """bling_debug_sppm_records: the splats of a range of one photon sampler's photons as a structured array
        (thread, photon, seq, depth, sx, sy, x, y, z, pad), sorted by (photon, seq), from an eye pass of the call's
        own for the context's current radii.  Without cap the buffer is sized by a first counting call; a given cap
        that is too small raises."""
        if n_photons is None:
            cfg = self.job.config
            threads = max(1, cfg.sppm_threads)
            sn = max(1, int(np.ceil(np.sqrt(np.float32(cfg.sppm_photons) / np.float32(threads)))))
            n_photons = sn * sn - first_photon
        lib = _ffi.hip()
        n = C.c_size_t()
        if cap is None:
            rc = lib.bling_debug_sppm_records(self._h, seed, pass_index, thread, first_photon, n_photons, None, 0, C.byref(n))
            if rc != 0 and n.value == 0:
                _check(rc)
            cap = n.value
        rec = np.zeros(cap, SPPM_RECORD)
        _check(lib.bling_debug_sppm_records(self._h, seed, pass_index, thread, first_photon, n_photons,
                                            rec.ctypes.data_as(C.POINTER(_ffi.SppmRecord)), cap, C.byref(n)))
        return rec[:n.value]

    def splat_merge(self, records, splat):
        """bling_debug_splat_merge: the ordered merge alone, of a SPLAT_REC array into a device splat image."""
        rec = np.ascontiguousarray(records, SPLAT_REC)
        ptr = self._splat_tensor(splat)
        _check(_ffi.hip().bling_debug_splat_merge(self._h, C.c_void_p(rec.ctypes.data) if len(rec) else None, len(rec),
                                                  C.c_void_p(ptr)))

    def set_splat_budget(self, max_records=0):
        """bling_debug_set_splat_budget: the record budget of this context's ordered passes (0: the default)."""
        _check(_ffi.hip().bling_debug_set_splat_budget(self._h, int(max_records)))

    def splat_times(self):
        """bling_debug_splat_times: (ms in the photon / chain launches, ms in the merges) of the last ordered pass."""
        a, b = C.c_double(), C.c_double()
        _check(_ffi.hip().bling_debug_splat_times(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def mlt_set_boot(self, values=None):
        """bling_debug_mlt_set_boot: bootstrap contributions that replace the evaluated ones (None: off)."""
        v = np.zeros(0, np.float32) if values is None else np.ascontiguousarray(values, np.float32)
        _check(_ffi.hip().bling_debug_mlt_set_boot(self._h, _ffi.f32ptr(v) if len(v) else None, len(v)))

    def close(self):
        if self._h:
            _ffi.hip().bling_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------- Renderer interface
@dataclass
class Progress:
    kind: str                     # "Started" | "PassDone"
    pass_num: int = 0
    film: np.ndarray | None = None
    stats: dict = field(default_factory=dict)


class SamplerRenderer:
    """``SamplerRenderer`` with the path integrator (Rendering.hs:111-140) on the MI355X core."""

    def __init__(self, device: int = 0, seed: int = DEFAULT_SEED, ordered: bool = False):
        self.device = device
        self.seed = seed
        self.ordered = ordered       # BLING_PASS_ORDERED_FILM on every pass

    def render(self, job: Job, report) -> np.ndarray:
        """Passes 1, 2, ... through bling_render (the core's own pass loop) until the reporter
        returns False; each PassDone carries the accumulated film."""
        ctx = Context(self.device)
        ctx.upload(job)
        report(Progress("Started"))
        film, _ = ctx.render_loop(lambda p, f, st: bool(report(Progress("PassDone", p, f, st))), seed=self.seed,
                                  first_pass=1, ordered=self.ordered)
        ctx.close()
        return film


class SPPMRenderer:
    """``instance Renderer SPPM`` (Renderer/SPPM.hs:466-480) on the MI355X core: passes 1, 2, ...
    until the reporter returns False; each PassDone carries the film, the photon splat and the
    splat weight 1 / (threads * pass * sn^2) that getPixel applies (:460)."""

    def __init__(self, device: int = 0, seed: int = DEFAULT_SEED):
        self.device = device
        self.seed = seed

    def render(self, job: Job, report):
        cfg = job.config
        threads = max(1, cfg.sppm_threads)
        sn = max(1, int(np.ceil(np.sqrt(np.float32(cfg.sppm_photons) / np.float32(threads)))))
        ctx = Context(self.device)
        ctx.upload(job)
        film = np.zeros(job.width * job.height * 4, np.float32)
        splat = np.zeros(job.width * job.height * 3, np.float32)
        report(Progress("Started"))
        p = 1
        while True:
            film, splat, st = ctx.sppm_pass(seed=self.seed, pass_index=p, film=film, splat=splat)
            info = st.as_dict()
            info["splat"] = splat
            info["splat_weight"] = 1.0 / (threads * p * sn * sn)
            if not report(Progress("PassDone", p, film, info)):
                break
            p += 1
        ctx.close()
        return film, splat


def _device_splat(job: Job, device: int):
    """A zeroed splat image (w * h * 3 float32) on the device, as a torch tensor."""
    import torch
    return torch.zeros(job.width * job.height * 3, dtype=torch.float32, device=f"cuda:{device}")


class LightTracerRenderer:
    """``instance Renderer LightTracer`` (Renderer/LightTracer.hs:37-52) on the MI355X core: passes
    1, 2, ... until the reporter returns False; each PassDone carries the (empty) film, the
    accumulated splat image and the splat weight 1 / (pass * passPhotons) of `PassDone n img'` (:50).
    device_film keeps the splat image in a device tensor for the whole run (PassDone then carries that
    tensor, and render returns it); ordered adds the splats in the reference's order (BLING_SPLAT_ORDERED)
    and implies a device image during the passes -- without device_film it comes back as a numpy array."""

    def __init__(self, device: int = 0, seed: int = DEFAULT_SEED, ordered: bool = False, device_film: bool = False):
        self.device = device
        self.seed = seed
        self.ordered = ordered
        self.device_film = device_film

    def render(self, job: Job, report):
        ppp = job.light.pass_photons
        ctx = Context(self.device)
        ctx.upload(job)
        film = np.zeros(job.width * job.height * 4, np.float32)
        on_device = self.ordered or self.device_film
        splat = _device_splat(job, self.device) if on_device else np.zeros(job.width * job.height * 3, np.float32)
        report(Progress("Started"))
        p = 1
        while True:
            if on_device:
                st = ctx.light_pass_device(splat, seed=self.seed, pass_index=p, ordered=self.ordered)
            else:
                splat, st = ctx.light_pass(seed=self.seed, pass_index=p, splat=splat)
            info = st.as_dict()
            info["splat"] = splat if self.device_film or not on_device else splat.cpu().numpy()
            info["splat_weight"] = 1.0 / (p * ppp)
            if not report(Progress("PassDone", p, film, info)):
                break
            p += 1
        ctx.close()
        return film, splat if self.device_film or not on_device else splat.cpu().numpy()


class MetropolisRenderer:
    """``instance Renderer Metropolis`` (Renderer/Metropolis.hs:59-120) on the MI355X core: passes 1, 2,
    ... until the reporter returns False; each PassDone carries the (empty) film, the accumulated splat
    image and the splat weight bnext / p of `PassDone p img' (bnext / p)` (:115-117).  ordered and
    device_film as LightTracerRenderer's."""

    def __init__(self, device: int = 0, seed: int = DEFAULT_SEED, ordered: bool = False, device_film: bool = False):
        self.device = device
        self.seed = seed
        self.ordered = ordered
        self.device_film = device_film

    def render(self, job: Job, report):
        from .film import mlt_bnext
        ctx = Context(self.device)
        ctx.upload(job)
        film = np.zeros(job.width * job.height * 4, np.float32)
        on_device = self.ordered or self.device_film
        splat = _device_splat(job, self.device) if on_device else np.zeros(job.width * job.height * 3, np.float32)
        report(Progress("Started"))
        p, b = 1, np.float32(1)
        while True:
            if on_device:
                st = ctx.mlt_pass_device(splat, seed=self.seed, pass_index=p, ordered=self.ordered)
            else:
                splat, st = ctx.mlt_pass(seed=self.seed, pass_index=p, splat=splat)
            b = mlt_bnext(p, b, st.b)
            info = st.as_dict()
            info["splat"] = splat if self.device_film or not on_device else splat.cpu().numpy()
            info["splat_weight"] = float(np.float32(b / np.float32(p)))
            if not report(Progress("PassDone", p, film, info)):
                break
            p += 1
        ctx.close()
        return film, splat if self.device_film or not on_device else splat.cpu().numpy()


RENDERER_LIGHT = 3   # BLING_RENDERER_LIGHT (include/bling_scene.h)
RENDERER_METROPOLIS = 4   # BLING_RENDERER_METROPOLIS


def render(job: Job, passes: int = 1, device: int = 0, seed: int = DEFAULT_SEED, ordered: bool = False) -> np.ndarray:
    """Render `passes` progressive passes (the commented bling CLI harness renders exactly one,
    src/cmdline/Main.hs:15-26).  A sampler job returns its film (W, X, Y, Z); a `light` job, which
    only splats, returns the RGB image (h, w, 3) of its accumulated splats with the weight
    1 / (passes * passPhotons).  ordered: the sampler renderer's ordered film (the splat renderers have
    their own switch and ignore it)."""
    count = {"n": 0}

    def rep(pr: Progress) -> bool:
        if pr.kind == "PassDone":
            count["n"] += 1
            return count["n"] < passes
        return True

    if job.config.renderer == RENDERER_LIGHT:
        from .scene import film_splat_to_rgb
        film, splat = LightTracerRenderer(device, seed).render(job, rep)
        sw = np.float32(1.0) / np.float32(count["n"] * job.light.pass_photons)
        return film_splat_to_rgb(film, splat, sw, job.width, job.height)
    if job.config.renderer == RENDERER_METROPOLIS:
        from .scene import film_splat_to_rgb
        last = {}

        def rep_mlt(pr: Progress) -> bool:
            if pr.kind == "PassDone":
                last["sw"] = pr.stats["splat_weight"]
            return rep(pr)

        film, splat = MetropolisRenderer(device, seed).render(job, rep_mlt)
        return film_splat_to_rgb(film, splat, np.float32(last["sw"]), job.width, job.height)
    return SamplerRenderer(device, seed, ordered).render(job, rep)
