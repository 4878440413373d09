"""bling on the MI355X: the HIP core (render.py) and the host loader (scene.py) behind ctypes (_ffi.py)."""


class LbvhDepthError(ValueError):
    """host_lbvh: the linear BVH is deeper than the cap; .depth holds its depth."""

    def __init__(self, depth, cap):
        super().__init__(f"linear BVH of depth {depth} exceeds the cap {cap}")
        self.depth = depth


def host_lbvh(boxes, refs, depth_cap=0, with_keys=False):
    """bling_host_lbvh (include/bling_host.h): the device BVH builder's algorithm on the CPU, no context and no
    GPU.  boxes: (n, 6) or (n, 2, 3) float32 (lo, hi); refs: n uint32.  Returns (nodes (m, 16) float32, refs in
    sorted order, info dict), with the n sorted keys (uint64) as a fourth item if with_keys.  LbvhDepthError for a
    tree deeper than depth_cap (0: 31), ValueError for what the library refuses."""
    import ctypes as C

    import numpy as np

    from . import _ffi
    b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
    r = np.ascontiguousarray(refs, np.uint32).reshape(-1)
    n = len(r)
    if len(b) != n:
        raise ValueError(f"{len(b)} boxes but {n} refs")
    nodes = np.zeros((max(1, n - 1), 16), np.float32)
    refs_out = np.zeros(n, np.uint32)
    keys = np.zeros(n, np.uint64)
    info = _ffi.LbvhInfo()
    rc = _ffi.host().bling_host_lbvh(_ffi.f32ptr(b), _ffi.u32ptr(r), n, int(depth_cap), _ffi.f32ptr(nodes), _ffi.u32ptr(refs_out),
                                     keys.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(info))
    if rc == -2:
        raise LbvhDepthError(int(info.depth), int(depth_cap) or 31)
    if rc != 0:
        raise ValueError("bling_host_lbvh: a bad argument (3 <= n <= 2^24 items, depth_cap in 0 .. 31)")
    d = {k: int(getattr(info, k)) for k, _ in info._fields_}
    out = (nodes[:d["nodes"]].copy(), refs_out, d)
    return out + (keys,) if with_keys else out


def host_bvh4(nodes):
    """bling_host_bvh4 (include/bling.h): the host's collapse of a BVH2 ((n, 16) float32, as Context.bvh() and
    host_lbvh return it) into the BVH4, no context and no GPU.  Returns (nodes4 (m, 28) float32, {"depth",
    "stack_need"}).  render.BlingError for a BVH2 whose links form no tree."""
    import ctypes as C

    import numpy as np

    from . import _ffi
    from .render import _check
    n2 = np.ascontiguousarray(nodes, np.float32).reshape(-1, 16)
    out = np.zeros((len(n2), 28), np.float32)
    n4, depth, need = C.c_size_t(), C.c_int(), C.c_int()
    _check(_ffi.hip().bling_host_bvh4(_ffi.f32ptr(n2), len(n2), _ffi.f32ptr(out), len(out), C.byref(n4), C.byref(depth), C.byref(need)))
    return out[:int(n4.value)].copy(), {"depth": int(depth.value), "stack_need": int(need.value)}


def host_threaded(nodes):
    """bling_host_threaded (include/bling.h): the host's threaded entry list of a BVH2, (e, 8) float32."""
    import ctypes as C

    import numpy as np

    from . import _ffi
    from .render import _check
    n2 = np.ascontiguousarray(nodes, np.float32).reshape(-1, 16)
    out = np.zeros((2 * len(n2), 8), np.float32)
    ne = C.c_size_t()
    _check(_ffi.hip().bling_host_threaded(_ffi.f32ptr(n2), len(n2), _ffi.f32ptr(out), len(out), C.byref(ne)))
    return out[:int(ne.value)].copy()


def scene_plan(job) -> dict:
    """bling_debug_scene_plan (include/bling.h): the acceleration / kernel plan an upload of the job would settle
    with the host builder -- Context.scene_info()'s dict -- from the description alone, no context and no GPU.
    render.BlingError for a description bling_scene_validate refuses."""
    import ctypes as C
    import json

    from . import _ffi
    from .render import _check
    buf = C.create_string_buffer(1024)
    _check(_ffi.hip().bling_debug_scene_plan(C.c_void_p(job.desc), buf, len(buf), None))
    return json.loads(buf.value.decode())
