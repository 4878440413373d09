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
