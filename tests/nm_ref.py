"""ctypes wrapper of the normal-map integrator's CPU restatement (tests/ref/normals_ref.cpp) -- test
infrastructure only, loaded by tests the way bd_ref loads the bidirectional integrator's.  The library
(tests/ref/_build/libnm_ref.so) is built by ``make nmref`` (part of ``make all``)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(HERE, "ref", "_build", "libnm_ref.so")
f32p = C.POINTER(C.c_float)
i32p = C.POINTER(C.c_int)


class RefStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("samples", "hits", "dropped")]


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            subprocess.check_call(["make", "nmref"], cwd=ROOT)
        L = C.CDLL(LIB)
        L.oracle_build.argtypes = [C.c_void_p]
        L.oracle_build.restype = C.c_void_p
        L.oracle_free.argtypes = [C.c_void_p]
        L.nm_ref_colour.argtypes = [f32p, f32p]
        L.nm_ref_colour.restype = None
        L.nm_ref_sample_li.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, i32p, C.c_size_t, f32p, f32p, f32p, C.c_int,
                                       C.POINTER(RefStats)]
        L.nm_ref_render.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, f32p,
                                    C.POINTER(RefStats)]
        _lib = L
    return _lib


def colour(n) -> np.ndarray:
    """intToSpectrum of one normal: rgbToSpectrumRefl ((1 + n) / 2), 16 floats."""
    v = np.ascontiguousarray(n, np.float32).reshape(3)
    out = np.zeros(16, np.float32)
    lib().nm_ref_colour(v.ctypes.data_as(f32p), out.ctypes.data_as(f32p))
    return out


def all_samples(job) -> np.ndarray:
    """Every (x, y, n) sample of the job's sample extent, in scanline order."""
    x0, x1, y0, y1 = job.extent()
    ys, xs, ns = np.meshgrid(np.arange(y0, y1 + 1), np.arange(x0, x1 + 1), np.arange(job.spp), indexing="ij")
    return np.stack([xs.ravel(), ys.ravel(), ns.ravel()], 1).astype(np.int32)


class NormalsRef:
    """The restatement over one parsed Job (which must outlive it)."""

    def __init__(self, job):
        self.job = job
        self._h = lib().oracle_build(C.c_void_p(job.desc))

    def sample_li(self, samples, seed, pass_index=0, threads=0):
        """(L (n, 16), img (n, 2), geo (n, 7) = hit, shading normal, geometric normal, RefStats) of the
        (x, y, n) samples."""
        s = np.ascontiguousarray(samples, np.int32).reshape(-1, 3)
        n = len(s)
        L = np.zeros((n, 16), np.float32)
        img = np.zeros((n, 2), np.float32)
        geo = np.zeros((n, 7), np.float32)
        st = RefStats()
        rc = lib().nm_ref_sample_li(self._h, seed, pass_index, s.ctypes.data_as(i32p), n, L.ctypes.data_as(f32p),
                                    img.ctypes.data_as(f32p), geo.ctypes.data_as(f32p), threads, C.byref(st))
        assert rc == 0
        return L, img, geo, st

    def render(self, seed, pass_index=0, film=None, shard_rank=0, shard_world=1, threads=0):
        """One pass into film (h * w * 4, accumulated): (film, RefStats)."""
        job = self.job
        if film is None:
            film = np.zeros(job.width * job.height * 4, np.float32)
        st = RefStats()
        rc = lib().nm_ref_render(self._h, seed, pass_index, shard_rank, shard_world, threads, film.ctypes.data_as(f32p),
                                 C.byref(st))
        assert rc == 0
        return film, st

    def close(self):
        if self._h:
            lib().oracle_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
