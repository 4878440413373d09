"""ctypes wrapper of the bidirectional integrator's CPU restatement (tests/ref/bidir_ref.cpp) -- test
infrastructure only, loaded by tests the way lt_ref loads the light tracer's.  The library
(tests/ref/_build/libbd_ref.so) is built by ``make bdref`` (part of ``make all``)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import cov_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(HERE, "ref", "_build", "libbd_ref.so")
f32p = C.POINTER(C.c_float)
i32p = C.POINTER(C.c_int)

STAT_NAMES = ("samples", "rays_camera", "rays_continuation", "rays_mis", "rays_shadow", "path_vertices", "dropped")
RAY_NAMES = STAT_NAMES[1:6]


class RefStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in STAT_NAMES] + [("seconds", C.c_double)]

    def rays(self) -> list:
        """[camera, continuation, mis, shadow, path vertices] -- bling_stats' mapping (include/bling.h)."""
        return [int(getattr(self, k)) for k in RAY_NAMES]


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            subprocess.check_call(["make", "bdref"], cwd=ROOT)
        L = C.CDLL(LIB)
        L.oracle_build.argtypes = [C.c_void_p]
        L.oracle_build.restype = C.c_void_p
        L.oracle_free.argtypes = [C.c_void_p]
        L.bd_ref_sample_li.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, i32p, C.c_size_t, f32p, f32p, i32p, C.c_int,
                                       C.POINTER(RefStats)]
        L.bd_ref_render.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, f32p,
                                    C.POINTER(RefStats)]
        L.bd_ref_results.argtypes = [f32p, C.c_size_t, f32p]
        L.bd_ref_results.restype = None
        L.bd_ref_count_spec.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32, f32p]
        _lib = L
    return _lib


def parity_samples(job, k=512, seed=2) -> np.ndarray:
    """k random (x, y, n) camera samples over the job's sample extent: the GPU parity tests' samples
    (tests/test_gpu_bidir.py), whose condition on the specular scene tests/test_bidir.py checks."""
    rng = np.random.default_rng(seed)
    x0, x1, y0, y1 = job.extent()
    return np.stack([rng.integers(x0, x1 + 1, k), rng.integers(y0, y1 + 1, k), rng.integers(0, job.spp, k)],
                    1).astype(np.int32)


def results(L) -> np.ndarray:
    """What addSample keeps of the spectra L (n, 16): (n, 4) = X, Y, Z, 1, zeros for a NaN / Inf sample."""
    L = np.ascontiguousarray(L, np.float32).reshape(-1, 16)
    out = np.zeros((len(L), 4), np.float32)
    lib().bd_ref_results(L.ctypes.data_as(f32p), len(L), out.ctypes.data_as(f32p))
    return out


def count_spec(ne: int, nl: int, emask: int, lmask: int) -> np.ndarray:
    """countSpec's nspec[0 .. ne + nl + 1] for subpath lengths and specular masks (bit i = vertex i)."""
    out = np.zeros(ne + nl + 2, np.float32)
    assert lib().bd_ref_count_spec(ne, nl, emask, lmask, out.ctypes.data_as(f32p)) == 0
    return out


class BidirRef:
    """The restatement over one parsed Job (which must outlive it)."""

    def __init__(self, job):
        self.job = job
        self._h = lib().oracle_build(C.c_void_p(job.desc))

    def sample_li(self, samples, seed, pass_index=1, threads=0):
        """(L (n, 16), terms (n, 3, 16) = ld, le, l, lens (n, 4) = eye length, light length, eye and
        light specular masks, RefStats) of the (x, y, n) samples."""
        s = np.ascontiguousarray(samples, np.int32).reshape(-1, 3)
        n = len(s)
        L = np.zeros((n, 16), np.float32)
        terms = np.zeros((n, 3, 16), np.float32)
        lens = np.zeros((n, 4), np.int32)
        st = RefStats()
        rc = lib().bd_ref_sample_li(self._h, seed, pass_index, s.ctypes.data_as(i32p), n, L.ctypes.data_as(f32p),
                                    terms.ctypes.data_as(f32p), lens.ctypes.data_as(i32p), threads, C.byref(st))
        assert rc == 0
        self.coverage = cov_ref.read(lib().bd_ref_coverage)     # what this call's light subpaths met
        return L, terms, lens, st

    def render(self, seed, pass_index=1, film=None, shard_rank=0, shard_world=1, term_mask=7, threads=0):
        """One pass into film (h * w * 4, accumulated): (film, RefStats)."""
        job = self.job
        if film is None:
            film = np.zeros(job.width * job.height * 4, np.float32)
        st = RefStats()
        rc = lib().bd_ref_render(self._h, seed, pass_index, shard_rank, shard_world, term_mask, threads,
                                 film.ctypes.data_as(f32p), C.byref(st))
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
