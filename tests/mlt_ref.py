"""ctypes wrapper of the Metropolis renderer's CPU restatement (tests/ref/mlt_ref.cpp) -- test
infrastructure only, loaded by tests the way lt_ref / bd_ref load theirs.  The library
(tests/ref/_build/libmlt_ref.so) is built by ``make mltref`` (part of ``make all``)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import cov_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(HERE, "ref", "_build", "libmlt_ref.so")
f32p = C.POINTER(C.c_float)
f64p = C.POINTER(C.c_double)

# bling_mlt_record (include/bling.h)
RECORD = np.dtype([("chain", "<u4"), ("mutation", "<u4"), ("x", "<f4"), ("y", "<f4"), ("i_prop", "<f4"), ("a", "<f4"),
                   ("flags", "<u4"), ("pad", "<u4")])
COUNT_NAMES = ("mutations", "large_steps", "accepted", "splats", "dropped", "rays_camera", "rays_continuation",
               "rays_mis", "rays_shadow", "path_vertices")


class RefStats(C.Structure):
    _fields_ = [("b", C.c_double)] + [(k, C.c_uint64) for k in COUNT_NAMES] + [("seconds", C.c_double)]

    def counts(self) -> list:
        return [int(getattr(self, k)) for k in COUNT_NAMES]


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            subprocess.check_call(["make", "mltref"], cwd=ROOT)
        L = C.CDLL(LIB)
        L.oracle_build.argtypes = [C.c_void_p]
        L.oracle_build.restype = C.c_void_p
        L.oracle_free.argtypes = [C.c_void_p]
        L.mlt_ref_pass.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, f64p, f32p, C.c_void_p, C.c_size_t,
                                   C.POINTER(C.c_uint32), C.POINTER(RefStats), f64p, C.POINTER(C.c_uint32)]
        L.mlt_ref_pass.restype = C.c_int
        L.mlt_ref_jitter.argtypes = [C.c_float] * 5
        L.mlt_ref_jitter.restype = C.c_float
        L.mlt_ref_mutate.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_float, C.c_float,
                                     C.c_float, f32p, f32p, C.POINTER(C.c_int)]
        L.mlt_ref_mutate.restype = C.c_int
        L.mlt_ref_boot_select.argtypes = [f32p, C.c_int, C.c_float, f32p, C.POINTER(C.c_int)]
        L.mlt_ref_boot_select.restype = C.c_int
        L.mlt_ref_boot_starts.argtypes = [f32p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, f32p, C.POINTER(C.c_uint32),
                                          C.POINTER(C.c_uint32)]
        L.mlt_ref_boot_starts.restype = C.c_int
        L.mlt_ref_chain_mutations.argtypes = [C.c_uint64] * 3
        L.mlt_ref_chain_mutations.restype = C.c_uint64
        L.bd_ref_sample_li.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_int), C.c_size_t, f32p, f32p,
                                       C.POINTER(C.c_int), C.c_int, C.c_void_p]
        L.bd_ref_sample_li.restype = C.c_int
        L.bd_ref_results.argtypes = [f32p, C.c_size_t, f32p]
        _lib = L
    return _lib


def mutations(job) -> int:
    """M = floor (mpp * nPixels) in binary32 (Metropolis.hs:86)."""
    return int(np.floor(np.float32(job.metropolis.mpp) * np.float32(job.width * job.height)))


class MltRef:
    """The restatement over one parsed Job (which must outlive it)."""

    def __init__(self, job):
        self.job = job
        self._h = lib().oracle_build(C.c_void_p(job.desc))

    def run(self, seed, pass_index=1, threads=0, splat32=None):
        """One pass: (records sorted by (chain, mutation), start samples, splat64, splat32, RefStats);
        raises ValueError where the reference would stop with an error."""
        job = self.job
        n = job.width * job.height * 3
        s64 = np.zeros(n, np.float64)
        s32 = np.zeros(n, np.float32) if splat32 is None else splat32
        m = mutations(job)
        rec = np.zeros(m, RECORD)
        starts = np.zeros(job.metropolis.chains, np.uint32)
        st = RefStats()
        self.abs64 = np.zeros(n, np.float64)            # per channel sum of |contribution|, per pixel splat count
        self.count = np.zeros(n // 3, np.uint32)
        rc = lib().mlt_ref_pass(self._h, seed, pass_index, threads, s64.ctypes.data_as(f64p), s32.ctypes.data_as(f32p),
                                rec.ctypes.data_as(C.c_void_p), m, starts.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(st),
                                self.abs64.ctypes.data_as(f64p), self.count.ctypes.data_as(C.POINTER(C.c_uint32)))
        self.coverage = cov_ref.read(lib().mlt_ref_coverage)    # what this pass's light subpaths met
        if rc == -2:
            raise ValueError("the bootstrap selection reads an unwritten slot")
        if rc != 0:
            raise ValueError("bad metropolis block")
        return rec, starts, s64, s32, st

    def sample_li(self, seed, pass_index, samples, threads=0):
        """bd_ref_sample_li of (x, y, n) camera samples with the sampler renderer's keys: (n, 16) spectra."""
        smp = np.ascontiguousarray(samples, np.int32).reshape(-1, 3)
        out = np.zeros((len(smp), 16), np.float32)
        rc = lib().bd_ref_sample_li(self._h, seed, pass_index, smp.ctypes.data_as(C.POINTER(C.c_int)), len(smp),
                                    out.ctypes.data_as(f32p), None, None, threads, None)
        assert rc == 0
        return out

    def close(self):
        if self._h:
            lib().oracle_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def xyz(L):
    """spectrumToXYZ of (n, 16) spectra -> (n, 3) float64 (zeros for a NaN / infinite one)."""
    L = np.ascontiguousarray(L, np.float32)
    out = np.zeros((len(L), 4), np.float32)
    lib().bd_ref_results(L.ctypes.data_as(f32p), len(L), out.ctypes.data_as(f32p))
    return out[:, :3].astype(np.float64)


def jitter(v, vmin, vmax, u1, u2):
    return np.float32(lib().mlt_ref_jitter(v, vmin, vmax, u1, u2))


def mutate(seed, pass_index, chain, m, md, sx, sy, plarge, cur):
    """(proposal, large, draws taken) of one mutation of the primary sample cur."""
    cur = np.ascontiguousarray(cur, np.float32)
    prop = np.zeros_like(cur)
    large = C.c_int()
    n = lib().mlt_ref_mutate(seed, pass_index, chain, m, md, sx, sy, plarge, cur.ctypes.data_as(f32p),
                             prop.ctypes.data_as(f32p), C.byref(large))
    return prop, bool(large.value), n


def boot_select(I, u):
    """(slot or -1, bootstrap sample held there, b') of hand-built bootstrap contributions."""
    I = np.ascontiguousarray(I, np.float32)
    b = np.zeros(1, np.float32)
    smp = C.c_int()
    slot = lib().mlt_ref_boot_select(I.ctypes.data_as(f32p), len(I), u, b.ctypes.data_as(f32p), C.byref(smp))
    return slot, smp.value, np.float32(b[0])


def boot_starts(I, seed, pass_index, chains):
    """(b', start samples, None), or (b', None, refused chain) where the reference would stop."""
    I = np.ascontiguousarray(I, np.float32)
    b = np.zeros(1, np.float32)
    starts = np.zeros(chains, np.uint32)
    bad = C.c_uint32()
    rc = lib().mlt_ref_boot_starts(I.ctypes.data_as(f32p), len(I), seed, pass_index, chains, b.ctypes.data_as(f32p),
                                   starts.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(bad))
    return (np.float32(b[0]), starts, None) if rc == 0 else (np.float32(b[0]), None, bad.value)


def chain_mutations(M, C_, c):
    return int(lib().mlt_ref_chain_mutations(M, C_, c))
