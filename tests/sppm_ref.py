"""ctypes wrapper of the SPPM photon pass's per-splat records (tests/ref/sppm_ref.cpp) -- test
infrastructure only, loaded by tests the way oracle_py loads the oracle.  The library
(tests/ref/_build/libsppm_ref.so) is built by ``make sppmref`` (part of ``make all``)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(HERE, "ref", "_build", "libsppm_ref.so")
f32p = C.POINTER(C.c_float)

# bling_sppm_record (include/bling.h)
RECORD = np.dtype([("thread", "<u4"), ("photon", "<u4"), ("seq", "<u4"), ("depth", "<u4"), ("sx", "<i4"), ("sy", "<i4"),
                   ("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("pad", "<u4")])
STAT_NAMES = ("hitpoints", "photons", "photon_rays", "photon_hits")


class RefStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in STAT_NAMES]

    def counts(self) -> list:
        return [int(getattr(self, k)) for k in STAT_NAMES]


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            subprocess.check_call(["make", "sppmref"], cwd=ROOT)
        L = C.CDLL(LIB)
        L.oracle_build.argtypes = [C.c_void_p]
        L.oracle_build.restype = C.c_void_p
        L.oracle_free.argtypes = [C.c_void_p]
        L.oracle_sppm_new.argtypes = [C.c_void_p]
        L.oracle_sppm_new.restype = C.c_void_p
        L.oracle_sppm_free.argtypes = [C.c_void_p]
        L.oracle_sppm_pass.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, f32p, f32p, C.c_void_p]
        L.oracle_sppm_pixel_stats.argtypes = [C.c_void_p, f32p, f32p]
        L.sppm_ref_records.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(RefStats)]
        L.sppm_ref_records.restype = C.c_size_t
        L.sppm_ref_sn.argtypes = [C.c_void_p]
        _lib = L
    return _lib


def fold_two_level(rec, nth, w, h, image=None):
    """The reference's splat image of one pass from its records (sorted by (thread, photon, seq)): every
    sampler's image from zero, its splats added one at a time in binary32, then image = image + image_k
    in k order (SPPM.hs:451-453)."""
    image = np.zeros(w * h * 3, np.float32) if image is None else image
    for k in range(nth):
        r = rec[rec["thread"] == k]
        image += fold_flat(r, w, h)
    return image


def fold_flat(rec, w, h, image=None):
    """Every splat added one at a time in binary32 into one image, in the records' order."""
    image = np.zeros(w * h * 3, np.float32) if image is None else image
    img = image.reshape(h * w, 3)
    pix = rec["sy"].astype(np.int64) * w + rec["sx"]
    xyz = np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(np.float32)
    # round j adds every pixel's j-th splat: the splats of one pixel are added in their order
    order = np.argsort(pix, kind="stable")
    pix, xyz = pix[order], xyz[order]
    start = np.flatnonzero(np.r_[True, pix[1:] != pix[:-1]])
    rank = np.arange(len(pix)) - np.repeat(start, np.diff(np.r_[start, len(pix)]))
    for j in range(int(rank.max()) + 1 if len(pix) else 0):
        m = rank == j
        img[pix[m]] = img[pix[m]] + xyz[m]
    return image


class SppmRef:
    """The restatement over one parsed Job (which must outlive it); its radii advance with advance()."""

    def __init__(self, job):
        self.job = job
        self._os = lib().oracle_build(C.c_void_p(job.desc))
        self._h = lib().oracle_sppm_new(self._os)
        if not self._h:
            raise RuntimeError("scene renderer is not sppm")
        self.sn = int(lib().sppm_ref_sn(self._h))

    def records(self, seed, pass_index, threads=0):
        """(records in (thread, photon, seq) order, RefStats) of the pass, for the current radii."""
        st = RefStats()
        n = lib().sppm_ref_records(self._h, seed, pass_index, threads, None, 0, C.byref(st))
        rec = np.zeros(n, RECORD)
        if n:
            lib().sppm_ref_records(self._h, seed, pass_index, threads, rec.ctypes.data_as(C.c_void_p), n, None)
        return rec, st

    def advance(self, seed, pass_index, threads=0):
        """Runs the pass itself (the oracle's onePass, compiled into this library) so the radii move on."""
        w, h = self.job.width, self.job.height
        film = np.zeros(w * h * 4, np.float32)
        splat = np.zeros(w * h * 3, np.float32)
        if lib().oracle_sppm_pass(self._h, seed, pass_index, threads, film.ctypes.data_as(f32p), splat.ctypes.data_as(f32p), None) != 0:
            raise RuntimeError("oracle_sppm_pass failed")
        return film, splat

    def close(self):
        if self._h:
            lib().oracle_sppm_free(self._h)
            self._h = None
        if self._os:
            lib().oracle_free(self._os)
            self._os = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
