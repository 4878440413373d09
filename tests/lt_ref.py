"""ctypes wrapper of the light tracer's CPU restatement (tests/ref/lighttracer_ref.cpp) -- test
infrastructure only, loaded by tests the way oracle_py loads the oracle.  The library
(tests/ref/_build/liblt_ref.so) is built by ``make ltref`` (part of ``make all``)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import cov_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(HERE, "ref", "_build", "liblt_ref.so")
f32p = C.POINTER(C.c_float)

# bling_light_record (include/bling.h)
RECORD = np.dtype([("photon", "<u4"), ("depth", "<u4"), ("sx", "<i4"), ("sy", "<i4"),
                   ("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("pad", "<u4")])
STAT_NAMES = ("photons", "photon_rays", "shadow_rays", "splats", "dropped")


class RefStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in STAT_NAMES] + [("seconds", C.c_double)]

    def counts(self) -> list:
        return [int(getattr(self, k)) for k in STAT_NAMES]


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            subprocess.check_call(["make", "ltref"], cwd=ROOT)
        L = C.CDLL(LIB)
        L.oracle_build.argtypes = [C.c_void_p]
        L.oracle_build.restype = C.c_void_p
        L.oracle_free.argtypes = [C.c_void_p]
        L.lt_ref_pass.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, f32p,
                                  C.c_void_p, f32p, C.c_size_t, C.POINTER(RefStats)]
        L.lt_ref_pass.restype = C.c_size_t
        L.lt_ref_sample_cam.argtypes = [C.c_void_p, f32p, f32p]
        L.lt_ref_eval_adj.argtypes = [C.c_void_p, C.c_int, f32p, f32p, f32p, f32p]
        L.lt_ref_first_hit.argtypes = [C.c_void_p, f32p, C.POINTER(C.c_int)]
        _lib = L
    return _lib


def _f(a):
    a = np.ascontiguousarray(a, np.float32)
    return a, a.ctypes.data_as(f32p)


class LightRef:
    """The restatement over one parsed Job (which must outlive it)."""

    def __init__(self, job):
        self.job = job
        self._h = lib().oracle_build(C.c_void_p(job.desc))

    def run(self, seed, pass_index=1, first=0, count=None, splat=None, records=True, threads=0):
        """Photons first .. first + count - 1 of a pass: (records sorted by (photon, depth), splat
        (h * w * 3, accumulated in photon order), RefStats)."""
        job = self.job
        if count is None:
            count = job.light.pass_photons - first
        if splat is None:
            splat = np.zeros(job.width * job.height * 3, np.float32)
        st = RefStats()
        n = lib().lt_ref_pass(self._h, seed, pass_index, first, count, threads, splat.ctypes.data_as(f32p), None, None,
                              0, C.byref(st))
        self.coverage = cov_ref.read(lib().lt_ref_coverage)     # what this pass's photons met
        rec = np.zeros(n if records else 0, RECORD)
        self.camz = np.zeros(len(rec), np.float32)      # camera-space z of each record's vertex
        if records and n:
            # a second walk fills the records; the splat image is not touched again
            lib().lt_ref_pass(self._h, seed, pass_index, first, count, threads, None, rec.ctypes.data_as(C.c_void_p),
                              self.camz.ctypes.data_as(f32p), n, None)
        return rec, splat, st

    def sample_cam(self, p):
        """sampleCam of a world point: (px, py, pLens (3,), pdf, camera-space z of the point)."""
        _p, pp = _f(p)
        out, po = _f(np.zeros(7))
        lib().lt_ref_sample_cam(self._h, pp, po)
        return out[0], out[1], out[2:5].copy(), out[5], out[6]

    def eval_adj(self, material, ng, ns, dpdu, wo, wi):
        """evalBsdf True of the material's BSDF on (ng; shading frame ns, dpdu) -> (16,) spectrum."""
        fr, pf = _f(np.concatenate([ng, ns, dpdu]))
        a, pa = _f(wo)
        b, pb = _f(wi)
        out, po = _f(np.zeros(16))
        lib().lt_ref_eval_adj(self._h, material, pf, pa, pb, po)
        return out

    def first_hit(self, o, d):
        """(hit, emitter light index or -1) of the closest hit of a ray."""
        r, pr = _f(np.concatenate([o, d]))
        out = (C.c_int * 2)()
        lib().lt_ref_first_hit(self._h, pr, out)
        return bool(out[0]), int(out[1])

    def close(self):
        if self._h:
            lib().oracle_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
