"""The coverage counters of the three restatements (tests/ref/coverage.h): what the light paths of the
last run met.  read(fn) -> {name: count} through a library's *_ref_coverage function."""
import ctypes as C

# the order of coverage.h's enum
COV_NAMES = ("verts", "shading", "bump", "lamb", "oren", "lamb_btdf", "oren_btdf", "micro_diel", "micro_cond", "srefl",
             "srefl_cond", "strans", "fblend_iso", "fblend_aniso", "fblend_depth", "fractal", "env_rays")


def read(fn) -> dict:
    out = (C.c_uint64 * len(COV_NAMES))()
    fn.argtypes = [C.POINTER(C.c_uint64)]
    fn.restype = None
    fn(out)
    return {k: int(v) for k, v in zip(COV_NAMES, out)}
