#!/usr/bin/env python3
"""In-process A/B of the pipelined pass (include/bling.h BLING_PASS_NO_PIPELINE): passes of one config
as two half-waves on two streams and as one wave, alternating, with BLING_PASS_KERNEL_TIMING.  Prints
one JSON line per arm: the pass time (median, min, max over the passes), how the passes ran, and the
summed launch times of the closest-hit and shading kernels and, for the single wave, the rest of the
bounce loop (any-hit, staging, compaction).  In the pipelined arm the launches of the two halves
overlap, so those sums count shared time twice, ms_bounce includes the first half's film and ms_film
is the second half's alone: only ms_pass compares across the arms.

  python tools/ab_pipeline.py [--config C2] [--passes 8] [--arms pipe,single] [--force] [--stride 1]

--arms single alone measures an experiment build (BLING_HIP_VARIANT) as one wave; --force pipelines
a config whose profile keeps the single wave by default (bling_debug_set_pipeline).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bling_amd import _ffi  # noqa: E402
from bling_amd.render import Context  # noqa: E402
from bling_amd.scene import load_config  # noqa: E402

ARMS = {"pipe": _ffi.PASS_KERNEL_TIMING, "single": _ffi.PASS_KERNEL_TIMING | _ffi.PASS_NO_PIPELINE}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--passes", type=int, default=8)
    ap.add_argument("--arms", default="pipe,single")
    ap.add_argument("--force", action="store_true")
    ap.add_argument("--tag", default="")
    ap.add_argument("--stride", type=int, default=1, help="every n-th tile of the pass (a sub-sample)")
    a = ap.parse_args()
    arms = {k: ARMS[k] for k in a.arms.split(",")}
    ctx = Context(0)
    ctx.upload(load_config(a.config))
    if a.force:
        ctx.set_pipeline(1)
    has_waves = hasattr(_ffi.hip(), "bling_debug_pass_results")
    acc = {k: {"ms": [], "closest": 0.0, "shade": 0.0, "bounce": 0.0, "film": 0.0, "rays": 0, "waves": set()} for k in arms}
    for k, fl in arms.items():                                    # warm-up: allocations, code objects
        ctx.render_pass(pass_index=0, tile_stride=a.stride, flags=fl)
    for p in range(a.passes):
        for k, fl in arms.items():
            _, st = ctx.render_pass(pass_index=1 + p, tile_stride=a.stride, flags=fl)
            r = acc[k]
            r["ms"].append(st.ms_total)
            r["closest"] += st.ms_closest; r["shade"] += st.ms_shade; r["bounce"] += st.ms_bounce; r["film"] += st.ms_film
            r["rays"] += st.rays()
            if has_waves:
                r["waves"].add(ctx_waves(ctx))
    for k, r in acc.items():
        n = a.passes
        print(json.dumps({"config": a.config, "variant": os.environ.get("BLING_HIP_VARIANT", ""), "tag": a.tag, "arm": k,
                          "passes": n, "ms_pass_median": round(statistics.median(r["ms"]), 3),
                          "ms_pass_min": round(min(r["ms"]), 3), "ms_pass_max": round(max(r["ms"]), 3),
                          "waves": sorted(r["waves"]), "ms_closest": round(r["closest"] / n, 3),
                          "ms_shade": round(r["shade"] / n, 3),
                          # the rest of the bounce loop; undefined where the launches overlap (the pipelined arm)
                          "ms_any_stage_compact": round((r["bounce"] - r["closest"] - r["shade"]) / n, 3) if k == "single" else None,
                          "ms_bounce": round(r["bounce"] / n, 3), "ms_film": round(r["film"] / n, 3),
                          "rays_per_pass": r["rays"] // n}), flush=True)


def ctx_waves(ctx):
    """How the last pass ran, without copying a large pass's results back."""
    import ctypes as C
    n, waves = C.c_size_t(), C.c_int()
    _ffi.hip().bling_debug_pass_results(ctx._h, None, 0, C.byref(n), C.byref(waves))
    return int(waves.value)


if __name__ == "__main__":
    main()
