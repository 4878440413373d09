#!/usr/bin/env python3
"""In-process A/B of the sampler renderer's ordered film (include/bling.h BLING_PASS_ORDERED_FILM): passes
of one config with the atomic film and with the ordered one, alternating in one process.  Prints one
JSON line per arm: the pass time (median, min, max over the passes), the film time (ms_film: the film
kernels of the pass; in a pipelined pass the second half's film alone, plus -- ordered -- the final
addTile launch), Mrays/s from the median pass time, and how the passes ran.  The ordered arm also says
whether every one of its films of a pass index equals the first run's bytes (a second sweep repeats the
same pass indices into fresh films).

  python tools/ab_film_ordered.py [--config C2] [--passes 6] [--stride 1] [--tag T]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bling_amd import _ffi  # noqa: E402
from bling_amd.render import Context  # noqa: E402
from bling_amd.scene import load_config  # noqa: E402


def ctx_waves(ctx):
    """How the last pass ran, without copying a large pass's results back."""
    n, waves = C.c_size_t(), C.c_int()
    _ffi.hip().bling_debug_pass_results(ctx._h, None, 0, C.byref(n), C.byref(waves))
    return int(waves.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--passes", type=int, default=6)
    ap.add_argument("--tag", default="")
    ap.add_argument("--stride", type=int, default=1, help="every n-th tile of the pass (a sub-sample)")
    a = ap.parse_args()
    arms = {"atomic": False, "ordered": True}
    ctx = Context(0)
    ctx.upload(load_config(a.config))
    acc = {k: {"ms": [], "film": [], "rays": 0, "waves": set()} for k in arms}
    for ordered in arms.values():                                 # warm-up: allocations, code objects
        ctx.render_pass(pass_index=0, tile_stride=a.stride, ordered=ordered)
    first, same = {}, True
    for p in range(a.passes):
        index = 1 + p % max(1, a.passes // 2)                     # the second half repeats the first half's passes
        for k, ordered in arms.items():
            film, st = ctx.render_pass(pass_index=index, tile_stride=a.stride, ordered=ordered)
            r = acc[k]
            r["ms"].append(st.ms_total)
            r["film"].append(st.ms_film)
            r["rays"] += st.rays()
            r["waves"].add(ctx_waves(ctx))
            if ordered:
                same = same and first.setdefault(index, film.tobytes()) == film.tobytes()
    for k, r in acc.items():
        n = a.passes
        med = statistics.median(r["ms"])
        print(json.dumps({"config": a.config, "tag": a.tag, "arm": k, "passes": n, "stride": a.stride,
                          "ms_total_median": round(med, 3), "ms_total_min": round(min(r["ms"]), 3),
                          "ms_total_max": round(max(r["ms"]), 3), "ms_film_median": round(statistics.median(r["film"]), 3),
                          "ms_film_min": round(min(r["film"]), 3), "ms_film_max": round(max(r["film"]), 3),
                          "mrays_per_s": round(r["rays"] / n / (med * 1e3), 1), "waves": sorted(r["waves"]),
                          "rays_per_pass": r["rays"] // n,
                          "repeat_same_bytes": same if arms[k] else None}), flush=True)


if __name__ == "__main__":
    main()
