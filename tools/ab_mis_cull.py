#!/usr/bin/env python3
"""In-process A/B of the MIS cull (include/bling.h BLING_PASS_NO_MIS_CULL): passes of one config with
and without the cull, alternating, with BLING_PASS_KERNEL_TIMING.  Prints one JSON line per arm:
closest-hit and shading ms per pass, the rest of the bounce loop (any-hit, staging, compaction), the
pass time, and the queries the closest-hit kernel walked.

  python tools/ab_mis_cull.py [--config C2] [--passes 4] [--stride 1]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bling_amd import _ffi  # noqa: E402
from bling_amd.render import Context  # noqa: E402
from bling_amd.scene import load_config  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--stride", type=int, default=1)
    a = ap.parse_args()
    ctx = Context(0)
    ctx.upload(load_config(a.config))
    arms = {"cull": _ffi.PASS_KERNEL_TIMING, "no_cull": _ffi.PASS_KERNEL_TIMING | _ffi.PASS_NO_MIS_CULL}
    acc = {k: {"closest": 0.0, "shade": 0.0, "bounce": 0.0, "total": 0.0, "walked": 0, "mis": 0, "culled": 0} for k in arms}
    for k, fl in arms.items():                                    # warm-up: allocations, code objects
        ctx.render_pass(pass_index=0, tile_stride=a.stride, flags=fl)
    for p in range(a.passes):
        for k, fl in arms.items():
            _, st = ctx.render_pass(pass_index=1 + p, tile_stride=a.stride, flags=fl)
            c = ctx.mis_culled()
            r = acc[k]
            r["closest"] += st.ms_closest; r["shade"] += st.ms_shade; r["bounce"] += st.ms_bounce; r["total"] += st.ms_total
            r["walked"] += st.rays_camera + st.rays_continuation + st.rays_mis - c
            r["mis"] += st.rays_mis; r["culled"] += c
    for k, r in acc.items():
        n = a.passes
        print(json.dumps({"config": a.config, "arm": k, "passes": n, "ms_closest": round(r["closest"] / n, 3),
                          "ms_shade": round(r["shade"] / n, 3),
                          "ms_any_stage_compact": round((r["bounce"] - r["closest"] - r["shade"]) / n, 3),
                          "ms_pass": round(r["total"] / n, 3), "closest_walked": r["walked"] // n,
                          "rays_mis": r["mis"] // n, "mis_culled": r["culled"] // n}))


if __name__ == "__main__":
    main()
