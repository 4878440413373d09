"""Device time of bling_camera_samples_device ("The sampler and camera seam"): C2's
first-pass samples of every 16th tile -- the samples the surface_li entry measured -- one warm-up and three
runs, with the bytes written and the rate.  Prints one JSON line per output set.

    python tools/camera_samples_bench.py [--config C2] [--stride 16] [--runs 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bling_amd.render import Context  # noqa: E402
from bling_amd.scene import load_config  # noqa: E402
from film_ref import pass_tiles  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--stride", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    job = load_config(a.config)
    windows = pass_tiles(job, stride=a.stride)
    import torch
    torch.cuda.init()          # torch's HIP runtime first, as in the tests, then the core's context
    ctx = Context(0)
    ctx.upload(job)
    for name, off, per in (("xy+ids+rays+lens", {}, 52), ("xy+ids+rays", {"lens": False}, 44)):
        bufs = {}
        ms = []
        for _ in range(a.runs + 1):
            xy, ids, rays, lens, st = ctx.camera_samples(windows, pass_index=1, out=dict(off, **bufs))
            bufs = {k: t for k, t in (("xy", xy), ("ids", ids), ("rays", rays), ("lens", lens)) if t is not None}
            ms.append(st.ms_total)
        n = int(st.samples)
        best = min(ms[1:])
        print(json.dumps({"probe": "camera_samples", "config": a.config, "tile_stride": a.stride, "windows": int(st.windows),
                          "samples": n, "outputs": name, "bytes_written": n * per, "ms_warmup": round(ms[0], 4),
                          "ms_total": [round(m, 4) for m in ms[1:]], "GB_per_s_best": round(n * per / best / 1e6, 1)}))
    ctx.close()


if __name__ == "__main__":
    main()
