"""Times the develop step of a written pass at one image size, on the device and on the host.

  python tools/develop_bench.py [--size 1024] [--reps 20] [--out file.json]

Reports, each as the median and the min / max of the repetitions after a warm-up, in milliseconds:
  device_rgb8, device_rgbe   bling_film_develop_device on a device film (wall time of the blocking call:
                             launch + kernel + stream synchronise)
  host_variant_rgb8, _rgbe   bling_film_develop from a host film (16 B/pixel up, 3 or 4 B/pixel back)
  film_copy_d2h              the 16 B/pixel film copy to the host that the host path needs first
  host_develop               bling_host_rgb_pixels + bling_host_film_to_rgb on the copied film (CPU)
Needs a GPU except with --host-only, which times host_develop alone.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    from bling_amd import film as bfilm
    w = h = a.size
    rng = np.random.default_rng(7)
    f = np.zeros((w * h, 4), np.float32)
    f[:, 0] = rng.uniform(0.5, 64.0, w * h)
    f[:, 1:] = rng.uniform(0.0, 1.2, (w * h, 3)) * f[:, :1]
    f = f.reshape(-1)
    res = {"size": [w, h]}
    res["host_develop"] = timed(lambda: (bfilm.rgb_pixels(f, w, h), bfilm.to_rgb(f, w, h)), 5, warmup=1)
    if not a.host_only:
        import torch
        from bling_amd.render import Context
        from bling_amd.scene import load_config
        ctx = Context(0)
        ctx.upload(load_config("C1", f"image={w},{h}"))
        ft = torch.from_numpy(f).cuda()
        px = torch.zeros(w * h * 3, dtype=torch.uint8, device="cuda")
        pe = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
        back = torch.empty(w * h * 4, dtype=torch.float32)
        torch.cuda.synchronize()

        def copy_back():
            back.copy_(ft)
            torch.cuda.synchronize()

        res["device_rgb8"] = timed(lambda: ctx.develop(ft, fmt="rgb8", out=px), a.reps)
        res["device_rgbe"] = timed(lambda: ctx.develop(ft, fmt="rgbe", out=pe), a.reps)
        o8, oe = np.zeros((h, w, 3), np.uint8), np.zeros((h, w, 4), np.uint8)
        res["host_variant_rgb8"] = timed(lambda: ctx.develop(f, fmt="rgb8", out=o8), a.reps)
        res["host_variant_rgbe"] = timed(lambda: ctx.develop(f, fmt="rgbe", out=oe), a.reps)
        res["film_copy_d2h"] = timed(copy_back, a.reps)
        assert (o8 == bfilm.rgb_pixels(f, w, h)).all() and (px.cpu().numpy().reshape(h, w, 3) == o8).all()
        ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
