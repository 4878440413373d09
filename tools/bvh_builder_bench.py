#!/usr/bin/env python3
"""Build time and tree quality of the two BVH builders (bling_scene_upload_with: the host's binned SAH and
the device's linear BVH), measured through bling_debug_bvh_build_info.  Reads nothing outside the repository.

  python tools/bvh_builder_bench.py [--name NAME] [--soup N] [--skip-soup] [--derive host,device]

writes profiles/NAME.jsonl: one line per (scene, builder, derivation, upload) with ms_build, ms_derive (host wall
time of everything after the BVH2), ms_derive_device (HIP events around the derive kernels), ms_plan_host (the
host's share) and ms_upload (wall time of the whole upload call) -- one warm-up upload, then three -- and one line
per builder with node_visits, tri_tests and ms_closest of a pass over ducky
at 48 x 48 (BLING_PASS_TRAVERSAL_STATS | BLING_PASS_KERNEL_TIMING).  Scenes:
  ducky    fixtures/scenes/ducky.bling (14 129 items)
  bezier   fixtures/scenes/bezier.bling with both patches at subdivs 81: 26 244 triangles, the size of the
           reference's gumbo.bling at subdivs 16 (26 112), which this repository does not hold
  soup     one generated mesh of N (default 1 000 000) small triangles scattered in a box
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bling_amd import _ffi  # noqa: E402
from bling_amd.render import Context  # noqa: E402
from bling_amd.scene import load_config, parse_job  # noqa: E402

SCENES = os.path.join(ROOT, "fixtures", "scenes")
HEAD = """filter mitchell 2 2 0.333333 0.333333
imageSize 64 64
renderer { sampler sampled { sampler { stratified 2 2 } integrator { path maxDepth 5 sampleDepth 3 } } }
transform { lookAt { pos 0 0 -40 look 0 0 1 up 0 1 0 } }
camera { perspective fov 40 lensRadius 0 focalDistance 10 }
material { matte kd { constant rgbR 0.5 0.5 0.5 } sigma { constant 0 } }
emission { rgbI 12 12 12 }
newTransform { rotateX -90 translate 0 30 0 }
prim { shape { quad 10 10 } }
emission { none }
newTransform { }
"""


def bezier_scene(dirname, subdivs=81):
    text = open(os.path.join(SCENES, "bezier.bling")).read()
    text = re.sub(r"subdivs\s+\d+", f"subdivs {subdivs}", text)
    path = os.path.join(dirname, f"bezier_{subdivs}.bling")
    open(path, "w").write(text)
    return path


def soup_scene(dirname, n, seed=1):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-20, 20, (n, 1, 3))
    v = (c + rng.uniform(-0.05, 0.05, (n, 3, 3))).reshape(-1, 3)
    path = os.path.join(dirname, f"soup_{n}.bling")
    with open(path, "w") as f:
        f.write(HEAD + f"prim {{ mesh vertexCount {3 * n} faceCount {n}\n")
        f.write("".join("   v %.6f %.6f %.6f\n" % (x, y, z) for x, y, z in v))
        f.write("".join(f"   f {3 * k} {3 * k + 1} {3 * k + 2}\n" for k in range(n)))
        f.write("}\n")
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--name", default="bvh_builder")
    ap.add_argument("--soup", type=int, default=1_000_000)
    ap.add_argument("--skip-soup", action="store_true")
    ap.add_argument("--derive", default="host", help="comma-separated derivations to measure: host, device")
    a = ap.parse_args()
    rows = []
    ctx = Context(0)
    with tempfile.TemporaryDirectory() as tmp:
        jobs = [("ducky", load_config("C3", "image=48,48")), ("bezier_81", parse_job(bezier_scene(tmp)))]
        if not a.skip_soup:
            jobs.append((f"soup_{a.soup}", parse_job(soup_scene(tmp, a.soup))))
        for name, job in jobs:
            for builder in ("host", "device"):
                for derive in a.derive.split(","):
                    for k in range(4):                           # upload 0 warms up
                        t0 = time.perf_counter()
                        ctx.upload(job, bvh=builder, derive=derive)
                        ms_upload = (time.perf_counter() - t0) * 1e3
                        bi, di = ctx.bvh_build_info(), ctx.derive_info()
                        rows.append({"kind": "build", "scene": name, "builder": builder, "derive": derive, "upload": k,
                                     "warmup": k == 0, **bi, "derive_used": di["used"], "bvh4_nodes": di["bvh4_nodes"],
                                     "level_launches": di["level_launches"], "ms_derive_device": di["ms_derive_device"],
                                     "ms_plan_host": di["ms_plan_host"], "ms_upload": ms_upload})
                        print(json.dumps(rows[-1]), flush=True)
                if name == "ducky":
                    _, st = ctx.render_pass(seed=0x0B11A6, pass_index=0, flags=_ffi.PASS_TRAVERSAL_STATS | _ffi.PASS_KERNEL_TIMING)
                    rows.append({"kind": "walk", "scene": name, "builder": builder, "node_visits": int(st.node_visits),
                                 "tri_tests": int(st.tri_tests), "ms_closest": float(st.ms_closest), "rays": st.rays(),
                                 "ms_total": float(st.ms_total)})
                    print(json.dumps(rows[-1]), flush=True)
    ctx.close()
    out = os.path.join(ROOT, "profiles", a.name + ".jsonl")
    with open(out, "w") as f:
        f.write("".join(json.dumps(r) + "\n" for r in rows))
    print("wrote", out)


if __name__ == "__main__":
    main()
