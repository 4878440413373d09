"""Times bling_light_pass on one scene (tools/gpu/light_time.sh): photons/s and photon + shadow rays
per second from the pass's own HIP-event time, and the CPU restatement's time for the same pass.

    python3 tools/light_probe.py --config X5 --photons 2000000 --passes 3 [--ref-threads 16]
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

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="X5")
    ap.add_argument("--over", default="")
    ap.add_argument("--photons", type=int, default=100000)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--ref-threads", type=int, default=0, help="> 0: also time the CPU restatement")
    a = ap.parse_args()
    job = load_config(a.config, ";".join(x for x in (a.over, f"light={a.photons}") if x))
    ctx = Context(0)
    ctx.upload(job)
    splat = None
    for p in range(1, a.passes + 1):
        splat, st = ctx.light_pass(pass_index=p, splat=splat)
        rays = st.photon_rays + st.shadow_rays
        print(json.dumps({"config": a.config, "photons": a.photons, "pass": p, "ms": st.ms_total,
                          "photon_rays": st.photon_rays, "shadow_rays": st.shadow_rays, "splats": st.splats,
                          "Mphotons_per_s": st.photons / (st.ms_total * 1e3), "Mrays_per_s": rays / (st.ms_total * 1e3)}))
    if a.ref_threads > 0:
        from lt_ref import LightRef
        _, _, rst = LightRef(job).run(0x0B11A6, 1, records=False, threads=a.ref_threads)
        print(json.dumps({"config": a.config, "photons": a.photons, "restatement_threads": a.ref_threads,
                          "restatement_s": rst.seconds}))
