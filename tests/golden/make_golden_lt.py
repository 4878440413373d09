"""Regenerates tests/golden/LT1.npz: one 4096-photon pass of the light tracer's CPU restatement
(tests/ref/lighttracer_ref.cpp) on fixtures/scenes/light-tracer.bling -- the records' digest, the
counters and the splat image (tests/test_light_tracer.py::test_restatement_matches_its_golden).

    python tests/golden/make_golden_lt.py        (after `make ltref host`)
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bling_amd.scene import SCENES, parse_job  # noqa: E402
from lt_ref import LightRef  # noqa: E402

SEED = 0x0B11A6

if __name__ == "__main__":
    job = parse_job(os.path.join(SCENES, "light-tracer.bling"))
    rec, splat, st = LightRef(job).run(SEED, 1)
    np.savez_compressed(os.path.join(HERE, "LT1.npz"),
                        stats=np.array(st.counts(), np.uint64),
                        records_sha256=hashlib.sha256(np.ascontiguousarray(rec).tobytes()).hexdigest(),
                        splat=splat.reshape(job.height, job.width, 3))
    print("LT1:", st.counts(), len(rec), "records")
