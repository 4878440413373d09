"""The yardstick of the ordered splat films, shared by tests/test_splat_ordered.py (CPU) and
tests/test_gpu_splat_ordered.py: numpy's binary32 sequential add of splat records in key order."""
import os

import numpy as np

from bling_amd.scene import SCENES, load_config, parse_job

FIXTURE = os.path.join(SCENES, "light-tracer.bling")
# the four light tracer scenes of tests/test_gpu_light_tracer.py
LT_SCENES = {
    "fixture": lambda: parse_job(FIXTURE),
    "delta-lights": lambda: load_config("X13", "light=4096"),
    "sun-sky": lambda: load_config("X6", "light=4096;image=48,27"),
    "cornell": lambda: load_config("C1", "light=4096;image=48,48"),
}

# added in this order the binary32 sum keeps one of the two ones; in the reverse order it keeps the other
ORDER_EXAMPLE = (1e8, 1.0, -1e8, 1.0)


def sequential_add(image, records):
    """image (w * h * 3 float32) plus the records (fields pixel, key, x, y, z), one at a time in binary32, every
    pixel's records in ascending key order (equal keys in the order given).  Returns a new array."""
    out = np.array(image, np.float32).reshape(-1).copy()
    order = np.lexsort((records["key"], records["pixel"]))
    pix = records["pixel"][order].astype(np.int64)
    xyz = np.stack([records[k][order] for k in "xyz"], axis=1).astype(np.float32)
    for i in range(len(pix)):
        o = 3 * pix[i]
        out[o] = np.float32(out[o] + xyz[i, 0])
        out[o + 1] = np.float32(out[o + 1] + xyz[i, 1])
        out[o + 2] = np.float32(out[o + 2] + xyz[i, 2])
    return out
