"""Shared helpers of the integrator-seam tests (tests/test_surface_li_chain.py, tests/test_gpu_surface_li.py):
a pass's samples in the reference's window order, their camera rays and ids as bling_surface_li takes them,
and cornell-box with another camera."""
import os

import numpy as np

from bling_amd import _ffi
from bling_amd.scene import CONFIGS, SCENES, load_config, parse_job
from film_ref import pass_samples, pass_tiles

SEED = 0x0B11A6
_LOOKAT = "pos 278.0 273.0 -800.0\n      look 278.0 273.0 0.0\n"
_CAMERA = "camera {\n   perspective\n   fov 37.5\n   lensRadius 0\n   focalDistance 10\n}\n"
# another lookAt with a thin lens focused on the blocks; an environment camera inside the box
CAMERAS = {"lens": ("pos 150.0 400.0 -600.0\n      look 300.0 200.0 300.0\n",
                    "camera {\n   perspective\n   fov 50\n   lensRadius 12\n   focalDistance 900\n}\n"),
           "environment": ("pos 278.0 273.0 200.0\n      look 278.0 273.0 559.0\n", "camera { environment }\n")}


def windows_of(job):
    """(samples (k, 3) int32 of (x, y, n), windows [(x0, x1, y0, y1)], counts): splitWindow's 16 x 16 sample windows
    of the extent in tile order, each window's samples in (iy, ix, n) order -- prender's order."""
    tiles = pass_tiles(job)
    counts = [(x1 - x0 + 1) * (y1 - y0 + 1) * job.spp for x0, x1, y0, y1 in tiles]
    return pass_samples(job, 0), tiles, counts


def stream_ids(job, samples):
    """(k, 2) uint32 (pixel, n): the built-in camera's stream of each (x, y, n) sample."""
    ex0, ex1, ey0, _ = job.extent()
    s = np.asarray(samples, np.int64)
    return np.stack([(s[:, 1] - ey0) * (ex1 - ex0 + 1) + (s[:, 0] - ex0), s[:, 2]], 1).astype(np.uint32)


def camera_rays(orc, samples, seed=SEED, pass_index=0):
    """(rays (7, k) float32 with tmin = 0, xy (k, 2) float32) of the oracle's camera for the (x, y, n) samples."""
    out = np.stack([orc.camera_ray(int(x), int(y), int(n), seed=seed, pass_index=pass_index) for x, y, n in samples])
    rays = np.zeros((7, len(out)), np.float32)
    rays[:6] = out[:, 2:8].T
    return rays, np.ascontiguousarray(out[:, :2])


def c1(over):
    return load_config("C1", over)


def c1_with_camera(which, dirname, over):
    """C1 (cornell-box with the benchmark's overrides, then `over`) seen through CAMERAS[which]: the same geometry,
    filter and sampler."""
    text = open(CONFIGS["C1"].path).read()
    look, cam = CAMERAS[which]
    assert text.count(_LOOKAT) == 1 and text.count(_CAMERA) == 1
    path = os.path.join(str(dirname), f"cornell_{which}.bling")
    with open(path, "w") as f:
        f.write(text.replace(_LOOKAT, look).replace(_CAMERA, cam))
    return parse_job(path, CONFIGS["C1"].overrides + ";" + over)


def job_desc(job):
    """The job's film as the image API describes it: its size and its filter's table."""
    desc = _ffi.ImageDesc()
    desc.width, desc.height = job.width, job.height
    desc.filter.kind = _ffi.FILTER_KINDS["mitchell"]
    desc.filter.width, desc.filter.height = job.filter_size
    desc.filter.table[:] = [float(v) for v in job.filter_table().reshape(-1)]
    return desc


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


__all__ = ["SEED", "SCENES", "windows_of", "stream_ids", "camera_rays", "c1", "c1_with_camera", "job_desc", "bits"]
