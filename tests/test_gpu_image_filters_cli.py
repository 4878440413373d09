"""`bling --image-filters` (the reference's imageFilters, src/cmdline/Examples.hs:10-58): the ten PNGs it writes
from device films equal, byte for byte, the PNGs bling_host_write_png makes of bling_host_image_add_samples of
the same samples, restated here from Examples.hs; a second run writes the same bytes.
"""
import ctypes as C
import ctypes.util
import os
import subprocess

import numpy as np
import pytest

from bling_amd import _ffi
from bling_amd import image as bimage

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLING = os.path.join(ROOT, "bling_amd", "_lib", "bling")
FILTERS = [("box", ("box",)), ("gauss", ("gauss", 3, 3, 2)), ("mitchell", ("mitchell", 3, 3, f32(1) / f32(3), f32(1) / f32(3))),
           ("sinc", ("sinc", 3, 3, 3)), ("triangle", ("triangle", 3, 3))]
W, H, SHOW = 48, 27, 64


def cover(desc):
    """coverWindow of the sample extent: (px, py) rows first."""
    x0, x1, y0, y1 = bimage.image_extent(desc)
    ys, xs = np.meshgrid(np.arange(y0, y1 + 1), np.arange(x0, x1 + 1), indexing="ij")
    return xs.reshape(-1).astype(f32), ys.reshape(-1).astype(f32)


def show_samples(spec):
    """fltShow (Examples.hs:39-49)."""
    desc = bimage.image_desc(("box",), SHOW, SHOW)
    x, y = cover(desc)
    xs, ys = (x / f32(SHOW) - f32(0.5)) * f32(4), (y / f32(SHOW) - f32(0.5)) * f32(4)
    d = np.array([bimage.eval_filter(spec, a, b) for a, b in zip(xs, ys)], f32)
    rgb = np.zeros((len(d), 3), f32)
    rgb[:, 0] = np.where(d > 0, d, f32(0))
    rgb[:, 1] = np.where(d > 0, f32(0), -d)
    return desc, np.stack([x, y], 1), bimage.rgb_to_spectrum_illum(rgb)


def zone_samples(spec):
    """fltTest (Examples.hs:25-35): 25 offsets a pixel, sx outer, sy inner; sin is the C library's sinf."""
    libm = C.CDLL(ctypes.util.find_library("m"))
    libm.sinf.argtypes, libm.sinf.restype = [C.c_float], C.c_float
    desc = bimage.image_desc(spec, W, H)
    px, py = cover(desc)
    offs = np.array([0, 0.2, 0.4, 0.6, 0.8], f32)
    x = (px[:, None, None] + offs[None, :, None] + np.zeros((1, 1, 5), f32)).reshape(-1)
    y = (py[:, None, None] + offs[None, None, :] + np.zeros((1, 5, 1), f32)).reshape(-1)
    sz = f32(min(W, H))
    dx, dy = x / sz - f32(0.5), f32(1) - y / sz
    arg = f32(150) * (dx * dx + dy * dy)
    d = np.abs(np.array([libm.sinf(float(a)) for a in arg], f32))
    return desc, np.stack([x, y], 1), bimage.rgb_to_spectrum_illum(np.stack([d, d, d], 1))


def reference_png(path, desc, xy, spectra):
    film = bimage.host_add_samples(desc, desc.width, desc.height, xy, spectra)
    assert _ffi.host().bling_host_write_png(str(path).encode(), _ffi.f32ptr(film.reshape(-1)), desc.width, desc.height) == 0
    return open(path, "rb").read()


def test_image_filters_writes_the_reference_images(tmp_path):
    outs = []
    for run, develop in (("a", "host"), ("b", "host"), ("c", "device")):
        d = tmp_path / run
        d.mkdir()
        r = subprocess.run([BLING, "--image-filters", "--size", f"{W}x{H}", "--out", str(d), "--develop", develop],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        names = sorted(os.listdir(d))
        assert names == sorted(f"filter-{k}-{n}.png" for k in ("show", "test") for n, _ in FILTERS)
        outs.append({n: open(d / n, "rb").read() for n in names})
        for n, _ in FILTERS:
            assert n in r.stdout                                      # putStrLn fname
    assert outs[0] == outs[1]                                         # a second run writes the same bytes
    assert outs[0] == outs[2]                                         # and so does developing on the device
    for name, spec in FILTERS:
        assert outs[0][f"filter-show-{name}.png"] == reference_png(tmp_path / "ref-show.png", *show_samples(spec)), name
        assert outs[0][f"filter-test-{name}.png"] == reference_png(tmp_path / "ref-test.png", *zone_samples(spec)), name
