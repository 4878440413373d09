"""The sampler and camera seam on the device (bling_camera_samples_device, include/bling.h): k_cam_samples against
the host library bit for bit, windows that end inside waves, the chain camera_samples -> surface_li ->
Image.add_windowed against the ordered pass without a host-made ray, cut calls, the refusals and the command line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from bling_amd import _ffi
from bling_amd.scene import SCENES, load_config, parse_job
from camera_samples_cases import (CASES, algebra_windows, case_job, counts_of, host, one_pixel_windows, same_bits,
                                  window_samples)
from surface_li_cases import SEED, bits, c1, job_desc, windows_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLING = os.path.join(ROOT, "bling_amd", "_lib", "bling")


@pytest.fixture(scope="module")
def ctx():
    from bling_amd.render import Context
    c = Context(0)
    yield c
    c.close()


def device(ctx, windows, pass_index=0, first=None, out=None):
    """camera_samples as a dict of numpy arrays (None for an output left out), and the stats."""
    xy, ids, rays, lens, st = ctx.camera_samples(windows, SEED, pass_index, first, out)
    return {k: (None if t is None else t.cpu().numpy()) for k, t in zip(("xy", "ids", "rays", "lens"), (xy, ids, rays, lens))}, st


# ------------------------------------------------------------------ 1. device against host
@pytest.mark.parametrize("name,pass_index", CASES)
def test_device_equals_host(ctx, name, pass_index, tmp_path):
    job = case_job(name, tmp_path)
    _, windows, counts = windows_of(job)
    ctx.upload(job)
    want = host(job, windows, pass_index)
    got, st = device(ctx, windows, pass_index)
    assert st.samples == sum(counts) == len(want["xy"]) and st.windows == len(windows) and st.ms_total > 0
    assert all(got[k] is not None for k in got) and same_bits(got, want)
    for keep in (("rays",), ("xy", "ids"), ("lens",)):
        part, _ = device(ctx, windows, pass_index, out={k: False for k in got if k not in keep})
        assert all((part[k] is not None) == (k in keep) for k in part) and same_bits(part, want), keep
    if name == "strat32":
        alg = algebra_windows(job)
        got, st = device(ctx, alg)
        assert st.windows == len(alg) and same_bits(got, host(job, alg))


# ------------------------------------------------------------------ 2. lane boundaries
def test_windows_that_end_inside_waves(ctx):
    job = c1("image=16,16;stratified=3,2")
    ctx.upload(job)
    ones = one_pixel_windows(job, 300)
    got, st = device(ctx, ones)
    assert st.samples == 1800 and same_bits(got, host(job, ones))
    ex0, ex1, ey0, ey1 = job.extent()
    whole = [(ex0, ex1, ey0, ey1)]
    got, st = device(ctx, whole)
    assert st.samples == (ex1 - ex0 + 1) * (ey1 - ey0 + 1) * 6 and same_bits(got, host(job, whole))


# ------------------------------------------------------------------ 3. the chain without host rays
@pytest.mark.parametrize("name,over,tiles", [("C1", "image=33,17", 6), ("X4", "image=16,16", 4), ("N2", "image=16,16", 4)])
def test_the_chain_of_seams_is_the_ordered_pass(ctx, name, over, tiles):
    from bling_amd.image import Image
    job = c1(over) if name == "C1" else load_config(name, over)
    _, windows, counts = windows_of(job)
    assert len(windows) >= tiles and (name != "C1" or len(windows) == 6)       # splitWindow's six windows of 33 x 17
    ctx.upload(job)
    img = Image(job_desc(job).filter, job.width, job.height, context=ctx)
    film = None
    for p in ((0, 1) if name == "C1" else (0,)):                  # the second pass accumulates on both sides
        cst, lst, ist = ctx.render_pass_by_seams(img, windows, SEED, p)      # the host sends windows and offsets only
        film, pst = ctx.render_pass(seed=SEED, pass_index=p, film=film, ordered=True)
        assert cst.samples == lst.rays == pst.camera_samples == sum(counts) and lst.dropped == 0
        assert ist.dropped_spectrum == 0 and ist.dropped_position == 0
        mine = img.film.cpu().numpy().reshape(-1)
        assert (mine > 0).any() and np.array_equal(bits(mine), bits(film)), p
    rgb8 = img.develop("rgb8").cpu().numpy()
    assert np.array_equal(rgb8, ctx.develop(film, fmt="rgb8")) and rgb8.any()


# ------------------------------------------------------------------ 4. cut and reuse
def test_cut_calls_and_an_untouched_wave_state(ctx):
    from bling_amd.render import Context
    job = c1("image=16,16")
    windows = algebra_windows(job)
    counts = counts_of(windows, job.spp)
    k, n = len(windows) // 2, sum(counts)
    cut = sum(counts[:k])
    ctx.upload(job)
    film0, _ = ctx.render_pass(seed=SEED, pass_index=2, ordered=True)        # the wave state exists before the calls
    whole, _ = device(ctx, windows)
    xy = torch.zeros((n, 2), dtype=torch.float32, device="cuda:0")
    ids = torch.zeros((n, 2), dtype=torch.int32, device="cuda:0")
    lens = torch.zeros((n, 2), dtype=torch.float32, device="cuda:0")
    a, _ = device(ctx, windows[:k], out={"xy": xy[:cut], "ids": ids[:cut], "lens": lens[:cut]})
    b, _ = device(ctx, windows[k:], out={"xy": xy[cut:], "ids": ids[cut:], "lens": lens[cut:]})
    both = {"xy": xy.cpu().numpy(), "ids": ids.cpu().numpy(), "lens": lens.cpu().numpy(), "rays": np.concatenate([a["rays"], b["rays"]], 1)}
    assert same_bits(both, whole) and same_bits(whole, host(job, windows))
    film1, _ = ctx.render_pass(seed=SEED, pass_index=2, ordered=True)
    fresh = Context(0)
    try:
        fresh.upload(job)
        film2, _ = fresh.render_pass(seed=SEED, pass_index=2, ordered=True)
    finally:
        fresh.close()
    assert (film1 > 0).any() and np.array_equal(bits(film1), bits(film0)) and np.array_equal(bits(film1), bits(film2))


# ------------------------------------------------------------------ 5. refusals
def _raw(ctx, windows, first, xy, ids, rays, lens):
    arr = (_ffi.ImageWindow * max(1, len(windows)))(*(_ffi.ImageWindow(*w) for w in windows))
    f = np.ascontiguousarray(first, np.uint64)
    st = _ffi.CameraStats()
    return _ffi.hip().bling_camera_samples_device(ctx._h, SEED, 0, arr, f.ctypes.data_as(C.POINTER(C.c_uint64)), len(windows),
                                                  C.c_void_p(xy), C.c_void_p(ids), C.c_void_p(rays), C.c_void_p(lens), C.byref(st))


def test_refusals(ctx):
    from bling_amd.render import Context
    job = c1("image=16,16")
    ex0, ex1, ey0, ey1 = job.extent()
    good = (ex0, ex0 + 3, ey0, ey0 + 3)
    c = 16 * job.spp
    n = 4 * c
    bufs = {k: torch.full(s, 7.5, dtype=torch.float32, device="cuda:0") for k, s in (("xy", (n, 2)), ("rays", (7, n)), ("lens", (n, 2)))}
    bufs["ids"] = torch.full((n, 2), 0xABCD, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ptr = {k: t.data_ptr() for k, t in bufs.items()}

    def call(c_, windows, first=None, **over):
        p = dict(ptr, **over)
        if first is None:
            first = np.concatenate([[0], np.cumsum(counts_of(windows, c_.job.spp if c_.job else 4))])
        return _raw(c_, windows, first, p["xy"], p["ids"], p["rays"], p["lens"])

    fresh = Context(0)
    try:
        assert call(fresh, [good]) == -4                                                     # no scene
    finally:
        fresh.close()
    ctx.upload(job)
    for w in ((ex0 - 1, ex0 + 3, ey0, ey0 + 3), (ex1 - 3, ex1 + 1, ey0, ey0 + 3), (ex0, ex0 + 3, ey0 - 1, ey0 + 3),
              (ex0, ex0 + 3, ey1 - 3, ey1 + 1)):
        assert call(ctx, [good, w]) == -1, w                                                 # outside the extent
    assert call(ctx, [good, good], [0, c, 2 * c + 1]) == -1                                  # a first off by one
    assert call(ctx, [good, good], [0, c - 1, 2 * c]) == -1
    assert call(ctx, [good, good], [0, 2 * c, c]) == -1                                      # descending
    assert call(ctx, [good], xy=ptr["lens"]) == -1                                           # an output aliases another
    assert call(ctx, [good], rays=ptr["xy"] + 8) == -1
    assert call(ctx, [good], ids=ptr["ids"] + 2) == -1                                       # not aligned to 4 bytes
    for other in (load_config("X5", "image=16,16"), parse_job(os.path.join(SCENES, "light-tracer.bling"), "image=16,16"),
                  load_config("M1", "image=16,16")):
        ctx.upload(other)
        e = other.extent()
        assert call(ctx, [(e[0], e[0] + 3, e[2], e[2] + 3)], [0, 16 * max(1, other.spp)]) == -1   # not the sampler renderer
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == (0xABCD if k == "ids" else 7.5)).all() for k, t in bufs.items())   # nothing was written
    # the context still serves: n = 0, an xy aligned to 4 bytes only, and bidir
    ctx.upload(job)
    assert call(ctx, []) == 0 and call(ctx, [(5, 4, 0, 3)]) == 0
    assert _raw(ctx, [], [0], None, None, None, None) == 0
    want = host(job, [good])
    assert call(ctx, [good], xy=ptr["xy"] + 4) == 0
    flat = bufs["xy"].cpu().numpy().reshape(-1)
    assert flat[0] == 7.5 and np.array_equal(bits(flat[1:1 + 2 * c]), bits(want["xy"].reshape(-1))) and (flat[1 + 2 * c:] == 7.5).all()
    assert np.array_equal(bufs["ids"].cpu().numpy()[:c].astype(np.uint32), want["ids"]) and (bufs["ids"].cpu().numpy()[c:] == 0xABCD).all()
    assert np.array_equal(bits(bufs["rays"].cpu().numpy().reshape(-1)[:7 * c].reshape(7, c)), bits(want["rays"]))
    bidir = load_config("B8", "image=16,16")
    ctx.upload(bidir)
    _, windows, _ = windows_of(bidir)
    got, _ = device(ctx, windows)
    _, img, _ = ctx.sample_li(window_samples(windows, bidir.spp), seed=SEED)
    assert np.array_equal(bits(got["xy"]), bits(img)) and same_bits(got, host(bidir, windows))
    # the staged host variant is the device variant
    ctx.upload(job)
    arr = (_ffi.ImageWindow * 1)(_ffi.ImageWindow(*good))
    f = np.asarray([0, c], np.uint64)
    h = {"xy": np.zeros((c, 2), np.float32), "ids": np.zeros((c, 2), np.uint32), "rays": np.zeros((7, c), np.float32),
         "lens": np.zeros((c, 2), np.float32)}
    st = _ffi.CameraStats()
    assert _ffi.hip().bling_camera_samples(ctx._h, SEED, 0, arr, f.ctypes.data_as(C.POINTER(C.c_uint64)), 1, _ffi.f32ptr(h["xy"]),
                                           _ffi.u32ptr(h["ids"]), _ffi.f32ptr(h["rays"]), _ffi.f32ptr(h["lens"]), C.byref(st)) == 0
    assert st.samples == c and same_bits(h, want)


# ------------------------------------------------------------------ 6. command line
def _bling(*args):
    env = {k: v for k, v in os.environ.items() if k != "BLING_FILM_ORDERED"}
    return subprocess.run([BLING, *args], capture_output=True, text=True, timeout=120, env=env)


def test_the_command_line_by_seams_writes_the_same_files(tmp_path):
    scene = os.path.join(SCENES, "cornell-box.bling")
    base = [scene, "--overrides", "image=33,17;path=5,2", "--passes", "2", "--film", "ordered"]
    a = _bling(*base, "--seams", "--out", str(tmp_path / "a"))
    b = _bling(*base, "--out", str(tmp_path / "b"))
    assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
    for p in ("00001", "00002"):
        for ext in ("png", "hdr"):
            x, y = (open(tmp_path / f"{k}-{p}.{ext}", "rb").read() for k in "ab")
            assert len(x) > 100 and x == y, (p, ext)
    for args, word in (([os.path.join(SCENES, "light-tracer.bling"), "--overrides", "image=16,16", "--film", "ordered", "--seams"], "splats"),
                       ([scene, "--overrides", "image=16,16;stratified=2,2;bidir=5,3", "--film", "ordered", "--seams"], "bidir"),
                       ([scene, "--overrides", "image=16,16;path=5,2", "--seams"], "--film ordered")):
        r = _bling(*args, "--out", str(tmp_path / "no"))
        assert r.returncode != 0 and word in r.stderr, (args, r.stderr)
        assert not list(tmp_path.glob("no-*"))
