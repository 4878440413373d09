"""Developing the film on the device (include/bling.h bling_film_develop[_device]): linear RGB, the
8-bit display bytes and the RGBE bytes of a film and an optional splat image must equal the host
library's, bit for bit and byte for byte -- bling_host_film_splat_to_rgb, bling_host_rgb_pixels_splat
and the bytes bling_host_write_hdr puts after its header.  The one stated exception: a pixel with a +Inf
channel is left out of the RGBE comparison (the host's frexp exponent is unspecified there); the device
must still write it.  Every comparison runs through the host variant (numpy in, numpy out) and through
the device variant (torch tensors on the device).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from bling_amd import _ffi, film as bfilm
from bling_amd.render import BlingError, Context
from bling_amd.scene import CONFIGS, SCENES, load_config, parse_job, write_hdr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32 = np.float32
FMAX = np.finfo(np.float32).max
SIZES = [(1, 1), (3, 5), (37, 19), (65, 33), (257, 3)]
FORMATS = {"rgb_f32": (np.float32, 3), "rgb8": (np.uint8, 3), "rgbe": (np.uint8, 4)}
SENTINEL = {"rgb_f32": F32(-12345.5), "rgb8": np.uint8(0xA5), "rgbe": np.uint8(0xA5)}
SWS = [0.0, 1.0, float(F32(1) / F32(3))]

_ctx = {}


def ctx_for(w, h):
    """One context per image size, on the small Cornell box fixture (the develop calls only use its
    image size)."""
    if (w, h) not in _ctx:
        c = Context(0)
        c.upload(load_config("C1", f"image={w},{h}"))
        _ctx[(w, h)] = c
    return _ctx[(w, h)]


def _ulps(x, j):
    return (np.asarray(x, np.float32).view(np.int32) + np.asarray(j, np.int32)).view(np.float32)


def _hit(gain, target):
    """An input u near target / gain with fl(gain * u) == target exactly, or None."""
    cand = _ulps(F32(target / gain), np.arange(-16, 17))
    ok = np.nonzero(F32(gain) * cand == F32(target))[0]
    return cand[ok[0]] if len(ok) else None


def special_pixels():
    """(film (n, 4), splat (n, 3)) of the pixels every size gets first, as far as it has room: the values
    the formats treat specially, then the straddle of every RGB8 threshold through the splat path."""
    inf, nan = np.inf, np.nan
    fp, sp = [], []

    def film_px(w, x, y, z):
        fp.append([w, x, y, z]); sp.append([0.25, 0.5, 0.125])

    def splat_px(x, y, z):                    # empty film: the W == 0 branch, XYZ = sw * splat
        fp.append([0, 7.0, 7.0, 7.0]); sp.append([x, y, z])

    film_px(1, nan, 0.5, 0.5); film_px(1, 0.5, nan, nan); film_px(nan, 1, 1, 1)
    film_px(1, inf, 0, 0); film_px(1, 0, 0, inf); film_px(1, -inf, 0, 0); film_px(inf, 1, 1, 1)
    film_px(1, -1.0, -2.0, -0.5); film_px(2, -1e-3, 0.5, 0.25); film_px(-3, 1, 2, 3)
    film_px(1, 0.0, 0.0, 0.0); film_px(1, -0.0, -0.0, -0.0); film_px(-0.0, 1, 1, 1)
    film_px(1, 1e-40, 1e-40, 1e-40); film_px(1, 1e-45, 0, 1e-45); film_px(1e-40, 1e-42, 1e-42, 1e-42)
    film_px(1, FMAX / 2, FMAX / 2, FMAX / 2); film_px(1, FMAX / 2, 0, 0); film_px(1, 0, 0, FMAX / 2); film_px(0.5, 0, FMAX / 2, 0)
    splat_px(-0.0, 0, 0); splat_px(nan, 0, 0); splat_px(inf, 0, 0); splat_px(0, 0, -inf); splat_px(1e-40, 1e-41, 1e-42)
    # RGBE: z alone gives m = blue = fl(1.057311f * z).  m with an all-ones mantissa over a range of
    # exponents (r * sc may round to 256), m just below and at 1e-32f, m >= 2^127 (the exponent byte wraps)
    found = 0
    for e in (1, 30, 64, 100, 126, 127, 128, 130, 160, 200, 253):
        z = _hit(1.057311, np.uint32((e << 23) | 0x7FFFFF).view(np.float32))
        if z is not None:
            film_px(1, 0, 0, z); splat_px(0, 0, z); found += 1
    assert found >= 4
    tiny = F32(1e-32)
    z = _ulps(F32(tiny / F32(1.057311)), np.arange(-16, 17))
    b = F32(1.057311) * z
    i = int((b >= tiny).argmax())
    assert 0 < i and b[i - 1] < tiny <= b[i]
    film_px(1, 0, 0, z[i - 1]); film_px(1, 0, 0, z[i]); splat_px(0, 0, z[i - 1]); splat_px(0, 0, z[i])
    at = _hit(1.057311, tiny)
    if at is not None:
        film_px(1, 0, 0, at)
    for m in (2.0 ** 127, 1.9 * 2.0 ** 127, FMAX / 1.0574):
        film_px(1, 0, 0, m / 1.057311); splat_px(0, 0, m / 1.057311)
    # the straddle of every threshold: red = fl(3.240479f * x) just below and at or above t[k]
    t = bfilm.gamma_thresholds()
    cand = _ulps((t / F32(3.240479)).astype(np.float32)[:, None], np.arange(-8, 9)[None, :])
    red = F32(3.240479) * cand
    first = (red >= t[:, None]).argmax(1)
    assert (first > 0).all()
    for k in range(255):
        splat_px(cand[k, first[k] - 1], 0, 0); splat_px(cand[k, first[k]], 0, 0)
    return np.array(fp, np.float32), np.array(sp, np.float32)


_SPECIAL = None


def make_film(w, h):
    """Seeded film (h * w * 4) and splat (h * w * 3): W in [0.5, 64], XYZ / W across 1e-6 .. 1e4, a row
    (or, in a one-row image, a run) of W = 0, and the special pixels at seeded places."""
    global _SPECIAL
    if _SPECIAL is None:
        _SPECIAL = special_pixels()
    rng = np.random.default_rng(1000 * w + h)
    n = w * h
    f = np.zeros((n, 4), np.float32)
    f[:, 0] = rng.uniform(0.5, 64.0, n)
    f[:, 1:] = np.exp(rng.uniform(np.log(1e-6), np.log(1e4), (n, 3))) * f[:, :1]
    s = np.exp(rng.uniform(np.log(1e-6), np.log(1e4), (n, 3))).astype(np.float32)
    f.reshape(h, w, 4)[h // 2, : max(1, w // 2 if h == 1 else w), 0] = 0.0
    sf, ss = _SPECIAL
    k = min(n, len(sf))
    at = rng.permutation(n)[:k]
    f[at], s[at] = sf[:k], ss[:k]
    return f.reshape(-1), s.reshape(-1)


def _u8p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


_refs = {}


def reference(w, h, with_splat, sw):
    """The host library's three images of make_film(w, h), computed once: {fmt: array (h, w, c)}, and the
    mask (h, w) of pixels with a +Inf channel, which the RGBE comparison leaves out."""
    key = (w, h, with_splat, sw)
    if key not in _refs:
        f, s = make_film(w, h)
        sp = _ffi.f32ptr(s) if with_splat else None
        lib = _ffi.host()
        rgb = np.zeros(w * h * 3, np.float32)
        lib.bling_host_film_splat_to_rgb(_ffi.f32ptr(f), sp, sw, w, h, _ffi.f32ptr(rgb))
        px = np.zeros(w * h * 3, np.uint8)
        lib.bling_host_rgb_pixels_splat(_ffi.f32ptr(f), sp, sw, w, h, _u8p(px))
        rgbe = hdr_bytes(rgb.reshape(h, w, 3))
        ref = {"rgb_f32": rgb.reshape(h, w, 3), "rgb8": px.reshape(h, w, 3), "rgbe": rgbe}
        for a in ref.values():
            a.setflags(write=False)
        _refs[key] = (ref, np.isposinf(rgb.reshape(h, w, 3)).any(-1))
    return _refs[key]


def hdr_bytes(rgb):
    """The bytes the existing write_hdr puts after its header, (h, w, 4)."""
    import tempfile
    h, w, _ = rgb.shape
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "x.hdr")
        write_hdr(p, rgb)
        data = open(p, "rb").read()
    head = f"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y {h} +X {w}\n".encode()
    assert data.startswith(head) and len(data) == len(head) + 4 * w * h
    return np.frombuffer(data[len(head):], np.uint8).reshape(h, w, 4).copy()


def develop(ctx, variant, f, s, sw, fmt, window=None):
    """One develop into a sentinel-filled whole-image buffer; returns it as numpy (h, w, c)."""
    w, h = ctx.job.width, ctx.job.height
    dt, per = FORMATS[fmt]
    if variant == "host":
        out = np.full((h, w, per), SENTINEL[fmt], dt)
        got = ctx.develop(f, s, sw, fmt, window, out)
        assert got is out
        return out
    ft = torch.from_numpy(f).cuda()
    st = None if s is None else torch.from_numpy(s).cuda()
    out = torch.from_numpy(np.full(w * h * per, SENTINEL[fmt], dt)).cuda()
    torch.cuda.synchronize()
    assert ctx.develop(ft, st, sw, fmt, window, out) is out
    return out.cpu().numpy().reshape(h, w, per)


def assert_image(got, ref, inf_mask, fmt, inside=None):
    """got equals ref where inside (default: everywhere) and keeps the sentinel elsewhere."""
    h, w, _ = ref.shape
    inside = np.ones((h, w), bool) if inside is None else inside
    want = np.where(inside[..., None], ref, SENTINEL[fmt])
    if fmt == "rgb_f32":
        nan = np.isnan(want)
        np.testing.assert_array_equal(np.isnan(got), nan)            # a NaN of any payload
        np.testing.assert_array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])   # -0 is not +0
        return
    if fmt == "rgbe":
        skip = inside & inf_mask
        # outside the contract, but written: no pixel is left out
        assert not (got[skip] == SENTINEL[fmt]).all(-1).any()
        want = np.where(skip[..., None], got, want)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("with_splat", [True, False], ids=["splat", "nosplat"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_develop_equals_the_host_library(size, with_splat):
    w, h = size
    ctx = ctx_for(w, h)
    f, s = make_film(w, h)
    for sw in SWS:
        ref, inf_mask = reference(w, h, with_splat, sw)
        for variant in ("host", "device"):
            for fmt in FORMATS:
                got = develop(ctx, variant, f, s if with_splat else None, sw, fmt)
                assert_image(got, ref[fmt], inf_mask, fmt)


def test_the_film_meets_every_case():
    """The 37x19 and larger films hold every special pixel: NaN, +-Inf, negatives, both zeros, subnormals,
    the straddle of all 255 thresholds, and the RGBE cases -- both sides of 1e-32, exponent bytes that wrap."""
    w, h = 37, 19
    assert len(special_pixels()[0]) <= w * h
    ref, inf_mask = reference(w, h, True, 1.0)
    rgb, px, e = ref["rgb_f32"], ref["rgb8"], ref["rgbe"]
    assert np.isnan(rgb).any() and inf_mask.any() and np.isneginf(rgb).any() and (rgb < 0).any()
    assert np.signbit(rgb[rgb == 0]).any() and (~np.signbit(rgb[rgb == 0])).any()
    assert ((np.abs(rgb) < np.finfo(np.float32).tiny) & (rgb != 0)).any()
    assert len(np.unique(px[..., 0])) == 256                      # the straddles: every byte occurs in red
    m = np.maximum(np.nan_to_num(rgb, nan=0.0, posinf=0.0), 0).max(-1)
    assert ((m > 0) & (m < F32(1e-32))).any() and (e[(m > 0) & (m < F32(1e-32))] == 0).all()
    big = (m >= 2.0 ** 127) & ~inf_mask
    assert big.any() and (e[big][:, 3] == 0).all()                # ex + 128 = 256 wraps to 0
    ones = (m.view(np.uint32) & 0x7FFFFF) == 0x7FFFFF
    assert ones.sum() >= 4


WINDOWS = {
    "interior": (5, 20, 3, 10), "left": (0, 10, 4, 8), "right": (30, 36, 4, 8), "top": (4, 8, 0, 5),
    "bottom": (4, 8, 15, 18), "whole": (0, 36, 0, 18), "one": (36, 36, 18, 18), "neg": (-5, 3, -2, 4),
    "past": (30, 50, 10, 40), "around": (-100, 100, -100, 100), "outside_x": (40, 50, 0, 5),
    "outside_y": (0, 5, -9, -1), "x1<x0": (10, 5, 0, 18), "y1<y0": (0, 36, 9, 8),
}


@pytest.mark.parametrize("name", list(WINDOWS))
def test_windows_write_their_pixels_only(name):
    w, h = 37, 19
    x0, x1, y0, y1 = WINDOWS[name]
    ctx = ctx_for(w, h)
    f, s = make_film(w, h)
    sw = SWS[2]
    ref, inf_mask = reference(w, h, True, sw)
    yy, xx = np.mgrid[0:h, 0:w]
    inside = (xx >= x0) & (xx <= x1) & (yy >= y0) & (yy <= y1)
    assert inside.any() == (name not in ("outside_x", "outside_y", "x1<x0", "y1<y0"))
    for variant in ("host", "device"):
        for fmt in FORMATS:
            got = develop(ctx, variant, f, s, sw, fmt, WINDOWS[name])
            assert_image(got, ref[fmt], inf_mask, fmt, inside)


def test_refusals():
    lib = _ffi.hip()
    w, h = 37, 19
    n = w * h
    buf = torch.zeros(n * 16 + n * 12 + n * 12 + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    base = buf.data_ptr()
    film_p, splat_p, out_p = base, base + n * 16, base + n * 28
    hf, ho = np.zeros(n * 4, np.float32), np.zeros(n * 12, np.uint8)

    def dev(ctx, fmt, f, s, o):
        dp = _ffi.DevelopParams(fmt, 1.0, (C.c_int32 * 4)(0, w - 1, 0, h - 1))
        return lib.bling_film_develop_device(ctx._h, C.byref(dp), C.c_void_p(f), C.c_void_p(s), C.c_void_p(o))

    def host(ctx, fmt, f, o):
        dp = _ffi.DevelopParams(fmt, 1.0, (C.c_int32 * 4)(0, w - 1, 0, h - 1))
        return lib.bling_film_develop(ctx._h, C.byref(dp), None if f is None else _ffi.f32ptr(f), None,
                                      None if o is None else C.c_void_p(o.ctypes.data))

    empty = Context(0)
    assert dev(empty, 1, film_p, None, out_p) == -4 and host(empty, 1, hf, ho) == -4      # BLING_ENOSCENE
    assert b"no scene" in lib.bling_last_error()
    with pytest.raises(BlingError) as e:
        empty.develop(hf)
    assert e.value.rc == -4
    empty.close()

    ctx = ctx_for(w, h)
    for fmt in (-1, 3, 1 << 20):
        assert dev(ctx, fmt, film_p, None, out_p) == -1 and host(ctx, fmt, hf, ho) == -1  # BLING_EINVAL
        assert b"format" in lib.bling_last_error()
    assert dev(ctx, 1, None, None, out_p) == -1 and dev(ctx, 1, film_p, None, None) == -1
    assert host(ctx, 1, None, ho) == -1 and host(ctx, 1, hf, None) == -1
    assert lib.bling_film_develop_device(ctx._h, None, C.c_void_p(film_p), None, C.c_void_p(out_p)) == -1
    assert lib.bling_last_error()
    # out may touch the film or the splat image, not overlap them
    assert dev(ctx, 0, film_p, splat_p, out_p) == 0
    for bad in (film_p, film_p + n * 16 - 4, film_p - n * 12 + 4, splat_p, splat_p + n * 12 - 1):
        assert dev(ctx, 0, film_p, splat_p, bad) == -1, bad - base
        assert b"overlap" in lib.bling_last_error()
    assert dev(ctx, 0, film_p, None, splat_p) == 0                 # no splat buffer: its range is free
    assert dev(ctx, 1, film_p, splat_p, film_p + n * 16 - 1) == -1 and dev(ctx, 2, film_p, splat_p, splat_p + n * 12 - 4) == -1

    # the Python layer: element type, size and residence of the tensors
    ft = torch.zeros(n * 4, dtype=torch.float32, device="cuda")
    good = torch.zeros(n * 3, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert ctx.develop(ft, None, 0.0, "rgb8", None, good) is good
    for out in (torch.zeros(n * 3, dtype=torch.float32, device="cuda"), torch.zeros(n * 4, dtype=torch.uint8, device="cuda"),
                torch.zeros(n * 3, dtype=torch.uint8), None):
        with pytest.raises(ValueError):
            ctx.develop(ft, None, 0.0, "rgb8", None, out)
    with pytest.raises(ValueError):
        ctx.develop(ft.double(), None, 0.0, "rgb8", None, good)
    with pytest.raises(ValueError):
        ctx.develop(ft, torch.zeros(n * 3, dtype=torch.float32), 0.0, "rgb8", None, good)
    with pytest.raises(ValueError):
        ctx.develop(ft, None, 0.0, "rgb16", None, good)
    with pytest.raises(ValueError):
        ctx.develop(hf[:-4], None, 0.0, "rgb8")


def test_a_rendered_film_develops_on_the_device():
    """One path pass of C1 at 48x48 into a device film: developed where it lies, RGB8 and RGBE equal the
    host path's on the copied-back film."""
    job = load_config("C1", "image=48,48")
    w, h = job.width, job.height
    ctx = Context(0)
    ctx.upload(job)
    ft = torch.zeros(w * h * 4, dtype=torch.float32, device="cuda")
    px = torch.zeros(w * h * 3, dtype=torch.uint8, device="cuda")
    pe = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.render_pass_device(ft.data_ptr(), pass_index=1)
    ctx.develop(ft, fmt="rgb8", out=px)
    ctx.develop(ft, fmt="rgbe", out=pe)
    f = ft.cpu().numpy()
    assert np.isfinite(f).all() and (f.reshape(-1, 4)[:, 0] > 0).all()
    np.testing.assert_array_equal(px.cpu().numpy().reshape(h, w, 3), bfilm.rgb_pixels(f, w, h))
    np.testing.assert_array_equal(pe.cpu().numpy().reshape(h, w, 4), hdr_bytes(bfilm.to_rgb(f, w, h)))
    assert len(np.unique(px.cpu().numpy())) > 32                   # an image, not a constant
    ctx.close()


def test_a_light_tracer_pass_develops_with_its_splat_and_weight():
    """One light-tracer pass at a small image: its splat image and weight 1 / passPhotons over the empty
    film, developed by both variants, equal the host path's RGB8 and RGBE."""
    job = parse_job(os.path.join(SCENES, "light-tracer.bling"), "image=40,30")
    w, h = job.width, job.height
    ctx = Context(0)
    ctx.upload(job)
    splat, st = ctx.light_pass(pass_index=1)
    assert st.splats > 0
    f = np.zeros(w * h * 4, np.float32)
    sw = float(F32(1.0) / F32(job.light.pass_photons))
    lib = _ffi.host()
    px = np.zeros(w * h * 3, np.uint8)
    lib.bling_host_rgb_pixels_splat(_ffi.f32ptr(f), _ffi.f32ptr(splat), sw, w, h, _u8p(px))
    rgb = np.zeros(w * h * 3, np.float32)
    lib.bling_host_film_splat_to_rgb(_ffi.f32ptr(f), _ffi.f32ptr(splat), sw, w, h, _ffi.f32ptr(rgb))
    pe = hdr_bytes(rgb.reshape(h, w, 3))
    assert len(np.unique(px)) > 8
    for variant in ("host", "device"):
        np.testing.assert_array_equal(develop(ctx, variant, f, splat, sw, "rgb8"), px.reshape(h, w, 3))
        np.testing.assert_array_equal(develop(ctx, variant, f, splat, sw, "rgbe"), pe)
    ctx.close()


def test_cli_develops_the_same_files_on_the_device(tmp_path):
    """`bling --develop device` writes the .png and .hdr of `--develop host` (the default), byte for byte.
    The scene takes one sample per pixel through the box filter, so that every film pixel is one
    addition and the two runs' films cannot differ by the order of their float atomics."""
    exe = os.path.join(_ffi.LIBDIR, "bling")
    ov = CONFIGS["C1"].overrides + ";image=40,24;stratified=1,1;filter=box"
    for how in ("host", "device"):
        out = subprocess.run([exe, CONFIGS["C1"].path, "--overrides", ov, "--passes", "1", "--out", str(tmp_path / how),
                              "--develop", how], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
    for ext in ("png", "hdr"):
        a = open(tmp_path / f"host-00001.{ext}", "rb").read()
        b = open(tmp_path / f"device-00001.{ext}", "rb").read()
        assert len(a) > 40 * 24 * 3 and a == b, ext
    default = subprocess.run([exe, CONFIGS["C1"].path, "--overrides", ov, "--passes", "1", "--out", str(tmp_path / "plain")],
                             capture_output=True, text=True, timeout=120)
    assert default.returncode == 0, default.stderr
    assert open(tmp_path / "plain-00001.png", "rb").read() == open(tmp_path / "host-00001.png", "rb").read()
    bad = subprocess.run([exe, CONFIGS["C1"].path, "--develop", "gpu"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--develop" in bad.stderr
