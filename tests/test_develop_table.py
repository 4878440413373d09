"""The host side of the device develop (include/bling_host.h): rgbPixels' float -> byte step as a
table of 255 thresholds, and the pixel encoders factored out of the PNG and Radiance writers.

The device's RGB8 byte is the count of thresholds t[k] <= v (bling_film_develop, include/bling.h), so
these tests pin the table to the host expression nearbyint(min(1, max(0, powf(v, 1/2.2f))) * 255) it
was bisected from: at every threshold, around every threshold, over the whole float range and at the
values GHC's min / max treat specially.  That the expression is monotone in v -- without which no
table could restate it -- is checked once for every binary32 of [0, 1] by tools/gamma_monotone.cpp
(DESIGN.md section 5), not here.
"""
import ctypes as C

import numpy as np
import pytest

from bling_amd import _ffi, film

F32 = np.float32
RED_X = F32(3.240479)          # xyzToRgb's red row: r = 3.240479 x - 1.537150 y - 0.498535 z


@pytest.fixture(scope="module")
def table(built):
    t = film.gamma_thresholds()
    assert t.dtype == np.float32 and t.shape == (255,)
    assert (np.diff(t) > 0).all() and t[0] > 0 and t[-1] < 1
    return t


def lookup(t, v):
    """The device's byte: the count of t[k] <= v; NaN compares false everywhere.  -Inf is looked up as
    +Inf: powf (-Inf) (1 / 2.2) is +Inf, so the host's byte of -Inf is 255, unlike every other negative's."""
    v = np.asarray(v, np.float32)
    v = np.where(v == -np.inf, np.float32(np.inf), v)
    return np.where(np.isnan(v), 0, np.searchsorted(t, v, side="right")).astype(np.uint8)


def _ulps(x, j):
    """x moved by j units in the last place (positive finite float32 x, array j)."""
    return (np.asarray(x, np.float32).view(np.int32) + np.asarray(j, np.int32)).view(np.float32)


def straddle(t):
    """Per threshold the adjacent splat values (x_lo, x_hi = its successor) whose red channel
    fl(3.240479f * x) lies below t[k] and at or above it: t[k] itself need not be a product."""
    x0 = (t / RED_X).astype(np.float32)
    cand = _ulps(x0[:, None], np.arange(-8, 9)[None, :])
    red = RED_X * cand
    first = (red >= t[:, None]).argmax(1)          # red is non-decreasing along the candidates
    assert (first > 0).all() and (red[np.arange(255), first] >= t).all()
    x_hi = cand[np.arange(255), first]
    x_lo = cand[np.arange(255), first - 1]
    assert (RED_X * x_lo < t).all() and (RED_X * x_hi >= t).all()
    return x_lo, x_hi


def _host_red(x):
    """Red byte of bling_host_rgb_pixels_splat for a one-pixel image: empty film (W = 0), splat
    (x, 0, 0), splat weight 1."""
    f = np.zeros(4, np.float32)
    s = np.array([x, 0, 0], np.float32)
    out = np.zeros(3, np.uint8)
    _ffi.host().bling_host_rgb_pixels_splat(_ffi.f32ptr(f), _ffi.f32ptr(s), 1.0, 1, 1, out.ctypes.data_as(C.POINTER(C.c_uint8)))
    return int(out[0])


def test_each_threshold_is_where_the_host_byte_steps(table):
    t = table
    x_lo, x_hi = straddle(t)
    for k in range(255):
        # the value just above stays below the next threshold, so the byte there is exactly k + 1
        assert k == 254 or RED_X * x_hi[k] < t[k + 1]
        assert _host_red(x_hi[k]) == k + 1, (k, x_hi[k])
        assert _host_red(x_lo[k]) == k, (k, x_lo[k])
    # the lookup itself steps at the table's own entries: nextafter(t[k], -inf) is one byte down
    down = np.nextafter(t, F32(-np.inf))
    assert (lookup(t, t) == np.arange(1, 256)).all() and (lookup(t, down) == np.arange(255)).all()


def _check_lookup(t, xyz):
    """film.rgb_pixels of pixels with W = 1 and the given XYZ equals the lookup of film.to_rgb."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    f = np.concatenate([np.ones((n, 1), np.float32), xyz], 1).reshape(-1)
    rgb = film.to_rgb(f, n, 1)
    got = film.rgb_pixels(f, n, 1)
    np.testing.assert_array_equal(got, lookup(t, rgb))
    return rgb, got


def test_lookup_equals_the_host_around_every_threshold(table):
    """+-512 ulps around every threshold, as far as achromatic pixels (X = Y = Z = u) reach them: red is
    about 1.2048 u, so u sweeps 1025 neighbours of t[k] / 1.2048 and green and blue ride along."""
    t = table
    one = np.ones((1, 3), np.float32)
    gain = film.to_rgb(np.array([1, 1, 1, 1], np.float32), 1, 1).reshape(3)[0]
    u = _ulps((t / gain).astype(np.float32)[:, None], np.arange(-512, 513)[None, :]).reshape(-1, 1)
    rgb, got = _check_lookup(t, u * one)
    red = got.reshape(255, 1025, 3)[..., 0].astype(int)
    # every sweep does cross its threshold: both bytes occur in it
    assert (red.min(1) == np.arange(255)).all() and (red.max(1) == np.arange(1, 256)).all()


def test_lookup_equals_the_host_over_the_float_range(table):
    t = table
    rng = np.random.default_rng(20)
    n = 1 << 20
    # log-uniform over every positive binary32 (uniform bit patterns) ...
    wide = rng.integers(1, 0x7F800000, n, dtype=np.int64).astype(np.uint32).view(np.float32)
    # ... and log-uniform over the range the bytes live in
    near = np.exp(rng.uniform(np.log(1e-7), np.log(4.0), n)).astype(np.float32)
    one = np.ones((1, 3), np.float32)
    _, got = _check_lookup(t, wide[:, None] * one)
    rgb, got2 = _check_lookup(t, near[:, None] * one)
    assert len(np.unique(got2)) == 256                # every byte occurs


def test_lookup_equals_the_host_at_special_values(table):
    t = table
    fmax = np.finfo(np.float32).max
    inf, nan = F32(np.inf), F32(np.nan)
    xyz = [[nan] * 3, [nan, 0, 0], [inf, 0, 0], [-inf, 0, 0], [0, inf, 0], [0.0] * 3, [-0.0, 0, 0], [-1.0] * 3, [-1e-3, 0, 0],
           [1e-40] * 3, [1e-45, 0, 0], [fmax] * 3, [fmax / 4, 0, 0], [0, 0, fmax / 2], [1.0] * 3, [0.5] * 3]
    rgb, got = _check_lookup(t, xyz)
    rgb = rgb.reshape(-1, 3)
    # the cases the device's compares must reproduce: NaN, finite negatives and zero give 0, +-Inf 255
    # (film.to_rgb adds a +0 to every channel, so -0 is met only in the direct lookup below)
    assert (got.reshape(-1, 3)[np.isnan(rgb)] == 0).all() and np.isnan(rgb).any()
    finite_le0 = np.isfinite(rgb) & (rgb <= 0)
    assert (got.reshape(-1, 3)[finite_le0] == 0).all() and (rgb[finite_le0] < 0).any() and (rgb == 0).any()
    assert (got.reshape(-1, 3)[np.isinf(rgb)] == 255).all() and (rgb == np.inf).any() and (rgb == -np.inf).any()
    assert (lookup(t, [nan, -inf, -fmax, -1.0, -0.0, 0.0, 1e-40, 1.0, fmax, inf]) == [0, 255, 0, 0, 0, 0, 0, 255, 255, 255]).all()


def _film(rng, w, h):
    f = np.zeros((h, w, 4), np.float32)
    f[..., 0] = rng.uniform(0.5, 4.0, (h, w))
    f[..., 1:] = rng.uniform(-0.05, 1.5, (h, w, 3)) * f[..., :1]
    f[0, 0] = 0.0
    f[0, 1, 1:] = np.nan
    f[1, 2, 1:] = [3e38, 1e38, 1e38]                  # an exponent byte that wraps
    return f.reshape(-1)


def test_new_writers_reproduce_the_existing_files(tmp_path, built):
    rng = np.random.default_rng(21)
    w, h = 37, 19
    f = _film(rng, w, h)
    old_png, new_png, old_hdr, new_hdr = (str(tmp_path / n) for n in ("a.png", "b.png", "a.hdr", "b.hdr"))
    film.write_png(old_png, f, w, h)
    film.write_png_rgb8(new_png, film.rgb_pixels(f, w, h), w, h)
    assert open(old_png, "rb").read() == open(new_png, "rb").read()
    film.write_hdr(old_hdr, f, w, h)
    data = open(old_hdr, "rb").read()
    head = f"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y {h} +X {w}\n".encode()
    assert data.startswith(head) and len(data) == len(head) + 4 * w * h
    film.write_hdr_rgbe(new_hdr, np.frombuffer(data[len(head):], np.uint8), w, h)
    assert open(new_hdr, "rb").read() == data
    # the splat writer goes through the same encoder
    s = rng.uniform(0, 40.0, w * h * 3).astype(np.float32)
    lib = _ffi.host()
    assert lib.bling_host_write_png_splat(old_png.encode(), _ffi.f32ptr(f), _ffi.f32ptr(s), 0.01, w, h) == 0
    px = np.zeros(w * h * 3, np.uint8)
    lib.bling_host_rgb_pixels_splat(_ffi.f32ptr(f), _ffi.f32ptr(s), 0.01, w, h, px.ctypes.data_as(C.POINTER(C.c_uint8)))
    film.write_png_rgb8(new_png, px, w, h)
    assert open(old_png, "rb").read() == open(new_png, "rb").read()
    with pytest.raises(ValueError):
        film.write_png_rgb8(new_png, px[:-1], w, h)
    with pytest.raises(ValueError):
        film.write_hdr_rgbe(new_hdr, px, w, h)
