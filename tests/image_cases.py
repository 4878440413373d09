"""The cases of the image API tests (test_image_api.py on the CPU, test_gpu_image_api.py on the device): each
is the smallest at which one thing can go wrong.  Positions are multiples of 1/8, so every dx +- fw is exact in
binary32; spectra are float32 in [-1, 4) with finite XYZ.  A case is (filter, width, height, op, xy, spectra).
"""
import numpy as np

f32 = np.float32
MITCHELL = ("mitchell", 3, 3, 1 / 3, 1 / 3)
FILTERS = {"box": ("box",), "gauss": ("gauss", 3, 3, 2), "sinc": ("sinc", 3, 3, 3), "mitchell": MITCHELL,
           "triangle": ("triangle", 3, 3)}
T12 = {"mitchell32": ("mitchell", 3, 2, 1 / 3, 1 / 3), "triangle23": ("triangle", 2, 3)}


def positions(rng, n, lo, hi):
    """n (x, y) pairs, multiples of 1/8 in [lo, hi) on both axes (lo, hi are (x, y) pairs)."""
    x = rng.integers(int(lo[0] * 8), int(hi[0] * 8), n) / 8.0
    y = rng.integers(int(lo[1] * 8), int(hi[1] * 8), n) / 8.0
    return np.stack([x, y], 1).astype(f32)


def spectra(rng, n):
    return rng.uniform(-1.0, 4.0, (n, 16)).astype(f32)


def around(rng, n, w, h, m=4.0):
    """Positions over the image and a margin of m beyond every edge: inside, on the rim and outside."""
    return positions(rng, n, (-m, -m), (w + m, h + m))


def boundary_positions(w, h, fw):
    """Every pair of the axis values at which ceil / floor sit on an exact boundary: dx +- fw integral
    (k + 1/2), the image edges and the filter's reach beyond them."""
    xs = [-fw, -fw + 0.5, -0.5, 0.0, 0.5, 1.0, w - 0.5, float(w), w + 0.5, w + fw - 0.5, w + fw, w + fw + 0.5]
    ys = [-fw, -0.5, 0.0, 0.5, h - 0.5, float(h), h + fw, h + fw + 0.5]
    return np.array([(x, y) for y in ys for x in xs], f32)


def pixel_positions(w, h):
    """The single-pixel ops at the edges: x = -0.125, 0, W - 0.125, W and the same in y."""
    xs = [-0.125, 0.0, 0.875, w - 0.125, float(w)]
    ys = [-0.125, 0.0, h - 0.125, float(h)]
    return np.array([(x, y) for y in ys for x in xs], f32)


def cases():
    rng = np.random.default_rng(20261020)
    out = {}
    out["one_pixel"] = (MITCHELL, 1, 1, "add", positions(rng, 300, (-4, -4), (5, 5)), None)
    for w, h in ((5, 3), (17, 16), (33, 18)):
        out[f"size_{w}x{h}"] = (MITCHELL, w, h, "add", around(rng, 400, w, h), None)
    out["boundaries"] = (MITCHELL, 17, 16, "add", boundary_positions(17, 16, 3.0), None)
    out["boundaries_box"] = (("box",), 17, 16, "add", boundary_positions(17, 16, 0.5), None)
    for op in ("add_unfiltered", "splat"):
        out[f"edges_{op}"] = (MITCHELL, 17, 16, op, np.concatenate([pixel_positions(17, 16), around(rng, 200, 17, 16, 1.0)]), None)
    for name, flt in {**FILTERS, **T12}.items():
        out[f"filter_{name}"] = (flt, 17, 16, "add", around(rng, 300, 17, 16), None)
    for op in ("add", "add_unfiltered", "splat"):
        out[f"long_segment_{op}"] = (MITCHELL, 2, 2, op, positions(rng, 9000, (0, 0), (2, 2)), None)
    out["chunked"] = (MITCHELL, 33, 18, "add", around(rng, 2000, 33, 18), None)
    out["all_outside"] = (MITCHELL, 17, 16, "add", positions(rng, 50, (30, 30), (40, 40)), None)
    return {k: (f, w, h, op, xy, spectra(rng, len(xy)) if s is None else s) for k, (f, w, h, op, xy, s) in out.items()}


def drop_case():
    """17 x 16 mitchell: a NaN band, a +Inf band, a NaN x and x = 2^21 among ordinary neighbours.
    Returns (xy, spectra, the indices of the four)."""
    rng = np.random.default_rng(7)
    xy, sp = around(rng, 60, 17, 16, 2.0), spectra(rng, 60)
    xy[10] = (8.0, 8.0); sp[10, 3] = np.nan
    xy[20] = (8.5, 7.0); sp[20, 15] = np.inf
    xy[30, 0] = np.nan
    xy[40, 0] = 2.0 ** 21
    return xy, sp, (10, 20, 30, 40)
