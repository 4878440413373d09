"""The host side of the windowed image API (include/bling_host.h): bling_host_image_tile equals mkImageTile and the
tile's sampleExtent; bling_host_image_add_windowed -- the parity yardstick of bling_image_add_windowed[_device] --
equals, bit for bit, an independent numpy restatement of Image.hs (image_windowed_ref.py) and is NOT the flat
list's result; addTile's zeros turn a -0.0 under a tile into +0.0 (trap T36); bling_host_image_scale_splats is one
binary32 product a value.  No GPU.
"""
import ctypes as C

import numpy as np
import pytest

import image_cases
import image_windowed_cases as wc
import image_windowed_ref as wref
from bling_amd import _ffi
from bling_amd import image as bimage

CASES = wc.cases()
TILE_FILTERS = {"box": ("box",), "triangle": ("triangle", 3, 3), "mitchell": image_cases.MITCHELL, "gauss": ("gauss", 3, 3, 2)}
# inside, across each edge, negative starts, one pixel, a single kept column, far outside
TILE_WINDOWS = [(5, 20, 4, 15), (-3, 12, 3, 9), (30, 50, 3, 9), (4, 9, -7, 3), (4, 9, 20, 33), (-9, -1, -9, -1), (7, 7, 9, 9), (0, 0, 0, 0),
                (39, 39, 23, 23), (-20, -2, 0, 5), (100, 120, 50, 60)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1)


def host(case, op, film=None, splat=None, stats=None):
    flt, w, h, windows, first, xy, sp = case
    return bimage.host_add_windowed(flt, w, h, windows, first, xy, sp, op, film=film, splat=splat, stats=stats)


def ref(case, op, film=None, splat=None):
    flt, w, h, windows, first, xy, sp = case
    d = bimage.image_desc(flt, w, h)
    film = np.zeros((h, w, 4), np.float32) if film is None else film
    splat = np.zeros((h, w, 3), np.float32) if splat is None else splat
    return wref.add_windowed(np.array(d.filter.table), (d.filter.width, d.filter.height), w, h, windows, first, xy, sp, op, film, splat)


@pytest.mark.parametrize("name", sorted(TILE_FILTERS))
def test_tile_geometry_equals_mk_image_tile(name):
    desc = bimage.image_desc(TILE_FILTERS[name], 40, 24)
    fw, fh = desc.filter.width, desc.filter.height
    for wnd in TILE_WINDOWS:
        px, py, w, h = wref.mk_image_tile((wnd[0], wnd[1], wnd[2], wnd[3]), fw, fh)
        if w < 1 or h < 1:
            with pytest.raises(ValueError):
                bimage.image_tile(desc, wnd)
            continue
        got = bimage.image_tile(desc, wnd)
        assert (got["px"], got["py"], got["w"], got["h"]) == (px, py, w, h), (name, wnd)
        assert got["extent"] == wref.tile_extent(px, py, w, h, fw, fh), (name, wnd)


def test_tile_below_one_pixel_is_refused():
    desc = bimage.image_desc(image_cases.MITCHELL, 40, 24)
    for wnd in ((-20, -3, 0, 5), (0, 5, -20, -3), (10, 6, 0, 5), (-9, -4, -9, -4)):
        with pytest.raises(ValueError):
            bimage.image_tile(desc, wnd)
    assert bimage.image_tile(desc, (-20, -2, 0, 5))["w"] == 1
    box = bimage.image_desc(("box",), 40, 24)
    with pytest.raises(ValueError):
        bimage.image_tile(box, (-5, -1, 0, 0))                      # w = -1 - 0 + 1
    lib = _ffi.host()
    assert lib.bling_host_image_tile(None, None, None) == -1


@pytest.mark.parametrize("op", wc.OPS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_equals_the_numpy_restatement(name, op):
    case = CASES[name]
    st = _ffi.ImageStats()
    film, splat = host(case, op, stats=st)
    rfilm, rsplat = ref(case, op)
    assert np.array_equal(bits(film), bits(rfilm)), f"{name} {op}: {np.count_nonzero(bits(film) != bits(rfilm))} film words differ"
    assert np.array_equal(bits(splat), bits(rsplat))
    assert (st.samples, st.dropped_spectrum, st.dropped_position) == (len(case[5]), 0, 0)
    target = splat if op == "splat" else film
    assert np.any(target != 0) and not np.any((film if op == "splat" else splat) != 0)


@pytest.mark.parametrize("name,op", [("split_2x2", "add"), ("nested", "add"), ("nested", "add_unfiltered"), ("nested", "splat"),
                                     ("outside_own_tile", "add_unfiltered")])
def test_windowed_is_not_the_flat_list(name, op):
    """Per-window partial sums are added to the film, and a tile does not reach left of or above its window: a
    flat implementation cannot pass."""
    flt, w, h, windows, first, xy, sp = CASES[name]
    film, splat = host(CASES[name], op)
    flat = bimage.host_add_samples(flt, w, h, xy, sp, op)
    assert np.any(bits(splat if op == "splat" else film) != bits(flat))


def test_incoming_values_are_the_first_operand_and_calls_compose():
    case = CASES["nested"]
    flt, w, h, windows, first, xy, sp = case
    rng = np.random.default_rng(2)
    film0, splat0 = rng.uniform(-2, 2, (h, w, 4)).astype(np.float32), rng.uniform(-2, 2, (h, w, 3)).astype(np.float32)
    film, splat = host(case, "add", film0.copy(), splat0.copy())
    rfilm, rsplat = ref(case, "add", film0.copy(), splat0.copy())
    assert np.array_equal(bits(film), bits(rfilm)) and np.array_equal(bits(splat), bits(rsplat))
    k = 3
    cut = int(first[k])
    a = (flt, w, h, windows[:k], first[:k + 1], xy[:cut], sp[:cut])
    b = (flt, w, h, windows[k:], first[k:] - first[k], xy[cut:], sp[cut:])
    f2, s2 = host(a, "add", film0.copy(), splat0.copy())
    f2, s2 = host(b, "add", f2, s2)
    assert np.array_equal(bits(film), bits(f2)) and np.array_equal(bits(splat), bits(s2))


def test_drops_are_counted():
    case, (nspec, npos) = wc.drop_case()
    for op in wc.OPS:
        st = _ffi.ImageStats()
        film, splat = host(case, op, stats=st)
        assert (st.dropped_spectrum, st.dropped_position, st.samples) == (nspec, npos, len(case[5]))
        rfilm, rsplat = ref(case, op)
        assert np.array_equal(bits(film), bits(rfilm)) and np.array_equal(bits(splat), bits(rsplat))
        assert np.isfinite(film).all() and np.isfinite(splat).all()


@pytest.mark.parametrize("op", wc.OPS)
def test_add_tile_adds_its_zeros(op):
    """Trap T36: -0.0 becomes +0.0 under every tile -- an empty window's too, in the image the op does not write
    too -- and stays -0.0 elsewhere."""
    flt, w, h = image_cases.MITCHELL, 40, 24
    windows = [(2, 6, 3, 5), (20, 24, 10, 12), (30, 50, 18, 30)]
    xy = np.array([(4.5, 4.5), (3.0, 4.0)], np.float32)               # window 0 only; the others are empty
    sp = wc.spectra(np.random.default_rng(1), 2)
    first = [0, 2, 2, 2]
    film, splat = np.full((h, w, 4), -0.0, np.float32), np.full((h, w, 3), -0.0, np.float32)
    bimage.host_add_windowed(flt, w, h, windows, first, xy, sp, op, film=film, splat=splat)
    under = np.zeros((h, w), bool)
    for wnd in windows:
        px, py, tw, th = wref.mk_image_tile(wnd, 3, 3)
        under[py:py + th, px:px + tw] = True
    assert under.any() and not under.all()
    for img in (film, splat):
        b = img.view(np.uint32)
        assert np.all(b[~under] == 0x80000000)
        assert not np.any(b[under] == 0x80000000)
    rfilm, rsplat = np.full((h, w, 4), -0.0, np.float32), np.full((h, w, 3), -0.0, np.float32)
    d = bimage.image_desc(flt, w, h)
    wref.add_windowed(np.array(d.filter.table), (3, 3), w, h, windows, first, xy, sp, op, rfilm, rsplat)
    assert np.array_equal(bits(film), bits(rfilm)) and np.array_equal(bits(splat), bits(rsplat))
    # an image given as NULL is not touched, and the other still is
    keep = np.full((h, w, 3 if op != "splat" else 4), -0.0, np.float32)
    only = np.full((h, w, 4 if op != "splat" else 3), -0.0, np.float32)
    if op == "splat":
        bimage.host_add_windowed(flt, w, h, windows, first, xy, sp, op, film=False, splat=only)
    else:
        bimage.host_add_windowed(flt, w, h, windows, first, xy, sp, op, film=only, splat=False)
    assert np.array_equal(bits(only), bits(splat if op == "splat" else film))


def test_bad_arguments_leave_the_images_alone():
    flt, w, h, windows, first, xy, sp = CASES["nested"]
    film = np.full((h, w, 4), 1.5, np.float32)
    splat = np.full((h, w, 3), 2.5, np.float32)
    call = lambda **k: bimage.host_add_windowed(flt, w, h, k.get("windows", windows), k.get("first", first), xy, sp, k.get("op", "add"),
                                                film=k.get("film", film), splat=k.get("splat", splat))
    bad = first.copy(); bad[2], bad[3] = bad[3], bad[2]
    short = first.copy(); short[-1] -= 1
    late = first.copy(); late[0] = 1
    for kw in ({"first": bad}, {"first": short}, {"first": late}, {"windows": windows[:-1] + [(-20, -3, 0, 5)]}, {"film": False},
               {"op": "splat", "splat": False}):
        with pytest.raises(ValueError):
            call(**kw)
    assert np.all(film == 1.5) and np.all(splat == 2.5)


def test_scale_splats_is_one_product_a_value():
    rng = np.random.default_rng(9)
    w, h = 13, 7
    desc = bimage.image_desc(("box",), w, h)
    splat = (10.0 ** rng.uniform(-3, 4, (h, w, 3)) * rng.choice([-1, 1], (h, w, 3))).astype(np.float32)
    factors = rng.uniform(0, 3, (h, w)).astype(np.float32)
    factors[0, 0], factors[1, 1] = 0.0, -0.0
    got = bimage.host_scale_splats(desc, splat.copy(), factors)
    assert np.array_equal(bits(got), bits(wref.scale_splats(splat, factors)))
    assert np.array_equal(bits(got), bits(splat * factors[:, :, None]))
    s = np.float32(1) / np.float32(7)
    got = bimage.host_scale_splats(desc, splat.copy(), s)
    assert np.array_equal(bits(got), bits(splat * s))


def test_symbols_are_exported_and_declared():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hip, hosth = open(os.path.join(root, "include", "bling.h")).read(), open(os.path.join(root, "include", "bling_host.h")).read()
    for n in ("bling_image_add_windowed_device", "bling_image_add_windowed", "bling_image_scale_splats_device"):
        assert n in hip and n in _ffi.HIP_SYMBOLS
    lib = _ffi.host()
    for n in ("bling_host_image_tile", "bling_host_image_add_windowed", "bling_host_image_scale_splats"):
        assert n in hosth and hasattr(lib, n)
    assert C.sizeof(_ffi.ImageWindow) == 16 and C.sizeof(_ffi.ImageTile) == 32
