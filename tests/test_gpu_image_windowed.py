"""The windowed image API on the device (include/bling.h bling_image_add_windowed[_device],
bling_image_scale_splats_device): film and splat after a call equal, bit for bit, what the host library's
sequential restatement (bling_host_image_add_windowed, itself pinned to image_windowed_ref.py by
test_image_windowed.py) makes of the same windows and samples -- one zeroed tile image a window, addTile in window
order -- for any windows, under any chunking, on every run; `bling --image-filters --windows N` writes the PNGs
of that restatement.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import image_cases
import image_windowed_cases as wc
from bling_amd import _ffi
from bling_amd import image as bimage
from bling_amd.render import Context
from bling_amd.scene import load_config

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CASES = wc.cases()
_shared = {}


def ctx():
    """One scene-less context for the whole module."""
    if "ctx" not in _shared:
        _shared["ctx"] = Context(0)
    return _shared["ctx"]


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def host(case, op, film=None, splat=None, stats=None):
    flt, w, h, windows, first, xy, sp = case
    return bimage.host_add_windowed(flt, w, h, windows, first, xy, sp, op, film=film, splat=splat, stats=stats)


def host_ref(name, op):
    """The host restatement of a case from zero images, computed once."""
    if (name, op) not in _shared:
        _shared[(name, op)] = host(CASES[name], op)
    return _shared[(name, op)]


def device(case, op, film=None, splat=None, budget=0, context=None):
    flt, w, h, windows, first, xy, sp = case
    img = bimage.Image(flt, w, h, context=context or ctx())
    if film is not None:
        img.film.copy_(torch.from_numpy(film))
    if splat is not None:
        img.splat.copy_(torch.from_numpy(splat))
    torch.cuda.synchronize()
    img.set_budget(budget)
    try:
        st = img.add_windowed(windows, first, xy, sp, op)
    finally:
        img.set_budget(0)
    return img, st


@pytest.mark.parametrize("op", wc.OPS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_host(name, op):
    case = CASES[name]
    img, st = device(case, op)
    film, splat = host_ref(name, op)
    assert same(img.film, film), f"{name} {op}: {np.count_nonzero(bits(img.film) != bits(film))} film words differ"
    assert same(img.splat, splat), f"{name} {op}: {np.count_nonzero(bits(img.splat) != bits(splat))} splat words differ"
    assert (st.samples, st.dropped_spectrum, st.dropped_position, st.chunks) == (len(case[5]), 0, 0, 1)
    assert st.tile_pairs > 0


def test_order_matters_for_the_chosen_inputs():
    """On the CPU: the windowed result is not the flat list's, so a flat device implementation cannot pass."""
    for name, op in (("split_2x2", "add"), ("nested", "add"), ("nested", "add_unfiltered"), ("nested", "splat")):
        flt, w, h, windows, first, xy, sp = CASES[name]
        film, splat = host_ref(name, op)
        flat = bimage.host_add_samples(flt, w, h, xy, sp, op)
        assert np.any(bits(splat if op == "splat" else film) != bits(flat)), (name, op)


@pytest.mark.parametrize("op", wc.OPS)
def test_drops_are_counted(op):
    case, (nspec, npos) = wc.drop_case()
    img, st = device(case, op)
    hs = _ffi.ImageStats()
    film, splat = host(case, op, stats=hs)
    assert (st.dropped_spectrum, st.dropped_position, st.samples) == (nspec, npos, len(case[5]))
    assert (hs.dropped_spectrum, hs.dropped_position, hs.samples) == (nspec, npos, len(case[5]))
    assert same(img.film, film) and same(img.splat, splat)
    assert bool(torch.isfinite(img.film).all()) and bool(torch.isfinite(img.splat).all())


@pytest.mark.parametrize("op", ["add", "splat"])
def test_composition_first_operand_and_run_to_run(op):
    case = CASES["nested"]
    flt, w, h, windows, first, xy, sp = case
    rng = np.random.default_rng(3)
    film0, splat0 = rng.uniform(-2, 2, (h, w, 4)).astype(np.float32), rng.uniform(-2, 2, (h, w, 3)).astype(np.float32)
    one, _ = device(case, op, film0, splat0)
    again, _ = device(case, op, film0, splat0)
    film, splat = host(case, op, film0.copy(), splat0.copy())
    assert same(one.film, film) and same(one.splat, splat)
    assert one.film.cpu().numpy().tobytes() == again.film.cpu().numpy().tobytes()
    assert one.splat.cpu().numpy().tobytes() == again.splat.cpu().numpy().tobytes()
    k = 3
    cut = int(first[k])
    two, _ = device((flt, w, h, windows[:k], first[:k + 1], xy[:cut], sp[:cut]), op, film0, splat0)
    two.add_windowed(windows[k:], first[k:] - first[k], xy[cut:], sp[cut:], op)
    assert same(one.film, two.film) and same(one.splat, two.splat)


@pytest.mark.parametrize("op", wc.OPS)
def test_chunks_cut_inside_a_window_give_the_same_bits(op):
    """split_2x2 has 500 samples a window.  A mitchell sample makes up to 4 pairs and a one-pixel op's makes one, so
    these budgets are 128 samples a chunk: every window is cut three times and its tile image carried."""
    budget = 512 if op == "add" else 128
    img, st = device(CASES["split_2x2"], op, budget=budget)
    film, splat = host_ref("split_2x2", op)
    assert st.chunks > 4
    assert same(img.film, film) and same(img.splat, splat)
    whole, st1 = device(CASES["split_2x2"], op)
    assert st1.chunks == 1 and st1.tile_pairs == st.tile_pairs


def test_chunks_end_at_window_boundaries_where_they_can():
    """nested has 150 samples a window: 1 024 pairs are 256 samples a chunk, one window each, no carry."""
    img, st = device(CASES["nested"], "add", budget=1024)
    film, splat = host_ref("nested", "add")
    assert st.chunks == 6
    assert same(img.film, film) and same(img.splat, splat)


def test_a_budget_below_one_sample_is_raised():
    case = CASES["empty_between"]
    img, st = device(case, "add", budget=1)
    film, splat = host_ref("empty_between", "add")
    assert st.chunks == len(case[5])
    assert same(img.film, film) and same(img.splat, splat)


@pytest.mark.parametrize("op", wc.OPS)
def test_add_tile_adds_its_zeros(op):
    """Trap T36 on the device: -0.0 becomes +0.0 under every tile, an empty window's too, in both images."""
    flt, w, h = image_cases.MITCHELL, 40, 24
    windows = [(2, 6, 3, 5), (20, 24, 10, 12), (30, 50, 18, 30)]
    xy = np.array([(4.5, 4.5), (3.0, 4.0)], np.float32)
    sp = wc.spectra(np.random.default_rng(1), 2)
    first = np.array([0, 2, 2, 2], np.uint64)
    case = (flt, w, h, windows, first, xy, sp)
    film0, splat0 = np.full((h, w, 4), -0.0, np.float32), np.full((h, w, 3), -0.0, np.float32)
    img, _ = device(case, op, film0, splat0)
    film, splat = host(case, op, film0.copy(), splat0.copy())
    assert same(img.film, film) and same(img.splat, splat)
    neg = bits(img.film).reshape(h, w, 4) == 0x80000000
    assert neg[0, 0].all() and not neg[4, 4].any() and not neg[11, 22].any() and not neg[23, 39].any()
    # no samples at all: the tiles' zeros are still added
    none, _ = device((flt, w, h, windows, np.zeros(4, np.uint64), xy[:0], sp[:0]), op, film0, splat0)
    film, splat = host((flt, w, h, windows, np.zeros(4, np.uint64), xy[:0], sp[:0]), op, film0.copy(), splat0.copy())
    assert same(none.film, film) and same(none.splat, splat)


def test_host_buffer_variant_and_null_images():
    case = CASES["off_edges"]
    flt, w, h, windows, first, xy, sp = case
    desc = bimage.image_desc(flt, w, h)
    rng = np.random.default_rng(5)
    film0, splat0 = rng.uniform(-1, 1, (h, w, 4)).astype(np.float32), np.full((h, w, 3), -0.0, np.float32)
    arr, f, nw = bimage._windows(windows, first, len(xy))
    fp = f.ctypes.data_as(C.POINTER(C.c_uint64))
    lib = _ffi.hip()
    film, splat = film0.copy(), splat0.copy()
    st = _ffi.ImageStats()
    rc = lib.bling_image_add_windowed(ctx()._h, C.byref(desc), 0, arr, fp, nw, _ffi.f32ptr(xy), _ffi.f32ptr(sp), len(xy), _ffi.f32ptr(film),
                                      _ffi.f32ptr(splat), C.byref(st))
    assert rc == 0 and st.samples == len(xy)
    rfilm, rsplat = host(case, "add", film0.copy(), splat0.copy())
    assert same(film, rfilm) and same(splat, rsplat)
    # the image the op does not write may be NULL: the other one gets the same bits
    film = film0.copy()
    assert lib.bling_image_add_windowed(ctx()._h, C.byref(desc), 0, arr, fp, nw, _ffi.f32ptr(xy), _ffi.f32ptr(sp), len(xy), _ffi.f32ptr(film),
                                        None, None) == 0
    assert same(film, rfilm)
    splat = splat0.copy()
    assert lib.bling_image_add_windowed(ctx()._h, C.byref(desc), 2, arr, fp, nw, _ffi.f32ptr(xy), _ffi.f32ptr(sp), len(xy), None,
                                        _ffi.f32ptr(splat), None) == 0
    assert same(splat, host(case, "splat", False, splat0.copy())[1])


def test_tensor_inputs_are_read_in_place():
    case = CASES["split_2x2"]
    flt, w, h, windows, first, xy, sp = case
    img = bimage.Image(flt, w, h, context=ctx())
    txy, tsp = torch.from_numpy(xy).cuda(), torch.from_numpy(sp).cuda()
    img.add_windowed(windows, np.diff(first.astype(np.int64)), txy, tsp)          # counts instead of offsets
    assert same(img.film, host_ref("split_2x2", "add")[0])
    assert same(txy, xy) and same(tsp, sp)
    assert img.tile(windows[1]) == bimage.image_tile(img.desc, windows[1])


def test_scale_splats_then_develop():
    case = CASES["nested"]
    flt, w, h, windows, first, xy, sp = case
    img, _ = device(case, "splat")
    img.add_windowed(windows, first, xy, sp, "add")
    film, splat = host_ref("nested", "splat")[0].copy(), host_ref("nested", "splat")[1].copy()
    film, splat = host(case, "add", film, splat)
    rng = np.random.default_rng(8)
    factors = rng.uniform(0, 2, (h, w)).astype(np.float32)
    factors[0, 0] = -0.0
    img.scale_splats(torch.from_numpy(factors).cuda())
    bimage.host_scale_splats(img.desc, splat, factors)
    assert same(img.splat, splat)
    s = np.float32(1) / np.float32(3)
    img.scale_splats(s)
    bimage.host_scale_splats(img.desc, splat, s)
    assert same(img.splat, splat) and same(img.film, film)
    out = img.develop("rgb8", splat_weight=1.0).cpu().numpy()
    ref = np.zeros((h, w, 3), np.uint8)
    _ffi.host().bling_host_rgb_pixels_splat(_ffi.f32ptr(film.reshape(-1)), _ffi.f32ptr(splat.reshape(-1)), 1.0, w, h,
                                            ref.ctypes.data_as(C.POINTER(C.c_uint8)))
    assert np.array_equal(out, ref)


def test_refusals_leave_the_targets_alone_and_the_context_serving():
    lib = _ffi.hip()
    h = ctx()._h
    desc = bimage.image_desc(image_cases.MITCHELL, 8, 8)
    xy = torch.full((2 * 4,), 3.5, dtype=torch.float32, device="cuda")
    sp = torch.ones(16 * 4, dtype=torch.float32, device="cuda")
    film = torch.zeros(8 * 8 * 4, dtype=torch.float32, device="cuda")
    splat = torch.zeros(8 * 8 * 3, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    P = lambda t: C.c_void_p(t.data_ptr())
    wins = (_ffi.ImageWindow * 2)(_ffi.ImageWindow(0, 7, 0, 3), _ffi.ImageWindow(0, 7, 4, 7))
    U = lambda *v: (C.c_uint64 * len(v))(*v)

    def call(d=desc, op=0, w=wins, f=U(0, 2, 4), nw=2, x=P(xy), s=P(sp), n=4, t=P(film), u=P(splat), c=h):
        return lib.bling_image_add_windowed_device(c, C.byref(d) if d is not None else None, op, w, f, nw, x, s, n, t, u, None)

    assert call() == 0
    snap, ssnap = film.clone(), splat.clone()
    assert bool(torch.any(snap != 0))
    refused = [dict(op=3), dict(d=None), dict(c=None), dict(w=None), dict(f=None), dict(x=None), dict(s=None), dict(t=None),
               dict(op=2, u=None),                                   # the image the op writes
               dict(f=U(0, 3, 2)), dict(f=U(0, 2, 3)), dict(f=U(1, 2, 4)), dict(f=U(0, 2, 5)),   # not ascending / not 0 .. n
               dict(w=(_ffi.ImageWindow * 2)(_ffi.ImageWindow(0, 7, 0, 3), _ffi.ImageWindow(-9, -3, 0, 7))),   # w = -3 - 0 + 3 < 1
               dict(w=(_ffi.ImageWindow * 2)(_ffi.ImageWindow(0, 7, 5, 1), _ffi.ImageWindow(0, 7, 4, 7))),     # h = 1 - 5 + 3 < 1
               dict(x=P(film)), dict(s=C.c_void_p(splat.data_ptr() + 64), n=2, f=U(0, 1, 2)),                 # a target overlaps an input
               dict(u=C.c_void_p(film.data_ptr() + 16))]                                                      # film overlaps splat
    for kw in refused:
        assert call(**kw) == -1, kw
        assert bool(torch.equal(film, snap)) and bool(torch.equal(splat, ssnap)), kw
    d0 = bimage.image_desc(image_cases.MITCHELL, 8, 8)
    d0.filter.width = np.nan
    assert call(d=d0) == -1
    assert lib.bling_image_scale_splats_device(h, C.byref(desc), None, None, 1.0) == -1
    assert lib.bling_image_scale_splats_device(h, C.byref(desc), P(splat), P(splat), 1.0) == -1
    assert bool(torch.equal(film, snap)) and bool(torch.equal(splat, ssnap))
    assert call(nw=0, f=U(0), x=None, s=None, n=0) == 0             # nothing to do
    assert bool(torch.equal(film, snap))
    assert call() == 0                                               # the context still serves
    assert not bool(torch.equal(film, snap))


def test_independent_of_an_uploaded_scene():
    """With C1 uploaded at 16 x 16 and one ordered pass rendered, the windowed calls change nothing of the next
    pass and do not use the scene's size or filter."""
    case = CASES["nested"]
    films = []
    for with_image_calls in (True, False):
        c = Context(0)
        c.upload(load_config("C1", "image=16,16"))
        film0, _ = c.render_pass(seed=11, pass_index=0, ordered=True)
        if with_image_calls:
            img, _ = device(case, "add", context=c)
            img.add_windowed(case[3], case[4], case[5], case[6], "splat")
            img.scale_splats(0.5)
            film, splat = host_ref("nested", "add")
            assert same(img.film, film)
        film1, st = c.render_pass(seed=11, pass_index=1, ordered=True)
        films.append((film0, film1, st.camera_samples))
        c.close()
    assert same(films[0][0], films[1][0]) and same(films[0][1], films[1][1]) and films[0][2] == films[1][2]


def test_cli_windows(tmp_path):
    """`bling --image-filters --windows 4`: the test images are those of the host restatement over splitWindow's
    16 x 16 windows of the extent, the same on every run; without the flag the files are the flat path's."""
    import test_gpu_image_filters_cli as cli
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "bling_amd", "_lib", "bling")
    outs = []
    for run, extra in (("a", ["--windows", "4"]), ("b", ["--windows", "4"]), ("c", [])):
        d = tmp_path / run
        d.mkdir()
        r = subprocess.run([exe, "--image-filters", "--size", f"{cli.W}x{cli.H}", "--out", str(d)] + extra, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append({n: open(d / n, "rb").read() for n in sorted(os.listdir(d))})
    assert outs[0] == outs[1]
    assert sorted(outs[0]) == sorted(outs[2]) == sorted(f"filter-{k}-{n}.png" for k in ("show", "test") for n, _ in cli.FILTERS)
    differ = 0
    for name, spec in cli.FILTERS:
        desc, xy, spectra = cli.zone_samples(spec)
        x0, x1, y0, y1 = bimage.image_extent(desc)
        nx, ny = x1 - x0 + 1, y1 - y0 + 1
        xy, spectra = xy.reshape(ny, nx, 25, 2), spectra.reshape(ny, nx, 25, 16)
        windows, counts, wxy, wsp = [], [], [], []
        for wy in range(y0, y1 + 1, 16):                              # splitWindow (Sampling.hs:55-58)
            for wx in range(x0, x1 + 1, 16):
                wnd = (wx, min(wx + 15, x1), wy, min(wy + 15, y1))
                rows, cols = slice(wnd[2] - y0, wnd[3] - y0 + 1), slice(wnd[0] - x0, wnd[1] - x0 + 1)
                windows.append(wnd)
                wxy.append(xy[rows, cols].reshape(-1, 2))
                wsp.append(spectra[rows, cols].reshape(-1, 16))
                counts.append(len(wxy[-1]))
        film, _ = bimage.host_add_windowed(desc, desc.width, desc.height, windows, counts, np.concatenate(wxy), np.concatenate(wsp), "add",
                                           splat=False)
        path = tmp_path / "ref.png"
        assert _ffi.host().bling_host_write_png(str(path).encode(), _ffi.f32ptr(film.reshape(-1)), desc.width, desc.height) == 0
        assert outs[0][f"filter-test-{name}.png"] == path.read_bytes(), name
        assert outs[2][f"filter-test-{name}.png"] == cli.reference_png(tmp_path / "flat.png", desc, xy.reshape(-1, 2), spectra.reshape(-1, 16)), name
        assert outs[0][f"filter-show-{name}.png"] == outs[2][f"filter-show-{name}.png"]
        differ += outs[0][f"filter-test-{name}.png"] != outs[2][f"filter-test-{name}.png"]
    assert differ > 0                                                 # a tile does not reach left of or above its window
