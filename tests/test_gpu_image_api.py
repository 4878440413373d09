"""The image API on the device (include/bling.h bling_image_add_samples[_device], bling_image_develop_device):
the film and the splat image after the call equal, bit for bit, what the host library's sequential restatement
(bling_host_image_add_samples, itself pinned to image_ref.py by test_image_api.py) makes of the same samples in
order, on every case of image_cases.py; no scene is needed and an uploaded one is left alone.
"""
import ctypes as C

import numpy as np
import pytest

import image_cases
from bling_amd import _ffi
from bling_amd import image as bimage
from bling_amd.render import Context
from bling_amd.scene import load_config

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CASES = image_cases.cases()
_shared = {}


def ctx():
    """One scene-less context for the whole module."""
    if "ctx" not in _shared:
        _shared["ctx"] = Context(0)
    return _shared["ctx"]


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a).reshape(-1), bits(b).reshape(-1))


def device_target(img, op):
    return img.splat if op == "splat" else img.film


def run_case(name, budget=0):
    flt, w, h, op, xy, sp = CASES[name]
    img = bimage.Image(flt, w, h, context=ctx())
    img.set_budget(budget)
    try:
        st = img.add_samples(xy, sp, op)
    finally:
        img.set_budget(0)
    ref = bimage.host_add_samples(img.desc, w, h, xy, sp, op)
    return img, st, ref


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_host(name):
    img, st, ref = run_case(name)
    flt, w, h, op, xy, sp = CASES[name]
    got = device_target(img, op)
    assert same(got, ref), f"{name}: {np.count_nonzero(bits(got).reshape(-1) != bits(ref).reshape(-1))} words differ"
    other = img.film if op == "splat" else img.splat
    assert not bool(torch.any(other != 0))                       # the op's own image only
    assert st.samples == len(xy) and st.dropped_spectrum == 0 and st.dropped_position == 0 and st.chunks == 1
    if name == "all_outside":
        assert st.tile_pairs == 0 and not bool(torch.any(got != 0))
    else:
        assert st.tile_pairs > 0


def test_long_segment_is_longer_than_the_lds_sort():
    img, st, ref = run_case("long_segment_add")
    assert st.tile_pairs == 9000 > 4096                          # one tile: SM_LDS_RECORDS is 4 096


def test_chunked_pair_buffer_gives_the_same_bits():
    img, st, ref = run_case("chunked", budget=512)
    assert st.chunks > 1
    assert same(img.film, ref)
    whole, st1, _ = run_case("chunked")
    assert st1.chunks == 1 and st1.tile_pairs == st.tile_pairs
    assert same(img.film, whole.film)


def test_host_buffer_variant():
    flt, w, h, op, xy, sp = CASES["size_33x18"]
    desc = bimage.image_desc(flt, w, h)
    start = np.random.default_rng(5).uniform(-1, 1, (h, w, 4)).astype(np.float32)
    got = start.copy()
    st = _ffi.ImageStats()
    rc = _ffi.hip().bling_image_add_samples(ctx()._h, C.byref(desc), 0, _ffi.f32ptr(xy), _ffi.f32ptr(sp), len(xy), _ffi.f32ptr(got),
                                            C.byref(st))
    assert rc == 0 and st.samples == len(xy)
    assert same(got, bimage.host_add_samples(desc, w, h, xy, sp, "add", target=start.copy()))


def test_tensor_inputs_are_read_in_place():
    flt, w, h, op, xy, sp = CASES["filter_gauss"]
    img = bimage.Image(flt, w, h, context=ctx())
    txy, tsp = torch.from_numpy(xy).cuda(), torch.from_numpy(sp).cuda()
    img.add_samples(txy, tsp)
    assert same(img.film, bimage.host_add_samples(img.desc, w, h, xy, sp))
    assert same(txy, xy) and same(tsp, sp)


def test_drops_are_counted_and_leave_neighbours_alone():
    xy, sp, bad = image_cases.drop_case()
    keep = np.ones(len(xy), bool)
    keep[list(bad)] = False
    for op in ("add", "add_unfiltered", "splat"):
        img = bimage.Image(image_cases.MITCHELL, 17, 16, context=ctx())
        st = img.add_samples(xy, sp, op)
        assert (st.dropped_spectrum, st.dropped_position, st.samples) == (2, 2, len(xy))
        got = device_target(img, op)
        assert bool(torch.isfinite(got).all())
        assert same(got, bimage.host_add_samples(img.desc, 17, 16, xy, sp, op))
        assert same(got, bimage.host_add_samples(img.desc, 17, 16, xy[keep], sp[keep], op))


def test_composition_and_first_operand():
    flt, w, h, op, xy, sp = CASES["size_33x18"]
    start = np.random.default_rng(3).uniform(-2, 2, (h, w, 4)).astype(np.float32)
    one = bimage.Image(flt, w, h, context=ctx())
    one.film.copy_(torch.from_numpy(start))
    two = bimage.Image(flt, w, h, context=ctx())
    two.film.copy_(torch.from_numpy(start))
    torch.cuda.synchronize()
    one.add_samples(xy, sp)
    two.add_samples(xy[:150], sp[:150])
    two.add_samples(xy[150:], sp[150:])
    assert same(one.film, two.film)
    assert same(one.film, bimage.host_add_samples(one.desc, w, h, xy, sp, target=start.copy()))


def test_no_samples_leave_the_target_as_it_was():
    img = bimage.Image(image_cases.MITCHELL, 17, 16, context=ctx())
    start = np.random.default_rng(4).uniform(-2, 2, (16, 17, 4)).astype(np.float32)
    img.film.copy_(torch.from_numpy(start))
    torch.cuda.synchronize()
    st = img.add_samples(np.zeros((0, 2), np.float32), np.zeros((0, 16), np.float32))
    assert (st.samples, st.chunks, st.tile_pairs) == (0, 0, 0)
    assert same(img.film, start)


def test_run_to_run():
    a, _, ref = run_case("filter_mitchell")
    b, _, _ = run_case("filter_mitchell")
    assert a.film.cpu().numpy().tobytes() == b.film.cpu().numpy().tobytes() == ref.tobytes()


def test_independent_of_an_uploaded_scene():
    """With C1 uploaded and one pass rendered, the image calls change nothing of the next pass and do not use
    the scene's size or filter."""
    flt, w, h, op, xy, sp = CASES["filter_sinc"]
    films = []
    for with_image_calls in (True, False):
        c = Context(0)
        c.upload(load_config("C1", "image=48,48"))
        film0, _ = c.render_pass(seed=11, pass_index=0, ordered=True)
        if with_image_calls:
            img = bimage.Image(flt, w, h, context=c)
            img.add_samples(xy, sp)
            img.add_samples(xy, sp, "splat")
            img.develop("rgb8")
            assert same(img.film, bimage.host_add_samples(img.desc, w, h, xy, sp))
            assert same(img.splat, bimage.host_add_samples(img.desc, w, h, xy, sp, "splat"))
        film1, st = c.render_pass(seed=11, pass_index=1, ordered=True)
        films.append((film0, film1, st.camera_samples))
        c.close()
    assert same(films[0][0], films[1][0]) and same(films[0][1], films[1][1]) and films[0][2] == films[1][2]


@pytest.mark.parametrize("fmt", ["rgb_f32", "rgb8", "rgbe"])
def test_develop_without_a_scene_equals_the_host(fmt, tmp_path):
    flt, w, h, op, xy, sp = CASES["filter_mitchell"]
    img = bimage.Image(flt, w, h, context=ctx())
    img.add_samples(xy, sp)
    img.add_samples(xy[:80], sp[:80], "splat")
    sw = float(np.float32(1) / np.float32(3))
    film, splat = img.film.cpu().numpy().reshape(-1), img.splat.cpu().numpy().reshape(-1)
    out = img.develop(fmt, splat_weight=sw).cpu().numpy()
    lib = _ffi.host()
    rgb = np.zeros((h, w, 3), np.float32)
    lib.bling_host_film_splat_to_rgb(_ffi.f32ptr(film), _ffi.f32ptr(splat), sw, w, h, _ffi.f32ptr(rgb))
    if fmt == "rgb_f32":
        assert np.array_equal(out, rgb, equal_nan=True)
    elif fmt == "rgb8":
        ref = np.zeros((h, w, 3), np.uint8)
        lib.bling_host_rgb_pixels_splat(_ffi.f32ptr(film), _ffi.f32ptr(splat), sw, w, h, ref.ctypes.data_as(C.POINTER(C.c_uint8)))
        assert np.array_equal(out, ref)
    else:
        path = tmp_path / "ref.hdr"
        assert lib.bling_host_write_hdr(str(path).encode(), _ffi.f32ptr(rgb), w, h) == 0
        assert out.tobytes() == path.read_bytes()[-w * h * 4:]
    # a window develops its pixels only
    part = torch.full_like(img.develop(fmt, splat_weight=sw), 7)
    img.develop(fmt, window=(2, 5, 1, 3), splat_weight=sw, out=part)
    part = part.cpu().numpy()
    assert np.array_equal(part[1:4, 2:6], out[1:4, 2:6], equal_nan=True)
    part[1:4, 2:6] = 7
    assert np.all(part == 7)


def test_bad_arguments_are_einval():
    lib = _ffi.hip()
    h = ctx()._h
    desc = bimage.image_desc(image_cases.MITCHELL, 8, 8)
    xy = torch.zeros(2 * 4, dtype=torch.float32, device="cuda")
    sp = torch.zeros(16 * 4, dtype=torch.float32, device="cuda")
    film = torch.zeros(8 * 8 * 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    P = lambda t: C.c_void_p(t.data_ptr())

    def call(d=desc, op=0, x=P(xy), s=P(sp), n=4, t=P(film), c=h):
        return lib.bling_image_add_samples_device(c, C.byref(d) if d is not None else None, op, x, s, n, t, None)

    assert call() == 0
    snap = film.clone()
    assert call(op=3) == -1 and call(op=-1) == -1
    assert call(d=None) == -1 and call(x=None) == -1 and call(s=None) == -1 and call(t=None) == -1 and call(c=None) == -1
    for w, hh, fw, fh in ((0, 8, 3, 3), (8, 0, 3, 3), (8, 8, 0, 3), (8, 8, 3, -1), (8, 8, np.inf, 3), (8, 8, 3, np.nan)):
        d = bimage.image_desc(image_cases.MITCHELL, w, hh)
        d.filter.width, d.filter.height = fw, fh
        assert call(d=d) == -1, (w, hh, fw, fh)
    assert call(x=P(film), n=4) == -1                               # the target overlaps an input
    assert call(s=C.c_void_p(film.data_ptr() + 64), n=2) == -1
    assert call(x=None, s=None, n=0) == 0                           # n == 0 needs no inputs
    assert bool(torch.equal(film, snap))                            # no refused call and no empty one wrote anything
    dp = _ffi.DevelopParams(_ffi.DEVELOP_RGB8, 0.0, (C.c_int32 * 4)(0, 7, 0, 7))
    out = torch.zeros(8 * 8 * 3, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dev = lambda d=desc, p=dp, f=P(film), o=P(out): lib.bling_image_develop_device(h, C.byref(d), C.byref(p), f, None, o)
    assert dev() == 0
    assert dev(f=None) == -1 and dev(o=None) == -1 and dev(o=P(film)) == -1
    assert dev(p=_ffi.DevelopParams(9, 0.0, (C.c_int32 * 4)(0, 7, 0, 7))) == -1
    assert dev(d=bimage.image_desc(image_cases.MITCHELL, 0, 8)) == -1
