"""The host side of the image API (include/bling_host.h): bling_host_image_add_samples -- the parity yardstick
of the device calls -- equals the independent numpy restatement (image_ref.py) bit for bit on every case of
image_cases.py; bling_host_make_filter equals the table of a loaded job with the same `filter` line;
bling_host_image_extent equals sampleExtent's formula; the ABI symbols are exported.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import image_cases
import image_ref
from bling_amd import _ffi
from bling_amd import image as bimage
from bling_amd.scene import parse_job

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = image_cases.cases()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def table_of(desc):
    return np.array(desc.filter.table, np.float32), (desc.filter.width, desc.filter.height)


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_equals_numpy_restatement(built, name):
    flt, w, h, op, xy, sp = CASES[name]
    desc = bimage.image_desc(flt, w, h)
    table, fsize = table_of(desc)
    got = bimage.host_add_samples(desc, w, h, xy, sp, op)
    ref = image_ref.add_samples(table, fsize, w, h, xy, sp, op)
    assert got.shape == ref.shape
    assert np.array_equal(bits(got), bits(ref)), f"{name}: {np.count_nonzero(bits(got) != bits(ref))} words differ"
    if name != "all_outside":
        assert np.any(got != 0)
    else:
        assert not np.any(got != 0)


def test_host_first_operand_and_composition(built):
    flt, w, h, op, xy, sp = CASES["size_33x18"]
    desc = bimage.image_desc(flt, w, h)
    table, fsize = table_of(desc)
    start = np.random.default_rng(3).uniform(-2, 2, (h, w, 4)).astype(np.float32)
    one = bimage.host_add_samples(desc, w, h, xy, sp, op, target=start.copy())
    two = bimage.host_add_samples(desc, w, h, xy[:150], sp[:150], op, target=start.copy())
    two = bimage.host_add_samples(desc, w, h, xy[150:], sp[150:], op, target=two)
    assert np.array_equal(bits(one), bits(two))
    assert np.array_equal(bits(one), bits(image_ref.add_samples(table, fsize, w, h, xy, sp, op, target=start)))


def test_host_drops(built):
    xy, sp, bad = image_cases.drop_case()
    desc = bimage.image_desc(image_cases.MITCHELL, 17, 16)
    table, fsize = table_of(desc)
    keep = np.ones(len(xy), bool)
    keep[list(bad)] = False
    got = bimage.host_add_samples(desc, 17, 16, xy, sp)
    assert np.isfinite(got).all()
    assert np.array_equal(bits(got), bits(bimage.host_add_samples(desc, 17, 16, xy[keep], sp[keep])))
    assert np.array_equal(bits(got), bits(image_ref.add_samples(table, fsize, 17, 16, xy, sp)))
    pos, spec = image_ref.dropped(xy, sp)
    assert (int(pos.sum()), int(spec.sum())) == (2, 2)


def test_host_rejects_bad_arguments(built):
    lib = _ffi.host()
    desc = bimage.image_desc(image_cases.MITCHELL, 4, 4)
    xy, sp, t = np.zeros(2, np.float32), np.zeros(16, np.float32), np.zeros(64, np.float32)
    call = lambda d, op: lib.bling_host_image_add_samples(C.byref(d), op, _ffi.f32ptr(xy), _ffi.f32ptr(sp), 1, _ffi.f32ptr(t))
    assert call(desc, 0) == 0
    assert call(desc, 3) != 0
    for w, h, fw in ((0, 4, 3.0), (4, -1, 3.0), (4, 4, 0.0), (4, 4, -1.0), (4, 4, np.inf), (4, 4, np.nan)):
        d = bimage.image_desc(image_cases.MITCHELL, w, h)
        d.filter.width = fw
        assert call(d, 0) != 0, (w, h, fw)


@pytest.mark.parametrize("line,spec", [("box", ("box",)), ("gauss 3 3 2", ("gauss", 3, 3, 2)), ("sinc 3 3 3", ("sinc", 3, 3, 3)),
                                       ("mitchell 3 2 0.25 0.5", ("mitchell", 3, 2, 0.25, 0.5)),
                                       ("triangle 2 3", ("triangle", 2, 3))])
def test_make_filter_equals_loaded_job(built, tmp_path, line, spec):
    # the small Cornell box with its `filter` line replaced (gauss and sinc have no override)
    text = open(os.path.join(ROOT, "fixtures", "scenes", "cornell-box.bling")).read()
    assert "\nfilter mitchell 2 2 0.333333 0.333333\n" in text
    scene = tmp_path / "filter.bling"
    scene.write_text(text.replace("\nfilter mitchell 2 2 0.333333 0.333333\n", f"\nfilter {line}\n"))
    job = parse_job(str(scene), "image=8,8")
    flt = bimage.make_filter(spec)
    assert np.array_equal(bits(np.array(flt.table, np.float32)), bits(np.asarray(job.filter_table(), np.float32).reshape(-1)))
    assert (flt.width, flt.height) == tuple(np.float32(v) for v in job.filter_size)
    # the table is evalFilter at the cell centres (mkTableFilter, Image.hs:48-61)
    fw, fh = np.float32(flt.width), np.float32(flt.height)
    for ty, tx in ((0, 0), (3, 11), (15, 15)):
        fx = (np.float32(tx) + np.float32(0.5)) * fw / np.float32(16)
        fy = (np.float32(ty) + np.float32(0.5)) * fh / np.float32(16)
        assert bits(bimage.eval_filter(spec, fx, fy)) == bits(np.float32(flt.table[ty * 16 + tx]))


def test_make_filter_rejects(built):
    with pytest.raises(ValueError):
        bimage.make_filter(("gauss", 3, 3))
    with pytest.raises(ValueError):
        bimage.make_filter(("lanczos", 3, 3))


@pytest.mark.parametrize("spec,w,h", [(("box",), 64, 64), (image_cases.MITCHELL, 480, 270), (("triangle", 2, 3), 5, 3),
                                      (("gauss", 1.25, 0.75, 2), 17, 16)])
def test_extent_equals_formula(built, spec, w, h):
    desc = bimage.image_desc(spec, w, h)
    assert bimage.image_extent(desc) == image_ref.extent(w, h, desc.filter.width, desc.filter.height)


def test_rgb_to_spectrum_illum_is_linear_in_grey(built):
    s1 = bimage.rgb_to_spectrum_illum([[0.5, 0.5, 0.5]])[0]
    s0 = bimage.rgb_to_spectrum_illum([[0.0, 0.0, 0.0]])[0]
    assert s1.shape == (16,) and np.all(s0 == 0) and np.all(s1 > 0)


def test_abi_symbols_exported(built):
    hip = os.path.join(ROOT, "bling_amd", "_lib", "libbling_hip.so")
    host = os.path.join(ROOT, "bling_amd", "_lib", "libbling_host.so")
    for path, names in ((hip, ["bling_image_add_samples_device", "bling_image_add_samples", "bling_image_develop_device",
                               "bling_debug_set_image_budget"]),
                        (host, ["bling_host_make_filter", "bling_host_eval_filter", "bling_host_image_extent",
                                "bling_host_image_add_samples", "bling_host_rgb_to_spectrum_illum"])):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        exported = {line.split()[-1] for line in syms.splitlines() if line.strip()}
        for n in names:
            assert n in exported, f"{n} is not exported by {os.path.basename(path)}"
    for n in ("bling_image_add_samples_device", "bling_image_add_samples", "bling_image_develop_device",
              "bling_debug_set_image_budget"):
        assert n in _ffi.HIP_SYMBOLS
