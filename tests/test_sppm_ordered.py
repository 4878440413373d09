"""The order of SPPM's photon image (BLING_SPLAT_ORDERED, include/bling.h), on the CPU.

The reference forms the image of a pass in two levels (Renderer/SPPM.hs:441-453): every photon sampler
("thread") k splats into an image of its own, from zero, one splat at a time; the samplers' images are then
added in k order.  tests/ref/sppm_ref.cpp writes the splats out as records; folded in those two levels in
numpy binary32 they must give oracle_sppm_pass's image bit for bit -- which pins the records (values, pixels
and order) to the oracle's -- and folded flat they must not, which shows that the order is observable and
the test has power.
"""
import ctypes as C

import numpy as np
import pytest

from bling_amd import _ffi
from bling_amd.scene import load_config
from oracle_py import OracleSppm

import sppm_ref

SEED = 0x0B11A6
CASES = {"X13": ("X13", "image=48,36;sppm=20000,6,0.25;sppm_threads=4", 4621),
         "X5": ("X5", "image=40,40;sppm_threads=4", 23121)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_two_level_fold_of_the_records_is_the_oracles_splat_image(name):
    scene, ov, pairs1 = CASES[name]
    job = load_config(scene, ov)
    w, h = job.width, job.height
    nth = max(1, job.config.sppm_threads)
    ref = sppm_ref.SppmRef(job)
    ora = OracleSppm(job)
    film = np.zeros(w * h * 4, np.float32)
    splat = np.zeros(w * h * 3, np.float32)
    mine = np.zeros(w * h * 3, np.float32)
    flat = np.zeros(w * h * 3, np.float32)
    for p in (1, 2):
        rec, rst = ref.records(SEED, p)                  # for the radii before the pass
        film, splat, st = ora.render_pass(seed=SEED, pass_index=p, film=film, splat=splat)
        ref.advance(SEED, p)
        assert rst.counts() == [st.hitpoints, st.photons, st.photon_rays, st.photon_hits]
        if p == 1:
            assert st.photon_hits == pairs1
        # sorted by (thread, photon, seq) as delivered; seq counts every pair of the photon
        key = (rec["thread"].astype(np.uint64) << np.uint64(48)) | (rec["photon"].astype(np.uint64) << np.uint64(24)) | rec["seq"]
        assert (np.diff(key.astype(np.int64)) > 0).all()
        assert len(rec) <= st.photon_hits and (rec["sx"] >= 0).all() and (rec["sx"] < w).all() and (rec["sy"] < h).all()
        mine = sppm_ref.fold_two_level(rec, nth, w, h, image=mine)
        flat = sppm_ref.fold_flat(rec, w, h, image=flat)
        assert np.array_equal(mine.view(np.uint32), splat.view(np.uint32)), (name, p, int((mine != splat).sum()))
    r2a, na = ora.pixel_stats()
    r2b = np.zeros_like(r2a); nb = np.zeros_like(na)
    sppm_ref.lib().oracle_sppm_pixel_stats(ref._h, r2b.ctypes.data_as(sppm_ref.f32p), nb.ctypes.data_as(sppm_ref.f32p))
    assert np.array_equal(r2a, r2b) and np.array_equal(na, nb)
    # the flat fold -- one image for all samplers -- is another sum
    ndiff = int((flat.view(np.uint32) != splat.view(np.uint32)).reshape(-1, 3).any(axis=1).sum())
    print(f"{name}: flat fold differs from the two-level image on {ndiff} pixels")
    assert ndiff >= 1
    ref.close(); ora.close()


def test_fold_helpers_add_one_at_a_time():
    """fold_flat adds a pixel's splats in their order, in binary32: a case where the order shows."""
    rec = np.zeros(3, sppm_ref.RECORD)
    rec["x"] = [1.0, 2.0 ** -24, 2.0 ** -24]
    rec["thread"] = [0, 1, 1]
    a = sppm_ref.fold_flat(rec, 1, 1)
    b = sppm_ref.fold_two_level(rec, 2, 1, 1)
    assert a[0] == np.float32(1.0)                                  # (1 + e) + e, each e lost
    assert b[0] == np.float32(1.0) + np.float32(2.0 ** -23)         # 1 + (e + e)


@pytest.mark.parametrize("case", ["X5:", "X5:image=40,40;sppm_threads=4", "X13:image=48,36;sppm=20000,6,0.25;sppm_threads=4",
                                  "X13:sppm=1000,3,2.5;sppm_threads=3;image=16,16"])
def test_cli_splat_weight_is_one_over_threads_k_sn2(case):
    """The command-line renderer weighs pass k's photon image with bling_host_sppm_splat_weight:
    1 / (threads * k * sn^2) (SPPM.hs:460) on the loader's config."""
    scene, ov = case.split(":")
    job = load_config(scene, ov)
    cfg = job.config
    threads = max(1, cfg.sppm_threads)
    sn = max(1, int(np.ceil(np.sqrt(np.float32(cfg.sppm_photons) / np.float32(threads)))))
    got_sn = C.c_int()
    for k in (1, 2, 7, 1000):
        sw = _ffi.host().bling_host_sppm_splat_weight(C.byref(cfg), k, C.byref(got_sn))
        assert got_sn.value == sn
        assert np.float32(sw) == np.float32(1.0) / np.float32(threads * k * sn * sn)
    assert _ffi.host().bling_host_sppm_splat_weight(C.byref(cfg), 0, None) == 0.0
    path = load_config("C1", "image=16,16")
    assert _ffi.host().bling_host_sppm_splat_weight(C.byref(path.config), 1, None) == 0.0


def test_device_symbols_are_exported():
    lib = _ffi.hip()
    assert hasattr(lib, "bling_sppm_pass_device") and hasattr(lib, "bling_debug_sppm_records")
    assert _ffi.SPLAT_ORDERED == 1 and C.sizeof(_ffi.SppmRecord) == sppm_ref.RECORD.itemsize == 40
