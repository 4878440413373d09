"""Light tracer on the device (k_lt_photon, bling_light_pass, bling_debug_light_records) against the
CPU restatement (tests/ref/lighttracer_ref.cpp).

Parity is pinned on the records: keys (photon, depth, pixel), every counter and the XYZ bits are
EQUAL to the restatement's -- measured on MI355X on all four scenes below (10 197 / 560 / 928 /
12 126 records), no residue in final ulps.  The splat image differs from the restatement's only in
the order of its binary32 sums (float atomics): relative L2 measured 6.6e-8 (fixture), 1.1e-9
(delta-lights), 1.2e-9 (sun-sky), 6.5e-8 (cornell); the device image against its own records summed
in float64 5.6e-8; two passes into one buffer against the sum of two 6.8e-8.  The bar is twice the
largest of these: 1.36e-7.
"""
import os

import numpy as np
import pytest

from bling_amd.render import BlingError, Context, render
from bling_amd.scene import SCENES, film_splat_to_rgb, load_config, parse_job
from lt_ref import LightRef

pytestmark = pytest.mark.gpu
SEED = 0x0B11A6
ORDER_BAR = 1.36e-7
FIXTURE = os.path.join(SCENES, "light-tracer.bling")

SCENE_DEFS = {
    "fixture": lambda: parse_job(FIXTURE),
    "delta-lights": lambda: load_config("X13", "light=4096"),                 # point, directional and area emission
    "sun-sky": lambda: load_config("X6", "light=4096;image=48,27"),           # infinite light, glass
    "cornell": lambda: load_config("C1", "light=4096;image=48,48"),           # triangles: the kProfiles[0] kernel
}
_cache = {}


def _scene(name):
    """(job, context, restatement, its records / splat / stats of pass 1), computed once."""
    if name not in _cache:
        job = SCENE_DEFS[name]()
        ctx = Context(0)
        ctx.upload(job)
        ref = LightRef(job)
        _cache[name] = (job, ctx, ref) + ref.run(SEED, 1)
    return _cache[name]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _same_records(g, r):
    assert len(g) == len(r)
    for k in ("photon", "depth", "sx", "sy"):
        assert np.array_equal(g[k], r[k]), k
    for k in "xyz":
        assert np.array_equal(g[k].view(np.uint32), r[k].view(np.uint32)), k     # bit-equal


def _counts(st):
    return [st.photons, st.photon_rays, st.shadow_rays, st.splats, st.dropped]


@pytest.mark.parametrize("name", list(SCENE_DEFS))
def test_records_and_stats_equal_the_restatement(name):
    job, ctx, _, rrec, _, rst = _scene(name)
    grec = ctx.light_records(seed=SEED, pass_index=1)
    _same_records(grec, rrec)
    _, gst = ctx.light_pass(seed=SEED, pass_index=1)
    assert _counts(gst) == rst.counts()


@pytest.mark.parametrize("name", list(SCENE_DEFS))
def test_splat_image_against_the_restatement_and_its_own_records(name):
    job, ctx, _, _, rsplat, _ = _scene(name)
    gsplat, _ = ctx.light_pass(seed=SEED, pass_index=1)
    r = _rel(gsplat, rsplat)
    grec = ctx.light_records(seed=SEED, pass_index=1)
    acc = np.zeros(job.width * job.height * 3, np.float64)
    idx = 3 * (grec["sy"].astype(np.int64) * job.width + grec["sx"])
    for c, k in enumerate("xyz"):
        np.add.at(acc, idx + c, grec[k].astype(np.float64))
    own = _rel(gsplat, acc)
    print(name, "splat rel L2 vs restatement", r, "vs own records", own)
    assert np.isfinite(gsplat).all() and r <= ORDER_BAR and own <= ORDER_BAR


@pytest.mark.parametrize("n", [1, 63, 257, 4096])
def test_launch_shapes(n):
    """Partial wave, partial block, several blocks: every photon count is record-equal."""
    job = parse_job(FIXTURE, f"light={n}")
    ctx = Context(0)
    ctx.upload(job)
    rrec, _, rst = LightRef(job).run(SEED, 3)
    _same_records(ctx.light_records(seed=SEED, pass_index=3), rrec)
    _, gst = ctx.light_pass(seed=SEED, pass_index=3)
    assert _counts(gst) == rst.counts()
    ctx.close()


def test_photon_ranges_compose():
    _, ctx, _, rrec, _, _ = _scene("fixture")
    a = ctx.light_records(seed=SEED, pass_index=1, first_photon=0, n_photons=300)
    b = ctx.light_records(seed=SEED, pass_index=1, first_photon=300, n_photons=4096 - 300)
    _same_records(np.concatenate([a, b]), rrec)


def test_accumulation_and_repeatability():
    job, ctx, ref, rrec, _, _ = _scene("fixture")
    s1, _ = ctx.light_pass(seed=SEED, pass_index=1)
    s2, _ = ctx.light_pass(seed=SEED, pass_index=2)
    both, _ = ctx.light_pass(seed=SEED, pass_index=2, splat=s1.copy())
    assert _rel(both, s1.astype(np.float64) + s2) <= ORDER_BAR
    assert not np.array_equal(s1, s2)
    r1 = ctx.light_records(seed=SEED, pass_index=1)
    r2 = ctx.light_records(seed=SEED, pass_index=1)
    assert np.array_equal(r1, r2)                                 # two runs of one pass: identical records
    _same_records(ctx.light_records(seed=SEED, pass_index=2), ref.run(SEED, 2)[0])


def test_refusals():
    for name, ov in (("X5", None), ("C1", "image=16,16")):        # an SPPM scene, a path scene
        ctx = Context(0)
        ctx.upload(load_config(name, ov))
        with pytest.raises(BlingError) as e:
            ctx.light_pass()
        assert e.value.rc == -1 and "light tracer" in str(e.value)
        ctx.close()
    with pytest.raises(BlingError) as e:                          # passPhotons < 1: refused at upload, as sppm's count
        Context(0).upload(load_config("C1", "light=0;image=16,16"))
    assert e.value.rc == -1
    empty = Context(0)
    with pytest.raises(BlingError) as e:
        empty.job = load_config("C1", "light=16;image=16,16")
        empty.light_pass()
    assert e.value.rc == -4                                       # BLING_ENOSCENE
    with pytest.raises(BlingError) as e:                          # a context holding several devices
        import os as _os
        _os.environ["BLING_ALLOW_REPEATED_DEVICES"] = "1"
        try:
            two = Context([0, 0])
            two.upload(load_config("C1", "light=16;image=16,16"))
            two.light_pass()
        finally:
            del _os.environ["BLING_ALLOW_REPEATED_DEVICES"]
    assert e.value.rc == -1 and "single-device" in str(e.value)


def test_environment_camera_is_unsupported(tmp_path):
    src = open(FIXTURE).read().replace("camera { perspective fov 60 lensRadius 0 focalDistance 10 }",
                                       "camera { environment }")
    p = tmp_path / "env.bling"
    p.write_text(src)
    ctx = Context(0)
    ctx.upload(parse_job(str(p)))
    with pytest.raises(BlingError) as e:
        ctx.light_pass()
    assert e.value.rc == -5                                       # BLING_EUNSUPPORTED


def test_computed_textures_are_unsupported():
    ctx = Context(0)
    ctx.upload(load_config("X11", "light=64"))                    # blend / gradient / checker / cellNoise
    with pytest.raises(BlingError) as e:
        ctx.light_pass()
    assert e.value.rc == -5


def test_too_small_record_capacity_is_reported():
    _, ctx, _, rrec, _, _ = _scene("fixture")
    with pytest.raises(BlingError) as e:
        ctx.light_records(seed=SEED, pass_index=1, cap=len(rrec) - 1)
    assert e.value.rc == -1 and "exceed the capacity" in str(e.value)
    assert len(ctx.light_records(seed=SEED, pass_index=1, cap=len(rrec))) == len(rrec)


def test_render_returns_the_weighted_splat_image():
    job = parse_job(FIXTURE)
    rgb = render(job, passes=2, seed=SEED)
    assert rgb.shape == (32, 48, 3) and np.isfinite(rgb).all() and rgb.max() > 0
    ctx = Context(0)
    ctx.upload(job)
    splat, _ = ctx.light_pass(seed=SEED, pass_index=1)
    splat, _ = ctx.light_pass(seed=SEED, pass_index=2, splat=splat)
    want = film_splat_to_rgb(None, splat, np.float32(1) / np.float32(2 * 4096), 48, 32)
    # the two accumulated images differ in their atomics' order only; xyzToRgb is linear, so the
    # relative L2 error grows by at most the matrix's condition number (Spectrum.hs:162-168)
    m = np.array([[3.240479, -1.537150, -0.498535], [-0.969256, 1.875991, 0.041556], [0.055648, -0.204043, 1.057311]])
    assert _rel(rgb, want) <= np.linalg.cond(m) * ORDER_BAR
    ctx.close()
