"""Ordered splat films (BLING_SPLAT_ORDERED) and device splat images: bling_light_pass_device,
bling_mlt_pass_device and the ordered merge alone (bling_debug_splat_merge) against numpy's binary32
sequential add and the CPU restatements (tests/ref/lighttracer_ref.cpp, tests/ref/mlt_ref.cpp).

The ordered image is pinned bit for bit: every pixel is its old value plus its splats, one at a time in
binary32, in (photon, depth) or (chain, mutation, current before proposal) order -- the order the
restatements add in.  The atomic mode through a device pointer is held to the bars of the host-buffer
calls: ORDER_BAR of tests/test_gpu_light_tracer.py, and the derived bound of tests/test_gpu_mlt.py.
"""
import os
import subprocess

import numpy as np
import pytest
import torch

from bling_amd import _ffi
from bling_amd.render import SPLAT_REC, BlingError, Context
from bling_amd.scene import load_config, parse_job
from lt_ref import LightRef
from mlt_cases import CASES, bound, ratio
from mlt_ref import MltRef, mutations
from splat_ordered_util import FIXTURE, LT_SCENES, ORDER_EXAMPLE, sequential_add

pytestmark = pytest.mark.gpu
SEED = 0x0B11A6
ORDER_BAR = 1.36e-7                       # tests/test_gpu_light_tracer.py
LDS_RECORDS = 4096                        # splat_merge.h SM_LDS_RECORDS; SM_SHORT is 32

_lt = {}
_mlt = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def _dev(values):
    return torch.from_numpy(np.ascontiguousarray(values, np.float32).reshape(-1).copy()).to("cuda:0")


def _zeros(job):
    return torch.zeros(job.width * job.height * 3, dtype=torch.float32, device="cuda:0")


def _lt_scene(name):
    """(job, context, restatement's splat image and stats of pass 1), computed once."""
    if name not in _lt:
        job = LT_SCENES[name]()
        ctx = Context(0)
        ctx.upload(job)
        _, rsplat, rst = LightRef(job).run(SEED, 1, records=False)
        _lt[name] = (job, ctx, rsplat, rst)
    return _lt[name]


def _lt_counts(st):
    return [st.photons, st.photon_rays, st.shadow_rays, st.splats, st.dropped]


def _mlt_counts(st):
    return [st.mutations, st.large_steps, st.accepted, st.splats, st.dropped, st.rays_camera, st.rays_continuation,
            st.rays_mis, st.rays_shadow, st.path_vertices]


# ---------------------------------------------------------------- 1. the merge alone
def _merge_ctx():
    ctx = Context(0)
    ctx.upload(load_config("C1", "image=4,2"))                     # the hook needs W and H only
    return ctx


def _records(lengths, rng):
    """One segment of each length in its own pixel; keys unique and increasing within a pixel, values of
    mixed sign and magnitude so that the order of a sum matters."""
    rec = np.zeros(sum(lengths), SPLAT_REC)
    at = 0
    for pixel, n in enumerate(lengths):
        r = rec[at:at + n]
        r["pixel"] = pixel
        r["key"] = (np.arange(n, dtype=np.uint64) * np.uint64(0x100000003)) + np.uint64(pixel)
        for k in "xyz":
            r[k] = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)).astype(np.float32)
        at += n
    return rec


@pytest.mark.parametrize("lengths", [(0, 1, 2, 63, 64, 65, 4097, LDS_RECORDS + 1), (32, 33, 31, 0, 4096, 4095, 255, 257)],
                         ids=["issue", "thresholds"])
def test_merge_alone_every_segment_shape(lengths):
    """Lengths at and around every path's threshold (one lane up to 32, LDS up to 4 096, global memory
    beyond), all in one call; then the same records shuffled by a fixed permutation: the same image."""
    rng = np.random.default_rng(7)
    ctx = _merge_ctx()
    rec = _records(lengths, rng)
    start = rng.standard_normal(24).astype(np.float32)             # a non-zero starting image
    want = sequential_add(start, rec)
    img = _dev(start)
    ctx.splat_merge(rec, img)
    assert np.array_equal(_bits(img.cpu().numpy()), _bits(want))
    img = _dev(start)
    ctx.splat_merge(rec[np.random.default_rng(11).permutation(len(rec))], img)
    assert np.array_equal(_bits(img.cpu().numpy()), _bits(want))
    if lengths[0] == 0:
        assert np.array_equal(_bits(img.cpu().numpy())[:3], _bits(start)[:3])   # a pixel without records stays
    ctx.close()


@pytest.mark.parametrize("repeats", [2, 20, 2000], ids=["short", "lds", "global"])
def test_merge_alone_order_matters(repeats):
    """(+1e8, +1, -1e8, +1) repeated, keys in that order: ascending and descending binary32 sums differ on
    the CPU, and the device gives the ascending one."""
    vals = np.tile(np.array(ORDER_EXAMPLE, np.float32), repeats)
    rec = np.zeros(len(vals), SPLAT_REC)
    rec["pixel"] = 5
    rec["key"] = np.arange(len(vals), dtype=np.uint64)
    for k in "xyz":
        rec[k] = vals
    zero = np.zeros(24, np.float32)
    up = sequential_add(zero, rec)
    down_rec = rec.copy()
    down_rec["key"] = np.uint64(len(vals)) - down_rec["key"]
    down = sequential_add(zero, down_rec)
    assert not np.array_equal(_bits(up), _bits(down))
    ctx = _merge_ctx()
    img = _dev(zero)
    ctx.splat_merge(rec[::-1], img)                                # handed over in descending order
    assert np.array_equal(_bits(img.cpu().numpy()), _bits(up))
    ctx.close()


def test_merge_alone_signed_zeros_and_no_records():
    ctx = _merge_ctx()
    start = np.array([-0.0, 0.0, -0.0] * 8, np.float32)
    rec = np.zeros(6, SPLAT_REC)
    rec["pixel"] = [0, 0, 1, 1, 2, 2]
    rec["key"] = [1, 0, 5, 9, 3, 2]
    rec["x"] = [-0.0, -0.0, 0.0, -0.0, 1.5, -1.5]
    rec["y"] = [-0.0, 0.0, -0.0, -0.0, -0.0, -0.0]
    rec["z"] = [-0.0, -0.0, -0.0, -0.0, -2.0, 2.0]
    want = sequential_add(start, rec)
    assert np.signbit(want[0]) and not np.signbit(want[1])         # -0 + -0 + -0 = -0; +0 + anything zero = +0
    img = _dev(start)
    ctx.splat_merge(rec, img)
    assert np.array_equal(_bits(img.cpu().numpy()), _bits(want))
    img = _dev(start)
    ctx.splat_merge(np.zeros(0, SPLAT_REC), img)                   # n = 0
    assert np.array_equal(_bits(img.cpu().numpy()), _bits(start))
    with pytest.raises(BlingError) as e:
        bad = np.zeros(1, SPLAT_REC)
        bad["pixel"] = 8
        ctx.splat_merge(bad, img)
    assert e.value.rc == -1 and "pixel 8 of 8" in str(e.value)
    ctx.close()


# ---------------------------------------------------------------- 2. light tracer = restatement
@pytest.mark.parametrize("name", list(LT_SCENES))
def test_light_tracer_ordered_equals_the_restatement(name):
    job, ctx, rsplat, rst = _lt_scene(name)
    img = _zeros(job)
    st = ctx.light_pass_device(img, seed=SEED, pass_index=1, ordered=True)
    one = img.cpu().numpy()
    assert np.array_equal(_bits(one), _bits(rsplat))
    assert _lt_counts(st) == rst.counts()
    # pass 2 into pass 1's tensor: pass 2's own records (sorted by (photon, depth)) added onto pass 1's image
    st2 = ctx.light_pass_device(img, seed=SEED, pass_index=2, ordered=True)
    rec = ctx.light_records(seed=SEED, pass_index=2)
    srec = np.zeros(len(rec), SPLAT_REC)
    srec["pixel"] = rec["sy"].astype(np.int64) * job.width + rec["sx"]
    srec["key"] = (rec["photon"].astype(np.uint64) << np.uint64(32)) | rec["depth"].astype(np.uint64)
    for k in "xyz":
        srec[k] = rec[k]
    assert np.array_equal(_bits(img.cpu().numpy()), _bits(sequential_add(one, srec)))
    assert st2.splats == len(rec)


# ---------------------------------------------------------------- 3. reproducible and geometry-free
def test_light_tracer_ordered_is_reproducible_and_chunking_free():
    job, ctx, rsplat, rst = _lt_scene("fixture")
    a, b = _zeros(job), _zeros(job)
    ctx.light_pass_device(a, seed=SEED, pass_index=1, ordered=True)
    ctx.light_pass_device(b, seed=SEED, pass_index=1, ordered=True)
    assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))
    # a budget of about a third of the records: the whole range and its halves overflow, quarters fit
    ctx.set_splat_budget(int(rst.splats) // 3)
    try:
        c = _zeros(job)
        st = ctx.light_pass_device(c, seed=SEED, pass_index=1, ordered=True)
    finally:
        ctx.set_splat_budget(0)
    assert np.array_equal(_bits(c.cpu().numpy()), _bits(rsplat))
    assert _lt_counts(st) == rst.counts()


def test_light_tracer_one_photon_over_the_budget_is_refused():
    job, ctx, _, _ = _lt_scene("fixture")
    rec = ctx.light_records(seed=SEED, pass_index=1)
    most = int(np.bincount(rec["photon"]).max())
    assert most >= 2
    ctx.set_splat_budget(most - 1)
    try:
        with pytest.raises(BlingError) as e:
            ctx.light_pass_device(_zeros(job), seed=SEED, pass_index=1, ordered=True)
    finally:
        ctx.set_splat_budget(0)
    assert e.value.rc == -1 and "alone writes" in str(e.value) and f"budget {most - 1}" in str(e.value)


@pytest.mark.parametrize("ov", ["light=1", "light=63", "light=257", "light=4096;image=2,2"])
def test_light_tracer_ordered_launch_and_image_shapes(ov):
    """Partial wave, partial block, several blocks; and a 2 x 2 image, where every segment is long."""
    job = parse_job(FIXTURE, ov)
    ctx = Context(0)
    ctx.upload(job)
    _, rsplat, rst = LightRef(job).run(SEED, 3, records=False)
    img = _zeros(job)
    st = ctx.light_pass_device(img, seed=SEED, pass_index=3, ordered=True)
    assert np.array_equal(_bits(img.cpu().numpy()), _bits(rsplat))
    assert _lt_counts(st) == rst.counts()
    ctx.close()


# ---------------------------------------------------------------- 4. Metropolis = restatement
def _mlt_case(name, chains=None):
    key = (name, chains)
    if key not in _mlt:
        cfg, ov = CASES[name]
        job = load_config(cfg, ov if chains is None else (ov + ";" if ov else "") + f"chains={chains}")
        ctx = Context(0)
        ctx.upload(job)
        ref = MltRef(job)
        _mlt[key] = (job, ctx, ref) + ref.run(SEED, 1)
    return _mlt[key]


@pytest.mark.parametrize("chains", [None, 1], ids=["own-chains", "one-chain"])
@pytest.mark.parametrize("name", list(CASES))
def test_metropolis_ordered_equals_the_restatement(name, chains):
    job, ctx, ref, _, _, _, r32, rst = _mlt_case(name, chains)
    img = _zeros(job)
    st = ctx.mlt_pass_device(img, seed=SEED, pass_index=1, ordered=True)
    assert np.array_equal(_bits(img.cpu().numpy()), _bits(r32))
    assert _mlt_counts(st) == rst.counts()
    assert np.float32(st.b).view(np.uint32) == np.float32(rst.b).view(np.uint32)


def test_metropolis_budget_below_two_m_is_refused():
    job, ctx, *_ = _mlt_case("wave")
    m = mutations(job)
    start = np.full(job.width * job.height * 3, 0.25, np.float32)
    img = _dev(start)
    ctx.set_splat_budget(2 * m - 1)
    try:
        with pytest.raises(BlingError) as e:
            ctx.mlt_pass_device(img, seed=SEED, pass_index=1, ordered=True)
    finally:
        ctx.set_splat_budget(0)
    assert e.value.rc == -1 and str(2 * m) in str(e.value) and str(2 * m - 1) in str(e.value)
    assert np.array_equal(_bits(img.cpu().numpy()), _bits(start))
    ctx.set_splat_budget(2 * m)                                    # exactly 2 M is served
    try:
        ctx.mlt_pass_device(_zeros(job), seed=SEED, pass_index=1, ordered=True)
    finally:
        ctx.set_splat_budget(0)


# ---------------------------------------------------------------- 5. atomic mode through the device pointer
def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_light_tracer_atomic_device_pointer_and_develop():
    job, ctx, _, rst = _lt_scene("fixture")
    host, hst = ctx.light_pass(seed=SEED, pass_index=1)
    img = _zeros(job)
    st = ctx.light_pass_device(img, seed=SEED, pass_index=1)
    got = img.cpu().numpy()
    r = _rel(got, host)
    print("light tracer, device pointer against host buffer: rel L2", r)
    assert r <= ORDER_BAR and _lt_counts(st) == _lt_counts(hst) == rst.counts()
    sw = np.float32(1) / np.float32(job.light.pass_photons)
    film = torch.zeros(job.width * job.height * 4, dtype=torch.float32, device="cuda:0")
    for fmt, per in (("rgb8", 3), ("rgbe", 4)):
        out = torch.zeros(job.width * job.height * per, dtype=torch.uint8, device="cuda:0")
        ctx.develop(film, splat=img, splat_weight=sw, fmt=fmt, out=out)
        want = ctx.develop(np.zeros(job.width * job.height * 4, np.float32), splat=got, splat_weight=sw, fmt=fmt)
        assert np.array_equal(out.cpu().numpy(), want.reshape(-1))


def test_metropolis_atomic_device_pointer():
    job, ctx, ref, _, _, r64, r32, rst = _mlt_case("M1")
    bnd = bound(ref)
    host, hst = ctx.mlt_pass(seed=SEED, pass_index=1)
    img = _zeros(job)
    st = ctx.mlt_pass_device(img, seed=SEED, pass_index=1)
    got = img.cpu().numpy().astype(np.float64)
    own = ratio(np.abs(got - r64), bnd)
    both = ratio(np.abs(got - host.astype(np.float64)), 2 * bnd)
    print("metropolis, device pointer: |image - F64| / bound", own, "against the host buffer's / 2 bound", both)
    assert own <= 1.0 and both <= 1.0 and _mlt_counts(st) == _mlt_counts(hst) == rst.counts()


# ---------------------------------------------------------------- 6. refusals
def test_refusals(tmp_path):
    job, ctx, _, _ = _lt_scene("fixture")
    img = _zeros(job)
    with pytest.raises(BlingError) as e:
        ctx.light_pass_device(img, seed=SEED, pass_index=1, flags=2)
    assert e.value.rc == -1 and "flag" in str(e.value)
    st = _ffi.LightStats()
    assert _ffi.hip().bling_light_pass_device(ctx._h, SEED, 1, 0, None, st) == -1     # NULL splat_device
    mjob, mctx, *_ = _mlt_case("wave")
    with pytest.raises(BlingError) as e:
        mctx.mlt_pass_device(_zeros(mjob), seed=SEED, pass_index=1, flags=6)
    assert e.value.rc == -1 and "flag" in str(e.value)
    assert _ffi.hip().bling_mlt_pass_device(mctx._h, SEED, 1, 1, None, _ffi.MltStats()) == -1
    with pytest.raises(BlingError) as e:                          # wrong renderer, both ways
        mctx.light_pass_device(_zeros(mjob), ordered=True)
    assert e.value.rc == -1 and "light tracer" in str(e.value)
    with pytest.raises(BlingError) as e:
        ctx.mlt_pass_device(img, ordered=True)
    assert e.value.rc == -1 and "not metropolis" in str(e.value)
    with pytest.raises(ValueError):                               # a host array is no device image
        ctx.light_pass_device(np.zeros(job.width * job.height * 3, np.float32))
    with pytest.raises(ValueError):
        ctx.light_pass_device(torch.zeros(5, dtype=torch.float32, device="cuda:0"))
    os.environ["BLING_ALLOW_REPEATED_DEVICES"] = "1"              # a context holding several devices
    try:
        two = Context([0, 0])
        try:
            small = load_config("C1", "light=16;image=16,16")
            two.upload(small)
            with pytest.raises(BlingError) as e:
                two.light_pass_device(_zeros(small), ordered=True)
        finally:
            two.close()
    finally:
        del os.environ["BLING_ALLOW_REPEATED_DEVICES"]
    assert e.value.rc == -1 and "single-device" in str(e.value)
    src = open(FIXTURE).read().replace("camera { perspective fov 60 lensRadius 0 focalDistance 10 }", "camera { environment }")
    p = tmp_path / "env.bling"
    p.write_text(src)
    env = Context(0)
    ejob = parse_job(str(p))
    env.upload(ejob)
    with pytest.raises(BlingError) as e:
        env.light_pass_device(_zeros(ejob), ordered=True)
    assert e.value.rc == -5                                       # BLING_EUNSUPPORTED
    env.close()
    tex = Context(0)
    tjob = load_config("X11", "light=64")                         # computed textures
    tex.upload(tjob)
    with pytest.raises(BlingError) as e:
        tex.light_pass_device(_zeros(tjob), ordered=True)
    assert e.value.rc == -5
    tex.close()


# ---------------------------------------------------------------- the command line
def test_cli_ordered_device_film_writes_identical_files(tmp_path):
    exe = os.path.join(_ffi.LIBDIR, "bling")
    for run in ("a", "b"):
        out = subprocess.run([exe, FIXTURE, "--passes", "2", "--splat", "ordered", "--develop", "device", "--out",
                              str(tmp_path / run)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
    for p in (1, 2):
        for ext in ("png", "hdr"):
            a, b = tmp_path / f"a-{p:05d}.{ext}", tmp_path / f"b-{p:05d}.{ext}"
            assert os.path.getsize(a) > 0
            assert subprocess.run(["cmp", str(a), str(b)]).returncode == 0
