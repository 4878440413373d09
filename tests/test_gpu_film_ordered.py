"""The ordered film of the sampler renderer (BLING_PASS_ORDERED_FILM, k_film_ordered / k_film_add_ordered):
bit-equal to the binary32 restatement (tests/film_ordered_ref.py) of the device's own per-sample results,
to the oracle's film wherever the per-sample results agree, and the same bits however the pass is cut,
sharded, reported or repeated.  Every comparison is np.array_equal; no pixel is excluded except, in the
oracle test alone, those a bitwise differing sample reaches (capped, counted and reported)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the core library is loaded, as the other device-tensor tests do)

import shape_scenes as sc
from bling_amd import _ffi
from film_ordered_ref import film_ordered
from film_ref import film_ref, pass_samples, pass_tiles
from parity_util import report
from test_film_ordered_ref import SEED, oracle_samples, scene_dir  # noqa: F401  (scene_dir: the shared fixture)

pytestmark = pytest.mark.gpu
C4_32 = sc.SLOT_CASES[2]
assert C4_32.tag == "C4 stratified=3,2"
_X1 = "image=24,16;stratified=3,2;"
INTEGRATOR_CASES = [sc.Case("X1 direct", "X1", _X1 + "direct=3"), sc.Case("X1 bidir", "X1", _X1 + "bidir=4,3"),
                    sc.Case("X1 normals", "X1", _X1 + "normals")]
SHARD_CASES = [sc.SIZE_CASES[3], sc.C1_32, sc.FILTER_CASES[5]]          # 33 x 17: six tiles; K = 5; the generic kernel
_jobs = {}


@pytest.fixture(scope="module")
def ctx():
    from bling_amd.render import Context
    c = Context(0)
    yield c
    c.close()


def _job(case, scene_dir):
    if case.tag not in _jobs:
        _jobs[case.tag] = sc.load(case, scene_dir)
    return _jobs[case.tag]


def _waves(ctx):
    """How the last pass ran: the number of waves, or -2 for two half-waves."""
    n, waves = C.c_size_t(), C.c_int()
    _ffi.hip().bling_debug_pass_results(ctx._h, None, 0, C.byref(n), C.byref(waves))   # refuses a multi-wave pass; waves is set
    return int(waves.value)


def _restate(ctx, job, case, shard=(0, 1), stride=1, pass_index=None, **kw):
    """film_ordered of the device's own per-sample results of the pass it just ran (one or two waves)."""
    res, waves = ctx.pass_results()
    major = ctx.scene_info()["sample_major"]
    s = pass_samples(job, major, shard, stride)
    assert waves in (1, -2) and len(res) == len(s)
    _, img, _ = ctx.sample_li(s, seed=SEED, pass_index=case.pass_index if pass_index is None else pass_index)
    return film_ordered(res, img, job.filter_table(), job.filter_size, job.width, job.height,
                        pass_tiles(job, shard, stride), job.spp, sample_major=major, **kw), res, img, major


def _contract(ctx, case, scene_dir):
    job = _job(case, scene_dir)
    ctx.upload(job)
    film, st = ctx.render_pass(seed=SEED, pass_index=case.pass_index, ordered=True)
    ref, res, img, major = _restate(ctx, job, case)
    assert st.camera_samples == job.camera_samples() == len(res) and st.ms_film > 0
    assert np.isfinite(film).all() and (film.reshape(-1, 4)[:, 1:] > 0).any()
    assert np.array_equal(film, ref)
    return job, film, res, img, major


# ------------------------------------------------------------------ 1. the contract
@pytest.mark.parametrize("case", sc.FILM_CASES, ids=str)
def test_film_is_the_restatement_of_its_own_samples(ctx, case, scene_dir):
    _, _, _, _, major = _contract(ctx, case, scene_dir)
    if case in sc.SLOT_CASES:
        assert major == (1 if case.base == "C4" else 0)


# ------------------------------------------------------------------ 2. the oracle
@pytest.mark.parametrize("case", sc.FILM_CASES, ids=str)
def test_film_is_the_oracles(ctx, case, scene_dir):
    job, orc, res_o, img_o = oracle_samples(case, scene_dir)
    film_o, st_o = orc.render(seed=SEED, pass_index=case.pass_index)
    ctx.upload(job)
    film, st = ctx.render_pass(seed=SEED, pass_index=case.pass_index, ordered=True)
    res, _ = ctx.pass_results()
    major = ctx.scene_info()["sample_major"]
    minor_s, slot_s = pass_samples(job, 0), pass_samples(job, major)
    index = {tuple(s): i for i, s in enumerate(minor_s.tolist())}
    to_oracle = np.array([index[tuple(s)] for s in slot_s.tolist()])          # device slot -> the oracle's sample
    differ = (res.view(np.uint32) != res_o[to_oracle].view(np.uint32)).any(1)
    excluded = np.zeros((job.height, job.width), bool)
    if differ.any():                                                          # the pixels a differing sample reaches
        mask = np.zeros_like(res)
        mask[differ, 3] = 1
        _, _, n = film_ref(mask, img_o[to_oracle], job.filter_table(), job.filter_size, job.width, job.height,
                           pass_tiles(job), job.spp)
        excluded = n > 0
    share = float(excluded.mean())
    report("film_ordered_oracle", case=case.tag, samples=len(res), differing_samples=int(differ.sum()),
           excluded_pixels=int(excluded.sum()), share=share)
    assert share <= 0.01, (int(differ.sum()), int(excluded.sum()))
    assert st.camera_samples == st_o.samples
    a, b = film.reshape(job.height, job.width, 4), film_o.reshape(job.height, job.width, 4)
    assert np.array_equal(a[~excluded], b[~excluded])


# ------------------------------------------------------------------ 3. however the pass is cut
@pytest.mark.parametrize("case", [sc.C1_32, C4_32], ids=str)
def test_pass_shape_does_not_change_the_bits(ctx, case, scene_dir):
    job = _job(case, scene_dir)
    ctx.upload(job)
    kw = dict(seed=SEED, pass_index=case.pass_index, ordered=True)
    try:
        ctx.set_pipeline(1)
        piped, _ = ctx.render_pass(**kw)
        w_piped = _waves(ctx)
    finally:
        ctx.set_pipeline(-1)
    one, _ = ctx.render_pass(flags=_ffi.PASS_NO_PIPELINE, **kw)
    w_one = _waves(ctx)
    ref, _, _, _ = _restate(ctx, job, case)
    many, st = ctx.render_pass(chunk_paths=job.camera_samples() // 3, flags=_ffi.PASS_NO_PIPELINE, **kw)
    w_many = _waves(ctx)
    report("film_ordered_shapes", case=case.tag, waves=[w_piped, w_one, w_many])
    assert w_piped == -2 and w_one == 1 and w_many >= 3
    assert st.camera_samples == job.camera_samples()
    assert np.array_equal(one, ref)
    assert np.array_equal(piped, one)
    assert np.array_equal(many, one)


# ------------------------------------------------------------------ 4. the other integrators
@pytest.mark.parametrize("case", INTEGRATOR_CASES, ids=str)
def test_integrators(ctx, case, scene_dir):
    _contract(ctx, case, scene_dir)


# ------------------------------------------------------------------ 5. accumulation, reproducibility
def test_passes_accumulate_in_order_and_a_second_context_repeats_them(ctx, scene_dir):
    from bling_amd.render import Context
    case = sc.C1_32_PASS0
    job = _job(case, scene_dir)

    def two_passes(c, restate):
        c.upload(job)
        film, ref = None, None
        for p in (0, 1):
            film, _ = c.render_pass(seed=SEED, pass_index=p, film=film, ordered=True)
            if restate:
                ref, _, _, _ = _restate(c, job, case, pass_index=p, film0=ref)
        return film, ref

    film, ref = two_passes(ctx, True)
    assert np.array_equal(film, ref)
    other = Context(0)
    try:
        again, _ = two_passes(other, False)
    finally:
        other.close()
    assert again.tobytes() == film.tobytes()


# ------------------------------------------------------------------ 6. shards
def _device_zeros(n):
    """n zeroed floats on the device, the zeroing finished: hipMemset runs on the null stream, which the
    context's own (non-blocking) stream does not wait for."""
    from test_gpu_bidir import _DeviceFloats
    buf = _DeviceFloats(n)
    assert buf.rt.hipDeviceSynchronize() == 0
    return buf


def _shard_tiles(ctx, job, case, shard, stride, film0):
    """(device buffer, slots (n, sh, sw, 4), the restatement's slots, the restatement's film of this shard's tiles
    added onto film0) of one shard's ordered tile images.  The buffer is sized for the largest shard of its world,
    rank 0's: film_add_shards checks one capacity for all.  (Both restatements are made here, from one reading of
    the pass's results: sample_li, which gives the image positions, runs a wave of its own over them.)"""
    org, sw, sh = ctx.tile_layout(shard=shard, tile_stride=stride)
    most = len(ctx.tile_layout(shard=(0, shard[1]), tile_stride=stride)[0])
    buf = _device_zeros(max(1, most) * sw * sh * 4)
    ctx.render_pass_tiles(buf.p.value, seed=SEED, pass_index=case.pass_index, shard=shard, tile_stride=stride,
                          tiles_capacity=buf.n, ordered=True)
    ref, res, img, major = _restate(ctx, job, case, shard, stride, tiles_only=True)
    film = film_ordered(res, img, job.filter_table(), job.filter_size, job.width, job.height, pass_tiles(job, shard, stride),
                        job.spp, sample_major=major, film0=film0)
    return buf, buf.host()[:len(org) * sw * sh * 4].reshape(len(org), sh, sw, 4), ref, film


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("case", SHARD_CASES, ids=str)
def test_shards(ctx, case, stride, scene_dir):
    job = _job(case, scene_dir)
    ctx.upload(job)
    whole, _ = ctx.render_pass(seed=SEED, pass_index=case.pass_index, tile_stride=stride, ordered=True)
    ref_whole, _, _, _ = _restate(ctx, job, case, stride=stride)
    assert np.array_equal(whole, ref_whole)
    bufs = []
    try:
        for shard in ((0, 2), (1, 2)):
            buf, slots, ref, ref_alone = _shard_tiles(ctx, job, case, shard, stride, whole)
            bufs.append(buf)
            assert len(slots) > 0 and np.array_equal(slots, ref)
        merged = _device_zeros(job.width * job.height * 4)
        bufs.append(merged)
        ctx.film_add_shards([b.p.value for b in bufs[:2]], merged.p.value, tile_stride=stride,
                            tiles_capacity=min(b.n for b in bufs[:2]), ordered=True)
        assert np.array_equal(merged.host(), whole)
        # one shard alone, onto a film that is not empty: the restatement over that shard's tiles
        alone = _device_zeros(job.width * job.height * 4)
        bufs.append(alone)
        ctx.render_pass_device(alone.p.value, seed=SEED, pass_index=case.pass_index, tile_stride=stride, ordered=True)
        assert np.array_equal(alone.host(), whole)
        ctx.film_add_tiles(bufs[1].p.value, alone.p.value, shard=(1, 2), tile_stride=stride, tiles_capacity=bufs[1].n,
                           ordered=True)
        assert np.array_equal(alone.host(), ref_alone)                        # shard (1, 2)'s tiles onto the whole film
    finally:
        for b in bufs:
            b.free()


# ------------------------------------------------------------------ 7. region events
def test_region_events_carry_ordered_films(ctx, scene_dir):
    case = sc.SIZE_CASES[3]
    job = _job(case, scene_dir)
    ctx.upload(job)
    seen = []

    def regions(kind, p, window, film):
        if kind == "samples_added":
            seen.append((window, film.copy()))

    film, _ = ctx.render_loop(lambda p, f, st: False, seed=SEED, first_pass=case.pass_index, regions=regions, ordered=True)
    tiles = pass_tiles(job)
    assert [w for w, _ in seen] == tiles
    res, waves = ctx.pass_results()
    major = ctx.scene_info()["sample_major"]
    _, img, _ = ctx.sample_li(pass_samples(job, major), seed=SEED, pass_index=case.pass_index)
    off = 0
    for k, t in enumerate(tiles):                                             # the film up to and including window k
        off += (t[1] - t[0] + 1) * (t[3] - t[2] + 1) * job.spp
        ref = film_ordered(res[:off], img[:off], job.filter_table(), job.filter_size, job.width, job.height, tiles[:k + 1],
                           job.spp, sample_major=major)
        assert np.array_equal(seen[k][1], ref), k
    whole, _ = ctx.render_pass(seed=SEED, pass_index=case.pass_index, ordered=True)
    assert np.array_equal(film, whole) and np.array_equal(seen[-1][1], whole)


# ------------------------------------------------------------------ 8. a device film
def test_device_film(ctx, scene_dir):
    case = sc.FILTER_CASES[2]
    job = _job(case, scene_dir)
    ctx.upload(job)
    host, _ = ctx.render_pass(seed=SEED, pass_index=case.pass_index, ordered=True)
    dev = torch.zeros(job.width * job.height * 4, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()                                                  # the context renders on a stream of its own
    st = ctx.render_pass_device(dev.data_ptr(), seed=SEED, pass_index=case.pass_index, ordered=True)
    assert st.camera_samples == job.camera_samples()
    assert np.array_equal(dev.cpu().numpy(), host)


# ------------------------------------------------------------------ 9. refusal
def test_a_context_of_several_devices_refuses(scene_dir):
    from bling_amd.render import BlingError, Context
    job = _job(sc.C1_32, scene_dir)
    os.environ["BLING_ALLOW_REPEATED_DEVICES"] = "1"
    try:
        two = Context([0, 0])
    finally:
        del os.environ["BLING_ALLOW_REPEATED_DEVICES"]
    try:
        two.upload(job)
        with pytest.raises(BlingError) as e:
            two.render_pass(seed=SEED, pass_index=1, ordered=True)
        assert e.value.rc == -1 and "multi-device" in str(e.value)
        film, st = two.render_pass(seed=SEED, pass_index=1)
        assert st.camera_samples == job.camera_samples() and (film > 0).any()
    finally:
        two.close()


# ------------------------------------------------------------------ 10. the command line
def test_cli_writes_identical_files(tmp_path):
    from bling_amd.scene import SCENES
    exe = os.path.join(_ffi.LIBDIR, "bling")
    scene = os.path.join(SCENES, "cornell-box.bling")
    runs = {"a": [], "b": [], "dev": ["--develop", "device"]}
    for run, extra in runs.items():                                           # each in its own fresh process
        out = subprocess.run([exe, scene, "--overrides", "image=40,40;path=5,2;stratified=2,2", "--film", "ordered", "--passes", "2",
                              "--out", str(tmp_path / run)] + extra, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
    for p in (1, 2):
        for ext in ("png", "hdr"):
            a = (tmp_path / f"a-{p:05d}.{ext}").read_bytes()
            assert len(a) > 0
            assert a == (tmp_path / f"b-{p:05d}.{ext}").read_bytes()
            assert a == (tmp_path / f"dev-{p:05d}.{ext}").read_bytes()
    bad = subprocess.run([exe, os.path.join(SCENES, "light-tracer.bling"), "--film", "ordered", "--out", str(tmp_path / "lt")],
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "--splat" in bad.stderr
