"""SPPM on device images (bling_sppm_pass_device), atomic and ordered (BLING_SPLAT_ORDERED), and its
records hook (bling_debug_sppm_records) against bling_sppm_pass, the oracle's onePass (oracle_sppm_pass)
and the records of tests/ref/sppm_ref.cpp.

flags = 0 is held to the atomic-order bars of tests/test_sppm.py (1e-6 film, 1e-5 splat) against the
host-buffer call, with every integer statistic and every pixel's radius equal.  The ordered mode is pinned
bit for bit: against itself (runs, a reset, a small record budget), against the two-level binary32 fold
of the device's own records, and against the oracle's film and splat image.
"""
import os
import subprocess

import numpy as np
import pytest
import torch

from bling_amd import _ffi
from bling_amd.render import BlingError, Context
from bling_amd.scene import load_config
from oracle_py import OracleSppm

import sppm_ref

pytestmark = pytest.mark.gpu
SEED = 0x0B11A6
X13 = ("X13", "image=48,36;sppm=20000,6,0.25;sppm_threads=4")
X13Q = ("X13", "image=64,48;sppm=20000,6,0.8,0.1;sppm_threads=4")
X5 = ("X5", "image=40,40;sppm_threads=4")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def _rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _images(job):
    w, h = job.width, job.height
    return (torch.zeros(w * h * 4, dtype=torch.float32, device="cuda:0"),
            torch.zeros(w * h * 3, dtype=torch.float32, device="cuda:0"))


def _counts(st):
    return [int(st.hitpoints), int(st.photons), int(st.photon_rays), int(st.photon_hits), int(st.cam_rays), int(st.dropped)]


def _ctx(case):
    job = load_config(*case)
    ctx = Context(0)
    ctx.upload(job)
    return job, ctx


def _run(ctx, job, passes=2, ordered=False):
    """Passes 1 .. passes into fresh device images: (film, splat as numpy, per-pass counts, radii, n)."""
    film, splat = _images(job)
    counts = []
    for p in range(1, passes + 1):
        counts.append(_counts(ctx.sppm_pass_device(film, splat, seed=SEED, pass_index=p, ordered=ordered)))
    r2, n = ctx.sppm_pixel_stats()
    return film.cpu().numpy(), splat.cpu().numpy(), counts, r2, n


_atomic = {}


def _host_run(case):
    """bling_sppm_pass over two passes, computed once per case: (film, splat, counts, r2, n)."""
    if case not in _atomic:
        job, ctx = _ctx(case)
        film = np.zeros(job.width * job.height * 4, np.float32)
        splat = np.zeros(job.width * job.height * 3, np.float32)
        counts = []
        for p in (1, 2):
            film, splat, st = ctx.sppm_pass(seed=SEED, pass_index=p, film=film, splat=splat)
            counts.append(_counts(st))
        r2, n = ctx.sppm_pixel_stats()
        ctx.close()
        _atomic[case] = (film, splat, counts, r2, n)
    return _atomic[case]


# ---------------------------------------------------------------- flags = 0
@pytest.mark.parametrize("case", [X5, X13], ids=["X5", "X13"])
def test_atomic_device_images_match_the_host_buffer_call(case):
    hf, hs, hc, hr2, hn = _host_run(case)
    job, ctx = _ctx(case)
    film, splat = _images(job)
    st1 = ctx.sppm_pass_device(film, splat, seed=SEED, pass_index=1)
    f1, s1 = film.cpu().numpy(), splat.cpu().numpy()
    st2 = ctx.sppm_pass_device(film, splat, seed=SEED, pass_index=2)
    f2, s2 = film.cpu().numpy(), splat.cpu().numpy()
    r2, n = ctx.sppm_pixel_stats()
    assert [_counts(st1), _counts(st2)] == hc
    assert np.array_equal(r2, hr2) and np.array_equal(n, hn)
    rf, rs = _rel_l2(f2, hf), _rel_l2(s2, hs)
    print("device pointers against host buffers: film rel L2", rf, "splat rel L2", rs)
    assert rf <= 1e-6 and rs <= 1e-5
    # the tensors accumulate: pass 2 added to what pass 1 left
    assert f2[0::4].sum() > 1.5 * f1[0::4].sum() and s2.sum() > s1.sum() > 0
    # either image may be left out; the statistics do not depend on it
    ctx.sppm_reset()
    only_f, only_s = _images(job)
    assert _counts(ctx.sppm_pass_device(only_f, None, seed=SEED, pass_index=1)) == hc[0]
    ctx.sppm_reset()
    assert _counts(ctx.sppm_pass_device(None, only_s, seed=SEED, pass_index=1)) == hc[0]
    assert _rel_l2(only_f.cpu().numpy(), f1) <= 1e-6 and _rel_l2(only_s.cpu().numpy(), s1) <= 1e-5
    ctx.close()


# ---------------------------------------------------------------- ordered: determinism
def test_ordered_is_bit_identical_over_runs_resets_and_budgets():
    hf, hs, hc, hr2, hn = _host_run(X5)
    job, ctx = _ctx(X5)
    fa, sa, ca, r2a, na = _run(ctx, job, ordered=True)
    ctx.sppm_reset()
    fb, sb, cb, r2b, nb = _run(ctx, job, ordered=True)
    job2, ctx2 = _ctx(X5)
    fc, sc, cc, r2c, nc = _run(ctx2, job2, ordered=True)
    # a sampler of pass 1 writes about 23 121 / 4 records: a budget of a fifth of that forces the whole range
    # and its halves to overflow (more than three ranges, more than one halving)
    budget = hc[0][3] // 4 // 5
    ctx2.sppm_reset()
    # every sampler's records of pass 1 exceed twice the budget: its whole range and both halves are redone
    assert all(len(ctx2.sppm_records(seed=SEED, pass_index=1, thread=k)) > 2 * budget for k in range(4))
    ctx2.set_splat_budget(budget)
    try:
        fd, sd, cd, r2d, nd = _run(ctx2, job2, ordered=True)
        kernel_ms, merge_ms = ctx2.splat_times()
    finally:
        ctx2.set_splat_budget(0)
    for f, s, c, r2, n in ((fb, sb, cb, r2b, nb), (fc, sc, cc, r2c, nc), (fd, sd, cd, r2d, nd)):
        assert np.array_equal(_bits(f), _bits(fa)) and np.array_equal(_bits(s), _bits(sa))
        assert c == ca and np.array_equal(r2, r2a) and np.array_equal(n, na)
    # the ordered statistics are the atomic mode's, exactly; the images differ from its only in the order
    assert ca == hc and np.array_equal(r2a, hr2) and np.array_equal(na, hn)
    assert _rel_l2(fa, hf) <= 1e-6 and _rel_l2(sa, hs) <= 1e-5
    assert kernel_ms > 0 and merge_ms > 0
    ctx.close(); ctx2.close()


def test_one_photon_over_the_budget_is_refused():
    job, ctx = _ctx(X5)
    film, splat = _images(job)
    ctx.set_splat_budget(1)                           # some photon of the 40 x 40 cornell box meets two hit points
    try:
        with pytest.raises(BlingError) as e:
            ctx.sppm_pass_device(film, splat, seed=SEED, pass_index=1, ordered=True)
    finally:
        ctx.set_splat_budget(0)
    assert e.value.rc == -1 and "alone writes" in str(e.value) and "budget 1" in str(e.value)
    ctx.close()


# ---------------------------------------------------------------- ordered against the device's own records
def _device_records(ctx, job, p):
    nth = max(1, job.config.sppm_threads)
    return np.concatenate([ctx.sppm_records(seed=SEED, pass_index=p, thread=k) for k in range(nth)])


@pytest.mark.parametrize("case", [X5, X13Q], ids=["X5", "X13q"])
def test_ordered_splat_is_the_two_level_fold_of_the_device_records(case):
    job, ctx = _ctx(case)
    w, h = job.width, job.height
    nth = max(1, job.config.sppm_threads)
    film, splat = _images(job)
    want = np.zeros(w * h * 3, np.float32)
    for p in (1, 2):
        r2_before, n_before = ctx.sppm_pixel_stats()
        rec = _device_records(ctx, job, p)                 # for the radii before the pass
        r2_after, n_after = ctx.sppm_pixel_stats()
        assert np.array_equal(r2_before, r2_after) and np.array_equal(n_before, n_after)   # the hook updates nothing
        st = ctx.sppm_pass_device(film, splat, seed=SEED, pass_index=p, ordered=True)
        assert len(rec) <= st.photon_hits
        want = sppm_ref.fold_two_level(rec, nth, w, h, image=want)
        got = splat.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want)), (p, int((_bits(got) != _bits(want)).sum()))
    # capacity contract: a capacity below the count is BLING_EINVAL with the count set
    n = sppm_ref.C.c_size_t()
    one = np.zeros(1, sppm_ref.RECORD)
    rc = _ffi.hip().bling_debug_sppm_records(ctx._h, SEED, 1, 0, 0, 64, one.ctypes.data_as(sppm_ref.C.POINTER(_ffi.SppmRecord)), 1,
                                             sppm_ref.C.byref(n))
    full = ctx.sppm_records(seed=SEED, pass_index=1, thread=0, first_photon=0, n_photons=64)
    assert n.value == len(full) and (rc == -1 if len(full) > 1 else rc == 0)
    ctx.close()


# ---------------------------------------------------------------- ordered against the oracle
def _first_difference(dev, ref):
    """The first record and field in which two record arrays differ, for the assertion's message."""
    for i in range(min(len(dev), len(ref))):
        for f in ("thread", "photon", "seq", "depth", "sx", "sy", "x", "y", "z"):
            a, b = dev[f][i], ref[f][i]
            if (a.view(np.uint32) != b.view(np.uint32)) if f in "xyz" else (a != b):
                return f"record {i}: field {f}: device {a!r}, restatement {b!r} (photon {ref['photon'][i]}, seq {ref['seq'][i]})"
    return f"lengths {len(dev)} and {len(ref)}"


@pytest.mark.parametrize("case", [X13, X13Q], ids=["X13", "X13q"])
def test_ordered_equals_the_oracle(case):
    """Integer statistics and radii first; then the device's records against the restatement's field for
    field (XYZ bit for bit), and the film and the splat image against oracle_sppm_pass's bit for bit."""
    job, ctx = _ctx(case)
    w, h = job.width, job.height
    ora = OracleSppm(job)
    ref = sppm_ref.SppmRef(job)
    film, splat = _images(job)
    ofilm = np.zeros(w * h * 4, np.float32)
    osplat = np.zeros(w * h * 3, np.float32)
    for p in (1, 2):
        dev = _device_records(ctx, job, p)
        rrec, _ = ref.records(SEED, p)
        st = ctx.sppm_pass_device(film, splat, seed=SEED, pass_index=p, ordered=True)
        ofilm, osplat, ost = ora.render_pass(seed=SEED, pass_index=p, film=ofilm, splat=osplat)
        ref.advance(SEED, p)
        want = [int(ost.hitpoints), int(ost.photons), int(ost.photon_rays), int(ost.photon_hits), int(ost.cam_rays), int(ost.dropped)]
        print(f"pass {p}: device {_counts(st)} oracle {want}; records device {len(dev)} restatement {len(rrec)}")
        assert _counts(st) == want, (p, _counts(st), want)
        r2, n = ctx.sppm_pixel_stats()
        or2, on = ora.pixel_stats()
        assert np.array_equal(r2, or2) and np.array_equal(n, on), (p, float(np.mean(r2 == or2)))
        same = len(dev) == len(rrec) and all(np.array_equal(dev[f], rrec[f]) for f in ("thread", "photon", "seq", "depth", "sx", "sy")) \
            and all(np.array_equal(_bits(dev[f]), _bits(rrec[f])) for f in "xyz")
        assert same, _first_difference(dev, rrec)
        gf, gs = film.cpu().numpy(), splat.cpu().numpy()
        nf, ns = int((_bits(gf) != _bits(ofilm)).sum()), int((_bits(gs) != _bits(osplat)).sum())
        print(f"pass {p}: film words differing {nf}, splat words differing {ns}")
        assert nf == 0, (p, nf)
        assert ns == 0, (p, ns)
    ctx.close(); ora.close(); ref.close()


# ---------------------------------------------------------------- develop, refusals, the command line
def test_develop_of_the_device_images_equals_the_host_develop():
    job, ctx = _ctx(X5)
    film, splat = _images(job)
    ctx.sppm_pass_device(film, splat, seed=SEED, pass_index=1, ordered=True)
    sw = np.float32(_ffi.host().bling_host_sppm_splat_weight(sppm_ref.C.byref(job.config), 1, None))
    hf, hs = film.cpu().numpy(), splat.cpu().numpy()
    for fmt, per in (("rgb8", 3), ("rgbe", 4)):
        out = torch.zeros(job.width * job.height * per, dtype=torch.uint8, device="cuda:0")
        ctx.develop(film, splat=splat, splat_weight=sw, fmt=fmt, out=out)
        want = ctx.develop(hf, splat=hs, splat_weight=sw, fmt=fmt)
        assert np.array_equal(out.cpu().numpy(), want.reshape(-1))
    ctx.close()


def test_refusals():
    job, ctx = _ctx(X5)
    film, splat = _images(job)
    with pytest.raises(BlingError) as e:
        ctx.sppm_pass_device(film, splat, seed=SEED, pass_index=1, flags=2)
    assert e.value.rc == -1 and "flag" in str(e.value)
    with pytest.raises(BlingError) as e:
        ctx.sppm_pass_device(film, splat, seed=SEED, pass_index=1, flags=5)
    assert e.value.rc == -1 and "flag" in str(e.value)
    with pytest.raises(ValueError):                               # a host array is no device image
        ctx.sppm_pass_device(np.zeros(job.width * job.height * 4, np.float32), splat)
    with pytest.raises(ValueError):
        ctx.sppm_pass_device(film, torch.zeros(5, dtype=torch.float32, device="cuda:0"))
    with pytest.raises(BlingError) as e:
        ctx.sppm_records(seed=SEED, pass_index=1, thread=4)
    assert e.value.rc == -1
    ctx.close()
    pjob, pctx = _ctx(("C1", "image=16,16"))                        # not an SPPM scene
    with pytest.raises(BlingError) as e:
        pctx.sppm_pass_device(*_images(pjob), ordered=True)
    assert e.value.rc == -1 and "not sppm" in str(e.value)
    pctx.close()
    tjob, tctx = _ctx(("X11", "sppm=2000,3,1"))                     # computed textures
    for ordered in (False, True):
        with pytest.raises(BlingError) as e:
            tctx.sppm_pass_device(*_images(tjob), ordered=ordered)
        assert e.value.rc == -5 and "SPPM" in str(e.value)         # BLING_EUNSUPPORTED
    tctx.close()


def test_a_multi_device_context_is_refused():
    os.environ["BLING_ALLOW_REPEATED_DEVICES"] = "1"              # a context holding several devices, on one GPU
    try:
        two = Context([0, 0])
        try:
            job = load_config(*X5)
            two.upload(job)
            with pytest.raises(BlingError) as e:
                two.sppm_pass_device(*_images(job), ordered=True)
        finally:
            two.close()
    finally:
        del os.environ["BLING_ALLOW_REPEATED_DEVICES"]
    assert e.value.rc == -1 and "single-device" in str(e.value)


def _cli(tmp_path, run, *args):
    exe = os.path.join(_ffi.LIBDIR, "bling")
    scene = os.path.join(os.path.dirname(_ffi.LIBDIR), "..", "fixtures", "scenes", "cornell-box.bling")
    out = subprocess.run([exe, os.path.normpath(scene), "--overrides", X5[1], "--passes", "2", "--out", str(tmp_path / run), *args],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "hit points" in out.stdout and "photons" in out.stdout and "pairs" in out.stdout
    return [(tmp_path / f"{run}-{p:05d}.{ext}").read_bytes() for p in (1, 2) for ext in ("png", "hdr")]


def test_cli_ordered_runs_write_identical_files(tmp_path):
    a = _cli(tmp_path, "a", "--splat", "ordered")
    b = _cli(tmp_path, "b", "--splat", "ordered")
    assert all(len(x) > 0 for x in a) and a == b


def test_cli_device_develop_writes_what_host_develop_writes_from_the_same_images(tmp_path):
    """Ordered images are the same on every run, so the two develops see the same film and splat image."""
    dev = _cli(tmp_path, "d", "--splat", "ordered", "--develop", "device")
    host = _cli(tmp_path, "h", "--splat", "ordered", "--develop", "host")
    assert dev == host
    alone = _cli(tmp_path, "o", "--develop", "device")            # --develop device alone: atomic, on the device
    assert all(len(x) > 0 for x in alone)
