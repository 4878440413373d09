"""The Metropolis renderer on the device (k_mlt_propose, k_mlt_walk, k_mlt_accept, bling_mlt_pass,
bling_debug_mlt_records) against the CPU restatement (tests/ref/mlt_ref.cpp).

Parity is pinned on the records: every (chain, mutation) record -- the proposal's image position, iProp,
a, the large-step and accepted flags -- the chains' start samples, b' and every counter EQUAL the
restatement's, bit for bit; the per-sample bidirectional radiance is bit-exact already
(tests/test_gpu_bidir.py), so no ulp bar is set.  The splat image differs only in the order of its
binary32 sums (float atomics) and is held to the derived bound of DESIGN.md section 2 per pixel and
channel: |image - F64| <= 1.01 (n + 2) 2^-24 A64 against the float64 sum of the contributions (n the
pixel's splats, A64 the sum of their magnitudes), twice that against the restatement's binary32 image.
The records carry no XYZ, so "the device's own records summed in float64" is taken from the restatement:
its float64 image is that sum exactly because the record test above shows every record -- and with it every
contribution, which is spectrumToXYZ of the same spectra scaled by the same a, iProp and iCurr -- equal.
That the restatement's own binary32 image is inside the bound is checked without a device, for the same
cases, in tests/test_mlt.py.
"""
import numpy as np
import pytest

import os
import subprocess

from bling_amd import _ffi
from bling_amd.film import mlt_bnext
from bling_amd.render import BlingError, Context, render
from bling_amd.scene import SCENES as SCENE_DIR, load_config
from mlt_cases import CASES, bound, ratio
from mlt_ref import MltRef, boot_starts, mutations

pytestmark = pytest.mark.gpu
SEED = 0x0B11A6

_cache = {}


def _case(name):
    """(job, context, restatement, its records / starts / splat64 / splat32 / stats of pass 1), computed once."""
    if name not in _cache:
        cfg, ov = CASES[name]
        job = load_config(cfg, ov)
        ctx = Context(0)
        ctx.upload(job)
        ref = MltRef(job)
        _cache[name] = (job, ctx, ref) + ref.run(SEED, 1)
    return _cache[name]


def _counts(st):
    return [st.mutations, st.large_steps, st.accepted, st.splats, st.dropped, st.rays_camera, st.rays_continuation,
            st.rays_mis, st.rays_shadow, st.path_vertices]


@pytest.mark.parametrize("name", list(CASES))
def test_records_starts_b_and_counters_equal_the_restatement(name):
    job, ctx, ref, rrec, rstarts, r64, r32, rst = _case(name)
    grec, gstarts, gb = ctx.mlt_records(seed=SEED, pass_index=1)
    assert len(grec) == len(rrec) == mutations(job)
    for k in ("chain", "mutation", "flags"):
        assert np.array_equal(grec[k], rrec[k]), k
    for k in ("x", "y", "i_prop", "a"):
        assert np.array_equal(grec[k].view(np.uint32), rrec[k].view(np.uint32)), k   # bit-equal, NaN included
    assert np.array_equal(gstarts, rstarts)
    assert np.float32(gb).view(np.uint32) == np.float32(rst.b).view(np.uint32)
    _, gst = ctx.mlt_pass(seed=SEED, pass_index=1)
    assert _counts(gst) == rst.counts()
    assert np.float32(gst.b).view(np.uint32) == np.float32(rst.b).view(np.uint32)


@pytest.mark.parametrize("name", list(CASES))
def test_splat_image_within_the_derived_bound(name):
    job, ctx, ref, _, _, r64, r32, _ = _case(name)
    bnd = bound(ref)
    cpu = ratio(np.abs(r32.astype(np.float64) - r64), bnd)
    gsplat, _ = ctx.mlt_pass(seed=SEED, pass_index=1)
    own = ratio(np.abs(gsplat.astype(np.float64) - r64), bnd)
    both = ratio(np.abs(gsplat.astype(np.float64) - r32.astype(np.float64)), 2 * bnd)
    print(name, "worst |image - F64| / bound: restatement", cpu, "device", own, "device vs restatement / 2 bound", both)
    assert np.isfinite(gsplat).all() and bool(r64.any()) == (name != "dark-start")
    assert cpu <= 1.0 and own <= 1.0 and both <= 1.0


def test_two_passes_accumulate():
    job, ctx, ref, _, _, r64, _, _ = _case("M1")
    s1, _ = ctx.mlt_pass(seed=SEED, pass_index=1)
    both, _ = ctx.mlt_pass(seed=SEED, pass_index=2, splat=s1.copy())
    second = ref.run(SEED, 2)
    count2, abs2 = ref.count.copy(), ref.abs64.copy()
    ref.run(SEED, 1)                                              # leaves ref.count / ref.abs64 as the cached pass's
    n = np.repeat((ref.count + count2).astype(np.float64), 3)
    bnd = 1.01 * (n + 2) * 2.0 ** -24 * (ref.abs64 + abs2)
    assert ratio(np.abs(both.astype(np.float64) - (r64 + second[2])), bnd) <= 1.0
    assert not np.array_equal(both, s1)


def test_record_ranges_compose_and_capacity_is_checked():
    job, ctx, _, rrec, rstarts, _, _, _ = _case("ragged")
    a, sa, _ = ctx.mlt_records(seed=SEED, pass_index=1, first_chain=0, n_chains=47)
    b, sb, _ = ctx.mlt_records(seed=SEED, pass_index=1, first_chain=47, n_chains=210)
    assert np.array_equal(np.concatenate([a, b]).view(np.uint8), rrec.view(np.uint8))
    assert np.array_equal(np.concatenate([sa, sb]), rstarts)
    with pytest.raises(BlingError) as e:
        ctx.mlt_records(seed=SEED, pass_index=1, cap=10)
    assert e.value.rc == -1 and "561 records exceed the capacity 10" in str(e.value)


def test_refusals_leave_the_context_rendering():
    ctx = Context(0)
    ctx.upload(load_config("C1", "image=16,16"))                  # a path scene
    with pytest.raises(BlingError) as e:
        ctx.mlt_pass()
    assert e.value.rc == -1 and "not metropolis" in str(e.value)
    film, st = ctx.render_pass(seed=SEED, pass_index=1)
    assert np.isfinite(film).all() and st.camera_samples > 0
    ctx.close()
    os.environ["BLING_ALLOW_REPEATED_DEVICES"] = "1"              # a context holding several devices
    try:
        two = Context([0, 0])
        try:
            two.upload(load_config("C1", "image=8,8;metropolis=1,1,4,0.25,4"))
            with pytest.raises(BlingError) as e:
                two.mlt_pass()
        finally:
            two.close()
    finally:
        del os.environ["BLING_ALLOW_REPEATED_DEVICES"]
    assert e.value.rc == -1 and "single-device" in str(e.value)


def test_unwritten_bootstrap_slot_is_refused_and_the_context_goes_on():
    """Bootstrap contributions with a NaN (the test hook replaces the evaluated ones): a chain whose
    selection reads the slot the NaN left unwritten makes the pass BLING_EINVAL with that reason, as the
    restatement's bookkeeping says; with the hook off the same context renders the pass, record for record."""
    job, ctx, _, rrec, rstarts, _, _, rst = _case("wave")         # bootstrap 100, 64 chains
    I = np.ones(100, np.float32)
    I[10] = np.nan                                                # is has 99 entries; slot 89 stays unwritten ...
    I[9] = 1000.0                                                 # ... and is[89] = I[9] draws nearly every chain there
    _, want_starts, bad = boot_starts(I, SEED, 1, 64)
    assert bad is not None                                        # some chain's draw lands there
    ctx.mlt_set_boot(I)
    for call in (lambda: ctx.mlt_pass(seed=SEED, pass_index=1), lambda: ctx.mlt_records(seed=SEED, pass_index=1, cap=128)):
        with pytest.raises(BlingError) as e:
            call()
        assert e.value.rc == -1 and f"chain {bad} reads slot 89" in str(e.value) and "unwritten" in str(e.value)
    I[10] = 3.0                                                   # no NaN: the hook's values steer the starts
    ctx.mlt_set_boot(I)
    _, gstarts, gb = ctx.mlt_records(seed=SEED, pass_index=1)
    wb, wstarts, bad = boot_starts(I, SEED, 1, 64)
    assert bad is None and np.array_equal(gstarts, wstarts) and gb.view(np.uint32) == wb.view(np.uint32)
    ctx.mlt_set_boot(None)
    grec, gstarts, _ = ctx.mlt_records(seed=SEED, pass_index=1)
    assert np.array_equal(grec.view(np.uint8), rrec.view(np.uint8)) and np.array_equal(gstarts, rstarts)
    _, gst = ctx.mlt_pass(seed=SEED, pass_index=1)
    assert _counts(gst) == rst.counts()


def test_cli_writes_the_weighted_pass_images(tmp_path):
    """`bling <scene> --passes 2` on a Metropolis scene: its printed b is bnext of the passes' b' values."""
    exe = os.path.join(_ffi.LIBDIR, "bling")
    ov = "image=16,16;chains=64"
    out = subprocess.run([exe, os.path.join(SCENE_DIR, "metropolis.bling"), "--overrides", ov, "--passes", "2", "--out",
                          str(tmp_path / "pass")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    for p in (1, 2):
        for ext in ("png", "hdr"):
            assert os.path.getsize(tmp_path / f"pass-{p:05d}.{ext}") > 0
    from bling_amd.scene import parse_job
    job = parse_job(os.path.join(SCENE_DIR, "metropolis.bling"), ov)
    ctx = Context(0)
    ctx.upload(job)
    b, want = np.float32(1), []
    for p in (1, 2):
        _, st = ctx.mlt_pass(seed=SEED, pass_index=p)
        b = mlt_bnext(p, b, st.b)
        want.append(f"b = {float(b):g},")
    ctx.close()
    got = [ln for ln in out.stdout.splitlines() if ln.startswith("pass ")]
    assert len(got) == 2 and all(w in g for w, g in zip(want, got)), (want, got)


def test_render_returns_the_weighted_splat_image():
    job = load_config("C1", "image=8,8;metropolis=5,2,100,0.25,64")
    rgb = render(job, passes=2, seed=SEED)
    assert rgb.shape == (8, 8, 3) and np.isfinite(rgb).all() and rgb.max() > 0
