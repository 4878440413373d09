"""The Metropolis renderer (Renderer/Metropolis.hs) on the host: the loader's `metropolis` block and
overrides, upload validation, and the CPU restatement (tests/ref/mlt_ref.cpp) that the device is pinned
against -- jitter and the draw order against numpy, the chain split, the bootstrap's reversed index
mapping, and convergence of the pass image to the bidirectional integrator's own image.

Convergence.  On the shielded diffuse room (48 x 32, maxDepth 3), 4 x 4 block means of 24 independent
one-pass images b' * splat against 24 passes of 8 uniformly placed bd_ref_sample_li samples per pixel
binned by floor, test_mwc_sampler's bars (max |z| < 4.5, mean z^2 < 2): the figures are printed by the
test.  Both sides run the same integrator, so its traps (T26, T30) cancel; with b replaced by 1 the
same statistic rejects the image.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from bling_amd import _ffi  # noqa: E402
from bling_amd.scene import SCENES, load_config, parse_job  # noqa: E402
from bling_amd.film import mlt_bnext, mlt_image  # noqa: E402
from bling_amd.render import BlingError, mlt_boot  # noqa: E402
from bling_amd.scene import film_splat_to_rgb  # noqa: E402
import mlt_ref  # noqa: E402
from mlt_cases import CASES, bound, ratio  # noqa: E402
from mlt_ref import MltRef  # noqa: E402

SEED = 0x0B11A6
DIFFUSE = os.path.join(SCENES, "light-tracer-diffuse.bling")
Z_MAX, Z2_MEAN = 4.5, 2.0                      # tests/test_mwc_sampler.py
f32 = np.float32
M32 = 0xFFFFFFFF
DIM_FRESH1D, MLT_CHAIN_PIXEL = 0x7000, 0x50000000


# ------------------------------------------------------------------ loader and validation
def _scene(tmp_path, block):
    src = open(os.path.join(SCENES, "cornell-box.bling")).read()
    p = tmp_path / "mlt.bling"
    p.write_text(src + "\nrenderer { " + block + " }\n")
    return str(p)


def test_loader_reads_the_metropolis_block(tmp_path):
    job = parse_job(_scene(tmp_path, "metropolis maxDepth 7 mpp 0.5 bootstrap 300 plarge 0.125 directSamples 0"),
                    "image=64,32")
    mp = job.metropolis
    assert job.config.renderer == 4                               # BLING_RENDERER_METROPOLIS
    assert (mp.max_depth, mp.mpp, mp.bootstrap, mp.plarge) == (7, 0.5, 300, 0.125)
    assert mp.chains == 1024                                      # the default 4096, capped at M = 0.5 * 64 * 32
    assert (job.config.integrator, job.config.max_depth, job.config.sample_depth) == (2, 7, 7)
    assert "renderer metropolis md=7" in job.summary()
    assert parse_job(job.path, "image=256,256").metropolis.chains == 4096
    assert parse_job(job.path, "image=64,32;chains=65").metropolis.chains == 65


def test_the_shipped_fixture_is_the_reference_block():
    job = parse_job(os.path.join(SCENES, "metropolis.bling"))
    mp = job.metropolis
    assert job.config.renderer == 4
    assert (mp.max_depth, mp.mpp, mp.bootstrap, mp.plarge, mp.chains) == (10, 1.0, 1000, 0.25, 4096)


def test_direct_samples_stay_unserved(tmp_path):
    job = parse_job(_scene(tmp_path, "metropolis maxDepth 5 mpp 10 bootstrap 100 plarge 0.3 directSamples 4"))
    assert job.config.renderer == 1                               # BLING_RENDERER_OTHER (trap T32)


def test_metropolis_override():
    job = load_config("X5", "image=16,16;metropolis=3,2,50,0.5,7")    # over the shipped sppm block
    mp = job.metropolis
    assert job.config.renderer == 4 and (mp.max_depth, mp.mpp, mp.bootstrap, mp.plarge, mp.chains) == (3, 2.0, 50, 0.5, 7)
    assert load_config("X5", "image=16,16;metropolis=3,2,50,0.5,7;force_path=1").config.renderer == 4


@pytest.mark.parametrize("ov,reason", [
    ("metropolis=0,1,10,0.25,4", "metropolis maxDepth outside [1, 16]"),
    ("metropolis=17,1,10,0.25,4", "metropolis maxDepth outside [1, 16]"),
    ("metropolis=5,1,0,0.25,4", "metropolis bootstrap < 1"),
    ("metropolis=5,0.001,10,0.25,4", "metropolis mpp gives no mutation"),
    ("metropolis=5,1,10,0.25,0", "metropolis chains < 1"),
])
def test_validate_refuses_with_its_reason(ov, reason):
    hip = _ffi.hip()
    job = load_config("C1", "image=16,16;" + ov)
    assert hip.bling_scene_validate(C.c_void_p(job.desc)) == -1
    assert reason in hip.bling_last_error().decode()


def test_validate_accepts_the_bounds():
    hip = _ffi.hip()
    for ov in ("metropolis=1,1,1,0,1", "metropolis=16,0.004,10,1,300"):      # M = 1 with chains above it
        job = load_config("C1", "image=16,16;" + ov)
        assert hip.bling_scene_validate(C.c_void_p(job.desc)) == 0, hip.bling_last_error().decode()


# ------------------------------------------------------------------ jitter and the draw order
def _jitter_np(v, vmin, vmax, u1, u2):
    """jitter (Metropolis.hs:221-239) in numpy binary32; exp / log rounded once from binary64."""
    v, vmin, vmax, u1, u2 = f32(v), f32(vmin), f32(vmax), f32(u1), f32(u2)
    a, b = f32(1) / f32(1024), f32(1) / f32(256)
    log_rat = -f32(np.log(np.float64(f32(b / a))))
    delta = f32(f32(f32(vmax - vmin) * b) * f32(np.exp(np.float64(f32(log_rat * u1)))))
    x = f32(v + delta) if u2 < f32(0.5) else f32(v - delta)
    if x >= vmax:
        return f32(vmin + f32(x - vmax))
    if x < vmin:
        return f32(vmax - f32(vmin - x))
    return x


def test_jitter_known_answers_at_both_edges():
    cases = [(0.999, 0, 1, 0.0, 0.25), (0.9999999, 0, 1, 0.7, 0.1),      # past vmax: wraps to the bottom
             (0.0005, 0, 1, 0.3, 0.75), (0.0, 0, 1, 1.0 - 2.0 ** -24, 0.5),  # below vmin: wraps to the top
             (47.99, 0, 48, 0.5, 0.0), (0.01, 0, 33, 0.2, 0.9), (0.5, 0, 1, 0.6, 0.4999), (0.5, 0, 1, 0.6, 0.5)]
    wrapped = 0
    for v, lo, hi, u1, u2 in cases:
        want, got = _jitter_np(v, lo, hi, u1, u2), mlt_ref.jitter(v, lo, hi, u1, u2)
        assert want.view(np.uint32) == got.view(np.uint32), (v, lo, hi, u1, u2, want, got)
        assert lo <= got < hi
        wrapped += abs(float(got) - v) > 0.5 * (hi - lo)
    assert wrapped == 6
    assert mlt_ref.jitter(0.5, 0, 1, 0.0, 0.0) == f32(0.5) + f32(1) / f32(256)        # the largest step, b
    assert abs(float(mlt_ref.jitter(0.5, 0, 1, 1.0, 0.0)) - 0.5 - 1 / 1024) < 1e-7    # the smallest, a


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M32


def _fmix(h):
    h ^= h >> 16; h = (h * 0x85ebca6b) & M32; h ^= h >> 13; h = (h * 0xc2b2ae35) & M32; h ^= h >> 16
    return h


def _mix(h, k):
    k = (k * 0xcc9e2d51) & M32; k = _rotl(k, 15); k = (k * 0x1b873593) & M32
    h ^= k; h = _rotl(h, 13)
    return (h * 5 + 0xe6546b64) & M32


def _draw(seed, pass_index, pixel, sample, ordinal):
    """u01 of common/counter_rng.h's draw at DIM_FRESH1D + ordinal."""
    sk = _fmix(_mix(_mix(seed, pass_index), pixel) ^ ((sample * 0x9E3779B9) & M32))
    return f32((_fmix(sk ^ _fmix((DIM_FRESH1D + ordinal) ^ 0x2C1B3C6D)) >> 8) * 2.0 ** -24)


def test_draw_order_on_each_side_of_plarge():
    """One mutation with the large-step draw forced on each side of plarge: ordinal 0 is the test; a
    large step reads ordinals 1 .. nv in initialSample's order and leaves nv + 1 for the acceptance; a
    small step reads one rnd2D per value in vector order, then x, y, lu, lv, and leaves 2 nv + 1."""
    md, sx, sy, chain, m, pss = 2, 33.0, 17.0, 65, 7, 3
    n1d, n2d = 12 * md + 1, 9 * md + 2
    nv = n1d + 2 * n2d + 4
    cur = np.random.default_rng(1).random(nv).astype(f32)
    cur[nv - 4], cur[nv - 3] = f32(32.99), f32(0.01)
    u = [_draw(SEED, pss, MLT_CHAIN_PIXEL | chain, m, k) for k in range(2 * nv + 2)]
    above = np.nextafter(u[0], f32(2))
    prop, large, n = mlt_ref.mutate(SEED, pss, chain, m, md, sx, sy, above, cur)          # u0 < plarge
    assert large and n == nv + 1
    want = np.array(u[1:nv + 1], f32)
    want[nv - 4] = f32(f32(f32(1) - u[nv - 3]) * f32(0)) + f32(u[nv - 3] * f32(sx))       # lerp ox 0 sx
    want[nv - 3] = f32(f32(f32(1) - u[nv - 2]) * f32(0)) + f32(u[nv - 2] * f32(sy))
    assert np.array_equal(prop.view(np.uint32), want.view(np.uint32))
    prop, large, n = mlt_ref.mutate(SEED, pss, chain, m, md, sx, sy, u[0], cur)           # not (u0 < plarge)
    assert not large and n == 2 * nv + 1
    hi = np.ones(nv, f32)
    hi[nv - 4], hi[nv - 3] = sx, sy                                                       # the image, not the sample extent
    want = np.array([_jitter_np(cur[r], 0, hi[r], u[1 + 2 * r], u[2 + 2 * r]) for r in range(nv)], f32)
    assert np.array_equal(prop.view(np.uint32), want.view(np.uint32))
    assert (prop[:nv - 4] < 1).all() and 0 <= prop[nv - 4] < sx and 0 <= prop[nv - 3] < sy


# ------------------------------------------------------------------ chains and the bootstrap
@pytest.mark.parametrize("chains", [1, 65])
def test_chain_split_does_exactly_m_mutations(chains):
    job = load_config("C1", f"image=20,10;metropolis=1,1,16,0.25,{chains}")
    assert mlt_ref.mutations(job) == 200
    rec, starts, s64, s32, st = MltRef(job).run(SEED, 1)
    assert len(rec) == 200 and st.mutations == 200
    per = np.bincount(rec["chain"], minlength=chains)
    want = [200 // chains + (1 if c < 200 % chains else 0) for c in range(chains)]
    assert per.tolist() == want == [mlt_ref.chain_mutations(200, chains, c) for c in range(chains)]
    for c in range(chains):
        assert rec["mutation"][rec["chain"] == c].tolist() == list(range(want[c]))
    assert len(starts) == chains and starts.max() < 16
    assert st.large_steps == int((rec["flags"] & 1).sum()) and st.accepted == int((rec["flags"] >> 1).sum())
    assert np.allclose(s32, s64, rtol=1e-4, atol=1e-7)


def test_bootstrap_index_mapping_is_the_reversed_one():
    """`is` is consed, smps written at n - i - 1: without a NaN slot j holds sample n - 1 - j, whose I
    is is[j].  A NaN sample is dropped from `is` but leaves its slot unwritten (trap T34)."""
    I = np.array([0.0, 0.0, 5.0, 0.0], f32)                       # only sample 2 can be chosen: is = [0, 5, 0, 0]
    slot, smp, b = mlt_ref.boot_select(I, 0.5)
    assert (slot, smp) == (1, 2) and b == f32(1.25)
    I = np.array([1.0, np.nan, 1.0, 1.0], f32)                    # is = [1, 1, 1]; slots 3, 1, 0 written, 2 not
    assert mlt_ref.boot_select(I, 0.1)[:2] == (0, 3)
    assert mlt_ref.boot_select(I, 0.5)[:2] == (1, 2)              # slot 1 holds sample 2
    assert mlt_ref.boot_select(I, 0.9)[0] == -1                   # slot 2 was never written: an error, refused
    assert mlt_ref.boot_select(I, 0.9)[2] == f32(0.75)            # the NaN counts as 0 in sumI / n
    assert mlt_ref.boot_select(np.array([np.nan], f32), 0.5)[0] == -1


def test_the_drivers_bookkeeping_equals_the_restatements():
    """bling_debug_mlt_boot runs the function the device pass runs on its bootstrap contributions
    (mlt_pass.hip mlt_boot_select): b' and every chain's start equal the restatement's, with and without
    NaN entries, and a selection on an unwritten slot is BLING_EINVAL with its reason."""
    rng = np.random.default_rng(7)
    for n, chains, nans in ((1, 3, ()), (4, 65, ()), (100, 257, ()), (100, 64, (0, 99)), (7, 16, (6,))):
        I = rng.random(n).astype(f32)
        I[rng.random(n) < 0.2] = 0                                # black samples: zero-width cdf steps
        I[list(nans)] = np.nan                                    # at the ends: slots n - 1 / 0 unwritten, weight 0 or small
        for pss in (1, 2):
            wb, wstarts, bad = mlt_ref.boot_starts(I, SEED, pss, chains)
            if bad is None:
                gb, gstarts = mlt_boot(I, SEED, pss, chains)
                assert gb.view(np.uint32) == wb.view(np.uint32) and np.array_equal(gstarts, wstarts), (n, chains, nans)
            else:
                with pytest.raises(BlingError) as e:
                    mlt_boot(I, SEED, pss, chains)
                assert e.value.rc == -1 and f"chain {bad} reads slot" in str(e.value)
    I = np.array([1.0, np.nan, 1.0, 1.0], f32)                    # the hand-built case above: slot 2 unwritten
    hit = [c for c in range(64) if mlt_ref.boot_starts(I, SEED, 1, c + 1)[2] == c]
    assert hit                                                    # some chain's draw lands on slot 2 ...
    with pytest.raises(BlingError) as e:
        mlt_boot(I, SEED, 1, hit[0] + 1)
    assert e.value.rc == -1 and f"chain {hit[0]} reads slot 2, which a NaN bootstrap sample left unwritten" in str(e.value)
    if hit[0] > 0:                                                # ... and the chains before it are served, literally
        gb, gstarts = mlt_boot(I, SEED, 1, hit[0])
        assert gb == f32(0.75) and np.array_equal(gstarts, mlt_ref.boot_starts(I, SEED, 1, hit[0])[1])
        assert set(gstarts.tolist()) <= {3, 2}                    # slot 0 holds sample 3, slot 1 sample 2
    with pytest.raises(BlingError):
        mlt_boot(np.array([np.nan], f32), SEED, 1, 1)


@pytest.mark.parametrize("name", list(CASES))
def test_restatements_binary32_image_is_inside_the_derived_bound(name):
    """|image32 - F64| <= 1.01 (n + 2) 2^-24 A64 per pixel and channel, for every device parity case."""
    cfg, ov = CASES[name]
    ref = MltRef(load_config(cfg, ov))
    rec, starts, s64, s32, st = ref.run(SEED, 1)
    r = ratio(np.abs(s32.astype(np.float64) - s64), bound(ref))
    print(name, "worst |image32 - F64| / bound", r)
    assert np.isfinite(s32).all() and r <= 1.0


def test_pass_image_weight_is_bnext_over_p():
    """film.mlt_image: getPixel with splat weight bnext / p, bnext = lerp (1 / p) b b' from b = 1."""
    bs = [f32(0.25), f32(0.75), f32(0.5)]
    b1 = f32(f32(f32(1) - f32(1)) * f32(1)) + f32(f32(1) * bs[0])                    # p = 1: b'
    b2 = f32(f32(f32(1) - f32(0.5)) * b1) + f32(f32(0.5) * bs[1])
    t3 = f32(1) / f32(3)
    b3 = f32(f32(f32(1) - t3) * b2) + f32(t3 * bs[2])
    assert mlt_bnext(1, 1, bs[0]) == b1 == f32(0.25) and mlt_bnext(2, b1, bs[1]) == b2 == f32(0.5)
    assert mlt_bnext(3, b2, bs[2]) == b3
    splat = np.random.default_rng(3).random(4 * 2 * 3).astype(f32)
    for k, b in ((1, b1), (2, b2), (3, b3)):
        want = film_splat_to_rgb(None, splat, f32(b / f32(k)), 4, 2)
        assert np.array_equal(mlt_image(splat, bs[:k], 4, 2), want) and want.any()


# ------------------------------------------------------------------ convergence
def _blocks(img, w, h, b=4):
    return img.reshape(h // b, b, w // b, b, 3).mean((1, 3)).ravel()


def _z(a, b):
    d = a.mean(0) - b.mean(0)
    se = np.sqrt(a.var(0, ddof=1) / len(a) + b.var(0, ddof=1) / len(b))
    flat = (se == 0) & (d == 0)
    return np.where(flat, 0.0, d / np.where(flat, 1.0, se))


def test_pass_image_converges_to_the_integrators_image():
    w, h, passes, spp = 48, 32, 24, 8
    job = parse_job(DIFFUSE, "random=8;metropolis=3,8,1000,0.25,64")
    ref = MltRef(job)
    mlt, one = [], []
    for p in range(passes):
        rec, starts, s64, s32, st = ref.run(SEED, 1 + p)
        assert st.dropped == 0
        mlt.append(_blocks(np.float64(f32(st.b)) * s64, w, h))     # pass 1: bnext = b', weight b' / 1
        one.append(_blocks(s64, w, h))                             # b replaced by 1
    ys, xs = np.mgrid[0:h, 0:w]
    want = []
    for p in range(passes):
        smp = np.stack([np.repeat(xs.ravel(), spp), np.repeat(ys.ravel(), spp), np.tile(np.arange(spp), w * h)], 1)
        xyz = mlt_ref.xyz(ref.sample_li(SEED, 1000 + p, smp))
        want.append(_blocks(xyz.reshape(h * w, spp, 3).mean(1), w, h))
    mlt, one, want = np.array(mlt), np.array(one), np.array(want)
    z = _z(mlt, want)
    print("mlt vs bidir: max |z|", np.abs(z).max(), "mean z^2", (z ** 2).mean(), "ratio", mlt.mean() / want.mean())
    assert np.isfinite(z).all()
    assert np.abs(z).max() < Z_MAX, np.abs(z).max()
    assert (z ** 2).mean() < Z2_MEAN, (z ** 2).mean()
    z1 = _z(one, want)
    print("b = 1: max |z|", np.abs(z1).max(), "mean z^2", (z1 ** 2).mean(), "ratio", one.mean() / want.mean())
    assert (z1 ** 2).mean() > 2 * Z2_MEAN and np.abs(z1).max() > Z_MAX
