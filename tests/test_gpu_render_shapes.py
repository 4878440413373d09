"""Sampler, filter, camera and image shapes the other parity tests never render (tests/shape_scenes.py):
non-power-of-two and non-square samplers, fractional, non-square, very narrow and very wide filters,
box and gauss, both slot orders at a non-power-of-two spp, image sizes around one tile, the
environment camera.

Per-sample parity is asserted as tests/test_gpu_parity.py::test_sample_li_full_config does: image
positions bit-exact, no spectrum off by more than 1e-4 (relative L1), equal ray counts.

The films are held to a derived bound, not to a measured bar (tests/film_ref.py):
the device's film against the float64 film of its own per-sample results, |film - F64| <= 1.01 (n + 2)
2^-24 A64 per pixel and channel, and against the oracle's binary32 film within twice that.  The CPU
tests of this file (not marked gpu) show the oracle's own film inside the same bound for every case
of the table, and that the shapes reach the edges they are there for.
"""
import numpy as np
import pytest

import shape_scenes as sc
from film_ref import film_ref, pair_bound, pass_samples, pass_tiles, spectra_to_results, worst_ratio
from oracle_py import Oracle
from parity_util import film_errors, report, spectra_mismatch

SEED = 0x0B11A6
PASS = 0
ALMOST_ONE = np.float32(1) - np.float32(2.0 ** -24)           # the largest binary32 below 1
RAY_KINDS = ("rays_camera", "rays_continuation", "rays_mis", "rays_shadow")
gpu = pytest.mark.gpu
_cache = {}


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("shape_scenes")


def _job(case, scene_dir):
    if ("job", case.tag) not in _cache:
        _cache["job", case.tag] = sc.load(case, scene_dir)
    return _cache["job", case.tag]


def _oracle(case, scene_dir):
    """(job, oracle, samples, L, img, stats): every sample of the case's extent, or 4 096 random ones
    if that is fewer, through the oracle -- computed once."""
    if ("smp", case.tag) not in _cache:
        job = _job(case, scene_dir)
        orc = Oracle(job)
        s = pass_samples(job, 0)
        if len(s) > 4096:
            s = s[np.sort(np.random.default_rng(11).choice(len(s), 4096, replace=False))]
        _cache["smp", case.tag] = (job, orc, s) + tuple(orc.sample_li_batch(s, seed=SEED, pass_index=case.pass_index))
    return _cache["smp", case.tag]


def _oracle_pass(case, scene_dir):
    """(job, the oracle's film and stats of the whole pass, F64, A64, n of the oracle's own per-sample
    results), computed once."""
    if ("film", case.tag) not in _cache:
        job = _job(case, scene_dir)
        orc = Oracle(job)
        s = pass_samples(job, 0)                               # render_tile's order: pixel-major
        L, img, _ = orc.sample_li_batch(s, seed=SEED, pass_index=case.pass_index)
        ref = film_ref(spectra_to_results(L), img, job.filter_table(), job.filter_size, job.width, job.height,
                       pass_tiles(job), job.spp)
        film, st = orc.render(seed=SEED, pass_index=case.pass_index)
        _cache["film", case.tag] = (job, film, st) + ref
    return _cache["film", case.tag]


# ------------------------------------------------------------------ CPU: the bound holds for the oracle
def test_xyz_restatement_is_the_oracles(scene_dir):
    """With a filter narrower than half a pixel at 1 spp no pixel receives more than one splat, so the
    oracle's film holds single rounded products X * weight: they equal film_ref's exact products
    rounded once, bit for bit -- spectra_to_results is the oracle's to_xyz."""
    case = sc.Case("xyz pin", "X1", "image=24,16;path=5,2;stratified=1,1", filter="filter triangle 0.4 0.4")
    job, film, st, F, A, n = _oracle_pass(case, scene_dir)
    assert n.max() == 1 and (n == 1).sum() > job.width * job.height // 2
    assert np.array_equal(film.reshape(F.shape), F.astype(np.float32))
    assert (F[..., 1:] > 0).any()


@pytest.mark.parametrize("case", sc.FILM_CASES, ids=str)
def test_oracle_film_is_within_the_derived_bound(case, scene_dir):
    job, film, st, F, A, n = _oracle_pass(case, scene_dir)
    assert st.samples == job.camera_samples() and st.dropped == 0
    assert np.isfinite(film).all() and (n > 0).any() and (A[..., 1:] > 0).any()
    r = worst_ratio(film, F, A, n)
    report("shape_film_oracle", case=case.tag, ratio=r, n_max=int(n.max()), samples=int(st.samples))
    assert r <= 1.0, r


def test_film_cases_reach_their_kernels(scene_dir):
    """K = 2 floor(0.5 + fw) + 1 per axis (core.hip launch_film): the table holds K = 5 and K = 7 at
    fractional widths, generic cases, a tile image narrower than its tile and the widest tile image."""
    k = {}
    for case in sc.FILM_CASES:
        fw, fh = _job(case, scene_dir).filter_size
        k[case.tag] = tuple(2 * int(np.floor(np.float32(0.5) + np.float32(v))) + 1 for v in (fw, fh))
    assert k["mitchell 1.5 1.5"] == k["triangle 2.4 2.4"] == k["gauss 2 2 1"] == (5, 5)
    assert k["mitchell 2.5 2.5"] == k["triangle 3 3"] == (7, 7)
    assert k["box"] == (3, 3) and k["triangle 2 3"] == (5, 7) and k["triangle 3 2"] == (7, 5)
    assert k["triangle 0.4 0.4"] == (1, 1) and k["triangle 15 15"] == (31, 31)
    assert _job(sc.FILTER_CASES[-1], scene_dir).tile_slot() == (30, 30)      # of the LDS tile's 32
    for case in sc.FILM_CASES:
        job = _job(case, scene_dir)
        assert job.width * job.height <= 40 * 24 and job.spp <= 9


# ------------------------------------------------------------------ CPU: non-vacuity
@pytest.mark.parametrize("shape", sc.CLAMPED)
def test_pixel_offsets_reach_the_clamp(shape, scene_dir):
    case = next(c for c in sc.SAMPLE_CASES if c.tag == "X1 lens " + shape)
    job, orc, s, L, img, st = _oracle(case, scene_dir)
    k = s[::7]
    cam = np.array([orc.sampler_probe(int(x), int(y), int(n), 2, seed=SEED, pass_index=case.pass_index) for x, y, n in k])
    clamped = cam[:, 0] == ALMOST_ONE
    nu = job.config.nu
    assert np.array_equal(clamped, k[:, 2] // nu >= nu)                    # trap T5: u = n / nu passes nu - 1
    assert 0 < clamped.mean() < 1
    # and the image position of such a sample is the next pixel's left edge (x >= 1: x + ALMOST_ONE rounds up)
    far = clamped & (k[:, 0] >= 1)
    assert far.any()
    _, _, _, _, img_all, _ = _oracle(case, scene_dir)
    assert np.array_equal(img_all[::7][far, 0], (k[far, 0] + 1).astype(np.float32))
    assert (cam[:, 2] == ALMOST_ONE).any()                                 # the lens sample clamps too


def _permute_rounds(i, l, p):
    """tests/test_rng_loader.py permute with its cycle walk counted: (result, rounds of the loop)."""
    M = 0xFFFFFFFF
    w = l - 1
    for s in (1, 2, 4, 8, 16):
        w |= w >> s
    rounds = 0
    while True:
        rounds += 1
        i ^= p; i = (i * 0xe170893d) & M; i ^= p >> 16; i ^= (i & w) >> 4; i ^= p >> 8
        i = (i * 0x0929eb3f) & M; i ^= p >> 23; i ^= (i & w) >> 1; i = (i * (1 | p >> 27)) & M
        i = (i * 0x6935fa69) & M; i ^= (i & w) >> 11; i = (i * 0x74dcb303) & M; i ^= (i & w) >> 2
        i = (i * 0x9e501cc3) & M; i ^= (i & w) >> 2; i = (i * 0xc860a3df) & M; i &= w; i ^= i >> 5
        if i < l:
            break
    return (i + p) % l, rounds


@pytest.mark.parametrize("shape,spp", [("stratified=1,5", 5), ("stratified=3,2", 6), ("random=7", 7),
                                       ("stratified=3,3", 9)])
def test_non_power_of_two_spp_reenters_the_cycle_walk(shape, spp, scene_dir):
    """The lens permutation's keys of the pass (camera_sample: permute(n, spp, hash5(seed, pass, pixel,
    ALL_SAMPLES, DIM_LENS_PERM))): for some (n, pixel) the masked value is >= spp and the loop runs
    again, which it never does at a power of two.  (random=7 draws no permutation; its spp is walked
    with the same keys to show the property is the length's.)"""
    from test_rng_loader import hash5, permute
    case = next(c for c in sc.SAMPLE_CASES if c.tag == "X1 lens " + shape)
    job = _job(case, scene_dir)
    assert job.spp == spp
    x0, x1, y0, y1 = job.extent()
    again = 0
    for pixel in range(0, (x1 - x0 + 1) * (y1 - y0 + 1), 5):
        p = hash5(SEED, PASS, pixel, 0xFFFFFFFF, 0x2000)
        for n in range(spp):
            k, rounds = _permute_rounds(n, spp, p)
            assert k == permute(n, spp, p)
            again += rounds > 1
    assert again > 0
    assert all(_permute_rounds(n, 8, 0x12345678 + n)[1] == 1 for n in range(8))


def test_the_lens_reaches_the_radiance(scene_dir):
    lens = next(c for c in sc.SAMPLE_CASES if c.tag == "X1 lens stratified=3,2")
    _, _, s, L, img, _ = _oracle(lens, scene_dir)
    _, _, s0, L0, img0, _ = _oracle(sc.PINHOLE, scene_dir)
    assert np.array_equal(s, s0) and np.array_equal(img, img0)             # same camera samples
    lit = (L != 0).any(1) | (L0 != 0).any(1)                               # the rest escapes, black, either way
    differs = (L != L0).any(1)
    assert lit.mean() > 0.25 and differs[lit].mean() > 0.9, (lit.mean(), differs[lit].mean())


def test_c1_pass0_shadow_rays_end_exactly_on_the_light(scene_dir):
    """Why C1 at stratified 3 2 renders pass 1 (tests/shape_scenes.py).  At three vertices of pass 0 the
    device's shadow ray is occluded and the oracle's is not, everything before it equal bit for bit
    (per-vertex records of a BLING_DEBUG_VERTEX build on MI355X; not changed by the MIS cull or by the
    exhaustive traversal).  This pins the cause as an exact tie inside the oracle: along the light
    sample's direction the closest hit is the light's own quad (primitive 0) at a distance t whose ulp
    exceeds the vertex's ray epsilon, so the shadow ray's tmax = len - eps is t itself; with tmax = t the
    kd-tree reports no hit, one ulp further it reports the quad.  Whether the quad at t == tmax counts
    is the traversal's choice (the kd-tree prunes its cell, a BVH tests it), as in tests/test_c2_tie.py."""
    job = _job(sc.C1_32_PASS0, scene_dir)
    orc = Oracle(job)
    s = np.array([[5, 1, 5], [18, 12, 2]], np.int32)
    _, v = orc.sample_li_vertices(s, seed=SEED, pass_index=0)
    for k, d in ((0, 5), (1, 4)):
        p, wi, eps = v[k, d, 7:10], v[k, d, 14:17], v[k, d, 13]
        assert v[k, d, 28] == 0                                           # the oracle: unoccluded

        def ray(tmax):
            return np.array([[p[0]], [p[1]], [p[2]], [wi[0]], [wi[1]], [wi[2]], [eps], [tmax]], np.float32)
        t, prim, _, _ = orc.trace(ray(np.inf))
        t = np.float32(t[0])
        assert prim[0] == 0 and np.float32(t - eps) == t                    # eps below the ulp of t
        assert orc.trace(ray(t), any_hit=True)[1][0] == 0                   # the quad at t == tmax: not found
        assert orc.trace(ray(np.nextafter(t, np.float32(np.inf))), any_hit=True)[1][0] == 1


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx():
    from bling_amd.render import Context
    c = Context(0)
    yield c
    c.close()


def _assert_samples(ctx, case, scene_dir):
    job, orc, s, Lo, img_o, st_o = _oracle(case, scene_dir)
    ctx.upload(job)
    Lg, img_g, st_g = ctx.sample_li(s, seed=SEED, pass_index=case.pass_index)
    bad, exact, worst, _ = spectra_mismatch(Lg, Lo)
    report("shape_samples", case=case.tag, samples=len(s), mismatch=bad, exact=exact, worst_rel_ok=worst,
           rays_gpu=st_g.rays(), rays_oracle=st_o.rays())
    np.testing.assert_array_equal(img_g, img_o)                             # camera samples: bit-exact
    assert bad == 0
    for nm in RAY_KINDS:
        assert getattr(st_g, nm) == getattr(st_o, nm), nm
    assert np.abs(Lo).sum() > 0


@gpu
@pytest.mark.parametrize("case", sc.SAMPLE_CASES, ids=str)
def test_sample_parity_across_sampler_shapes(ctx, case, scene_dir):
    _assert_samples(ctx, case, scene_dir)


def _device_pass(ctx, job, case, **kw):
    """One pass on the device: (film, stats, F64, A64, n of the device's own per-sample results)."""
    ctx.upload(job)
    film, st = ctx.render_pass(seed=SEED, pass_index=case.pass_index, **kw)
    res, waves = ctx.pass_results()
    major = ctx.scene_info()["sample_major"]
    s = pass_samples(job, major, kw.get("shard", (0, 1)))
    assert waves in (1, -2) and len(res) == len(s) == st.camera_samples
    _, img, _ = ctx.sample_li(s, seed=SEED, pass_index=case.pass_index)
    ref = film_ref(res, img, job.filter_table(), job.filter_size, job.width, job.height,
                   pass_tiles(job, kw.get("shard", (0, 1))), job.spp)
    return (film, st, major) + ref


def _assert_film(ctx, case, scene_dir):
    job, film_o, st_o, Fo, Ao, no = _oracle_pass(case, scene_dir)
    film, st, major, F, A, n = _device_pass(ctx, job, case)
    r_dev = worst_ratio(film, F, A, n)
    r_orc = worst_ratio(film_o, Fo, Ao, no)
    d = np.abs(film.astype(np.float64) - film_o.astype(np.float64)).reshape(F.shape)
    r_pair = float((d / pair_bound(A, n)).max())
    report("shape_film", case=case.tag, sample_major=major, ratio_device=r_dev, ratio_oracle=r_orc, ratio_pair=r_pair,
           n_max=int(n.max()), samples=int(st.camera_samples), **film_errors(film, film_o),
           **{"d_" + k: int(getattr(st, k)) - int(getattr(st_o, k)) for k in RAY_KINDS})
    assert np.isfinite(film).all()
    assert st.camera_samples == st_o.samples == job.camera_samples() and st.dropped_samples == 0
    for k in RAY_KINDS:
        assert getattr(st, k) == getattr(st_o, k), k
    assert np.array_equal(n, no)                                            # every splat lands where the oracle's does
    assert r_dev <= 1.0, r_dev
    assert r_pair <= 1.0, r_pair
    return major


@gpu
@pytest.mark.parametrize("case", sc.FILTER_CASES + sc.SIZE_CASES, ids=str)
def test_film_within_the_derived_bound(ctx, case, scene_dir):
    _assert_film(ctx, case, scene_dir)


@gpu
@pytest.mark.parametrize("case", sc.SLOT_CASES, ids=str)
def test_film_in_both_slot_orders(ctx, case, scene_dir):
    """stratified 3 2 and random 5 under pixel-major (C1) and sample-major (C4) slots: k_raygen's
    j / npix and fd_spp.div(j), k_film_gather's base + n * stride."""
    major = _assert_film(ctx, case, scene_dir)
    assert major == (1 if case.base == "C4" else 0)


@gpu
def test_both_slot_orders_occur(ctx, scene_dir):
    seen = set()
    for case in sc.SLOT_CASES:
        ctx.upload(_job(case, scene_dir))
        seen.add(ctx.scene_info()["sample_major"])
    assert seen == {0, 1}


@gpu
def test_environment_camera(ctx, scene_dir):
    from scene_desc import desc
    assert desc(_job(sc.ENV_CASE, scene_dir)).camera.kind == 1              # BLING_CAM_ENVIRONMENT
    _assert_samples(ctx, sc.ENV_CASE, scene_dir)
    _assert_film(ctx, sc.ENV_CASE, scene_dir)


def _tile_film(ctx, job, case, shards):
    """render_pass_tiles + film_add_tiles of each shard into one device film: (film, [stats])."""
    from test_gpu_bidir import _DeviceFloats
    bufs, stats = [_DeviceFloats(job.width * job.height * 4)], []
    try:
        for shard in shards:
            org, sw, sh = ctx.tile_layout(shard=shard)
            assert (sw, sh) == job.tile_slot() and np.array_equal(org, job.shard_tiles(*shard))
            t = _DeviceFloats(max(1, len(org)) * sw * sh * 4)
            bufs.append(t)
            stats.append(ctx.render_pass_tiles(t.p.value, seed=SEED, pass_index=case.pass_index, shard=shard, tiles_capacity=t.n))
            ctx.film_add_tiles(t.p.value, bufs[0].p.value, shard=shard, tiles_capacity=t.n)
        return bufs[0].host(), stats
    finally:
        for b in bufs:
            b.free()


@gpu
@pytest.mark.parametrize("case", sc.TILE_CASES, ids=str)
def test_tile_images_within_the_derived_bound(ctx, case, scene_dir):
    job = _job(case, scene_dir)
    _, st, _, F, A, n = _device_pass(ctx, job, case)
    one, _ = _tile_film(ctx, job, case, [(0, 1)])
    two, sts = _tile_film(ctx, job, case, [(0, 2), (1, 2)])
    r1, r2 = worst_ratio(one, F, A, n), worst_ratio(two, F, A, n)
    report("shape_tiles", case=case.tag, ratio_one=r1, ratio_shards=r2, slot=list(job.tile_slot()))
    for k in ("camera_samples",) + RAY_KINDS:
        assert getattr(sts[0], k) + getattr(sts[1], k) == getattr(st, k), k
    assert r1 <= 1.0 and r2 <= 1.0, (r1, r2)


@gpu
def test_too_wide_a_filter_is_refused_and_the_context_lives(ctx, scene_dir):
    from bling_amd.render import BlingError
    with pytest.raises(BlingError) as e:
        ctx.upload(_job(sc.REFUSED, scene_dir))
    assert "filter wider than the LDS film tile supports" in str(e.value)
    _assert_film(ctx, sc.FILTER_CASES[0], scene_dir)
