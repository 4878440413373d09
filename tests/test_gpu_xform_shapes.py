"""Scaled, mirrored and partial analytic shapes on the device against the oracle, on the generated
scenes of tests/xform_shape_scenes.py (the oracle itself is held against a float64 restatement of the
reference by tests/test_xform_shapes.py, on the CPU).

  * bling_trace, closest and any-hit, for every shape x transform case on the exhaustive, the packet
    and the BVH4 plan (filler triangles; the plan is asserted from scene_info()): no primitive id
    differs, t is bit-equal (or NaN on both sides), no any-hit boolean differs, and every special ray
    family in which the float64 restatement finds hits on the subject has hits on the device;
  * bling_sample_li on 2048 random samples of every radiance and lamp case: no spectrum off by more
    than 1e-4 relative L1, equal ray counts, the bit-exact count reported;
  * the MIS cull on the lamp cases: spectra bit-equal with the cull off and on, 0 < culled <
    rays_mis, ray counts equal to the oracle's (tests/test_gpu_mis_cull.py's pattern);
  * one film per lamp kind under `aniso` within the derived float64 bound of tests/film_ref.py;
  * the three emission paths (Light.sample', Light.hs:174-179) on an `aniso` annulus lamp and an
    `aniso` sphere lamp: the light tracer's records against lt_ref, the bidirectional terms against
    bd_ref (bit-equal, tests/test_gpu_light_tracer.py's and tests/test_gpu_bidir.py's bars), and one
    SPPM pass against the oracle's with the bars of tests/test_sppm.py.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import shape_ref as R  # noqa: E402
import xform_shape_scenes as X  # noqa: E402
from bd_ref import BidirRef, parity_samples  # noqa: E402
from bling_amd import _ffi  # noqa: E402
from film_ref import film_ref, pair_bound, pass_samples, pass_tiles, spectra_to_results, worst_ratio  # noqa: E402
from lt_ref import LightRef  # noqa: E402
from oracle_py import Oracle, OracleSppm  # noqa: E402
from parity_util import random_samples, report, spectra_mismatch  # noqa: E402
from scene_desc import desc  # noqa: E402

SEED = 0x0B11A6
FT_SPHERE, FT_SHAPES2, FT_MULTI_LIGHT = 1 << 9, 1 << 13, 1 << 21      # common/scene_features.h
PLAN = {"exhaustive": lambda si: si["bf_prims"] > 0,
        "packet": lambda si: si["bf_prims"] == 0 and si["pkt_n"] > 0 and si["prims"] > 16,
        "bvh4": lambda si: si["bf_prims"] == 0 and si["pkt_n"] == 0}


@pytest.fixture(scope="module")
def ctx():
    from bling_amd.render import Context
    return Context(0)


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("xform_shape_scenes_gpu")


def _features(job, case):
    f = job.counts()["features"]
    kind = X.SHAPES[case.shape][0]
    assert bool(f & FT_SPHERE) == (kind == "sphere")
    assert bool(f & FT_SHAPES2) == (kind in ("disk", "cylinder", "box"))
    assert bool(f & FT_MULTI_LIGHT) == (case.role == "two")


def _subject(job, shape_index):
    """The subject's primitive id in the loader's order."""
    d = desc(job)
    return [k for k in range(d.num_prims) if d.prim_kind[k] == 1 and d.prim_index[k] == shape_index][0]


@pytest.mark.gpu
@pytest.mark.parametrize("case", X.TRACE_CASES, ids=str)
def test_trace_parity_on_three_plans(ctx, scene_dir, case):
    _, prims = X.build(scene_dir, case)
    rays, fam = X.rays(case, prims, np.random.default_rng(3))
    # where the float64 restatement finds hits on the subject (away from every decision boundary), per family
    r = rays.astype(np.float64)
    pid, _, _, _, marg = R.Ref(prims).closest(r[0:3].T, r[3:6].T, r[6], r[7])
    expect = {k: int(((pid[s] == X.SUBJECT) & (marg[s] >= R.NEAR)).sum()) for k, s in fam.items()}
    variants = [(plan, X.Case(case.shape, case.xform, filler=n)) for plan, n in X.FILLERS.items()]
    variants.insert(1, ("packet", X.Case(case.shape, case.xform, filler=X.PACKET_FILLER, packet=True)))
    for plan, variant in variants:
        job, _ = X.build(scene_dir, variant)
        if not variant.packet:
            _features(job, case)
        ctx.upload(job)
        si = ctx.scene_info()
        assert PLAN[plan](si), (plan, si)
        orc = Oracle(job)
        t_o, p_o, _, _ = orc.trace(rays)
        t_g, p_g, _ = ctx.trace(rays)
        _, a_o, _, _ = orc.trace(rays, any_hit=True)
        _, a_g, _ = ctx.trace(rays, any_hit=True)
        same = p_o == p_g
        t_diff = int((~((t_g[same] == t_o[same]) | (np.isnan(t_g[same]) & np.isnan(t_o[same])))).sum())
        subject = p_g == _subject(job, 0 if variant.packet else X.SUBJECT)
        hits = {k: int(subject[s].sum()) for k, s in fam.items()}
        report(f"xform_trace[{case}/{plan}]", rays=rays.shape[1], prims=si["prims"], pkt_n=si["pkt_n"],
               id_mismatch=int((~same).sum()), t_diff=t_diff, any_mismatch=int((a_o != a_g).sum()), occluded=int(a_o.sum()),
               hits=hits, hits_restated=expect)
        assert (~same).sum() == 0 and t_diff == 0 and (a_o != a_g).sum() == 0
        assert hits["bounds"] > 0 and hits["tmax"] > 0 and hits["unnorm"] > 0
        # an empty family fails where the restatement says hits exist.  The restated scene holds no filler
        # triangles (a few of them hide part of a scaled subject), so the rule is held where the two scenes
        # are the same one; with filler the device's hits are the oracle's, primitive by primitive (above)
        for k in fam:
            assert variant.filler or hits[k] > 0 or expect[k] == 0, (plan, k, hits, expect)
        kind = X.SHAPES[case.shape][0]
        if kind in ("sphere", "cylinder"):
            assert hits["inside"] > 0 and hits["surface"] > 0
        if kind == "box":                        # intersect misses from inside (Shape.hs:90), intersects hits (AABB slabs)
            assert hits["inside"] == 0 and int(a_g[fam["inside"]].sum()) == X.N_FAMILY


@pytest.mark.gpu
@pytest.mark.parametrize("case", X.RADIANCE_CASES + X.LAMP_CASES, ids=str)
def test_sample_parity(ctx, scene_dir, case):
    job, _ = X.build(scene_dir, case)
    _features(job, case)
    ctx.upload(job)
    orc = Oracle(job)
    smp = random_samples(orc, job, 2048, seed=11)
    Lg, img_g, st_g = ctx.sample_li(smp, seed=SEED, pass_index=1)
    Lo, img_o, st_o = orc.sample_li_batch(smp, seed=SEED, pass_index=1)
    bad, exact, worst, _ = spectra_mismatch(Lg, Lo)
    lit = float((np.isfinite(Lo).all(1) & (np.abs(Lo).sum(1) > 0)).mean())
    report(f"xform_samples[{case}]", samples=len(smp), mismatch=bad, exact=exact, worst_rel_ok=worst, non_black=lit,
           rays_gpu=st_g.rays(), rays_oracle=st_o.rays())
    np.testing.assert_array_equal(img_g, img_o)
    assert lit > 0.25
    assert bad == 0
    assert st_g.rays() == st_o.rays()


def _counts(st):
    return (st.camera_samples, st.rays_camera, st.rays_continuation, st.rays_mis, st.rays_shadow)


@pytest.mark.gpu
@pytest.mark.parametrize("case", X.LAMP_CASES, ids=str)
def test_mis_cull_on_scaled_lamps(ctx, scene_dir, case):
    job, _ = X.build(scene_dir, case)
    ctx.upload(job)
    _, st_on = ctx.render_pass(seed=SEED, pass_index=0)
    culled_on = ctx.mis_culled()
    _, st_off = ctx.render_pass(seed=SEED, pass_index=0, flags=_ffi.PASS_NO_MIS_CULL)
    culled_off = ctx.mis_culled()
    orc = Oracle(job)
    _, st_o = orc.render(seed=SEED, pass_index=0)
    oracle = (st_o.samples, st_o.rays_camera, st_o.rays_continuation, st_o.rays_mis, st_o.rays_shadow)
    smp = random_samples(orc, job, 2048, seed=11)
    L_on, img_on, _ = ctx.sample_li(smp, seed=SEED, pass_index=0)
    ctx.set_mis_cull(False)
    try:
        L_off, img_off, _ = ctx.sample_li(smp, seed=SEED, pass_index=0)
    finally:
        ctx.set_mis_cull(True)
    words = int((L_on.view(np.uint32) != L_off.view(np.uint32)).sum())
    report(f"xform_mis_cull[{case}]", culled=culled_on, culled_with_flag=culled_off, counts_on=_counts(st_on),
           counts_off=_counts(st_off), counts_oracle=oracle, sample_words_differ=words)
    assert words == 0 and np.array_equal(img_on, img_off)
    assert _counts(st_on) == _counts(st_off) and culled_off == 0
    assert 0 < culled_on < st_on.rays_mis
    assert _counts(st_on) == oracle


RAY_KINDS = ("rays_camera", "rays_continuation", "rays_mis", "rays_shadow")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", X.KIND_ONCE)
def test_film_of_each_lamp_kind_within_the_derived_bound(ctx, scene_dir, shape):
    """tests/test_gpu_render_shapes.py's film check: the device's film against the float64 film of its own
    per-sample results, and against the oracle's film within the pair bound; equal counts."""
    job, _ = X.build(scene_dir, X.Case(shape, "aniso", "lamp"))
    orc = Oracle(job)
    so = pass_samples(job, 0)
    Lo, img_o, _ = orc.sample_li_batch(so, seed=SEED, pass_index=0)
    Fo, Ao, no = film_ref(spectra_to_results(Lo), img_o, job.filter_table(), job.filter_size, job.width, job.height,
                          pass_tiles(job), job.spp)
    film_o, st_o = orc.render(seed=SEED, pass_index=0)
    ctx.upload(job)
    film, st = ctx.render_pass(seed=SEED, pass_index=0)
    res, waves = ctx.pass_results()
    s = pass_samples(job, ctx.scene_info()["sample_major"])
    assert len(res) == len(s) == st.camera_samples == st_o.samples == job.camera_samples() and st.dropped_samples == 0
    _, img, _ = ctx.sample_li(s, seed=SEED, pass_index=0)
    F, A, n = film_ref(res, img, job.filter_table(), job.filter_size, job.width, job.height, pass_tiles(job), job.spp)
    r_dev = worst_ratio(film, F, A, n)
    d = np.abs(film.astype(np.float64) - film_o.astype(np.float64)).reshape(F.shape)
    r_pair = float((d / pair_bound(A, n)).max())
    report(f"xform_film[{shape}-aniso-lamp]", ratio_device=r_dev, ratio_pair=r_pair, n_max=int(n.max()),
           lit=float((np.abs(film.reshape(-1, 4)[:, 1:]).sum(1) > 0).mean()))
    assert np.isfinite(film).all() and (np.abs(film.reshape(-1, 4)[:, 1:]).sum(1) > 0).mean() > 0.25
    for k in RAY_KINDS:
        assert getattr(st, k) == getattr(st_o, k), k
    assert np.array_equal(n, no)
    assert r_dev <= 1.0 and r_pair <= 1.0


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("case", X.OTHER_RENDERER_CASES, ids=str)
def test_light_tracer_records_from_a_scaled_lamp(ctx, scene_dir, case):
    job, _ = X.build(scene_dir, X.Case(case.shape, case.xform, case.role, renderer="light"))
    ctx.upload(job)
    rrec, _, rst = LightRef(job).run(SEED, 1)
    grec = ctx.light_records(seed=SEED, pass_index=1)
    _, gst = ctx.light_pass(seed=SEED, pass_index=1)
    report(f"xform_light_records[{case}]", records=len(grec), records_ref=len(rrec),
           counts=[gst.photons, gst.photon_rays, gst.shadow_rays, gst.splats, gst.dropped], counts_ref=rst.counts())
    assert len(grec) == len(rrec) > 100
    for k in ("photon", "depth", "sx", "sy"):
        assert np.array_equal(grec[k], rrec[k]), k
    for k in "xyz":
        assert np.array_equal(_bits(grec[k]), _bits(rrec[k])), k
    assert [gst.photons, gst.photon_rays, gst.shadow_rays, gst.splats, gst.dropped] == rst.counts()


@pytest.mark.gpu
@pytest.mark.parametrize("case", X.OTHER_RENDERER_CASES, ids=str)
def test_bidir_terms_from_a_scaled_lamp(ctx, scene_dir, case):
    job, _ = X.build(scene_dir, X.Case(case.shape, case.xform, case.role, renderer="bidir"))
    ctx.upload(job)
    s = parity_samples(job, 512)
    L, terms, lens, rst = BidirRef(job).sample_li(s, SEED, 1)
    Lg, _, gst = ctx.sample_li(s, seed=SEED, pass_index=1)
    tg, lg = ctx.bidir_terms(s, seed=SEED, pass_index=1)
    exact = [int((_bits(tg[:, k]) == _bits(terms[:, k])).all(1).sum()) for k in range(3)]
    report(f"xform_bidir_terms[{case}]", n=len(s), ld_le_l_exact=exact, L_exact=int((_bits(Lg) == _bits(L)).all(1).sum()),
           nonblack=int((np.abs(L).sum(1) > 0).sum()), light_paths=int((lens[:, 1] > 0).sum()))
    assert np.array_equal(lg, lens) and (lens[:, 1] > 0).sum() > 64 and (np.abs(L).sum(1) > 0).sum() > 64
    for k in range(3):
        assert np.array_equal(_bits(tg[:, k]), _bits(terms[:, k])), ("ld", "le", "l")[k]
    assert np.array_equal(_bits(Lg), _bits(L))
    assert [gst.rays_camera, gst.rays_continuation, gst.rays_mis, gst.rays_shadow, gst.path_vertices] == rst.rays()


@pytest.mark.gpu
def test_sppm_pass_from_a_scaled_lamp(ctx, scene_dir):
    """One pass of an `aniso` annulus lamp against the oracle's SPPM pass, tests/test_sppm.py's bars."""
    job, _ = X.build(scene_dir, X.Case("annulus", "aniso", "lamp", renderer="sppm"))
    w, h = job.width, job.height
    fo, so, sto = OracleSppm(job).render_pass(seed=SEED, pass_index=1)
    ctx.upload(job)
    ctx.sppm_reset()
    f, sp, st = ctx.sppm_pass(seed=SEED, pass_index=1)
    f, fo = f.reshape(h, w, 4), fo.reshape(h, w, 4)
    hasw = (fo[..., 0] > 0) & (f[..., 0] > 0)
    l2 = lambda a, b: float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))  # noqa: E731
    film_l2 = l2(f[..., 1:][hasw] / f[..., :1][hasw], fo[..., 1:][hasw] / fo[..., :1][hasw])
    splat_l2 = l2(sp, so)
    report("xform_sppm[annulus-aniso-lamp]", hitpoints=[int(st.hitpoints), int(sto.hitpoints)],
           photon_rays=[int(st.photon_rays), int(sto.photon_rays)], pairs=[int(st.photon_hits), int(sto.photon_hits)],
           film_l2=film_l2, splat_l2=splat_l2)
    assert st.photons == sto.photons and sto.photon_hits > 100
    assert abs(int(st.hitpoints) - int(sto.hitpoints)) <= 0.005 * sto.hitpoints + 1
    assert abs(int(st.cam_rays) - int(sto.cam_rays)) <= 0.005 * sto.cam_rays + 1
    assert abs(int(st.photon_rays) - int(sto.photon_rays)) <= 0.01 * sto.photon_rays + 1
    assert abs(int(st.photon_hits) - int(sto.photon_hits)) <= 0.02 * sto.photon_hits + 1
    assert np.isfinite(f).all() and film_l2 <= 1e-2
    assert np.isfinite(sp).all() and splat_l2 <= 3e-2
