"""Scaled, mirrored and partial analytic shapes on the CPU: the binary32 oracle against the float64
restatement of the Haskell (tests/shape_ref.py), on the generated scenes of
tests/xform_shape_scenes.py.

Every shape the suite rendered before sat under a rigid transform, where the inverse transpose
equals the forward matrix, the object-space direction has length 1 and areas, distances and
epsilons mean the same in object and world space.  The oracle was written beside the device code
and checked on those scenes only, so here it is the thing measured, not the reference.

Per case: rays whose smallest float64 decision margin is below 1e-4 (shape_ref.NEAR) are near a
boundary and left out; they may be at most 2 % of the case's rays (measured: at most 0.012).  On all
other rays hit / miss, the primitive and the any-hit boolean agree exactly, and t, the normal, the hit point, the light
sample's wi / pdf / shadow-ray bounds agree within BARS: twice the oracle's worst error against
float64 as measured by this test (x86-64, the values in MEASURED), per transform case.

The mutation tests run the same comparison against five deliberately misread restatements; each
fails on its named case and passes on `rigid`, which is what the suite covered before.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import shape_ref as R  # noqa: E402
import xform_shape_scenes as X  # noqa: E402
from oracle_py import Oracle, lib  # noqa: E402
from parity_util import random_samples, report  # noqa: E402
from scene_desc import desc  # noqa: E402

SEED = 0x0B11A6
MISS = 0xFFFFFFFF
NEAR_SHARE = 0.02
SHORT = 0.05
orc_f32p = C.POINTER(C.c_float)

# the oracle's worst error against float64 per transform case, as this test measures it: relative
# error of t (closest hits), the hit point relative to its distance from the camera, the angle
# between the normals [rad], and of the lamp cases relative pdf, angle of wi, relative shadow tmax
# (t_short: rays whose hit lies within SHORT of the scene's size of their origin, where t is formed by
# cancellation; the worst of the rest graze a sphere or a cylinder).
# tiny / huge / id have trace cases only.
MEASURED = {
    "rigid": dict(t=1.6e-4, t_short=3.2e-3, p=3.2e-6, n=5.5e-5),
    "uni": dict(t=5.7e-4, t_short=1.7e-2, p=2.9e-6, n=1.2e-5),
    "aniso": dict(t=2.0e-4, t_short=1.0e-2, p=5.9e-6, n=1.6e-4),
    "mirror": dict(t=1.6e-4, t_short=1.3e-3, p=3.4e-6, n=5.5e-5),
    "tiny": dict(t=1.8e-4, t_short=8.0e-3),
    "huge": dict(t=2.1e-4, t_short=1.7e-2),
    "id": dict(t=4.2e-5, t_short=5.7e-4),
}
# lamp cases: relative pdf of Light.sample and of Light.pdf, angle / length of wi, relative shadow tmax, and of
# Light.sample' the origin (relative to its distance), the normal's / direction's angle and the relative pdf
LAMP_MEASURED = {
    "aniso": dict(pdf=9.9e-4, pdf_probe=1.7e-2, tmax=1.5e-5, wi=1.3e-5, emit_o=1.1e-7, emit_n=2.1e-6, emit_pdf=1.2e-4),
    "uni": dict(pdf=4.8e-5, pdf_probe=3.4e-6, tmax=4.6e-6, wi=5.2e-6, emit_o=1.6e-7, emit_n=1.4e-6, emit_pdf=2.5e-5),
    "rigid": dict(pdf=7.5e-5, pdf_probe=2.0e-5, tmax=1.3e-5, wi=5.1e-6, emit_o=7.1e-8, emit_n=1.4e-6, emit_pdf=2.6e-5),
}


def _bar(measured):
    return 2.0 * measured


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("xform_shape_scenes")


def _prim_map(job):
    """Oracle primitive id -> index in the scene file's order (the loader lists primitives in its own order)."""
    d = desc(job)
    assert all(d.prim_kind[k] == 1 for k in range(d.num_prims))
    return np.array([d.prim_index[k] for k in range(d.num_prims)])


def _split(rays):
    r = rays.astype(np.float64)
    return r[0:3].T, r[3:6].T, r[6], r[7]


def _angle(a, b):
    c = np.linalg.norm(np.cross(a, b), axis=-1)
    return np.arctan2(c, R.dot(a, b))


def trace_metrics(scene_dir, case, mutation=None):
    """The oracle's bling_trace equivalents against the restatement on the case's rays."""
    job, prims = X.build(scene_dir, case)
    orc = Oracle(job)
    rays, fam = X.rays(case, prims, np.random.default_rng(3))
    o, d, tmin, tmax = _split(rays)
    ref = R.Ref(prims, mutation)
    pid, t, _, _, marg = ref.closest(o, d, tmin, tmax)
    occ, marg_any = ref.occluded(o, d, tmin, tmax)
    t_o, p_o, _, _ = orc.trace(rays)
    _, a_o, _, _ = orc.trace(rays, any_hit=True)
    pmap = _prim_map(job)
    p_o = np.where(p_o == MISS, -1, pmap[np.minimum(p_o, len(pmap) - 1).astype(np.int64)])
    far, far_any = marg >= R.NEAR, marg_any >= R.NEAR
    both = far & (p_o == pid) & (pid >= 0)
    with np.errstate(all="ignore"):
        t_err = np.abs(t_o - t) / np.abs(t)
        # a ray that starts within SHORT of the scene's size of the surface it hits (a continuation ray, an
        # origin that happens to lie on the backdrop) has a tiny t, formed by cancellation: its own bar
        short = t * np.linalg.norm(d, axis=1) < SHORT * X.TRANSFORMS[case.xform][1]
    t_rel, t_rel_short = t_err[both & ~short], t_err[both & short]
    hits = {k: int((far[s] & (pid[s] == X.SUBJECT)).sum()) for k, s in fam.items()}
    return dict(rays=rays.shape[1], near=float(1 - far.mean()), near_any=float(1 - far_any.mean()),
                id_mismatch=int((far & (p_o != pid)).sum()), any_mismatch=int((far_any & (a_o.astype(bool) != occ)).sum()),
                t_rel=float(t_rel.max(initial=0.0)), t_rel_short=float(t_rel_short.max(initial=0.0)),
                short=int((both & short).sum()), hits=hits, occluded=int(occ.sum()),
                inside_box_any=int(occ[fam["inside"]].sum()) if case.shape == "box" else -1)


def test_transform_words_compose_first_word_first(scene_dir):
    """The restated `newTransform` matrices (Transform.hs Monoid, forward and inverse composed
    separately) are the loader's, for every transform case, within binary32 rounding of a product of
    four matrices -- and the first word of the block acts on the object first."""
    for x in X.TRANSFORMS:
        job, prims = X.build(scene_dir, X.Case("sphere", x))
        d = desc(job)
        for k, pr in enumerate(prims):
            m = np.array(d.shapes[k].o2w[:], np.float64).reshape(4, 4)
            i = np.array(d.shapes[k].w2o[:], np.float64).reshape(4, 4)
            assert np.abs(m - pr.o2w.m).max() <= 4e-7 * np.abs(m).max(), (x, k)
            assert np.abs(i - pr.w2o.m).max() <= 4e-7 * np.abs(i).max(), (x, k)
            assert np.abs(pr.o2w.m @ pr.w2o.m - np.eye(4)).max() < 1e-9
    t = R.from_spec([("scale", (2.0, 0.5, 1.25)), ("translate", (1.0, 0.0, 0.0))])
    np.testing.assert_allclose(R.trans_point(t, np.array([[1.0, 1.0, 1.0]])), [[3.0, 0.5, 1.25]])   # scaled, then moved


@pytest.mark.parametrize("case", X.TRACE_CASES, ids=str)
def test_oracle_trace_against_the_restatement(scene_dir, case):
    """Closest hit (hit / miss, primitive, t) and any-hit over the case's ~4096 rays."""
    m = trace_metrics(scene_dir, case)
    report(f"xform_trace_cpu[{case}]", **m)
    assert m["near"] <= NEAR_SHARE and m["near_any"] <= NEAR_SHARE
    assert m["id_mismatch"] == 0 and m["any_mismatch"] == 0
    assert m["t_rel"] <= _bar(MEASURED[case.xform]["t"]) and m["t_rel_short"] <= _bar(MEASURED[case.xform]["t_short"])
    assert m["hits"]["bounds"] > 0 and m["hits"]["tmax"] > 0 and m["hits"]["unnorm"] > 0
    if case.shape == "box":
        # a ray that starts inside a box: `intersect` says miss (Shape.hs:90), `intersects` says hit (AABB slabs)
        assert m["hits"]["inside"] == 0 and m["inside_box_any"] == X.N_FAMILY
    if case.shape.startswith("cyl") or case.shape == "sphere":
        assert m["hits"]["inside"] > 0 and m["hits"]["surface"] > 0


def geometry_metrics(scene_dir, case, mutation=None):
    """Depth-0 records of the oracle's path vertices (ray, t, shading point, normal) against the
    restatement's closest hit of the same camera ray."""
    job, prims = X.build(scene_dir, case)
    orc = Oracle(job)
    smp = random_samples(orc, job, 2048, seed=11)
    _, vtx = orc.sample_li_vertices(smp, seed=SEED, pass_index=1)
    v = vtx[:, 0, :].astype(np.float64)
    o, d = v[:, 0:3], v[:, 3:6]
    n = len(o)
    ref = R.Ref(prims, mutation)
    pid, t, p, nrm, marg = ref.closest(o, d, np.zeros(n), np.full(n, np.inf))
    far = marg >= R.NEAR
    hit_o = np.isfinite(v[:, 6])
    both = far & hit_o & (pid >= 0)
    subj = both & (pid == X.SUBJECT)
    with np.errstate(all="ignore"):
        t_rel = np.abs(v[both, 6] - t[both]) / np.abs(t[both])
        p_rel = np.linalg.norm(v[both, 7:10] - p[both], axis=1) / np.linalg.norm(p[both], axis=1)
        # the record holds the normal up to the sign the shading code gives it
        ang = np.minimum(_angle(v[both, 10:13], nrm[both]), _angle(-v[both, 10:13], nrm[both]))
        eps_rel = np.abs(v[both, 13] - 5e-4 * t[both]) / np.abs(5e-4 * t[both])
    # path vertices of every depth on either side of insideSphere (Shape.hs:330-331) of a sphere lamp: the
    # device's bling_sample_li walks the same vertices (its spectra are the oracle's bit for bit)
    ins = out = -1
    if case.role != "geo" and case.shape == "sphere":
        pv = vtx[:, :, 7:10].reshape(-1, 3).astype(np.float64)
        pv = pv[np.isfinite(pv).all(1)]
        inside = R.inside_sphere(prims[X.SUBJECT].shape[1], R.trans_point(prims[X.SUBJECT].w2o, pv))
        ins, out = int(inside.sum()), int((~inside).sum())
    return dict(samples=n, near=float(1 - far.mean()), hit_mismatch=int((far & (hit_o != (pid >= 0))).sum()),
                vertices_inside_sphere=ins, vertices_outside_sphere=out,
                on_subject=int(subj.sum()), t_rel=float(t_rel.max(initial=0)), p_rel=float(p_rel.max(initial=0)),
                n_angle=float(ang.max(initial=0)), eps_rel=float(eps_rel.max(initial=0)))


@pytest.mark.parametrize("case", X.RADIANCE_CASES + X.LAMP_CASES, ids=str)
def test_oracle_hit_geometry_against_the_restatement(scene_dir, case):
    """World-space hit point, normal (the inverse transpose, normalised) and ray epsilon at depth 0."""
    m = geometry_metrics(scene_dir, case)
    report(f"xform_geometry_cpu[{case}]", **m)
    bars = MEASURED[case.xform]
    assert m["near"] <= NEAR_SHARE and m["hit_mismatch"] == 0 and m["on_subject"] > 20
    assert m["t_rel"] <= _bar(bars["t"]) and m["eps_rel"] <= _bar(bars["t"])          # camera rays: none is short
    assert m["p_rel"] <= _bar(bars["p"]) and m["n_angle"] <= _bar(bars["n"])
    if case.role != "geo" and case.shape == "sphere":
        assert m["vertices_inside_sphere"] > 50 and m["vertices_outside_sphere"] > 50     # both branches of shape_pdf


def _light_of(job, shape_index):
    d = desc(job)
    return [i for i in range(d.num_lights) if d.lights[i].shape == shape_index][0]


def lamp_metrics(scene_dir, case, mutation=None):
    """Light.sample and Light.pdf of the subject lamp (the oracle's probes) against the restatement,
    at 2048 points around (for the sphere: also on and inside) the lamp."""
    job, prims = X.build(scene_dir, case)
    orc = Oracle(job)
    li = _light_of(job, X.SUBJECT)
    rng = np.random.default_rng(17)
    pts = X.lamp_points(case, prims, rng)
    n = len(pts)
    u1, u2 = rng.random(n).astype(np.float32), rng.random(n).astype(np.float32)
    eps = np.float32(5e-4) * np.linalg.norm(pts, axis=1).astype(np.float32)
    out = np.zeros((n, 28), np.float32)
    for k in range(n):
        lib().oracle_light_sample_probe(orc.h, li, pts[k].ctypes.data_as(orc_f32p), float(eps[k]), float(u1[k]), float(u2[k]),
                                        out[k].ctypes.data_as(orc_f32p))
    ref = R.Ref(prims, mutation)
    r = ref.light_sample(X.SUBJECT, pts.astype(np.float64), eps.astype(np.float64), u1.astype(np.float64), u2.astype(np.float64))
    far = r["margin"] >= R.NEAR
    o = out.astype(np.float64)
    lit_o = np.abs(o[:, :16]).sum(1) > 0
    zero_o, zero_r = o[:, 19] == 0, r["pdf"] == 0
    pos = far & ~zero_r & ~zero_o
    with np.errstate(all="ignore"):
        pdf_rel = np.abs(o[pos, 19] - r["pdf"][pos]) / r["pdf"][pos]
        wi = _angle(o[far, 16:19] / np.linalg.norm(o[far, 16:19], axis=1, keepdims=True),
                    r["wi"][far] / np.linalg.norm(r["wi"][far], axis=1, keepdims=True))
        wi_len = np.abs(np.linalg.norm(o[far, 16:19], axis=1) - np.linalg.norm(r["wi"][far], axis=1)) / np.linalg.norm(r["wi"][far], axis=1)
        tmax_rel = np.abs(o[far, 27] - r["tmax"][far]) / np.abs(r["tmax"][far])
        tmin_rel = np.abs(o[far, 26] - r["tmin"][far]) / np.abs(r["tmin"][far])
        org = np.linalg.norm(o[far, 20:23] - r["o"][far], axis=1) / np.linalg.norm(r["o"][far], axis=1)
        dirn = np.linalg.norm(o[far, 23:26] - r["wi"][far], axis=1) / np.linalg.norm(r["wi"][far], axis=1)
    # Light.pdf at the sampled directions (unit world vectors towards the sample) from the same points
    wiw = (r["wi"] / np.linalg.norm(r["wi"], axis=1, keepdims=True)).astype(np.float32)
    pd_o = np.array([lib().oracle_light_pdf_probe(orc.h, li, pts[k].ctypes.data_as(orc_f32p), wiw[k].ctypes.data_as(orc_f32p))
                     for k in range(n)], np.float64)
    pd_r, gen, ghit, m2 = ref.light_pdf(X.SUBJECT, pts.astype(np.float64), wiw.astype(np.float64))
    far2 = m2 >= R.NEAR
    pos2 = far2 & (pd_r > 0) & (pd_o > 0)
    with np.errstate(all="ignore"):
        pdfp_rel = np.abs(pd_o[pos2] - pd_r[pos2]) / pd_r[pos2]
    # Light.sample' (Light.hs:174-179): the emission of the light tracer, the bidirectional walk and SPPM
    ue = rng.random((n, 4)).astype(np.float32)
    eo = np.zeros((n, 12), np.float32)
    for k in range(n):
        lib().oracle_light_ray_probe(orc.h, li, float(ue[k, 0]), float(ue[k, 1]), float(ue[k, 2]), float(ue[k, 3]),
                                     eo[k].ctypes.data_as(orc_f32p))
    e_o, e_d, e_n, e_pd = ref.light_emit(X.SUBJECT, *(ue[:, c].astype(np.float64) for c in range(4)))
    eo = eo.astype(np.float64)
    with np.errstate(all="ignore"):
        emit = dict(emit_origin_rel=float((np.linalg.norm(eo[:, 0:3] - e_o, axis=1) / np.linalg.norm(e_o, axis=1)).max()),
                    emit_normal=float(_angle(eo[:, 6:9], e_n).max()), emit_dir=float(_angle(eo[:, 3:6], e_d).max()),
                    emit_pdf_rel=float((np.abs(eo[:, 9] - e_pd) / e_pd)[e_pd > 1e-3 * e_pd.max()].max()),
                    emit_tmin=float(np.abs(eo[:, 10] - np.float32(1e-3)).max()), emit_black=int((eo[:, 11] == 0).sum()))
    return dict(points=n, near=float(1 - far.mean()), near_pdf=float(1 - far2.mean()), **emit,
                lit_mismatch=int((far & (lit_o != r["lit"])).sum()), zero_mismatch=int((far & (zero_o != zero_r)).sum()),
                pdf_zero=int(zero_r.sum()), pdf_positive=int((~zero_r).sum()),
                general=int(r["general"].sum()), cone=int((~r["general"]).sum()),
                pdf_rel=float(pdf_rel.max(initial=0)), wi_angle=float(wi.max(initial=0)), wi_len_rel=float(wi_len.max(initial=0)),
                tmax_rel=float(tmax_rel.max(initial=0)), tmin_rel=float(tmin_rel.max(initial=0)),
                origin_rel=float(org.max(initial=0)), dir_rel=float(dirn.max(initial=0)),
                probe_zero_mismatch=int((far2 & ((pd_o == 0) != (pd_r == 0))).sum()), probe_pdf_rel=float(pdfp_rel.max(initial=0)))


@pytest.mark.parametrize("case", X.LAMP_CASES, ids=str)
def test_oracle_lamp_sample_and_pdf_against_the_restatement(scene_dir, case):
    """wi = transVector l2w wi is NOT a unit vector under a scale (Light.hs:156), the pdf and the shadow
    ray's bounds are object-space quantities (:158-160), and the area is the object-space area."""
    m = lamp_metrics(scene_dir, case)
    report(f"xform_lamp_cpu[{case}]", **m)
    assert m["near"] <= NEAR_SHARE and m["near_pdf"] <= NEAR_SHARE
    assert m["lit_mismatch"] == 0 and m["zero_mismatch"] == 0 and m["probe_zero_mismatch"] == 0
    assert m["pdf_rel"] <= _bar(LAMP_MEASURED[case.xform]["pdf"]) and m["probe_pdf_rel"] <= _bar(LAMP_MEASURED[case.xform]["pdf_probe"])
    assert m["wi_angle"] <= _bar(LAMP_MEASURED[case.xform]["wi"]) and m["wi_len_rel"] <= _bar(LAMP_MEASURED[case.xform]["wi"])
    assert m["dir_rel"] <= _bar(LAMP_MEASURED[case.xform]["wi"]) and m["origin_rel"] <= _bar(LAMP_MEASURED[case.xform]["wi"])
    assert m["tmax_rel"] <= _bar(LAMP_MEASURED[case.xform]["tmax"]) and m["tmin_rel"] == 0
    b = LAMP_MEASURED[case.xform]
    assert m["emit_origin_rel"] <= _bar(b["emit_o"]) and m["emit_normal"] <= _bar(b["emit_n"])
    assert m["emit_dir"] <= _bar(b["emit_n"]) and m["emit_pdf_rel"] <= _bar(b["emit_pdf"])
    assert m["emit_tmin"] == 0 and m["emit_black"] == 0
    if case.shape == "cyl135":
        # sampleShape' samples all of 2 pi (Shape.hs:394-398) while intersect rejects phi > phimax (:124-126):
        # generalPdf is 0 for the samples that land on the missing part, and both outcomes occur
        assert m["pdf_zero"] > 200 and m["pdf_positive"] > 200
    if case.shape == "sphere":
        assert m["general"] > 200 and m["cone"] > 200            # both branches of shapePdf (Shape.hs:338-342)


# ------------------------------------------------------------------ the test has power
def _fails_trace(m, xform):
    return m["id_mismatch"] > 0 or m["any_mismatch"] > 0 or m["t_rel"] > _bar(MEASURED[xform]["t"])


def _fails_geometry(m, xform):
    return m["hit_mismatch"] > 0 or m["n_angle"] > _bar(MEASURED[xform]["n"]) or m["t_rel"] > _bar(MEASURED[xform]["t_short"])


def _fails_lamp(m, xform):
    b = LAMP_MEASURED[xform]
    return (m["zero_mismatch"] > 0 or m["lit_mismatch"] > 0 or m["pdf_rel"] > _bar(b["pdf"])
            or m["wi_angle"] > _bar(b["wi"]) or m["tmax_rel"] > _bar(b["tmax"]) or m["emit_pdf_rel"] > _bar(b["emit_pdf"])
            or m["emit_origin_rel"] > _bar(b["emit_o"]))


MUTANTS = [
    # (mutation, metrics, failing case, passing rigid case, verdict)
    ("normal_forward", geometry_metrics, X.Case("sphere", "aniso"), X.Case("sphere", "rigid"), _fails_geometry),
    ("normalized_dir", trace_metrics, X.Case("sphere", "uni"), X.Case("sphere", "rigid"), _fails_trace),
    ("world_area", lamp_metrics, X.Case("sphere", "uni", "lamp"), X.Case("sphere", "rigid", "lamp"), _fails_lamp),
    ("cyl_sample_phimax", lamp_metrics, X.Case("cyl135", "aniso", "lamp"), None, _fails_lamp),
    ("box_inside_closest", trace_metrics, X.Case("box", "aniso"), None, _fails_trace),
]


@pytest.mark.parametrize("mutation,metrics,bad,good,verdict", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_a_misread_restatement_is_caught(scene_dir, mutation, metrics, bad, good, verdict):
    """Each misreading disagrees with the oracle on its named case; the ones a rigid transform hides
    agree with it on `rigid`, which is why the earlier suite could not have seen such an error.  (The
    last two are misreadings of a parameter and of a ray family the earlier scenes did not hold; the
    true restatement's pass on the same case is the control.)"""
    fails = lambda m: verdict(m, bad.xform)  # noqa: E731
    assert not fails(metrics(scene_dir, bad)), "the true restatement must pass"
    m = metrics(scene_dir, bad, mutation)
    report(f"xform_mutation[{mutation}]", case=str(bad), **{k: v for k, v in m.items() if not isinstance(v, dict)})
    assert fails(m)
    if good is not None:
        assert not verdict(metrics(scene_dir, good, mutation), good.xform)
