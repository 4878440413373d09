"""The scenes of tests/adjoint_scenes.py on the CPU, and the oracle's adjoint BxDF sampling against the
reference.

a. Every case reaches its code.  The restatements count what their light paths meet
   (tests/ref/coverage.h); at the sizes of tests/test_gpu_adjoint_scenes.py -- 512 parity samples, 4096
   photons, the Metropolis line -- each counter a case is about is at least FLOOR = 64.  The SPPM photon
   walk is inside the oracle: there the pass must change when the subject's material is swapped for the
   room's matte, and must pair more than 100 photons with hit points.

b. bxdfSample with adj = False (oracle_bxdf_probe) and adj = True (oracle_bxdf_sample_adj_probe)
   against numpy binary32 restatements written from the Haskell, bit for bit, in the manner of
   tests/test_kat_hotpath.py (whose helpers these use): cosSample (Diffuse.hs:14-22, :38-49) alone and
   through brdfToBtdf (Reflection.hs:188-195); mkMicrofacet's s (Microfacet.hs:42-54) with frConductor;
   mkFresnelBlend's s and p (Microfacet.hs:86-107) with the anisotropic sampling (:151-173); specRefl
   and sampleSpecTrans (Specular.hs:11-57).
"""
import numpy as np
import pytest

import adjoint_scenes as A
import oracle_py
import test_kat_hotpath as K
from bd_ref import BidirRef, parity_samples
from lt_ref import LightRef
from mlt_ref import MltRef
from oracle_py import OracleSppm
from scene_desc import arr, desc
from test_oracle_kat import aniso_d, fr_conductor

f32 = np.float32
ONE, ZERO, TWO, PI = K.ONE, K.ZERO, K.TWO, K.PI
SEED = 0x0B11A6
FT_PROCTEX = 1 << 18                       # common/scene_features.h


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("adjoint_scenes")


# ---------------------------------------------------------------- a. the cases reach their code
def _floor(case, renderer, cov):
    got = {k: cov[k] for k in A.TARGET[case]}
    print(case, renderer, got, {k: v for k, v in cov.items() if v})
    assert all(v >= A.FLOOR for v in got.values()), (case, renderer, got)


@pytest.mark.parametrize("case", A.served("bidir"))
def test_bidir_light_subpaths_reach_the_case(case, scene_dir):
    job = A.build(scene_dir, case, "bidir")
    ref = BidirRef(job)
    L, _, lens, _ = ref.sample_li(parity_samples(job, 512), SEED, 1)
    _floor(case, "bidir", ref.coverage)
    assert (lens[:, 1] > 0).sum() > 64 and (np.abs(L).sum(1) > 0).sum() > 64


@pytest.mark.parametrize("case", A.served("light"))
def test_light_tracer_photons_reach_the_case(case, scene_dir):
    job = A.build(scene_dir, case, "light")
    assert job.light.pass_photons == 4096 and not job.counts()["features"] & FT_PROCTEX
    ref = LightRef(job)
    rec, _, _ = ref.run(SEED, 1)
    _floor(case, "light", ref.coverage)
    assert len(rec) > 100


@pytest.mark.parametrize("case", A.served("light"))
def test_light_tracer_image_is_summable_in_binary32(case, scene_dir):
    """The premise of the device test's summation-order bar: the restatement's own image, a sequential
    binary32 sum in photon order, is within half of ORDER_BAR of the float64 sum of its records, so two
    binary32 sums in different orders have room to agree within the bar."""
    from test_gpu_light_tracer import ORDER_BAR
    job = A.build(scene_dir, case, "light")
    rec, splat, _ = LightRef(job).run(SEED, 1)
    acc = np.zeros(job.width * job.height * 3, np.float64)
    idx = 3 * (rec["sy"].astype(np.int64) * job.width + rec["sx"])
    for c, k in enumerate("xyz"):
        np.add.at(acc, idx + c, rec[k].astype(np.float64))
    err = float(np.linalg.norm(splat - acc) / np.linalg.norm(acc))
    print(case, "sequential binary32 image against the float64 sum", err)
    assert err <= ORDER_BAR / 2


@pytest.mark.parametrize("case", A.served("metropolis"))
def test_metropolis_light_subpaths_reach_the_case(case, scene_dir):
    job = A.build(scene_dir, case, "metropolis")
    ref = MltRef(job)
    ref.run(SEED, 1)
    _floor(case, "metropolis", ref.coverage)


@pytest.mark.parametrize("case", A.served("sppm"))
def test_sppm_pass_depends_on_the_case(case, scene_dir):
    job = A.build(scene_dir, case, "sppm")
    assert not job.counts()["features"] & FT_PROCTEX
    _, splat, st = OracleSppm(job).render_pass(seed=SEED, pass_index=1)
    assert st.photon_hits > 100
    if case == "envimage":                               # no subject: the image map is the only light there is
        assert desc(job).num_lights == 1
        return
    twin = A.build_matte_twin(scene_dir, case, "sppm")
    _, splat2, st2 = OracleSppm(twin).render_pass(seed=SEED, pass_index=1)
    assert st2.photon_hits > 100 and not np.array_equal(splat, splat2)


def test_envimage_has_one_light_and_it_is_the_image_map(scene_dir):
    ref = LightRef(A.build(scene_dir, "envimage", "light"))
    ref.run(SEED, 1)
    c = ref.coverage
    assert desc(ref.job).num_lights == 1 and c["env_rays"] > 4000 and c["verts"] >= A.FLOOR


# ---------------------------------------------------------------- b. bxdfSample, both adj values
def _probe(orc, mi, comp, wo, u, adj):
    """(f, wi, pdf) of bxdfSample adj wo u of component comp."""
    u = np.array(u, np.float32)
    if adj:
        out = np.zeros(20, np.float32)
        oracle_py.lib().oracle_bxdf_sample_adj_probe(orc.h, mi, comp, K.fp(wo), K.fp(wo), K.fp(u), K.fp(out))
        return out[:16], out[16:19], out[19]
    _, out = K.probe_bxdf(orc, mi, comp, wo, wo, u)
    return out[17:33], out[33:36], out[36]


def _sc(s, x):
    return (s * f32(x)).astype(np.float32)


def _dirs(rng, n, special):
    """n unit directions in both hemispheres, the hand-placed ones first."""
    ws = list(special) + [K.normalize(rng.normal(size=3).astype(np.float32)) for _ in range(n - len(special))]
    return ws


def _other(w):
    return K.V(w[0], w[1], -w[2])


def cos_sample(r, oren_sigma, adj, wo, u):
    """cosSample r (Diffuse.hs:14-22), or mkOrenNayar's s (:38-49) when oren_sigma is given."""
    wi = K.to_same_hemi(wo, K.cosine_hemisphere(u[0], u[1]))
    if not K.same_hemi(wo, wi):
        return np.zeros(16, np.float32), (wo if oren_sigma is None else wi), ZERO
    f = r if oren_sigma is None else K.oren_nayar(r, oren_sigma, wo, wi)
    if adj:
        f = _sc(f, abs(f32(wo[2] / wi[2])))
    return f, wi, K.cos_pdf(wo, wi)


@pytest.mark.parametrize("case,sigma", [("transmatte-lambert", None), ("transmatte-oren", 0.4)])
@pytest.mark.parametrize("adj", [False, True])
def test_cos_sample_and_its_btdf(case, sigma, adj, scene_dir):
    job = A.build(scene_dir, case, "bidir")
    d = desc(job)
    mi = [i for i in range(d.num_materials) if d.materials[i].kind == oracle_py_kind("transmatte")][0]
    m = d.materials[mi]
    orc = oracle_py.Oracle(job)
    rng = np.random.default_rng(41)
    wos = _dirs(rng, 80, [K.V(0, 0, 1), K.V(0, 0, -1), K.normalize(K.V(1, 0, 1e-3)), K.normalize(K.V(0, 1, -1e-3)),
                          K.V(1, 0, 0)])                # normal incidence both ways, grazing both ways, in the plane
    us = [(0.5, 0.5), (0.0, 0.0), (1.0, 0.5)] + [tuple(rng.uniform(0, 1, 2)) for _ in range(77)]   # disk centre and rim
    nz = 0
    for comp in (0, 1):                                  # the BRDF, and the same through brdfToBtdf
        r = arr(d.textures[m.tex[comp]].value)
        for wo, u in zip(wos, us):
            u = np.array(u, np.float32)
            f, wi, pdf = cos_sample(r, sigma, adj, wo, u)
            if comp == 1:
                wi = _other(wi)
            gf, gwi, gpdf = _probe(orc, mi, comp, wo, u, adj)
            np.testing.assert_array_equal(gwi, wi, err_msg=f"wi {comp} {wo} {u}")
            np.testing.assert_array_equal(gf, f, err_msg=f"f {comp} {wo} {u}")
            assert gpdf == pdf
            nz += int(f.any())
    assert nz > 128 and (np.array(wos)[:, 2] < 0).sum() > 20


MAT_KIND = {}


def oracle_py_kind(name):
    """bling_material kinds (include/bling_scene.h), read once from the header."""
    if not MAT_KIND:
        import os
        import re
        text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bling_scene.h")).read()
        for nm, v in re.findall(r"BLING_MAT_([A-Z]+)\s*=\s*(\d+)", text):
            MAT_KIND[nm.lower()] = int(v)
    return MAT_KIND[name]


def fix_exponent(e):
    return f32(10000) if (e > 10000 or np.isnan(e)) else e


def microfacet_sample(r, e, fr, adj, wo, u):
    """mkMicrofacet (Blinn e) fr r's s adj wo u (Microfacet.hs:42-54)."""
    whs, dd, pp = K.blinn_sample(e, u[0], u[1])
    wh = -whs if whs[2] < 0 else whs
    wi = (_sc(wh, f32(TWO * K.dot(wo, wh))) - wo).astype(np.float32)
    cos_h = K.dot(wo, wh)
    if not K.same_hemi(wo, wi):
        return np.zeros(16, np.float32), wo, ZERO
    fact = f32(f32(f32(dd * abs(cos_h)) / pp) * K.mf_g(wo, wi, wh))
    fp = (r * fr(cos_h)).astype(np.float32)
    f = _sc(fp, f32(fact / abs(wo[2]))) if adj else _sc(fp, f32(fact / abs(wi[2])))
    return f, wi, f32(pp / f32(f32(4) * abs(cos_h)))


@pytest.mark.parametrize("adj", [False, True])
def test_conductor_microfacet_sample(adj, scene_dir):
    """`metal`: mkMicrofacet (mkBlinn (1 / rough)) (frConductor eta k) white."""
    job = A.build(scene_dir, "metal", "bidir")
    d = desc(job)
    mi = [i for i in range(d.num_materials) if d.materials[i].kind == oracle_py_kind("metal")][0]
    m = d.materials[mi]
    eta, k = arr(d.textures[m.tex[0]].value), arr(d.textures[m.tex[1]].value)
    e = fix_exponent(f32(ONE / f32(m.scalar[0])))
    white = np.ones(16, np.float32)
    orc = oracle_py.Oracle(job)
    rng = np.random.default_rng(43)
    wos = _dirs(rng, 96, [K.V(0, 0, 1), K.normalize(K.V(1, 0, 1e-3)), K.normalize(K.V(0.3, 0.4, -0.8))])
    us = [tuple(rng.uniform(0, 1, 2)) for _ in range(96)]
    for j in range(48):                                  # near-mirror: cos theta_h = u1 ** (1 / (e + 1)) close to 1
        us[j] = (float(1 - rng.uniform(0, 1e-3)), us[j][1])
    nz = 0
    for wo, u in zip(wos, us):
        u = np.array(u, np.float32)
        f, wi, pdf = microfacet_sample(white, e, lambda c: fr_conductor(eta, k, c), adj, wo, u)
        gf, gwi, gpdf = _probe(orc, mi, 0, wo, u, adj)
        np.testing.assert_array_equal(gwi, wi)
        np.testing.assert_array_equal(gf, f)
        assert gpdf == pdf
        nz += int(f.any())
    assert nz >= 64


def spec_trans(t, ei_, et_, adj, wo):
    """sampleSpecTrans adj t ei' et' wo (Specular.hs:33-57)."""
    entering = wo[2] > 0
    ei, et = (f32(ei_), f32(et_)) if entering else (f32(et_), f32(ei_))
    sini2 = K.ghc_max(ZERO, f32(ONE - f32(wo[2] * wo[2])))          # sinTheta2
    eta = f32(ei / et)
    eta2 = f32(eta * eta)
    sint2 = f32(eta2 * sini2)
    if sint2 >= 1:
        return np.zeros(16, np.float32), wo, ZERO
    c = K.sqrtf(K.ghc_max(ZERO, f32(ONE - sint2)))
    cost = -c if entering else c
    wi = K.V(f32(eta * -wo[0]), f32(eta * -wo[1]), cost)
    fr = K.fr_dielectric(ei, et, wo[2] if adj else cost)
    fp = (f32(ONE - fr) * t).astype(np.float32)
    f = _sc(fp, abs(f32(wo[2] / cost))) if adj else _sc(fp, eta2)
    return f, wi, ONE


@pytest.mark.parametrize("adj", [False, True])
def test_specular_reflection_and_transmission(adj, scene_dir):
    """`glass` (envimage's sphere): specRefl (frDielectric 1 ior) kr and specTrans kt 1 ior; shinyMetal's
    second lobe: specRefl (frConductor ..) white."""
    job = A.build(scene_dir, "envimage", "bidir")
    d = desc(job)
    mi = [i for i in range(d.num_materials) if d.materials[i].kind == oracle_py_kind("glass")][0]
    m = d.materials[mi]
    ior = f32(m.scalar[0])
    kr = np.clip(arr(d.textures[m.tex[0]].value), 0, 1).astype(np.float32)
    kt = np.clip(arr(d.textures[m.tex[1]].value), 0, 1).astype(np.float32)
    orc = oracle_py.Oracle(job)
    rng = np.random.default_rng(47)
    crit = np.arcsin(1 / 1.5)
    wos = _dirs(rng, 80, [K.V(0, 0, 1), K.V(0, 0, -1),
                          K.V(np.sin(crit + 0.05), 0, -np.cos(crit + 0.05)),      # leaving, past the critical angle
                          K.V(np.sin(crit - 0.05), 0, -np.cos(crit - 0.05)),      # leaving, just inside it
                          K.normalize(K.V(1, 0, 1e-3)), K.normalize(K.V(0, 1, -1e-3))])   # grazing, both sides
    tir = leave = 0
    for wo in wos:
        u = rng.uniform(0, 1, 2).astype(np.float32)
        gf, gwi, gpdf = _probe(orc, mi, 0, wo, u, adj)                  # specRefl: adj is not read
        np.testing.assert_array_equal(gwi, K.V(-wo[0], -wo[1], wo[2]))
        np.testing.assert_array_equal(gf, (kr * K.fr_dielectric(1, ior, wo[2])).astype(np.float32))
        assert gpdf == 1
        f, wi, pdf = spec_trans(kt, 1, ior, adj, wo)
        gf, gwi, gpdf = _probe(orc, mi, 1, wo, u, adj)
        np.testing.assert_array_equal(gwi, wi)
        np.testing.assert_array_equal(gf, f)
        assert gpdf == pdf
        tir += int(pdf == 0)
        leave += int(wo[2] < 0 and pdf == 1)
    assert tir >= 5 and leave >= 5
    # shinyMetal: the conductor mirror
    job = A.build(scene_dir, "shinymetal", "bidir")
    d = desc(job)
    mi = [i for i in range(d.num_materials) if d.materials[i].kind == oracle_py_kind("shinymetal")][0]
    m = d.materials[mi]
    eta, k = arr(d.textures[m.tex[2]].value), arr(d.textures[m.tex[3]].value)
    orc = oracle_py.Oracle(job)
    for wo in wos[:64]:
        gf, gwi, gpdf = _probe(orc, mi, 1, wo, (0.5, 0.5), adj)
        np.testing.assert_array_equal(gwi, K.V(-wo[0], -wo[1], wo[2]))
        np.testing.assert_array_equal(gf, fr_conductor(eta, k, wo[2]))
        assert gpdf == 1


# ---- mkFresnelBlend (Microfacet.hs:56-107) over the anisotropic distribution (:139-173)
def aniso_pdf(ex, ey, wh):
    costh = abs(wh[2])
    e = f32(f32(f32(f32(ex * wh[0]) * wh[0]) + f32(f32(ey * wh[1]) * wh[1])) / K.ghc_max(ZERO, f32(ONE - f32(costh * costh))))
    return f32(f32(K.sqrtf(f32(f32(ex + ONE) * f32(ey + ONE))) * K.INV_TWO_PI) * K.powf(costh, e))


def aniso_sample(ex, ey, u1, u2):
    """mfDistSample (Anisotropic ex ey) (u1, u2) -> (wh, pdf)."""
    def quadrant(u1p):
        if ex == ey:
            p = f32(f32(PI * u1p) * f32(0.5))
        else:
            p = f32(np.float32(np.arctan(np.float64(f32(K.sqrtf(f32(f32(ex + ONE) / f32(ey + ONE))) *
                                                       K.tanf(f32(f32(PI * u1p) * f32(0.5))))))))
        cp, sp = K.cosf(p), K.sinf(p)
        c = K.powf(u2, f32(ONE / f32(f32(f32(f32(ex * cp) * cp) + f32(f32(ey * sp) * sp)) + ONE)))
        return p, c
    if u1 < f32(0.25):
        p, cost = quadrant(f32(f32(4) * u1))
        phi = p
    elif u1 < f32(0.5):
        p, cost = quadrant(f32(f32(4) * f32(f32(0.5) - u1)))
        phi = f32(PI - p)
    elif u1 < f32(0.75):
        p, cost = quadrant(f32(f32(4) * f32(u1 - f32(0.5))))
        phi = f32(p + PI)
    else:
        p, cost = quadrant(f32(f32(4) * f32(ONE - u1)))
        phi = f32(f32(TWO * PI) - p)
    sint = K.sqrtf(K.ghc_max(ZERO, f32(ONE - f32(cost * cost))))
    wh = K.V(f32(sint * K.cosf(phi)), f32(sint * K.sinf(phi)), cost)
    ds = f32(ONE - f32(cost * cost))
    e = f32(f32(f32(f32(ex * wh[0]) * wh[0]) + f32(f32(ey * wh[1]) * wh[1])) / ds)
    fv = f32(K.INV_TWO_PI * K.powf(cost, e))
    return wh, f32(K.sqrtf(f32(f32(ex + ONE) * f32(ey + ONE))) * fv)


def fblend_half(wo, wi):
    wh = K.normalize((wi + wo).astype(np.float32))
    return -wh if wh[2] < 0 else wh


def fblend_e(rd, rs, ra, ex, ey, depth, wo, wi):
    """mkFresnelBlend's e wo wi (Microfacet.hs:65-86)."""
    costi, costo = abs(wi[2]), abs(wo[2])
    if depth > 0 and costi * costo != 0:
        x = f32(f32(f32(-depth) * f32(costi + costo)) / f32(costi * costo))
        a = np.array([K.expf(v) for v in _sc(ra, x)], np.float32)
    else:
        a = np.ones(16, np.float32)
    p5 = lambda v: K.powf(v, f32(5))  # noqa: E731
    wd = f32(f32(f32(f32(f32(costo * f32(28)) / f32(23)) * PI) * f32(ONE - p5(f32(ONE - f32(f32(0.5) * costi))))) *
             f32(ONE - p5(f32(ONE - f32(f32(0.5) * costo)))))
    diff = _sc(((a * rd).astype(np.float32) * (ONE - rs).astype(np.float32)).astype(np.float32), wd)
    wh = fblend_half(wo, wi)
    costih = abs(K.dot(wi, wh))
    ws = f32(f32(aniso_d(ex, ey, wh) * costo) / f32(f32(f32(4) * costih) * K.ghc_max(costi, costo)))
    schlick = (rs + _sc((ONE - rs).astype(np.float32), p5(f32(ONE - costih)))).astype(np.float32)
    return (diff + _sc(schlick, ws)).astype(np.float32)


def fblend_sample(rd, rs, ra, ex, ey, depth, adj, wo, u):
    u1, u2 = f32(u[0]), f32(u[1])
    if u1 < f32(0.5):
        wi = K.to_same_hemi(wo, K.cosine_hemisphere(f32(u1 * TWO), u2))
        wh = fblend_half(wo, wi)
        pp = aniso_pdf(ex, ey, wh)
    else:
        wh, pp = aniso_sample(ex, ey, f32(TWO * f32(u1 - f32(0.5))), u2)
        wi = (_sc(wh, f32(TWO * K.dot(wo, wh))) - wo).astype(np.float32)
    if pp == 0:
        return np.zeros(16, np.float32), wi, ZERO
    pdf = f32(f32(0.5) * f32(f32(abs(wi[2]) * K.INV_PI) + f32(pp / f32(f32(4) * abs(K.dot(wo, wh))))))
    e = fblend_e(rd, rs, ra, ex, ey, depth, wi, wo) if adj else fblend_e(rd, rs, ra, ex, ey, depth, wo, wi)
    return _sc(e, f32(ONE / pdf)), wi, pdf


def fblend_pdf(ex, ey, wo, wi):
    if not K.same_hemi(wo, wi):
        return ZERO
    wh = fblend_half(wo, wi)
    return f32(f32(0.5) * f32(f32(abs(wi[2]) * K.INV_PI) + f32(aniso_pdf(ex, ey, wh) / f32(f32(4) * abs(K.dot(wo, wh))))))


@pytest.mark.parametrize("case", ["substrate-iso", "substrate-aniso"])
@pytest.mark.parametrize("adj", [False, True])
def test_fresnel_blend_sample_and_pdf(case, adj, scene_dir):
    job = A.build(scene_dir, case, "bidir")
    d = desc(job)
    mi = [i for i in range(d.num_materials) if d.materials[i].kind == oracle_py_kind("substrate")][0]
    m = d.materials[mi]
    rd, rs, ra = (arr(d.textures[m.tex[j]].value) for j in range(3))
    ex, ey, depth = f32(m.scalar[0]), f32(m.scalar[1]), f32(m.scalar[2])
    assert (ex == ey) == (case == "substrate-iso") and (depth > 0) == (case == "substrate-aniso")
    orc = oracle_py.Oracle(job)
    rng = np.random.default_rng(53)
    wos = _dirs(rng, 96, [K.V(0, 0, 1), K.normalize(K.V(1, 0, 0.05)), K.normalize(K.V(0.3, 0.4, -0.8))])
    us = [(0.5, 0.3), (0.0, 0.5), (0.25, 0.7), (0.75, 0.7), (0.49999997, 0.2), (0.625, 0.9), (0.875, 0.9)]
    us += [tuple(rng.uniform(0, 1, 2)) for _ in range(96 - len(us))]
    halves = [0, 0]
    nz = 0
    for wo, u in zip(wos, us):
        u = np.array(u, np.float32)
        f, wi, pdf = fblend_sample(rd, rs, ra, ex, ey, depth, adj, wo, u)
        gf, gwi, gpdf = _probe(orc, mi, 0, wo, u, adj)
        np.testing.assert_array_equal(gwi, wi, err_msg=f"wi {wo} {u}")
        assert gpdf == pdf, (wo, u)
        np.testing.assert_array_equal(gf, f, err_msg=f"f {wo} {u}")
        halves[int(u[0] >= 0.5)] += 1
        nz += int(f.any())
        if not adj:                                      # bxdfPdf wo wi of the sampled pair and of a random one
            wq = K.normalize(rng.normal(size=3).astype(np.float32))
            for w in (wi, wq):
                _, out = K.probe_bxdf(orc, mi, 0, wo, w, u)
                assert out[16] == fblend_pdf(ex, ey, wo, w)
    assert min(halves) >= 32 and nz >= 64
