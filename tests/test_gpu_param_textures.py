"""Textured material parameters on the device (make_bsdf, dev_shade.h; include/bling_scene.h "materials").

The oracle renders constant parameters only, so every comparison hands it a constant scene:

  * identity:    the value c delivered through a non-constant kind that evaluates to exactly c
                 (`scale c 0 tex { perlin }`, a checker of c and c) must give the oracle's radiance of the
                 constant scene bit for bit, at full depth, over every sample of the extent -- through the
                 path, directLighting and bidirectional integrators and the Metropolis renderer, the four
                 sites that keep a BSDF's computed spectra.
  * two-valued:  the value varies between A and B (a 2 x 2 Y8 image, a checker of two constants).  At
                 `path maxDepth 1` a sample's radiance depends on the first hit's BSDF only (Path.hs:51), so
                 each device sample must equal, bit for bit, the oracle's sample of the constant scene of
                 its class; the class comes from the oracle's first-hit point.  That A and B differ on the
                 samples compared is checked without a device in tests/test_param_textures.py.
  * refusal:     the SPPM renderer and the light tracer refuse such scenes, as they do computed textures.
"""
import numpy as np
import pytest

import oracle_py
import param_texture_scenes as pts
from bd_ref import BidirRef
from bling_amd.render import BlingError, Context, render
from bling_amd.scene import parse_job
from parity_util import spectra_mismatch

pytestmark = pytest.mark.gpu
SEED = 0x0B11A6


@pytest.fixture
def device():
    """upload(job) -> a context that is closed after the test: one context alive at a time."""
    made = []

    def upload(job):
        ctx = Context(0)
        made.append(ctx)
        ctx.upload(job)
        return ctx
    yield upload
    for ctx in made:
        ctx.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _pair(tmp_path, case, overrides=None):
    """(the constant job, the identity-textured job) of an identity case."""
    const = parse_job(pts.write_scene(str(tmp_path / "c"), case, pts.material(case, "const")), overrides)
    tex = parse_job(pts.write_scene(str(tmp_path / "t"), case, pts.material(case, "ident")), overrides)
    assert tex.counts()["features"] & (1 << 18) and not const.counts()["features"] & (1 << 18)
    return const, tex


def _report(what, Lg, Lo):
    same = (_bits(Lg) == _bits(Lo)).all(1)
    den = np.abs(Lo).astype(np.float64).sum(1)
    with np.errstate(invalid="ignore"):
        rel = np.abs(Lg.astype(np.float64) - Lo).sum(1) / np.where(den > 0, den, 1.0)
    print(f"{what}: {len(same)} samples, {int(same.sum())} bit-equal, {int((den > 0).sum())} non-black, "
          f"worst relative L1 {float(np.nanmax(rel)):.3e}")
    return same


# ---------------------------------------------------------------- identity
@pytest.mark.parametrize("case", pts.IDENTITY_CASES)
def test_identity_path(case, tmp_path, device):
    const, tex = _pair(tmp_path, case)                     # path maxDepth 5 sampleDepth 3
    s = pts.all_samples(const)
    Lo, _, _ = oracle_py.Oracle(const).sample_li_batch(s, seed=SEED)
    Lg, _, _ = device(tex).sample_li(s, seed=SEED)
    same = _report(case, Lg, Lo)
    assert Lo.any() and same.all(), int((~same).sum())


def test_identity_direct_lighting(tmp_path, device):
    """k_shade_dl sums a specular tree's terms in its own order, so against the oracle the directLighting
    integrator is held to the suite's per-sample bar (relative L1 1e-4, no sample over it:
    tests/test_gpu_parity.py, X4) and is not bit-exact on constant scenes either (measured here: 44 of
    2 704 samples one ulp off, 7.4e-8).  The identity is therefore pinned where it is exact -- the
    textured scene against the constant scene, both on the device, bit for bit -- and the oracle
    comparison keeps the suite's bar."""
    const, tex = _pair(tmp_path, "shinymetal", "direct=3")   # a specular lobe: the tree is walked
    s = pts.all_samples(const)
    Lo, _, _ = oracle_py.Oracle(const).sample_li_batch(s, seed=SEED)
    Lc, _, _ = device(const).sample_li(s, seed=SEED)
    Lg, _, _ = device(tex).sample_li(s, seed=SEED)
    _report("direct, constant on the device vs oracle", Lc, Lo)
    _report("direct, textured on the device vs oracle", Lg, Lo)
    same = _report("direct, textured vs constant on the device", Lg, Lc)
    assert Lo.any() and same.all(), int((~same).sum())
    bad, _, worst, _ = spectra_mismatch(Lg, Lo, 1e-4)
    assert bad == 0, (bad, worst)


def test_identity_bidir(tmp_path, device):
    const, tex = _pair(tmp_path, "transmatte", "bidir=5,3")
    s = pts.all_samples(const)
    L, terms, lens, _ = BidirRef(const).sample_li(s, SEED, 1)
    ctx = device(tex)
    Lg, _, _ = ctx.sample_li(s, seed=SEED, pass_index=1)
    tg, lg = ctx.bidir_terms(s, seed=SEED, pass_index=1)
    same = _report("bidir", Lg, L)
    assert L.any() and same.all(), int((~same).sum())
    assert np.array_equal(lg, lens)
    for k, nm in enumerate(("ld", "le", "l")):
        assert np.array_equal(_bits(tg[:, k]), _bits(terms[:, k])), nm
    assert tg[:, 0].any() and tg[:, 2].any()


def test_identity_metropolis(tmp_path, device):
    const, tex = _pair(tmp_path, "substrate", "metropolis=5,0.25,100,0.25,65")
    rc, sc, bc = device(const).mlt_records(seed=SEED, pass_index=1)
    rt, st_, bt = device(tex).mlt_records(seed=SEED, pass_index=1)
    assert len(rc) == len(rt) > 0
    assert np.array_equal(rt.view(np.uint8), rc.view(np.uint8))            # every record, bit for bit
    assert np.array_equal(st_, sc)
    assert np.float32(bt).view(np.uint32) == np.float32(bc).view(np.uint32) and bc > 0


# ---------------------------------------------------------------- two-valued
@pytest.mark.parametrize("case", pts.TWO_VALUED_CASES)
def test_two_valued(case, tmp_path, device):
    ov = "path=1,1"
    L, p = [], None
    for how in (0, 1):
        mat, _ = pts.two_valued(case, how)
        job = parse_job(pts.write_scene(str(tmp_path / str(how)), case, mat), ov)
        s = pts.all_samples(job)
        Lk, vtx = oracle_py.Oracle(job).sample_li_vertices(s, seed=SEED)
        L.append(Lk)
        p = vtx[:, 0, 7:10] if p is None else p
    mat, img = pts.two_valued(case, "tex")
    job = parse_job(pts.write_scene(str(tmp_path / "t"), case, mat, img), ov)
    Lg, _, _ = device(job).sample_li(s, seed=SEED)
    cls = pts.classify(p, img is not None)
    n_out = int((cls < 0).sum())
    for k in (0, 1):
        m = cls == k
        same = _report(f"{case} class {'AB'[k]}", Lg[m], L[k][m])
        other = (_bits(Lg[m]) == _bits(L[1 - k][m])).all(1)
        print(f"   ... {int(other.sum())} of them also equal the other class's value; {n_out} samples left out")
        assert m.sum() >= 0.1 * len(cls) and same.all(), (case, k, int((~same).sum()))
    assert n_out <= 0.02 * len(cls)


# ---------------------------------------------------------------- refusal
def test_sppm_and_light_tracer_refuse_a_textured_parameter(tmp_path, device):
    mat = dict(pts.SLOTS)["matte.sigma"]
    path = pts.write_scene(str(tmp_path), "refuse", mat)
    ctx = device(parse_job(path, "sppm=2000,3,0.5;sppm_threads=4"))
    with pytest.raises(BlingError) as e:
        ctx.sppm_pass()
    assert e.value.rc == -5                                                # BLING_EUNSUPPORTED
    ctx.upload(parse_job(path, "light=64"))
    with pytest.raises(BlingError) as e:
        ctx.light_pass()
    assert e.value.rc == -5
    ctx.upload(parse_job(path))                                            # the context still renders a path pass
    film, st = ctx.render_pass(seed=SEED, pass_index=0)
    assert np.isfinite(film).all() and film.any() and st.camera_samples == parse_job(path).camera_samples()


# ---------------------------------------------------------------- smoke
def test_smoke_substrate_with_a_checker_kd(tmp_path):
    """One film through the scene entry of render.py: a substrate whose kd is a checker of two constants
    renders finite and differs from the constant-kd film."""
    films = []
    for how in ("tex", 0):
        mat, _ = pts.two_valued("substrate_kd", how)
        films.append(render(parse_job(pts.write_scene(str(tmp_path / str(how)), "smoke", mat)), passes=1, seed=SEED))
    assert np.isfinite(films[0]).all() and films[0].any()
    assert not np.array_equal(films[0], films[1])
