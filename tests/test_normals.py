"""The normal-map integrator `integrator { debug normals }` (mkNormalMap, Integrator/Debug.hs:25-34) on
the host: loader, upload validation and the CPU restatement (tests/ref/normals_ref.cpp) that the device
is pinned against (tests/test_gpu_normals.py)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from bling_amd import _ffi  # noqa: E402
from bling_amd.scene import NORMAL_SCENES, SCENES, load_config, parse_job  # noqa: E402
import nm_ref  # noqa: E402
import scene_desc  # noqa: E402
from oracle_py import Oracle  # noqa: E402

f32 = np.float32
SEED = 0x0B11A6
FIXTURE = os.path.join(SCENES, "normals.bling")


# ---------------------------------------------------------------- loader
def _config(job):
    c = job.config
    return c.renderer, c.integrator, c.max_depth, c.sample_depth


def test_loader_reads_debug_normals():
    job = parse_job(FIXTURE)
    assert _config(job) == (0, 3, 0, 0)
    assert "renderer normals" in job.summary()
    assert (job.width, job.height, job.spp) == (48, 32, 4)        # the blocks after the integrator still parse


@pytest.mark.parametrize("word", ["kdtree", "reference", "foo"])
def test_loader_leaves_the_other_debug_integrators_unserved(tmp_path, word):
    """mkKdVision and mkReference are `undefined` (Debug.hs:23,37); any other word fails the reference's parser."""
    src = open(FIXTURE).read()
    block = "      integrator { debug normals }\n"                    # the renderer block's line, not the header comment's
    assert src.count(block) == 1
    p = tmp_path / f"debug-{word}.bling"
    p.write_text(src.replace(block, "      integrator { debug %s }\n" % word))
    job = parse_job(str(p))
    assert job.config.renderer == 1                               # BLING_RENDERER_OTHER
    assert (job.width, job.height) == (48, 32)


def test_normals_override_replaces_the_integrator():
    plain = load_config("C1", "image=16,16")
    job = load_config("C1", "image=16,16;normals")
    assert _config(job) == (0, 3, 0, 0)
    assert job.counts() == plain.counts()                         # the feature mask stays what it is
    assert (job.config.sampler, job.config.nu, job.config.nv) == (plain.config.sampler, plain.config.nu, plain.config.nv)


def test_normals_override_turns_an_sppm_job_into_a_sampler_job():
    assert load_config("X5", "image=16,16").config.renderer == 2  # as shipped: SPPM
    assert _config(load_config("X5", "image=16,16;normals")) == (0, 3, 0, 0)


def test_every_named_scene_loads_as_a_normals_job():
    for name in NORMAL_SCENES:
        job = load_config(name)
        assert _config(job) == (0, 3, 0, 0), name
        assert job.width <= 64 and job.height <= 64, name


# ---------------------------------------------------------------- validation
def test_validate_accepts_normals_and_refuses_the_next_value():
    hip = _ffi.hip()
    job = load_config("C1", "image=16,16;normals")
    assert hip.bling_scene_validate(C.c_void_p(job.desc)) == 0, hip.bling_last_error().decode()
    scene_desc.desc(job).config.integrator = 4
    assert hip.bling_scene_validate(C.c_void_p(job.desc)) == -1
    assert "unknown surface integrator" in hip.bling_last_error().decode()


# ---------------------------------------------------------------- the restatement's known answers
def _refl_bases():
    text = open(os.path.join(ROOT, "bling_amd", "csrc", "common", "spectral_data.h")).read()
    body = re.search(r"BLING_RGB_REFL_BANDS\[[^=]*=\s*\{(.*?)\};", text, re.S).group(1)
    return np.array([float.fromhex(x.rstrip("f")) for x in re.findall(r"-?0x[0-9a-fA-F.]+p[+-]?\d+f?", body)], f32)


REFL = _refl_bases()


def rgb_to_spectrum(bands, r, g, b):
    """rgbToSpectrum (Spectrum.hs:146-159) in binary32, bases r, g, b, c, m, y, w: three ordered cases,
    sScale of the bases, the sums in the order written."""
    rb, gb, bb, cb, mb, yb, wb = bands.reshape(7, 16)
    r, g, b = f32(r), f32(g), f32(b)

    def ss(base, k):
        return (base * f32(k)).astype(f32)

    def add(a, c):
        return (a + c).astype(f32)
    if r <= g and r <= b:
        return add(ss(wb, r), add(ss(cb, g - r), ss(bb, b - g)) if g <= b else add(ss(cb, b - r), ss(gb, g - b)))
    if g <= r and g <= b:
        return add(ss(wb, g), add(ss(mb, r - g), ss(bb, b - r)) if r <= b else add(ss(mb, b - g), ss(rb, r - b)))
    return add(ss(wb, b), add(ss(yb, r - b), ss(gb, g - r)) if r <= b else add(ss(yb, g - b), ss(rb, r - g)))


def normal_colour(n):
    """intToSpectrum (Debug.hs:31-34): rgbToSpectrumRefl ((vpromote 1 + n) / 2) in binary32."""
    c = ((f32(1) + np.asarray(n, f32)) / f32(2)).astype(f32)
    return rgb_to_spectrum(REFL, c[0], c[1], c[2])


def test_colour_function_covers_its_six_branches():
    """The restatement's rgbToSpectrumRefl against the numpy one, bit for bit, on normals that order
    (r, g, b) in each of the six ways, on ties and on the axes."""
    rng = np.random.default_rng(3)
    ns = [v / np.linalg.norm(v) for v in rng.normal(size=(600, 3))]
    ns += [np.array(v, float) for v in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 0),
                                         (0.5, 0.5, 0.5), (0.5, 0.5, -0.5), (0.5, -0.5, 0.5), (-0.5, 0.5, 0.5))]
    seen = set()
    for n in ns:
        n = np.asarray(n, f32)
        c = (f32(1) + n) / f32(2)
        seen.add(tuple(np.argsort(c, kind="stable")))
        np.testing.assert_array_equal(nm_ref.colour(n), normal_colour(n), err_msg=str(n))
    assert len(seen) == 6


SPHERE = """filter box
imageSize 24 24
renderer { sampler sampled { sampler { random 4 } integrator { debug normals } } }
transform { lookAt { pos 0 0 -4 look 0 0 0 up 0 1 0 } }
camera { perspective fov 40 lensRadius 0 focalDistance 10 }
newTransform { }
light { infinite { rotateX -90 } l { %s } }
material { matte kd { constant rgbR 0.5 0.5 0.5 } sigma { constant 0 } }
prim { shape { sphere radius 1 } }
"""
SKY = "sunSky east 0 0 1 sunDir 0.5 1 1 turbidity 5"


@pytest.mark.parametrize("env", ["constant rgbI 0.8 0.8 0.8", SKY], ids=["const-env", "sun-sky"])
def test_unit_sphere_known_answers(tmp_path, env):
    """An untransformed unit sphere with matte, under an environment light.  For every sample of the
    image, from Oracle.camera_ray and Oracle.trace alone (no BSDF code):

      a miss is exactly zero, whatever the environment;
      a hit's spectrum is, bit for bit, the numpy rgbToSpectrumRefl ((1 + ns) / 2) of the shading normal
          ns the restatement reports, and ns is the geometric normal (no bump, no mesh);
      ns is normalize (p_hit) up to rounding.  It is not that expression: the oracle's sphere normal
          is normalize (cross dpdu dpdv) of the parametric derivatives (Shape.hs:189-229), whose dpdv
          holds sin (acos (z / r)).  acos loses the bits of its argument near +-1, so the normal's error
          grows as 1 / sin theta towards the poles of the object's z axis (here the image centre: the
          camera looks along +z).  Measured over all 910 hits, the same in both scenes: max
          |ns - normalize p| sin theta = 5.06e-7 = 8.5 ulps of 1 (the plain maximum, 1.76e-5, is a sample
          with sin theta = 0.016).  Held to 9 ulps of 1 over sin theta.  The spectrum is linear in the
          colour (1 + n) / 2: three scaled bases of at most 1.07, scaled by one component and by two
          differences of components, so |dL| <= 1.07 (1/2 + 1 + 1) |dn| per sample, plus four roundings.
    """
    p = tmp_path / "sphere.bling"
    p.write_text(SPHERE % env)
    job = parse_job(str(p))
    orc = Oracle(job)
    ref = nm_ref.NormalsRef(job)
    smp = nm_ref.all_samples(job)
    L, img, geo, st = ref.sample_li(smp, SEED)
    rays = np.array([orc.camera_ray(int(x), int(y), int(n), seed=SEED) for x, y, n in smp], f32)
    np.testing.assert_array_equal(img, rays[:, :2])
    soa = np.concatenate([rays[:, 2:8].T, np.zeros((1, len(smp)), f32), np.full((1, len(smp)), np.inf, f32)], 0)
    t, prim, _, _ = orc.trace(np.ascontiguousarray(soa, f32))
    hit = prim != 0xFFFFFFFF
    assert 0.1 * len(smp) < hit.sum() < 0.9 * len(smp)            # both cases are well populated
    np.testing.assert_array_equal(geo[:, 0] != 0, hit)
    assert st.hits == hit.sum() and st.samples == len(smp)
    assert (L[~hit] == 0).all()                                   # black: no environment term
    o, d = rays[:, 2:5], rays[:, 5:8]
    ph = (o + d * t[:, None].astype(f32)).astype(f32)[hit]
    want_n = (ph / np.sqrt((ph * ph).sum(1, dtype=f32), dtype=f32)[:, None]).astype(f32)
    ns, ng = geo[hit, 1:4], geo[hit, 4:7]
    np.testing.assert_array_equal(ns, ng)
    want_L = np.array([normal_colour(n) for n in ns])
    np.testing.assert_array_equal(L[hit], want_L)
    ulp = 2.0 ** -24
    dn = np.abs(ns - want_n).max(1)
    sin_t = np.sqrt(np.maximum(0.0, 1.0 - want_n[:, 2].astype(np.float64) ** 2))
    dL = np.abs(L[hit] - np.array([normal_colour(n) for n in want_n])).max(1)
    print(f"unit sphere [{env[:8]}]: hits {hit.sum()} of {len(smp)}, max |ns - normalize p| {dn.max():.3g}, "
          f"max |ns - normalize p| sin theta {(dn * sin_t).max() / ulp:.2f} ulps, max |dL| {dL.max():.3g}")
    assert (dn * sin_t <= 9 * ulp).all()
    assert (dL <= 1.07 * 2.5 * dn + 4 * ulp).all()


# ---------------------------------------------------------------- shading against geometric normals
@pytest.mark.parametrize("name,over", [("X9", "image=40,24;stratified=2,2;normals"), ("N2", None)], ids=["bump", "fixture"])
def test_scenes_tell_shading_from_geometric_normals(name, over):
    """A condition of the parity tests: on the bump-mapped scene and on the fixture (smooth mesh, bumped
    sphere, mirrored cylinder) at least half of the hit samples have a colour that the geometric normal
    would not give, so a device that shaded with the geometric normal fails them.  Measured: X9 5 216 of
    5 676 hits (0.92), the fixture 4 564 of 4 658 (0.98)."""
    job = load_config(name, over)
    ref = nm_ref.NormalsRef(job)
    L, _, geo, _ = ref.sample_li(nm_ref.all_samples(job), SEED)
    hit = geo[:, 0] != 0
    assert hit.sum() > 1000
    Lg = np.array([nm_ref.colour(n) for n in geo[hit, 4:7]])
    differs = (L[hit] != Lg).any(1)
    print(f"{name}: {differs.sum()} of {hit.sum()} hit samples tell the shading from the geometric normal")
    assert differs.sum() >= 0.5 * hit.sum()


def test_render_adds_what_sample_li_returns():
    """The restatement's film: the W column is the filter weight of every sample (hit or not), and the
    film of two shards is the film of the whole pass up to the order of its tile sums."""
    job = load_config("N2")
    ref = nm_ref.NormalsRef(job)
    film, st = ref.render(SEED)
    assert st.samples == job.camera_samples() and st.dropped == 0 and 0 < st.hits < st.samples
    f = film.reshape(job.height, job.width, 4)
    assert np.isfinite(f).all() and (f[..., 0] > 0).all()
    halves = np.zeros_like(film)
    for r in (0, 1):
        halves, _ = ref.render(SEED, film=halves, shard_rank=r, shard_world=2)
    np.testing.assert_allclose(halves, film, rtol=2e-6, atol=1e-6)
