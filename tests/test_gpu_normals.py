"""The normal-map integrator `integrator { debug normals }` on the device (k_shade_nm, normals.h) against
its CPU restatement (tests/ref/normals_ref.cpp): a direct parity check of the per-hit shading frame.

Per-sample parity is pinned bit for bit on every scene: the hit reconstruction, the bump step and the
fractal normals are the functions the Path kernels are already bit-exact with, and the colour is three
scaled bases summed in the reference's order.  Measured on MI355X: 0 differing samples on every scene
below.  The film differs from the restatement's only in the order of its binary32
sums: C1 and C4 are held to the bars tests/test_gpu_parity.py holds for those scenes' Path films
(C1_48, sC4), the fixture, which has none, to twice the values measured against the restatement
(FIXTURE_L2 / FIXTURE_PIX).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from bling_amd import _ffi
from bling_amd.render import BlingError, Context, render
from bling_amd.scene import NORMAL_SCENES, SCENES, film_to_rgb, load_config, parse_job
import nm_ref
import test_gpu_parity as P
import xform_shape_scenes as X
from parity_util import film_errors, report

pytestmark = pytest.mark.gpu
SEED = 0x0B11A6
# the fixture's films against the restatement's, the largest values measured over this file's comparisons:
# relative L2 1.88e-7 (one pass; the worst pixel of one pass 8.1e-7), worst pixel 1.56e-6 (two passes
# accumulated); the order of the film's atomic adds moves both from run to run
FIXTURE_L2, FIXTURE_PIX = 3.76e-7, 3.12e-6
# tag -> (relative L2, worst pixel) of tests/test_gpu_parity.py, read, not copied
FILM_BARS = {
    "C1": (P.FILM_BARS["C1_48"][1], P.PIXEL_BARS["C1_48"][1]),
    "C4": (P.FILM_BARS["sC4"][1], P.PIXEL_BARS["sC4"][1]),
}
FILM_JOBS = {
    "C1": lambda: load_config("N1"),                                  # cornell-box 48 x 48, the C1_48 film's scene
    "C4": lambda: load_config("C4", "image=24,24;random=4;normals"),  # sun-sky 24 x 24, the sC4 film's scene
    "fixture": lambda: load_config("N2"),
}
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ref(key, make):
    """(job, every sample of its image, the restatement's L / img / geo / stats), computed once."""
    if key not in _cache:
        job = make()
        s = nm_ref.all_samples(job)
        _cache[key] = (job, s) + nm_ref.NormalsRef(job).sample_li(s, SEED)
    return _cache[key]


def _ref_film(tag):
    if ("film", tag) not in _cache:
        job = FILM_JOBS[tag]()
        _cache[("film", tag)] = (job,) + nm_ref.NormalsRef(job).render(SEED)
    return _cache[("film", tag)]


def _waves(ctx):
    """How bling_debug_pass_results says the last pass ran; it reports the waves also where it keeps no
    per-sample results (more than one wave), which Context.pass_results raises on."""
    n, waves = C.c_size_t(), C.c_int()
    _ffi.hip().bling_debug_pass_results(ctx._h, None, 0, C.byref(n), C.byref(waves))
    return int(waves.value)


def _film_bar(tag):
    return FILM_BARS.get(tag, (FIXTURE_L2, FIXTURE_PIX))


@pytest.fixture
def device():
    """upload(job) -> a context that is closed after the test: one context alive at a time."""
    made = []

    def upload(job, devices=0):
        ctx = Context(devices)
        made.append(ctx)
        ctx.upload(job)
        return ctx
    yield upload
    for ctx in made:
        ctx.close()


def _check_samples(tag, ctx, job, s, L, img, geo, rst):
    Lg, img_g, st = ctx.sample_li(s, seed=SEED)
    same = (_bits(Lg) == _bits(L)).all(1)
    hit = geo[:, 0] != 0
    den = np.abs(L).sum(1)
    rel = np.abs(Lg.astype(np.float64) - L).sum(1) / np.maximum(den, 1e-30)
    report(f"normals_samples[{tag}]", samples=len(s), hits=int(hit.sum()), differing=int((~same).sum()),
           worst_rel=float(rel[hit].max(initial=0.0)), miss_nonzero=int((Lg[~hit] != 0).any(1).sum()),
           plan=ctx.scene_info())
    np.testing.assert_array_equal(img_g, img)
    assert (Lg[~hit] == 0).all()                                   # escaped samples: exactly zero
    assert same.all(), (tag, int((~same).sum()), s[~same][:4])
    assert (st.camera_samples, st.rays_camera, st.path_vertices) == (len(s), len(s), rst.hits)
    assert (st.rays_continuation, st.rays_mis, st.rays_shadow, st.dropped_samples) == (0, 0, 0, 0)
    return st


# ---------------------------------------------------------------- 1. per-sample parity
@pytest.mark.parametrize("name", list(NORMAL_SCENES))
def test_every_sample_equals_the_restatement(name, device):
    """N1 cornell (triangles, BVH4 all-LDS), N2 the fixture, N3 analytic shapes, N4 bump, N5 heightMap, N6
    Bezier, N7 the ducky at 48 x 48 (LDS prefix with global fallback), N8 mandelbulb (pre-marched), N9
    Julia, N10 sun-sky (escaped samples are exactly zero), N11 the environment camera.  Measured: no
    differing sample on any of them."""
    job, s, L, img, geo, rst = _ref(name, lambda: load_config(name))
    ctx = device(job)
    _check_samples(name, ctx, job, s, L, img, geo, rst)
    if name == "N1":
        assert ctx.scene_info()["bf_prims"] == 0                  # a tree walk, not the exhaustive kernel
    if name == "N10":
        hit = geo[:, 0] != 0
        assert (~hit).sum() >= 500                                # hundreds of samples escape to the sky (821 of 6 784)


def test_exhaustive_plan(device, monkeypatch):
    """The cornell box once more on the exhaustive closest-hit kernel (BLING_BRUTE raises its limit)."""
    job, s, L, img, geo, rst = _ref("N1", lambda: load_config("N1"))
    monkeypatch.setenv("BLING_BRUTE", "64")
    ctx = device(job)
    monkeypatch.delenv("BLING_BRUTE")
    assert ctx.scene_info()["bf_prims"] > 0
    _check_samples("N1-exhaustive", ctx, job, s, L, img, geo, rst)


XFORM_CASES = [c for c in X.RADIANCE_CASES if c.xform in ("aniso", "mirror")] + [
    X.Case("cyl135", "mirror", filler=X.FILLERS["bvh4"]), X.Case("box", "aniso", filler=X.PACKET_FILLER, packet=True)]


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("normals_xform"))


@pytest.mark.parametrize("case", XFORM_CASES, ids=str)
def test_scaled_and_mirrored_shapes(case, scene_dir, device):
    """The generated scenes of tests/test_gpu_xform_shapes.py (every analytic shape kind under an
    anisotropic scale and under a mirror, 32 x 32), with the override: the normal through a transform
    whose inverse transpose is not its own, on the exhaustive, the BVH4 and the packet plan."""
    def make():
        plain, _ = X.build(scene_dir, case)
        return parse_job(plain.path, "normals")
    job, s, L, img, geo, rst = _ref(("xform", str(case)), make)
    _check_samples(f"xform-{case}", device(job), job, s, L, img, geo, rst)


# ---------------------------------------------------------------- 2. film parity
def _film_check(tag, what, film, ref_film):
    l2, pix = _film_bar(tag)
    e = film_errors(film, ref_film)
    report(f"normals_film[{tag}:{what}]", **e)
    assert np.isfinite(film).all()
    assert e["rel_l2"] <= l2 and e["pix_max"] <= pix, (tag, what, e, l2, pix)
    return e


@pytest.mark.parametrize("tag", list(FILM_JOBS))
def test_film_of_one_pass(tag, device):
    job, ref_film, rst = _ref_film(tag)
    ctx = device(job)
    film, st = ctx.render_pass(seed=SEED, pass_index=0)
    assert (st.camera_samples, st.rays_camera, st.path_vertices) == (rst.samples, rst.samples, rst.hits)
    assert (st.rays_continuation, st.rays_mis, st.rays_shadow, st.dropped_samples) == (0, 0, 0, 0)
    _film_check(tag, "pass", film, ref_film)
    assert ctx.pass_results()[1] == 1                             # one wave, not pipelined


class _DeviceFloats:
    """n zeroed floats on the device, from the HIP runtime the core itself is linked against."""

    def __init__(self, n):
        self.rt, self.n, self.p = _ffi.hip(), n, C.c_void_p()
        assert self.rt.hipMalloc(C.byref(self.p), C.c_size_t(4 * n)) == 0
        assert self.rt.hipMemset(self.p, 0, C.c_size_t(4 * n)) == 0

    def host(self):
        out = np.zeros(self.n, np.float32)
        assert self.rt.hipDeviceSynchronize() == 0
        assert self.rt.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.p, C.c_size_t(4 * self.n), 2) == 0   # device to host
        return out

    def free(self):
        if self.p:
            self.rt.hipFree(self.p)
            self.p = C.c_void_p()


def test_tile_images_reproduce_the_film(device):
    """bling_pass_tile_layout + a tile-image pass per shard + bling_film_add_tiles / _shards: the film of
    the whole pass, from one shard and from two."""
    job, ref_film, _ = _ref_film("fixture")
    ctx = device(job)
    bufs = []
    try:
        for world in (1, 2):
            tiles = []
            for r in range(world):
                org, sw, sh = ctx.tile_layout(shard=(r, world))
                np.testing.assert_array_equal(org, job.shard_tiles(r, world))
                t = _DeviceFloats(len(org) * sw * sh * 4)
                bufs.append(t)
                tiles.append(t)
                ctx.render_pass_tiles(t.p.value, seed=SEED, pass_index=0, shard=(r, world), tiles_capacity=t.n)
            film = _DeviceFloats(job.width * job.height * 4)
            bufs.append(film)
            if world == 1:
                ctx.film_add_tiles(tiles[0].p.value, film.p.value, tiles_capacity=tiles[0].n)
            else:
                ctx.film_add_shards([t.p.value for t in tiles], film.p.value, tiles_capacity=min(t.n for t in tiles))
            _film_check("fixture", f"tiles-{world}", film.host(), ref_film)
    finally:
        for b in bufs:
            b.free()


def test_two_passes_accumulate(device):
    job, _, _ = _ref_film("fixture")
    ref = nm_ref.NormalsRef(job)
    want, _ = ref.render(SEED, pass_index=0)
    want, _ = ref.render(SEED, pass_index=1, film=want)
    ctx = device(job)
    film, _ = ctx.render_pass(seed=SEED, pass_index=0)
    one = film.copy()
    film, _ = ctx.render_pass(seed=SEED, pass_index=1, film=film)
    assert not np.array_equal(one, film)
    _film_check("fixture", "two-passes", film, want)


def test_render_loop_with_region_events(device):
    """bling_render with its per-window reports: every window of the pass once, then PassDone, and the
    film of the plain loop."""
    job, ref_film, _ = _ref_film("fixture")
    ctx = device(job)
    events = []
    film, _ = ctx.render_loop(lambda p, f, s: False, seed=SEED, first_pass=0,
                              regions=lambda k, p, w, f: events.append((k, tuple(w))))
    windows = [w for k, w in events if k == events[0][0]]
    assert len(windows) == job.num_tiles() and len(set(windows)) == len(windows)
    _film_check("fixture", "render-loop", film, ref_film)


# ---------------------------------------------------------------- 3. launch shapes
@pytest.mark.parametrize("over", ["image=1,1;random=1", "image=7,5;stratified=3,3"])
def test_small_launches(over, device):
    """image=1,1 random 1: 36 samples of the extent, less than a wavefront, and one of them alone (a
    single lane); image=7,5 stratified 3 3: more than 315 samples, a partial wavefront and a partial block."""
    job, s, L, img, geo, rst = _ref(("shape", over), lambda: load_config("N2", over))
    ctx = device(job)
    _check_samples(f"launch[{over}]", ctx, job, s, L, img, geo, rst)
    k = int(np.flatnonzero(geo[:, 0] != 0)[0]) if (geo[:, 0] != 0).any() else 0
    Lg, _, st = ctx.sample_li(s[k:k + 1], seed=SEED)
    assert np.array_equal(_bits(Lg), _bits(L[k:k + 1])) and st.rays_camera == 1


def test_smallest_image_of_two_waves(device):
    """A wave holds whole tiles and, at the smallest chunk, up to 256 x spp samples (core.hip render): a
    pass runs as two waves as soon as its sample extent holds more than 256 pixels.  Under the fixture's
    filter (two pixels of apron and one more column and row) that is 38 x 1 -- 43 x 6 extent pixels,
    1 032 samples in tiles of 384, 384 and 264 -- the image of fewest pixels that does; 37 x 1 (1 008
    samples) is one wave."""
    one = load_config("N2", "image=37,1")
    assert one.camera_samples() == 1008
    ctx = device(one)
    ctx.render_pass(seed=SEED, pass_index=0, chunk_paths=1)
    assert ctx.pass_results()[1] == 1
    job, s, L, img, geo, rst = _ref(("shape", "two-waves"), lambda: load_config("N2", "image=38,1"))
    assert job.camera_samples() == 1032 and job.num_tiles() == 3
    ctx.upload(job)
    film, st = ctx.render_pass(seed=SEED, pass_index=0, chunk_paths=1)
    assert _waves(ctx) == 2                                       # two waves: their results are not kept
    assert st.camera_samples == len(s) and st.path_vertices == rst.hits
    want, _ = nm_ref.NormalsRef(job).render(SEED)
    _film_check("fixture", "two-waves", film, want)
    _check_samples("launch[two-waves]", ctx, job, s, L, img, geo, rst)


def test_path_state_follows_the_scene_on_a_reused_context(device):
    """One context: a Path pass, the normal map (which keeps four records per sample instead of the
    path set), a larger normal map, and Path again."""
    path_job = load_config("C1", "image=32,32;stratified=2,2;path=5,3")
    ctx = device(path_job)
    before, _ = ctx.render_pass(seed=SEED, pass_index=0)
    for tag in ("C4", "fixture"):
        job, ref_film, _ = _ref_film(tag)
        ctx.upload(job)
        film, _ = ctx.render_pass(seed=SEED, pass_index=0)
        _film_check(tag, "reused", film, ref_film)
    ctx.upload(path_job)
    after, _ = ctx.render_pass(seed=SEED, pass_index=0)
    e = film_errors(after, before)
    assert e["rel_l2"] <= P.FILM_BARS["C1_48"][1] and e["pix_max"] <= P.PIXEL_BARS["C1_48"][1], e


# ---------------------------------------------------------------- 4. multi-device
def test_two_device_contexts_split_the_tiles(device):
    job, ref_film, rst = _ref_film("fixture")
    single, _ = device(job).render_pass(seed=SEED, pass_index=0)
    os.environ["BLING_ALLOW_REPEATED_DEVICES"] = "1"
    try:
        two = device(job, [0, 0])
        film, st = two.render_pass(seed=SEED, pass_index=0)
    finally:
        del os.environ["BLING_ALLOW_REPEATED_DEVICES"]
    assert (st.camera_samples, st.path_vertices) == (rst.samples, rst.hits)
    _film_check("fixture", "two-devices", film, single)
    _film_check("fixture", "two-devices-ref", film, ref_film)


# ---------------------------------------------------------------- 5. refusals kept
def test_vertex_records_stay_path_only(device):
    job, s, _, _, _, _ = _ref("N1", lambda: load_config("N1"))
    ctx = device(job)
    with pytest.raises(BlingError) as e:
        ctx.sample_li_vertices(s[:4], seed=SEED)
    assert e.value.rc == -5                                       # BLING_EUNSUPPORTED
    with pytest.raises(BlingError) as e:
        ctx.bidir_terms(s[:4], seed=SEED)
    assert e.value.rc == -1 and "not bidir" in str(e.value)


def test_debug_kdtree_is_treated_as_every_unserved_renderer(tmp_path, device):
    """`debug kdtree` stays BLING_RENDERER_OTHER, like `bidirnod`: whatever the core answers to an
    unserved sampler block -- an error at upload, or a job it does not run as a normal map -- it
    answers the same to both, and neither reaches k_shade_nm (their integrator is not 3)."""
    src = open(os.path.join(SCENES, "normals.bling")).read()
    block = "      integrator { debug normals }\n"
    outcome = []
    for word in ("debug kdtree", "bidirnod maxDepth 5 sampleDepth 3"):
        p = tmp_path / (word.split()[-1] + word.split()[0] + ".bling")
        p.write_text(src.replace(block, "      integrator { %s }\n" % word))
        job = parse_job(str(p))
        assert job.config.renderer == 1 and job.config.integrator != 3
        try:
            ctx = device(job)
            _, st = ctx.render_pass(seed=SEED, pass_index=0)
            outcome.append(("ran", int(st.path_vertices > 0), int(st.rays_shadow + st.rays_mis > 0)))
        except BlingError as e:
            outcome.append(("refused", e.rc, str(e)))
    assert outcome[0] == outcome[1], outcome


# ---------------------------------------------------------------- 6. CLI
def test_cli_writes_the_normal_map(tmp_path):
    """`bling fixtures/scenes/normals.bling --passes 1` writes pass-00001.png and .hdr; the .hdr decodes to
    the image of the Python render() of the same pass.  The two films differ in their atomics' order
    only, and xyzToRgb is linear, so the images agree to cond (xyzToRgb) x the film bar
    (test_render_returns_the_weighted_splat_image's argument); RGBE then keeps 8 bits of the largest
    channel's mantissa, an error below 2^-7 of that channel."""
    exe = os.path.join(_ffi.LIBDIR, "bling")
    scene = os.path.join(SCENES, "normals.bling")
    out = subprocess.run([exe, scene, "--passes", "1", "--out", str(tmp_path / "pass")], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    assert "renderer normals" in out.stdout
    for ext in ("png", "hdr"):
        assert os.path.getsize(tmp_path / f"pass-00001.{ext}") > 0
    job = parse_job(scene)
    film = render(job, passes=1, seed=SEED)
    rgb = np.maximum(np.nan_to_num(film_to_rgb(film, job.width, job.height), nan=0.0), 0)
    data = open(tmp_path / "pass-00001.hdr", "rb").read()
    head, body = data.split(b"\n\n", 1)
    dims, body = body.split(b"\n", 1)
    assert head.startswith(b"#?RADIANCE") and dims == f"-Y {job.height} +X {job.width}".encode()
    e = np.frombuffer(body, np.uint8).reshape(job.height, job.width, 4).astype(np.float64)
    dec = np.where(e[..., 3:] > 0, e[..., :3] * np.ldexp(1.0, (e[..., 3:] - 136).astype(int)), 0.0)
    m = np.array([[3.240479, -1.537150, -0.498535], [-0.969256, 1.875991, 0.041556], [0.055648, -0.204043, 1.057311]])
    peak = rgb.max(-1, keepdims=True)
    err = np.abs(dec - rgb) / np.maximum(peak, 1e-9)
    lit = peak[..., 0] > 1e-3
    assert lit.sum() > 0.5 * lit.size
    assert (err[lit] <= 2.0 ** -7 + np.linalg.cond(m) * FIXTURE_L2).all(), float(err[lit].max())
