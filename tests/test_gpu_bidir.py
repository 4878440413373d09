"""The bidirectional path integrator on the device (k_bd_walk / k_bd_connect / k_bd_finish, bidir.h)
against its CPU restatement (tests/ref/bidir_ref.cpp).

Per-sample parity is pinned bit for bit: every operation of the three kernels is shared with code that
is already bit-exact against the oracle, and the ray counts follow the restatement's guard order.
The film differs from the restatement's only in the order of its binary32 sums; FILM_L2 / FILM_PIX are
twice the relative L2 and the worst relative pixel error measured on MI355X.
"""
import ctypes as C

import numpy as np
import pytest

from bling_amd import _ffi
from bling_amd.render import BlingError, Context
from bling_amd.scene import load_config
from bd_ref import BidirRef, parity_samples, results as bd_results
from film_ref import pass_samples as _pass_samples
from parity_util import film_errors, report

pytestmark = pytest.mark.gpu
SEED = 0x0B11A6
N = 512
# measured: relative L2 1.967e-7, worst pixel 7.13e-7 (the waves' and shards' films against the one-wave
# pass: 4.9e-8 / 3.8e-7)
FILM_L2, FILM_PIX = 3.94e-7, 1.43e-6

SCENES = ["B1", "B2", "B3", "B4", "B5", "B6", "B7"]
_cache = {}


def _scene(name):
    """(job, samples, the restatement's L / terms / lens / stats), computed once."""
    if name not in _cache:
        job = load_config(name)
        s = parity_samples(job, N)
        _cache[name] = (job, s) + BidirRef(job).sample_li(s, SEED, 1)
    return _cache[name]


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


def _rays(st):
    return [st.rays_camera, st.rays_continuation, st.rays_mis, st.rays_shadow, st.path_vertices]


@pytest.mark.parametrize("name", SCENES)
def test_samples_and_ray_counts_equal_the_restatement(name, device):
    job, s, L, terms, lens, rst = _scene(name)
    ctx = device(job)
    Lg, _, gst = ctx.sample_li(s, seed=SEED, pass_index=1)
    same = (_bits(Lg) == _bits(L)).all(1)
    tg, lg = ctx.bidir_terms(s, seed=SEED, pass_index=1)
    term_same = [int((_bits(tg[:, k]) == _bits(terms[:, k])).all(1).sum()) for k in range(3)]
    den = np.abs(L).astype(np.float64).sum(1)
    rel = np.abs(Lg.astype(np.float64) - L).sum(1) / np.where(den > 0, den, 1.0)
    report("bidir_samples", scene=name, n=len(s), exact=int(same.sum()), ld_le_l_exact=term_same,
           lens_equal=bool(np.array_equal(lg, lens)), worst_rel=float(np.nanmax(rel)), rays_device=_rays(gst),
           rays_ref=rst.rays(), nonblack=int((den > 0).sum()))
    assert np.array_equal(lg, lens)
    assert same.all(), (int((~same).sum()), term_same)
    assert _rays(gst) == rst.rays()
    assert (den > 0).sum() > N // 8                               # the scene lights its samples


def test_terms_hook_equals_the_restatement(device):
    job, s, _, terms, lens, _ = _scene("B1")
    ctx = device(job)
    tg, lg = ctx.bidir_terms(s, seed=SEED, pass_index=1)
    assert np.array_equal(lg, lens)
    for k, nm in enumerate(("ld", "le", "l")):
        assert np.array_equal(_bits(tg[:, k]), _bits(terms[:, k])), nm
    assert tg[:, 0].any() and tg[:, 2].any()


def _film_scene():
    if "film" not in _cache:
        job = load_config("B8")
        ref_film, rst = BidirRef(job).render(SEED, 1)
        _cache["film"] = (job, ref_film, rst)
    return _cache["film"]


def test_film_against_the_restatement(device):
    job, ref_film, rst = _film_scene()
    ctx = device(job)
    film, st = ctx.render_pass(seed=SEED, pass_index=1)
    e = film_errors(film, ref_film)
    report("bidir_film", **e, rays_device=_rays(st), rays_ref=rst.rays())
    assert np.isfinite(film).all() and _rays(st) == rst.rays() and st.camera_samples == rst.samples
    assert e["rel_l2"] <= FILM_L2 and e["pix_max"] <= FILM_PIX, e


@pytest.mark.parametrize("shard", [(0, 1), (1, 2)])
def test_pass_results_equal_the_restatement_sample_by_sample(device, shard):
    """The tile-mode walk (sample ids from the tile table, k_raygen's order): every per-sample result of
    a one-wave pass -- what the film kernels read -- is the restatement's for that slot's sample, bit
    for bit; the second shard's tile table has other offsets."""
    job, _, _ = _film_scene()
    ctx = device(job)
    _, st = ctx.render_pass(seed=SEED, pass_index=1, shard=shard)
    res, waves = ctx.pass_results()
    s = _pass_samples(job, ctx.scene_info()["sample_major"], shard)
    assert waves == 1 and len(res) == len(s) == st.camera_samples
    if shard == (0, 1):
        assert len(s) == job.camera_samples() and len(np.unique(s, axis=0)) == len(s)
    L, _, _, rst = BidirRef(job).sample_li(s, SEED, 1)
    want = bd_results(L)
    assert np.array_equal(_bits(res), _bits(want))
    assert _rays(st) == rst.rays() and want[:, 3].all() and want[:, :3].any()
    Lg, _, _ = ctx.sample_li(s, seed=SEED, pass_index=1)         # the list-mode walk of the same samples
    assert np.array_equal(_bits(Lg), _bits(L))


def test_waves_keep_the_pass(device):
    """chunk_paths = 1024 cuts the 52 x 52 x 4 samples at tile boundaries into 13 waves of the vertex
    buffers.  No hook returns the per-sample results of a pass of several waves
    (bling_debug_pass_results keeps one wave's), and films and tile images are summed with float
    atomics, so this comparison cannot be made exact: the ray counts and the
    vertex count are the one-wave pass's -- whose samples the test above pins one by one -- no sample
    is dropped, and the film differs within the bar of the film's own summation order."""
    job, _, _ = _film_scene()
    ctx = device(job)
    one, st1 = ctx.render_pass(seed=SEED, pass_index=1)
    many, stn = ctx.render_pass(seed=SEED, pass_index=1, chunk_paths=1024)
    with pytest.raises(BlingError):
        ctx.pass_results()
    assert stn.bounce_launches >= 3 * 3 and _rays(stn) == _rays(st1)
    assert stn.camera_samples == st1.camera_samples and stn.dropped_samples == st1.dropped_samples == 0
    e = film_errors(many, one)
    report("bidir_waves", **e, launches=int(stn.bounce_launches))
    assert e["rel_l2"] <= FILM_L2 and e["pix_max"] <= FILM_PIX, e


class _DeviceFloats:
    """n zeroed floats on the device, from the HIP runtime the core itself is linked against (its
    symbols resolve through the core library's handle)."""

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


def test_two_shards_add_up_to_the_whole_pass(device):
    job, _, _ = _film_scene()
    ctx = device(job)
    whole, _ = ctx.render_pass(seed=SEED, pass_index=1)
    bufs = []
    try:
        for r in range(2):
            org, sw, sh = ctx.tile_layout(shard=(r, 2))
            t = _DeviceFloats(len(org) * sw * sh * 4)
            bufs.append(t)
            ctx.render_pass_tiles(t.p.value, seed=SEED, pass_index=1, shard=(r, 2), tiles_capacity=t.n)
        film = _DeviceFloats(job.width * job.height * 4)
        bufs.append(film)
        ctx.film_add_shards([b.p.value for b in bufs[:2]], film.p.value, tiles_capacity=min(b.n for b in bufs[:2]))
        e = film_errors(film.host(), whole)
    finally:
        for b in bufs:
            b.free()
    report("bidir_shards", **e)
    assert e["rel_l2"] <= FILM_L2 and e["pix_max"] <= FILM_PIX, e


@pytest.mark.parametrize("md", [0, 17])
def test_depth_bounds_are_refused_at_upload(md, device):
    with pytest.raises(BlingError) as e:
        device(load_config("C1", f"image=16,16;bidir={md},3"))
    assert e.value.rc == -1 and "bidir maxDepth" in str(e.value)


def test_vertex_buffers_follow_the_scene_on_a_reused_context(device):
    """One context: a Path pass that leaves a larger path capacity behind, then a bidir scene (its
    vertex buffers are sized for its own waves), a larger request that grows them, another maxDepth and
    Path again."""
    ctx = device(load_config("C1", "image=96,96;stratified=2,2;path=5,3"))
    ctx.render_pass(seed=SEED, pass_index=0)
    for name, k in (("B1", 64), ("B1", N), ("B3", 300)):
        job, s, L, _, _, _ = _scene(name)
        ctx.upload(job)
        Lg, _, _ = ctx.sample_li(s[:k], seed=SEED, pass_index=1)
        assert np.array_equal(_bits(Lg), _bits(L[:k])), (name, k)
    job, ref_film, _ = _film_scene()
    ctx.upload(job)
    film, _ = ctx.render_pass(seed=SEED, pass_index=1)
    e = film_errors(film, ref_film)
    assert e["rel_l2"] <= FILM_L2 and e["pix_max"] <= FILM_PIX, e
    ctx.upload(load_config("C1", "image=32,32;stratified=2,2;path=5,3"))
    film, st = ctx.render_pass(seed=SEED, pass_index=0)
    assert np.isfinite(film).all() and st.rays_continuation > 0
