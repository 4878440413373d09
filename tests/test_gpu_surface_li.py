"""The integrator seam on the device (bling_surface_li[_device], li_rays.hip): surfaceLi of the uploaded scene's
integrator along rays the caller made.  A ray that equals the camera's, with the camera's stream ids, gives
bling_sample_li's spectrum bit for bit (and the oracle's wherever bling_sample_li does); the bits of a ray do not
depend on the batch, its order or its waves; dropped rays write +0 and touch nothing else; and a renderer written
as caller's rays -> surface_li -> Image.add_windowed equals the built-in ordered pass bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import nm_ref
from bling_amd import _ffi
from bling_amd.scene import SCENES, load_config, parse_job
from oracle_py import Oracle
from parity_util import report, spectra_mismatch
from surface_li_cases import SEED, bits, c1, c1_with_camera, camera_rays, job_desc, stream_ids, windows_of

pytestmark = pytest.mark.gpu
INF, NAN = np.float32(np.inf), np.float32(np.nan)


@pytest.fixture(scope="module")
def ctx():
    from bling_amd.render import Context
    c = Context(0)
    yield c
    c.close()


def dev(a):
    """A numpy array as a tensor on the device, the copy finished (the context runs on a stream of its own)."""
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")
    torch.cuda.synchronize()
    return t


def li(ctx, rays, ids, pass_index=0):
    """surface_li of numpy rays (7, n) and ids (n, 2) through device tensors: (L (n, 16) numpy, LiStats)."""
    L, st = ctx.surface_li(dev(rays), dev(ids), seed=SEED, pass_index=pass_index)
    return L.cpu().numpy(), st


class Pass:
    """Every sample of a job's extent in window order: the oracle's camera rays, positions, stream ids and spectra."""

    def __init__(self, job, pass_index=0, oracle_li=True):
        self.job, self.orc, self.p = job, Oracle(job), pass_index
        self.samples, self.windows, self.counts = windows_of(job)
        self.rays, self.xy = camera_rays(self.orc, self.samples, pass_index=pass_index)
        self.ids = stream_ids(job, self.samples)
        if oracle_li:
            self.L, img, self.st = self.orc.sample_li_batch(self.samples, seed=SEED, pass_index=pass_index)
            assert np.array_equal(img, self.xy)


_passes = {}


def the_pass(name, over="image=16,16"):
    if (name, over) not in _passes:
        # (the oracle's sample_li serves path and directLighting; the normal map's restatement is nm_ref's)
        _passes[name, over] = Pass(c1(over) if name == "C1" else load_config(name, over), oracle_li=name != "N2")
    return _passes[name, over]


def same_counts(st, ref):
    return (st.rays_continuation, st.rays_mis, st.rays_shadow) == (ref.rays_continuation, ref.rays_mis, ref.rays_shadow)


# ------------------------------------------------------------------ 1. identity, path
def test_camera_rays_give_sample_li_and_the_oracle_path(ctx):
    P = the_pass("C1")
    assert P.job.spp == 4 and len(P.samples) == P.job.camera_samples()
    ctx.upload(P.job)
    L, st = li(ctx, P.rays, P.ids)
    Ld, img, sd = ctx.sample_li(P.samples, seed=SEED)
    differ_dev = int((bits(L) != bits(Ld)).any(1).sum())
    differ_orc = int((bits(L) != bits(P.L)).any(1).sum())
    report("surface_li_identity", scene="C1", rays=len(L), differ_sample_li=differ_dev, differ_oracle=differ_orc,
           ms=st.ms_total, waves=st.waves)
    assert np.array_equal(img, P.xy)
    assert st.rays == len(L) and st.dropped == 0 and st.waves == 1 and (L > 0).any()
    assert differ_dev == 0
    assert same_counts(st, sd) and st.rays_continuation > 0 and st.rays_shadow > 0
    assert differ_orc == 0


# ------------------------------------------------------------------ 2. identity, directLighting and normals
def test_camera_rays_give_sample_li_direct_lighting(ctx):
    P = the_pass("X4")
    ctx.upload(P.job)
    L, st = li(ctx, P.rays, P.ids)
    Ld, _, sd = ctx.sample_li(P.samples, seed=SEED)
    bad, exact, worst, _ = spectra_mismatch(L, P.L, 1e-4)                     # the suite's bar: k_shade_dl is an ulp off
    report("surface_li_identity", scene="X4", rays=len(L), mismatch=bad, exact=exact, worst=worst)
    assert np.array_equal(bits(L), bits(Ld)) and (L > 0).any()
    assert same_counts(st, sd) and st.dropped == 0
    assert bad == 0


def test_camera_rays_give_sample_li_and_the_oracle_normals(ctx):
    P = the_pass("N2")
    ctx.upload(P.job)
    L, st = li(ctx, P.rays, P.ids)
    Ld, _, sd = ctx.sample_li(P.samples, seed=SEED)
    assert np.array_equal(bits(L), bits(Ld)) and (L > 0).any()
    assert st.path_vertices == sd.path_vertices == int((L != 0).any(1).sum())
    assert (st.rays_continuation, st.rays_mis, st.rays_shadow, st.dropped) == (0, 0, 0, 0)
    Lo, img, _, rst = nm_ref.NormalsRef(P.job).sample_li(P.samples, SEED)    # the normal map's CPU restatement
    assert np.array_equal(img, P.xy) and rst.hits == st.path_vertices
    assert np.array_equal(bits(L), bits(Lo))


# ------------------------------------------------------------------ 3. a camera that is not the scene's
@pytest.mark.parametrize("which", ["lens", "environment"])
def test_another_cameras_rays(ctx, which, tmp_path):
    A = the_pass("C1")
    job_b = c1_with_camera(which, tmp_path, "image=16,16")
    assert (job_b.width, job_b.height, job_b.spp, job_b.filter_size) == (A.job.width, A.job.height, A.job.spp, A.job.filter_size)
    B = Pass(job_b)
    assert not np.array_equal(B.rays, A.rays) and np.array_equal(B.ids, A.ids)
    if which == "lens":
        assert len(np.unique(B.rays[:3], axis=1).T) > 100                    # the origins lie on the lens
    ctx.upload(A.job)                                                        # scene A's context, B's rays
    L, st = li(ctx, B.rays, B.ids)
    differ = int((bits(L) != bits(B.L)).any(1).sum())
    report("surface_li_other_camera", camera=which, rays=len(L), differ_oracle=differ, lit=int((L > 0).any(1).sum()))
    assert st.dropped == 0 and (L > 0).any(1).sum() > len(L) // 8
    assert differ == 0


# ------------------------------------------------------------------ 4. chunking and independence
def test_chunks_order_and_neighbours_do_not_change_a_rays_bits(ctx):
    P = the_pass("C1")
    n = 1000
    rays, ids = P.rays[:, :n], P.ids[:n]
    ctx.upload(P.job)
    rng = np.random.default_rng(4)
    try:
        base, st = li(ctx, rays, ids)
        assert st.waves == 1 and st.rays == n
        for chunk in (64, 100):
            ctx.set_li_chunk(chunk)
            L, st = li(ctx, rays, ids)
            assert st.waves == -(-n // chunk)
            assert np.array_equal(bits(L), bits(base)), chunk
        perm = rng.permutation(n)
        L, _ = li(ctx, rays[:, perm], ids[perm])                             # still cut into waves of 100
        assert np.array_equal(bits(L), bits(base[perm]))
        # 37 dropped rays interleaved
        where = np.sort(rng.choice(n + 37, 37, replace=False))
        valid = np.ones(n + 37, bool)
        valid[where] = False
        r2, i2 = np.zeros((7, n + 37), np.float32), np.zeros((n + 37, 2), np.uint32)
        r2[:, valid], i2[valid] = rays, ids
        r2[:, ~valid], i2[~valid] = rays[:, :37], ids[:37]
        r2[0, ~valid] = NAN
        for chunk in (100, 0):
            ctx.set_li_chunk(chunk)
            L, st = li(ctx, r2, i2)
            assert st.dropped == 37 and st.rays == n + 37 and st.waves == (-(-(n + 37) // chunk) if chunk else 1)
            assert np.array_equal(bits(L[valid]), bits(base)) and not bits(L[~valid]).any()
    finally:
        ctx.set_li_chunk(0)


# ------------------------------------------------------------------ 5. dropped rays
def test_dropped_rays_write_zero_and_touch_nothing_else(ctx):
    P = the_pass("C1")
    ctx.upload(P.job)
    k = 9                                                                    # valid rays around and between the bad ones
    base, _ = li(ctx, P.rays[:, 400:400 + k], P.ids[400:400 + k])
    assert (base != 0).any()
    bad = [(0, NAN, None), (1, INF, None), (2, -INF, None), (4, NAN, None), (5, INF, None), ("zero", 0, None), (6, NAN, None),
           (None, 0, P.job.spp), (None, 0, 2 ** 31)]
    n = k + len(bad)
    rays, ids = np.zeros((7, n), np.float32), np.zeros((n, 2), np.uint32)
    valid = np.ones(n, bool)
    valid[1::2][:len(bad)] = False
    rays[:, valid], ids[valid] = P.rays[:, 400:400 + k], P.ids[400:400 + k]
    for j, (plane, value, sn) in zip(np.nonzero(~valid)[0], bad):
        rays[:, j], ids[j] = P.rays[:, 0], P.ids[0]                          # a valid ray but for one thing
        if plane == "zero":
            rays[3:6, j] = 0
        elif plane is not None:
            rays[plane, j] = value
        if sn is not None:
            ids[j, 1] = sn
    L, st = li(ctx, rays, ids)
    assert st.dropped == len(bad) and st.rays == n
    assert not bits(L[~valid]).any()                                         # all 16 words 0x00000000
    assert np.array_equal(bits(L[valid]), bits(base))
    Lh, sh = ctx.host_surface_li(rays, ids, seed=SEED)
    assert np.array_equal(bits(Lh), bits(L)) and sh.dropped == len(bad)


# ------------------------------------------------------------------ 6. tmin
def test_tmin(ctx):
    P = the_pass("N2")
    ctx.upload(P.job)
    n = len(P.samples)
    r8 = np.zeros((8, n), np.float32)
    r8[:7], r8[7] = P.rays, INF
    t0, prim0, bary0 = ctx.trace(r8)
    hit0 = prim0 != 0xFFFFFFFF
    assert hit0.any() and (~hit0).any()
    L0, st = li(ctx, P.rays, P.ids)
    assert np.array_equal((L0 != 0).any(1), hit0) and st.dropped == 0
    # just past the first hit: what bling_trace finds from there
    past = P.rays.copy()
    past[6, hit0] = np.nextafter(t0[hit0], INF)
    r8[6] = past[6]
    t1, prim1, bary1 = ctx.trace(r8)
    hit1 = prim1 != 0xFFFFFFFF
    L1, st = li(ctx, past, P.ids)
    assert hit1.any() and st.dropped == 0
    assert np.array_equal((L1 != 0).any(1), hit1)
    same = (prim1 == prim0) & (bits(bary1) == bits(bary0)).all(1)
    assert np.array_equal(bits(L1[same]), bits(L0[same]))
    # halfway to the first hit: the same primitive at the same place
    half = P.rays.copy()
    half[6, hit0] = t0[hit0] * np.float32(0.5)
    r8[6] = half[6]
    t2, prim2, bary2 = ctx.trace(r8)
    same = (prim2 == prim0) & (bits(bary2) == bits(bary0)).all(1)
    L2, _ = li(ctx, half, P.ids)
    assert (same & hit0).sum() > hit0.sum() // 2
    assert np.array_equal(bits(L2[same]), bits(L0[same]))
    # tmin = +inf: a valid ray that misses
    never = P.rays.copy()
    never[6] = INF
    L3, st = li(ctx, never, P.ids)
    assert not bits(L3).any() and st.dropped == 0 and st.rays == n and st.path_vertices == 0


# ------------------------------------------------------------------ 7. refusals
def _raw(ctx, rays_ptr, ids_ptr, n, L_ptr):
    st = _ffi.LiStats()
    return _ffi.hip().bling_surface_li_device(ctx._h, SEED, 0, C.c_void_p(rays_ptr), C.c_void_p(ids_ptr), n, C.c_void_p(L_ptr),
                                              C.byref(st))


def test_refusals(ctx):
    from bling_amd.render import BlingError, Context
    P = the_pass("C1")
    hr, hi = P.rays[:, 800:864], P.ids[800:864]                              # 64 rays that see the box
    rays, ids = dev(hr), dev(hi)
    out = torch.zeros((64, 16), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    fresh = Context(0)
    try:
        assert _raw(fresh, rays.data_ptr(), ids.data_ptr(), 64, out.data_ptr()) == -4        # no scene
    finally:
        fresh.close()
    others = {"bidir": (load_config("B8", "image=16,16"), -5), "sppm": (load_config("X5", "image=16,16"), -1),
              "light": (parse_job(os.path.join(SCENES, "light-tracer.bling"), "image=16,16"), -1),
              "metropolis": (load_config("M1", "image=16,16"), -1)}
    for name, (job, rc) in others.items():
        ctx.upload(job)
        with pytest.raises(BlingError) as e:
            ctx.surface_li(rays, ids, seed=SEED)
        assert e.value.rc == rc, name
        with pytest.raises(BlingError) as e:
            ctx.host_surface_li(hr, hi, seed=SEED)
        assert e.value.rc == rc, name
    ctx.upload(P.job)
    assert _raw(ctx, None, ids.data_ptr(), 64, out.data_ptr()) == -1                        # a NULL buffer
    assert _raw(ctx, rays.data_ptr(), None, 64, out.data_ptr()) == -1
    assert _raw(ctx, rays.data_ptr(), ids.data_ptr(), 64, None) == -1
    assert _raw(ctx, rays.data_ptr(), ids.data_ptr(), 64, rays.data_ptr()) == -1            # L aliases the rays
    assert _raw(ctx, rays.data_ptr(), ids.data_ptr(), 64, ids.data_ptr()) == -1
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()                                                      # nothing was written
    assert _raw(ctx, None, None, 0, None) == 0                                              # n = 0
    L, st = ctx.surface_li(rays[:, :0].contiguous(), ids[:0].contiguous(), seed=SEED)
    assert tuple(L.shape) == (0, 16) and st.rays == 0 and st.waves == 0
    # the host variant is the device variant
    Ld, sd = ctx.surface_li(rays, ids, seed=SEED, out=out)
    Lh, sh = ctx.host_surface_li(hr, hi, seed=SEED)
    assert Ld.data_ptr() == out.data_ptr() and np.array_equal(bits(Lh), bits(Ld.cpu().numpy())) and (Lh != 0).any()
    assert same_counts(sh, sd) and sh.path_vertices == sd.path_vertices
    # an L that is aligned to 4 bytes only takes the store's narrow path: the same rows, nothing beside them
    wide = torch.full((64 * 16 + 8,), -1.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    assert _raw(ctx, rays.data_ptr(), ids.data_ptr(), 64, wide.data_ptr() + 4) == 0
    w = wide.cpu().numpy()
    assert np.array_equal(bits(w[1:1 + 64 * 16].reshape(64, 16)), bits(Lh)) and (w[0] == -1) and (w[1 + 64 * 16:] == -1).all()


# ------------------------------------------------------------------ 8. a caller-made renderer
def test_a_renderer_made_of_surface_li_and_the_image_api_is_the_ordered_pass(ctx):
    from bling_amd.image import Image
    job = c1("image=33,17")
    ctx.upload(job)
    img = Image(job_desc(job).filter, job.width, job.height, context=ctx)
    film = None
    for p in (0, 1):                                                         # the second pass accumulates on both sides
        P = Pass(job, p, oracle_li=False)
        assert len(P.windows) == 6
        L, st = ctx.surface_li(dev(P.rays), dev(P.ids), seed=SEED, pass_index=p)
        ist = img.add_windowed(P.windows, P.counts, dev(P.xy), L, "add")
        film, pst = ctx.render_pass(seed=SEED, pass_index=p, film=film, ordered=True)
        assert st.dropped == 0 and ist.dropped_spectrum == 0 and ist.dropped_position == 0
        assert pst.camera_samples == st.rays == len(P.samples)
        assert (st.rays_continuation, st.rays_mis, st.rays_shadow) == (pst.rays_continuation, pst.rays_mis, pst.rays_shadow)
        mine = img.film.cpu().numpy().reshape(-1)
        assert (mine > 0).any() and np.array_equal(bits(mine), bits(film)), p
