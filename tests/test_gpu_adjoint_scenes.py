"""The light-path renderers on the device, on the materials and normals of tests/adjoint_scenes.py:
the bidirectional integrator, the light tracer and the Metropolis renderer against their CPU
restatements, bit for bit, and one SPPM pass against the oracle's.  tests/test_adjoint_scenes.py
shows on the CPU, at these very sizes, that each case's light paths meet its lobe or normal at least
64 times, so none of these tests passes with nothing tested.  Every bar is an existing one:
tests/test_gpu_bidir.py's and tests/test_gpu_xform_shapes.py's equalities, ORDER_BAR of
tests/test_gpu_light_tracer.py, mlt_cases.bound and test_sppm_pass_from_a_scaled_lamp's ratios.
"""
import numpy as np
import pytest

import adjoint_scenes as A
from bd_ref import BidirRef, parity_samples
from bling_amd.render import Context
from lt_ref import LightRef
from mlt_cases import bound, ratio
from mlt_ref import MltRef, mutations
from oracle_py import OracleSppm
from parity_util import report
from test_gpu_light_tracer import ORDER_BAR

pytestmark = pytest.mark.gpu
SEED = 0x0B11A6
N = 512


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


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("adjoint_scenes_gpu")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("case", A.served("bidir"))
def test_bidir_samples_and_terms_equal_the_restatement(case, device, scene_dir):
    job = A.build(scene_dir, case, "bidir")
    s = parity_samples(job, N)
    ref = BidirRef(job)
    L, terms, lens, rst = ref.sample_li(s, SEED, 1)
    ctx = device(job)
    Lg, _, gst = ctx.sample_li(s, seed=SEED, pass_index=1)
    tg, lg = ctx.bidir_terms(s, seed=SEED, pass_index=1)
    exact = [int((_bits(tg[:, k]) == _bits(terms[:, k])).all(1).sum()) for k in range(3)]
    rays = [gst.rays_camera, gst.rays_continuation, gst.rays_mis, gst.rays_shadow, gst.path_vertices]
    report(f"adjoint_bidir[{case}]", n=len(s), ld_le_l_exact=exact, L_exact=int((_bits(Lg) == _bits(L)).all(1).sum()),
           nonblack=int((np.abs(L).sum(1) > 0).sum()), light_paths=int((lens[:, 1] > 0).sum()), rays_device=rays,
           rays_ref=rst.rays(), reached={k: ref.coverage[k] for k in A.TARGET[case]})
    assert np.array_equal(lg, lens) and (lens[:, 1] > 0).sum() > 64 and (np.abs(L).sum(1) > 0).sum() > 64
    for k in range(3):
        assert np.array_equal(_bits(tg[:, k]), _bits(terms[:, k])), ("ld", "le", "l")[k]
    assert np.array_equal(_bits(Lg), _bits(L))
    assert rays == rst.rays()


@pytest.mark.parametrize("case", A.served("light"))
def test_light_tracer_records_and_splat_image(case, device, scene_dir):
    job = A.build(scene_dir, case, "light")
    ref = LightRef(job)
    rrec, rsplat, rst = ref.run(SEED, 1)
    ctx = device(job)
    grec = ctx.light_records(seed=SEED, pass_index=1)
    gsplat, gst = ctx.light_pass(seed=SEED, pass_index=1)
    counts = [gst.photons, gst.photon_rays, gst.shadow_rays, gst.splats, gst.dropped]
    same = len(grec) == len(rrec)
    xyz_exact = int(sum((_bits(grec[k]) == _bits(rrec[k])).sum() for k in "xyz")) if same else -1
    acc = np.zeros(job.width * job.height * 3, np.float64)
    idx = 3 * (grec["sy"].astype(np.int64) * job.width + grec["sx"])
    for c, k in enumerate("xyz"):
        np.add.at(acc, idx + c, grec[k].astype(np.float64))
    r, own = _rel(gsplat, rsplat), _rel(gsplat, acc)
    report(f"adjoint_light[{case}]", records=len(grec), records_ref=len(rrec), xyz_exact=xyz_exact, counts=counts,
           counts_ref=rst.counts(), splat_l2=r, splat_l2_own=own, reached={k: ref.coverage[k] for k in A.TARGET[case]})
    assert len(grec) == len(rrec) > 100
    for k in ("photon", "depth", "sx", "sy"):
        assert np.array_equal(grec[k], rrec[k]), k
    for k in "xyz":
        assert np.array_equal(_bits(grec[k]), _bits(rrec[k])), k
    assert counts == rst.counts()
    assert np.isfinite(gsplat).all() and r <= ORDER_BAR and own <= ORDER_BAR


@pytest.mark.parametrize("case", A.served("metropolis"))
def test_metropolis_records_and_splat_image(case, device, scene_dir):
    job = A.build(scene_dir, case, "metropolis")
    ref = MltRef(job)
    rrec, rstarts, r64, r32, rst = ref.run(SEED, 1)
    ctx = device(job)
    grec, gstarts, gb = ctx.mlt_records(seed=SEED, pass_index=1)
    gsplat, gst = ctx.mlt_pass(seed=SEED, pass_index=1)
    counts = [gst.mutations, gst.large_steps, gst.accepted, gst.splats, gst.dropped, gst.rays_camera, gst.rays_continuation,
              gst.rays_mis, gst.rays_shadow, gst.path_vertices]
    bnd = bound(ref)
    cpu = ratio(np.abs(r32.astype(np.float64) - r64), bnd)
    own = ratio(np.abs(gsplat.astype(np.float64) - r64), bnd)
    both = ratio(np.abs(gsplat.astype(np.float64) - r32.astype(np.float64)), 2 * bnd)
    exact = int(sum((grec[k].view(np.uint32) == rrec[k].view(np.uint32)).sum() for k in ("x", "y", "i_prop", "a"))
                if len(grec) == len(rrec) else -1)
    report(f"adjoint_mlt[{case}]", records=len(grec), fields_exact=exact, counts=counts, counts_ref=rst.counts(),
           b=[float(gb), float(rst.b)], ratio_restatement=cpu, ratio_device=own, ratio_both=both,
           reached={k: ref.coverage[k] for k in A.TARGET[case]})
    assert len(grec) == len(rrec) == mutations(job)
    for k in ("chain", "mutation", "flags"):
        assert np.array_equal(grec[k], rrec[k]), k
    for k in ("x", "y", "i_prop", "a"):
        assert np.array_equal(grec[k].view(np.uint32), rrec[k].view(np.uint32)), k   # bit-equal, NaN included
    assert np.array_equal(gstarts, rstarts)
    assert np.float32(gb).view(np.uint32) == np.float32(rst.b).view(np.uint32)
    assert counts == rst.counts()
    assert np.float32(gst.b).view(np.uint32) == np.float32(rst.b).view(np.uint32)
    assert np.isfinite(gsplat).all() and r64.any()
    assert cpu <= 1.0 and own <= 1.0 and both <= 1.0


@pytest.mark.parametrize("case", A.served("sppm"))
def test_sppm_pass_against_the_oracle(case, device, scene_dir):
    """One pass against the oracle's, with the assertions and bars of test_sppm_pass_from_a_scaled_lamp.
    The film of a pass holds the emission the camera sees directly; only envimage has an emitter in view,
    elsewhere the film's XYZ is zero on both sides and the photons' splat image carries the comparison
    (asserted to be lit)."""
    job = A.build(scene_dir, case, "sppm")
    w, h = job.width, job.height
    fo, so, sto = OracleSppm(job).render_pass(seed=SEED, pass_index=1)
    ctx = device(job)
    ctx.sppm_reset()
    f, sp, st = ctx.sppm_pass(seed=SEED, pass_index=1)
    f, fo = f.reshape(h, w, 4), fo.reshape(h, w, 4)
    hasw = (fo[..., 0] > 0) & (f[..., 0] > 0)
    l2 = lambda a, b: float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))  # noqa: E731
    film_l2 = l2(f[..., 1:][hasw] / f[..., :1][hasw], fo[..., 1:][hasw] / fo[..., :1][hasw])
    splat_l2 = l2(sp, so)
    report(f"adjoint_sppm[{case}]", hitpoints=[int(st.hitpoints), int(sto.hitpoints)],
           photon_rays=[int(st.photon_rays), int(sto.photon_rays)], pairs=[int(st.photon_hits), int(sto.photon_hits)],
           film_l2=film_l2, splat_l2=splat_l2)
    assert st.photons == sto.photons and sto.photon_hits > 100 and np.count_nonzero(so) > 100
    assert abs(int(st.hitpoints) - int(sto.hitpoints)) <= 0.005 * sto.hitpoints + 1
    assert abs(int(st.cam_rays) - int(sto.cam_rays)) <= 0.005 * sto.cam_rays + 1
    assert abs(int(st.photon_rays) - int(sto.photon_rays)) <= 0.01 * sto.photon_rays + 1
    assert abs(int(st.photon_hits) - int(sto.photon_hits)) <= 0.02 * sto.photon_hits + 1
    assert np.isfinite(f).all() and film_l2 <= 1e-2
    assert np.isfinite(sp).all() and splat_l2 <= 3e-2
