"""Every traversal kernel plan, on generated scenes (tests/plan_scenes.py), against the CPU oracle.

The core picks its closest-hit / any-hit kernels from the scene's size and make-up alone (scene_plan.cpp
scene_derive, plan_lds, plan_lds4; core_wave.h TraceLaunch, run_wave_prof).  The shipped scenes land
in three spots of that plan space; the cases here sit on its boundaries, and each one asserts its
regime from scene_info() before it compares anything:

  A   soup, 16 primitives (12 triangles + light + 3 shapes)  exhaustive kernels (bf_prims == 16)
  B   the same plus one triangle                           packet kernels, sample-major slots
  Bp  the largest soup that still has pkt_n > 0              (found by stepping; as B)
  C   the smallest soup with pkt_n == 0                     BVH4, all in LDS
  D   40 triangles + 9 shapes                               BVH4, shapes not in LDS (> kLdsShapesMax)
  E   the largest soup before lds_all4 first drops          BVH4, all in LDS, at the 26 KiB budget
  F   the smallest soup with lds_all4 == 0                  BVH4, triangles from global leaf_geo
  F2  the first soup (steps of 32) past the node prefix     BVH4, node prefix in LDS, the rest global
  G   chain(24), or the next n that needs them              BVH4 stack rows spilled to stack4_ovf
  H   chain(N_H)                                            BVH2 depth cap 31, leaves of > 2 primitives

No generated scene holds a fractal: the BVH2 queue kernels keep their C5 / X3 coverage
(test_gpu_parity.py).  The soups of A, C, E and F hold one zero-area triangle (two equal vertices); the
loader and the oracle accept it, and no ray hits it.

Three places where the cases had to differ from a plain reading of their description, all from the
builder's and the planner's arithmetic (bvh_build.cpp, plan_lds4), checked on the CPU with the builder:
  * at the smallest soup with lds_all4 == 0 (145 triangles, 36 BVH4 nodes) the node prefix still
    holds every node: 12 stack rows and the shapes leave 13.3 KiB, 100 nodes and more.  F asserts what
    holds there (lds4_tris == 0: leaf_hit_global), and F2, a soup of about 450 triangles, asserts
    lds4_nodes < bvh4_nodes, the prefix / global node fetch.
  * a threaded BVH has 2 x leaves - 2 entries, so a scene of 17 primitives has at most 16 entries
    only with leaves of two primitives, which the SAH makes only where two bounding boxes overlap
    (sum of their areas >= the area of their union).  The soup's triangles therefore come in pairs
    that share a screen cell, the two spheres share one, and the light lies within the backdrop's
    bounds: 17 primitives give 9 leaves.  18 primitives give 10, so Bp is B's scene (reported).
  * with distances and sizes growing by 1.5 per triangle the binned SAH peels three to five of the
    largest triangles off per level, not one: chain(48) has BVH depth 16 and leaves of one primitive
    (chain(24): depth 11).  The depth cap is reached from 116 triangles on and leaves past two
    primitives from N_H on, with the nearest triangle at 1e-9 so that squared distances stay finite.
    H keeps its asserted regime (bvh_depth == 31, max_leaf > 2) and uses that n.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bling_amd  # noqa: E402
import plan_scenes  # noqa: E402
from plan_scenes import CASES, FOUND, assert_regime, scan_plans  # noqa: E402
from plan_scenes import case_scene as _build  # noqa: E402
from bling_amd.scene import parse_job  # noqa: E402
from oracle_py import Oracle  # noqa: E402
from parity_util import film_errors, random_samples, report, spectra_mismatch  # noqa: E402
from scene_desc import desc  # noqa: E402
from test_gpu_parity import camera_rays, random_rays  # noqa: E402

SEED = 0x0B11A6
MISS = 0xFFFFFFFF
@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("plan_scenes")


# ------------------------------------------------------------------ CPU: the generator, oracle only
@pytest.mark.parametrize("name", CASES)
def test_generated_scenes_are_not_vacuous(scene_dir, name):
    """The generated scene parses, holds the intended primitives, is lit (at least half of the 4096
    samples have finite, non-black oracle radiance) and is seen (the 48 x 48 camera rays' closest hits
    name at least 75 % of its primitives; 60 % for the chains).  Conditions on the generator.
    Measured: non-black 0.67 .. 0.83, named 0.875 .. 0.99 (the light is out of view)."""
    path, nt, ns = _build(scene_dir, name)
    job = parse_job(path)
    c = job.counts()
    assert (c["triangles"], c["shapes"], c["prims"], c["fractal"], c["lights"]) == (nt, ns, nt + ns, 0, 1)
    orc = Oracle(job)
    smp = random_samples(orc, job, 4096, seed=11)
    L, _, _ = orc.sample_li_batch(smp, seed=SEED, pass_index=1)
    lit = float((np.isfinite(L).all(1) & (np.abs(L).sum(1) > 0)).mean())
    _, prim, _, _ = orc.trace(camera_rays(orc, job))
    named = len(set(prim[prim != MISS].tolist())) / c["prims"]
    print(f"generated[{name}] tris={nt} shapes={ns} non_black={lit:.3f} named={named:.3f}")
    assert lit >= 0.5
    assert named >= (0.6 if name in ("G", "H") else 0.75)


# ------------------------------------------------------------------ CPU: the plan, no device
def _plan_info(path):
    return bling_amd.scene_plan(parse_job(path))


def test_plan_scans_agree_with_the_recorded_counts(scene_dir, monkeypatch):
    """The boundaries of the plan space, scanned with the device-free plan, are the recorded ones."""
    monkeypatch.delenv("BLING_BRUTE", raising=False)
    assert scan_plans(_plan_info, scene_dir) == FOUND


@pytest.mark.parametrize("name", CASES)
def test_plan_puts_the_case_in_its_regime(scene_dir, monkeypatch, name):
    """Every case's regime, and the 26 KiB budget of an all-LDS block, from the device-free plan."""
    monkeypatch.delenv("BLING_BRUTE", raising=False)
    path, nt, ns = _build(scene_dir, name)
    assert_regime(name, nt, ns, _plan_info(path))


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx():
    from bling_amd.render import Context
    return Context(0)


def _upload_info(ctx, path):
    job = parse_job(path)
    ctx.upload(job)
    return job, ctx.scene_info()


@pytest.fixture(scope="module")
def plans(ctx, scene_dir):
    """The scanned cases' triangle counts, from uploads alone: {case: n}."""
    found = scan_plans(lambda path: _upload_info(ctx, path)[1], scene_dir)
    report("traversal_plans_scan", **found)
    return found


@pytest.mark.gpu
def test_scans_agree_with_the_recorded_counts(plans):
    """The counts the CPU test's scenes are built from are the ones the scans find."""
    assert plans == FOUND


def _case(ctx, scene_dir, plans, name):
    """Uploads the case's scene and asserts its regime: (job, oracle, scene_info)."""
    path, nt, ns = _build(scene_dir, name, plans.get(name))
    job, si = _upload_info(ctx, path)
    report(f"traversal_plan[{name}]", tris=nt, shapes=ns, **si)
    assert_regime(name, nt, ns, si)
    return job, Oracle(job), si


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_sample_parity(ctx, scene_dir, plans, name):
    """Per-sample radiance through the case's own kernels: 4096 samples, positions equal, no spectrum
    off by more than 1e-4 relative L1, the same number of rays."""
    job, orc, _ = _case(ctx, scene_dir, plans, name)
    smp = random_samples(orc, job, 4096, seed=11)
    Lg, img_g, st_g = ctx.sample_li(smp, seed=SEED, pass_index=1)
    Lo, img_o, st_o = orc.sample_li_batch(smp, seed=SEED, pass_index=1)
    bad, exact, worst, _ = spectra_mismatch(Lg, Lo)
    report(f"traversal_plan_samples[{name}]", samples=len(smp), mismatch=bad, exact=exact, worst_rel_ok=worst,
           pos_diff=int((img_g != img_o).any(1).sum()), rays_gpu=st_g.rays(), rays_oracle=st_o.rays())
    np.testing.assert_array_equal(img_g, img_o)
    assert bad == 0
    assert abs(st_g.rays() - st_o.rays()) == 0


def axis_rays(job, lo, hi, rng, n=256):
    """n rays along +-x, +-y, +-z (the other two direction components exactly 0): half pass through a
    point inside a triangle and start a few triangle sizes before it (an origin at the scale of its
    target: from the far side of a chain's bounds, 1e15 against a light of 1e9, the rounding of a
    shape's rotation matrix moves the object-space ray by more than the padding of its world box),
    half start exactly on a face plane of the bounds, every second of those along the plane instead
    of into the box."""
    d = desc(job)
    v = np.ctypeslib.as_array(d.vertices, shape=(3 * d.num_vertices,)).reshape(-1, 3).astype(np.float32)
    ix = np.ctypeslib.as_array(d.tri_indices, shape=(3 * d.num_triangles,)).reshape(-1, 3)
    rays = np.zeros((8, n), np.float32)
    rays[7] = np.inf
    ext = (hi - lo).astype(np.float32)
    for k in range(n):
        a, s = k % 3, (1.0 if (k // 3) % 2 == 0 else -1.0)
        if k < n // 2:
            w = rng.dirichlet([2.0, 2.0, 2.0]).astype(np.float32)
            tri = v[ix[rng.integers(0, len(ix))]]
            o = (w[:, None] * tri).sum(0).astype(np.float32)
            o[a] -= np.float32(s * 3.0 * np.abs(tri - tri.mean(0)).max())
            rays[3 + a, k] = s
        else:
            o = (lo + rng.random(3).astype(np.float32) * ext).astype(np.float32)
            o[a] = lo[a] if s > 0 else hi[a]                 # exactly on the face plane
            b = a if k % 2 == 0 else (a + 1 + (k // 2) % 2) % 3
            rays[3 + b, k] = s if b == a else (1.0 if rng.random() < 0.5 else -1.0)
        rays[0:3, k] = o
    return rays


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_trace_parity_on_the_case(ctx, scene_dir, plans, name):
    """bling_trace (the BVH2 walk) on the case's scene: camera rays, rays across the bounds and
    axis-parallel rays; test_trace_parity's bars."""
    job, orc, _ = _case(ctx, scene_dir, plans, name)
    lo, hi = plan_scenes.scene_bounds(job)
    rng = np.random.default_rng(7)
    rays = np.concatenate([camera_rays(orc, job), random_rays(lo, hi, 4000, rng), axis_rays(job, lo, hi, rng)], axis=1)
    t_o, p_o, b_o, _ = orc.trace(rays)
    t_g, p_g, b_g = ctx.trace(rays)
    same = p_o == p_g
    hit = same & (p_o != MISS)
    seg = rays.copy()
    seg[7] = np.where(np.isfinite(t_o), t_o * 0.5, 100.0)
    _, a_o, _, _ = orc.trace(seg, any_hit=True)
    _, a_g, _ = ctx.trace(seg, any_hit=True)
    # bit-equal t; a NaN t on both sides (H: a ray from 1e15 away at a triangle of 1e-9, the same
    # overflow in the same formula) is equal too
    t_diff = int((~((t_g[same] == t_o[same]) | (np.isnan(t_g[same]) & np.isnan(t_o[same])))).sum())
    report(f"traversal_plan_trace[{name}]", rays=rays.shape[1], hits=int((p_o != MISS).sum()),
           axis_hits=int((p_o[-256:] != MISS).sum()), id_mismatch=int((~same).sum()), t_diff=t_diff,
           bary_max_abs=float(np.abs(b_g[hit] - b_o[hit]).max(initial=0)), any_mismatch=int((a_o != a_g).sum()))
    assert (~same).sum() == 0
    assert t_diff == 0
    np.testing.assert_allclose(b_g[hit], b_o[hit], rtol=0, atol=1e-6)
    assert (a_o != a_g).sum() == 0


def _counts(st):
    return (st.camera_samples, st.rays_camera, st.rays_continuation, st.rays_mis, st.rays_shadow)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["B", "Bp", "C", "D"])
def test_tree_and_exhaustive_kernels_agree(ctx, scene_dir, plans, monkeypatch, name):
    """The case's tree kernels and the exhaustive kernels (BLING_BRUTE=64 at upload) render one pass of
    the same scene alike: test_exhaustive_and_tree_traversal_agree's bars."""
    job, _, si = _case(ctx, scene_dir, plans, name)
    assert si["prims"] <= 64
    a, sa = ctx.render_pass(seed=SEED, pass_index=0)
    monkeypatch.setenv("BLING_BRUTE", "64")
    ctx.upload(job)
    bf = ctx.scene_info()["bf_prims"]
    b, sb = ctx.render_pass(seed=SEED, pass_index=0)
    monkeypatch.delenv("BLING_BRUTE")
    ctx.upload(job)                                        # leave the default upload behind
    e = film_errors(a, b)
    report(f"traversal_plan_vs_exhaustive[{name}]", bf_prims=bf, **e,
           **{f"d_{k}": int(x) - int(y) for k, x, y in zip(("samples", "camera", "cont", "mis", "shadow"),
                                                           _counts(sa), _counts(sb))})
    assert bf > 0
    assert ctx.scene_info()["bf_prims"] == 0
    assert _counts(sa)[:2] == _counts(sb)[:2]
    assert all(abs(int(x) - int(y)) <= 8 for x, y in zip(_counts(sa), _counts(sb)))
    assert e["rel_l2"] <= 1e-4 and e["pix_over_1e-3"] <= 4
