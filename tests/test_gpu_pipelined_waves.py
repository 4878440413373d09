"""A pass as two half-waves on two streams (core.hip render, core_wave.h run_wave_pair_t) against the
same pass as one wave (BLING_PASS_NO_PIPELINE): only the wave a tile's paths belong to changes, so
every sample's result is bit-equal, every counter is equal, and the counters are the oracle's.

Films are not compared: their float atomics sum in an order that differs between any two passes
(tests/test_gpu_mis_cull.py).  The per-sample results (bling_debug_pass_results: what addSample
receives, written by one thread each) are the bar.

The context is switched to pipeline wherever that is legal (bling_debug_set_pipeline), whatever the
scene profile's default, and each test checks how the pass really ran (two half-waves in flight, or
one wave).  Scenes of tests/mis_cull_scenes.py; the sample extent of an n x n image under the 2 x 2
Mitchell filter is n + 5 pixels wide, so 40 x 40 gives 3 x 3 tiles (odd: a 5 / 4 cut), 11 x 11 one
tile, 32 x 32 nine tiles, 64 x 64 twenty-five.

  cornell   all-LDS BVH4 traversal, the factored one-light profile (the benchmark's), 25 tiles
  two       the meshes profile, two lamps; at 40 x 40 with maxDepth 5, 1 and 15, and at one tile
  sphere    analytic shapes only (BVH2 traversal), maxDepth 15
  brute     the exhaustive traversal kernels
  packet    the packet traversal kernels

None of those rooms leaves the all-LDS plan, so the global-fallback plan comes from the generated
scenes of tests/plan_scenes.py (the counts tests/test_traversal_plans.py found, 64 x 64, 25 tiles):

  fallback  soup of 40 triangles and 9 shapes: BVH4 with lds_all4 == 0 (more shapes than LDS keeps:
            their records come from global memory) and the whole stack in LDS -- the non-all-LDS
            kernels on half grids and two streams
  spill     chain(24), and the smallest soup whose triangles come from global memory (145: measured
            stack4_need 14 against the 12 rows that plan keeps in LDS): BVH4 stack rows spill to
            stack4_ovf, which a grid's thread id indexes, so two traversal launches in flight would
            share them: the pass must stay one wave even with the pipeline switched on for the context

Counters and the oracle: it reports samples, rays per kind and dropped samples, which are compared.
It has no count of path vertices or of culled MIS queries (tests/test_gpu_mis_cull.py takes the
culled count from the device too).  The device's path_vertices is by construction camera +
continuation rays, so it is held to the oracle's sum of those two; the culled count is held equal
between the pipelined and the single-wave pass, and to lie within the oracle's rays_mis.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mis_cull_scenes  # noqa: E402
import plan_scenes  # noqa: E402
from bling_amd import _ffi  # noqa: E402
from bling_amd.scene import parse_job  # noqa: E402
from oracle_py import Oracle  # noqa: E402
from parity_util import report  # noqa: E402

SEED = 0x0B11A6
PLAN = {"brute": lambda si: si["bf_prims"] == 16,
        "packet": lambda si: si["bf_prims"] == 0 and si["pkt_n"] > 0,
        "cornell": lambda si: si["bf_prims"] == 0 and si["pkt_n"] == 0 and si["lds_all4"] == 1}


@pytest.fixture(scope="module")
def ctx():
    from bling_amd.render import Context
    c = Context(0)
    c.set_pipeline(1)
    return c


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("pipelined_scenes")


def _two(scene_dir, size, depth):
    path = os.path.join(str(scene_dir), f"pipe_two_{size}_{depth}.bling")
    with open(path, "w") as f:
        f.write(mis_cull_scenes._text("two", size, depth))
    return parse_job(path)


def _counts(st):
    return (st.camera_samples, st.rays_camera, st.rays_continuation, st.rays_mis, st.rays_shadow, st.dropped_samples)


def _pass(ctx, flags, pass_index=0):
    _, st = ctx.render_pass(seed=SEED, pass_index=pass_index, flags=flags)
    res, waves = ctx.pass_results()
    return st, res, waves, ctx.mis_culled()


def _check(ctx, job, tag, want_waves, tiles=None, pass_index=0, oracle=True):
    st_p, r_p, w_p, cull_p = _pass(ctx, 0, pass_index)
    st_s, r_s, w_s, cull_s = _pass(ctx, _ffi.PASS_NO_PIPELINE, pass_index)
    words = int((r_p.view(np.uint32) != r_s.view(np.uint32)).sum())
    rec = dict(waves=(w_p, w_s), tiles=int(st_p.tiles), samples=int(r_p.shape[0]), result_words_differ=words,
               counts_pipelined=_counts(st_p), counts_single=_counts(st_s), vertices=(st_p.path_vertices, st_s.path_vertices),
               culled=(cull_p, cull_s))
    if oracle:
        _, st_o = Oracle(job).render(seed=SEED, pass_index=pass_index)
        rec["counts_oracle"] = (st_o.samples, st_o.rays_camera, st_o.rays_continuation, st_o.rays_mis, st_o.rays_shadow,
                                st_o.dropped)
    report(f"pipelined[{tag}]", **rec)
    assert w_p == want_waves and w_s == 1
    if tiles is not None:
        assert st_p.tiles == tiles
    assert r_p.shape == r_s.shape and r_p.shape[0] == st_p.camera_samples
    assert words == 0
    assert _counts(st_p) == _counts(st_s)
    assert st_p.path_vertices == st_s.path_vertices == st_p.rays_camera + st_p.rays_continuation
    assert cull_p == cull_s
    if oracle:
        assert _counts(st_p) == rec["counts_oracle"]
        assert st_p.path_vertices == st_o.rays_camera + st_o.rays_continuation
        assert cull_p <= st_o.rays_mis
    return st_p


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "sphere", "brute", "packet"])
def test_two_half_waves_equal_one_wave(ctx, scene_dir, name):
    job = mis_cull_scenes.build(scene_dir, name)
    ctx.upload(job)
    si = ctx.scene_info()
    report(f"pipelined_plan[{name}]", **si)
    if name in PLAN:
        assert PLAN[name](si), si
    _check(ctx, job, name, -2)


@pytest.mark.gpu
def test_global_fallback_plan_pipelines(ctx, scene_dir):
    job = parse_job(plan_scenes.soup(scene_dir, 40, 9))
    ctx.upload(job)
    si = ctx.scene_info()
    report("pipelined_plan[fallback]", **si)
    assert si["bf_prims"] == 0 and si["pkt_n"] == 0 and si["lds_all4"] == 0 and si["stack4_need"] <= si["stack4_lds"], si
    _check(ctx, job, "fallback", -2, tiles=25)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain24", "soup145"])
def test_spilled_stack_keeps_one_wave(ctx, scene_dir, name):
    path = plan_scenes.chain(scene_dir, 24) if name == "chain24" else plan_scenes.soup(scene_dir, 145, 4, degenerate=True)
    job = parse_job(path)
    ctx.upload(job)
    si = ctx.scene_info()
    report(f"pipelined_plan[spill_{name}]", **si)
    assert si["lds_all4"] == 0 and si["stack4_need"] > si["stack4_lds"], si
    _check(ctx, job, f"spill_{name}", 1, tiles=25)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [5, 1, 15])
def test_odd_tile_count_and_depths(ctx, scene_dir, depth):
    job = _two(scene_dir, 40, depth)
    ctx.upload(job)
    _check(ctx, job, f"two40_d{depth}", -2, tiles=9)


@pytest.mark.gpu
def test_one_tile_keeps_one_wave(ctx, scene_dir):
    job = _two(scene_dir, 11, 5)
    ctx.upload(job)
    _check(ctx, job, "two11", 1, tiles=1)


@pytest.mark.gpu
def test_consecutive_passes_on_one_context(ctx, scene_dir):
    """Buffer reuse and event ordering: pipelined passes back to back (each starts after the one
    before and after its film), then the same passes as single waves."""
    job = _two(scene_dir, 40, 5)
    ctx.upload(job)
    got = [_pass(ctx, 0, p) for p in (1, 2, 1)]
    ref = [_pass(ctx, _ffi.PASS_NO_PIPELINE, p) for p in (1, 2)]
    assert [g[2] for g in got] == [-2, -2, -2] and [r[2] for r in ref] == [1, 1]
    for g, r in ((got[0], ref[0]), (got[1], ref[1]), (got[2], ref[0])):
        assert np.array_equal(g[1].view(np.uint32), r[1].view(np.uint32))
        assert _counts(g[0]) == _counts(r[0]) and g[3] == r[3]
    assert not np.array_equal(got[0][1], got[1][1])          # the two passes do differ
    _, st_o = Oracle(job).render(seed=SEED, pass_index=2)
    assert _counts(got[1][0]) == (st_o.samples, st_o.rays_camera, st_o.rays_continuation, st_o.rays_mis, st_o.rays_shadow,
                                  st_o.dropped)
