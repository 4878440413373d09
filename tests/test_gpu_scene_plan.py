"""The device-free plan (bling_debug_scene_plan) against what an upload settles (bling_debug_scene_info), the
derive stage on a tree it did not build (the device builder's), and the one plan on every device of a fan-out."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bling_amd  # noqa: E402
from bling_amd.scene import load_config, parse_job  # noqa: E402
from plan_scenes import LDS4_BUDGET, case_scene, items, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 0x0B11A6


@pytest.fixture(scope="module")
def ctx():
    from bling_amd.render import Context
    return Context(0)


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("scene_plan")


def _job(scene_dir, name):
    if name in ("C1", "X3"):                                  # cornell-box, julia
        return load_config(name, "image=48,48")
    return parse_job(case_scene(scene_dir, name)[0])


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "F", "G", "C1", "X3"])
def test_upload_settles_the_plan(ctx, scene_dir, name):
    job = _job(scene_dir, name)
    ctx.upload(job)
    assert ctx.scene_info() == bling_amd.scene_plan(job)


def test_derive_takes_the_device_builders_tree(ctx, scene_dir):
    job = _job(scene_dir, "F")
    ctx.upload(job, bvh="device")
    info = ctx.bvh_build_info()
    assert (info["used"], info["fallback"]) == ("device", "none"), info
    nodes, lrefs = ctx.bvh()
    hn, hr, hi = bling_amd.host_lbvh(*items(job))
    assert same_bits(lrefs, hr) and same_bits(nodes.view(np.uint32), hn.view(np.uint32))
    si = ctx.scene_info()
    assert (si["prims"], si["bvh_depth"], si["bvh_leaves"], si["max_leaf"]) == (
        job.counts()["prims"], hi["depth"], hi["leaves"], hi["max_leaf"])
    # plan consistency: an all-LDS block stays within plan_lds4's budget at the size it launches with
    if si["lds_all4"] == 1:
        assert si["lds_trace4"] <= LDS4_BUDGET, si
        assert si["stack4_lds"] == si["stack4_need"] and si["lds4_nodes"] == si["bvh4_nodes"]
    else:
        assert si["stack4_lds"] <= si["stack4_need"] and si["lds4_nodes"] <= si["bvh4_nodes"]


def _counts(st):
    return (st.camera_samples, st.rays_camera, st.rays_continuation, st.rays_mis, st.rays_shadow, st.tiles)


@pytest.mark.parametrize("bvh", ["host", "device"])
@pytest.mark.parametrize("name", ["C1", "G"])
def test_every_device_of_a_fanout_gets_the_one_plan(ctx, scene_dir, monkeypatch, name, bvh):
    """Two contexts on device 0 (bling_create's test hook), each rendering every second tile from its own copy
    of the plan the first derived -- with bvh="device" over a tree the first device built -- against the single
    context: the same rays, and the film to float reordering.  cornell-box at 64 x 64, 2 x 2 samples, walks the
    all-LDS BVH4; G spills stack rows, so each peer's own stack4_lanes / stack4_ovf sizing is live.
    The bound is test_multidevice.py's: a pixel sums at most 4 samples x 25 filter taps = 100 identical terms
    in another order, 100 x 2^-24 = 6e-6 relative at the worst; the Mitchell filter's negative lobe can cancel,
    hence the absolute term.  An ordered, bit-equal film is not served on multi-device contexts."""
    from bling_amd.render import Context
    job = load_config("C1", "image=64,64") if name == "C1" else _job(scene_dir, name)
    assert (job.width, job.height, job.spp) == (64, 64, 4)
    ctx.upload(job, bvh=bvh)
    si = ctx.scene_info()
    if bvh == "host":                                         # the case's regime is stated for the SAH tree
        assert (si["stack4_need"] > si["stack4_lds"]) == (name == "G")
    f1, s1 = ctx.render_pass(seed=SEED, pass_index=0)
    monkeypatch.setenv("BLING_ALLOW_REPEATED_DEVICES", "1")
    multi = Context([0, 0])
    multi.upload(job, bvh=bvh)
    assert multi.scene_info() == si and multi.bvh_build_info()["used"] == bvh
    fm, sm = multi.render_pass(seed=SEED, pass_index=0)
    multi.close()
    assert _counts(sm) == _counts(s1)
    a, b = fm.reshape(-1, 4), f1.reshape(-1, 4)
    print(f"fan-out plan[{name}, {bvh}]: max abs diff {np.abs(a - b).max():.3e}")
    np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-5)
