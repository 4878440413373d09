"""The device BVH builder (bling_scene_upload_with, BLING_BVH_DEVICE; csrc/core/bvh_device.hip): its tree
against the CPU restatement bling_host_lbvh bit for bit, and everything downstream of the tree -- hits,
radiance, films, the CLI's files -- against the same scene uploaded with the host's SAH tree.

Scenes come from tests/plan_scenes.py (no two triangles share an edge or a plane, so exact ties have
measure zero and zero mismatches are required); the items are plan_scenes.prim_boxes and the refs
(kind << 30 | index) in primitive order, as scene_plan.cpp scene_items forms them.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bling_amd  # noqa: E402
import plan_scenes  # noqa: E402
from plan_scenes import items, same_bits  # noqa: E402
from bling_amd.render import BlingError, Context, host_camera_samples  # noqa: E402
from bling_amd.scene import load_config, parse_job  # noqa: E402
from scene_desc import desc  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 0x0B11A6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLING = os.path.join(ROOT, "bling_amd", "_lib", "bling")
f32 = np.float32


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("bvh_device")


def cell_scene(dirname):
    """200 small triangles whose centres share one Morton cell (the light and the backdrop span the grid)."""
    rng = np.random.default_rng(21)
    out = [plan_scenes.HEADER.format(tag="cell", fov=plan_scenes.FOV), plan_scenes._light_and_backdrop(18.0)]
    for k in range(200):
        c = np.array([0.3, 0.2, 14.0]) + rng.uniform(0, 1e-3, 3)
        pts = [tuple(c + rng.uniform(-0.05, 0.05, 3)) for _ in range(3)]
        out.append(plan_scenes._matte(k) + plan_scenes._mesh(pts))
    return plan_scenes._write(dirname, "cell_200", "".join(out))


def tree_scene(dirname, name):
    kind, n = name.split("_")
    if kind == "soup":
        return plan_scenes.soup(dirname, int(n), 4)
    if kind == "chain":
        return plan_scenes.chain(dirname, int(n))
    return cell_scene(dirname)


# ------------------------------------------------------------------ 5. / 6. the tree itself
TREES = ["soup_3", "soup_5", "soup_64", "soup_65", "soup_257", "chain_24", "soup_20000", "cell_200"]


@pytest.mark.parametrize("name", TREES)
def test_device_tree_equals_the_host_restatement(ctx, scene_dir, name):
    """One wave (7 items), one block (up to 1024), the multi-block sort (above), the many-block histogram
    and scan (20 004 items), a chain, and 200 items in one Morton cell (split on the index bits)."""
    job = parse_job(tree_scene(scene_dir, name))
    boxes, refs = items(job)
    ctx.upload(job, bvh="device")
    info = ctx.bvh_build_info()
    assert (info["requested"], info["used"], info["fallback"]) == ("device", "device", "none"), info
    nodes, lrefs = ctx.bvh()
    hn, hr, hi = bling_amd.host_lbvh(boxes, refs)
    assert same_bits(lrefs, hr)
    assert same_bits(nodes.view(np.uint32), hn.view(np.uint32))
    assert {k: info[k] for k in ("items", "nodes", "depth", "leaves", "max_leaf")} == hi
    si = ctx.scene_info()
    assert (si["bvh_depth"], si["bvh_leaves"], si["max_leaf"]) == (hi["depth"], hi["leaves"], hi["max_leaf"])
    print(f"lbvh[{name}] items={hi['items']} nodes={hi['nodes']} depth={hi['depth']} ms_build={info['ms_build']:.3f} "
          f"ms_derive={info['ms_derive']:.3f}")
    # 6. reproducible: a second upload gives the same bytes
    ctx.upload(job, bvh="device")
    nodes2, lrefs2 = ctx.bvh()
    assert same_bits(nodes, nodes2) and same_bits(lrefs, lrefs2)


# ------------------------------------------------------------------ 7. same hits
def plan_of(si):
    if si["bf_prims"] > 0:
        return "brute"
    if si["pkt_n"] > 0:
        return "packet"
    return "lds_all4" if si["lds_all4"] else "global"


def all_rays(job):
    _, _, rays, _ = host_camera_samples(job, [(0, job.width - 1, 0, job.height - 1)], seed=SEED, outputs=("rays",))
    cam = np.concatenate([rays, np.full((1, rays.shape[1]), np.inf, f32)], 0)
    lo, hi = plan_scenes.scene_bounds(job)
    rng = np.random.default_rng(77)
    o = rng.uniform(lo, hi, (4096, 3)).astype(f32)
    d = rng.normal(size=(4096, 3)).astype(f32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rnd = np.concatenate([o.T, d.T, np.zeros((1, 4096), f32), np.full((1, 4096), np.inf, f32)], 0).astype(f32)
    return np.ascontiguousarray(np.concatenate([cam, rnd], 1))


@pytest.mark.parametrize("plan,n_tris,brute", [("brute", 12, None), ("packet", 5, "0"), ("lds_all4", 40, None),
                                               ("global", 257, None)])
def test_same_hits_on_both_trees(ctx, scene_dir, monkeypatch, plan, n_tris, brute):
    """Closest and any-hit of the 64 x 64 image's camera rays and 4 096 random rays: t, prim and bary bit-equal
    between the device-built and the host-built upload, on a scene of each traversal plan (the packet walk is
    reached with the exhaustive kernels switched off, BLING_BRUTE=0, on a scene of 9 primitives)."""
    if brute is not None:
        monkeypatch.setenv("BLING_BRUTE", brute)
    job = parse_job(plan_scenes.soup(scene_dir, n_tris, 4))
    rays = all_rays(job)
    got = {}
    for b in ("host", "device"):
        ctx.upload(job, bvh=b)
        assert ctx.bvh_build_info()["used"] == b
        assert plan_of(ctx.scene_info()) == plan, (b, ctx.scene_info())
        got[b] = [ctx.trace(rays, any_hit=a) for a in (False, True)]
    for a in range(2):
        for k, what in enumerate(("t", "prim", "bary")):
            h, d = got["host"][a][k], got["device"][a][k]
            bad = int((h.view(np.uint32) != d.view(np.uint32)).reshape(len(h), -1).any(1).sum())
            print(f"hits[{plan}] any={a} {what}: {bad} of {len(h)} rays differ")
            assert bad == 0
    assert (got["host"][0][1] != 0xFFFFFFFF).mean() > 0.3          # the rays do hit the scene


# ------------------------------------------------------------------ 8. same radiance
def test_same_radiance_on_both_trees(ctx, scene_dir):
    job = parse_job(plan_scenes.soup(scene_dir, 64, 4), "image=16,16")
    x0, x1, y0, y1 = job.extent()
    smp = np.array([(x, y, n) for y in range(y0, y1 + 1) for x in range(x0, x1 + 1) for n in range(job.spp)], np.int32)
    out = {}
    for b in ("host", "device"):
        ctx.upload(job, bvh=b)
        L, _, _ = ctx.sample_li(smp, seed=SEED, pass_index=1)
        film, _ = ctx.render_pass(seed=SEED, pass_index=1, ordered=True)
        out[b] = (L, film)
    assert np.isfinite(out["host"][0]).all() and (out["host"][0] != 0).any()
    assert same_bits(out["host"][0].view(np.uint32), out["device"][0].view(np.uint32))
    assert same_bits(out["host"][1].view(np.uint32), out["device"][1].view(np.uint32))


# ------------------------------------------------------------------ 9. standing down
def test_fractal_scene_keeps_the_host_tree(ctx):
    job = load_config("C5", "image=16,16")
    ctx.upload(job)
    want = ctx.bvh()
    ctx.upload(job, bvh="device")
    info = ctx.bvh_build_info()
    assert (info["requested"], info["used"], info["fallback"]) == ("device", "host", "fractal")
    got = ctx.bvh()
    assert same_bits(want[0], got[0]) and same_bits(want[1], got[1])


def test_depth_cap_falls_back_to_the_host_tree(ctx, scene_dir):
    job = parse_job(plan_scenes.chain(scene_dir, 24))
    ctx.upload(job)
    want = ctx.bvh()
    ctx.upload(job, bvh="device")
    depth = ctx.bvh_build_info()["depth"]
    try:
        ctx.set_bvh_depth_cap(depth - 1)
        ctx.upload(job, bvh="device")
        info = ctx.bvh_build_info()
        assert (info["used"], info["fallback"]) == ("host", "depth")
        got = ctx.bvh()
        assert same_bits(want[0], got[0]) and same_bits(want[1], got[1])
        ctx.set_bvh_depth_cap(depth)
        ctx.upload(job, bvh="device")
        assert ctx.bvh_build_info()["used"] == "device"
    finally:
        ctx.set_bvh_depth_cap(0)
    with pytest.raises(BlingError):
        ctx.set_bvh_depth_cap(32)


def test_bad_builder_and_small_capacities(ctx, scene_dir):
    import ctypes as C
    from bling_amd import _ffi
    job = parse_job(plan_scenes.soup(scene_dir, 5, 4))
    with pytest.raises(BlingError) as e:
        ctx.upload(job, bvh=2)
    assert e.value.rc == -1                                     # BLING_EINVAL
    ctx.upload(job, bvh="device")
    nodes, refs = ctx.bvh()
    nn, nr = C.c_size_t(), C.c_size_t()
    small_n = np.full((max(1, len(nodes) - 1), 16), 7, f32)
    small_r = np.full(len(refs), 7, np.uint32)
    rc = _ffi.hip().bling_debug_bvh(ctx._h, _ffi.f32ptr(small_n), len(nodes) - 1, _ffi.u32ptr(small_r), len(refs), C.byref(nn),
                                    C.byref(nr))
    assert rc == -1 and (nn.value, nr.value) == (len(nodes), len(refs))
    assert (small_n == 7).all() and (small_r == 7).all()


# ------------------------------------------------------------------ 10. default untouched
def test_default_upload_is_the_host_builder(ctx, scene_dir):
    job = parse_job(plan_scenes.soup(scene_dir, 65, 4))
    ctx.upload(job)
    a, ia, ba = ctx.bvh(), ctx.scene_info(), ctx.bvh_build_info()
    ctx.upload(job, bvh="host")
    b, ib = ctx.bvh(), ctx.scene_info()
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and ia == ib
    assert (ba["requested"], ba["used"], ba["fallback"]) == ("host", "host", "none")


def test_multi_device_context_builds_once(scene_dir, monkeypatch):
    """Two contexts on one GPU (bling_create's test hook): the peers receive the tree built on the first device.
    Same sample contributions, summed by float atomics in another order: the tolerance of test_multidevice.py."""
    monkeypatch.setenv("BLING_ALLOW_REPEATED_DEVICES", "1")
    job = parse_job(plan_scenes.soup(scene_dir, 65, 4))
    one = Context(0)
    one.upload(job, bvh="device")
    f1, s1 = one.render_pass(seed=SEED, pass_index=2)
    one.close()
    multi = Context([0, 0])
    multi.upload(job, bvh="device")
    assert multi.bvh_build_info()["used"] == "device"
    fm, sm = multi.render_pass(seed=SEED, pass_index=2)
    multi.close()
    assert sm.camera_samples == s1.camera_samples and sm.rays() == s1.rays()
    np.testing.assert_allclose(fm, f1, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------ 11. CLI
def test_cli_bvh_device(scene_dir, tmp_path):
    path = plan_scenes.soup(scene_dir, 64, 4)
    runs = {}
    for tag, extra in (("host", []), ("device", ["--bvh", "device"])):
        out = str(tmp_path / tag)
        r = subprocess.run([BLING, path, "--passes", "1", "--film", "ordered", "--out", out] + extra, capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        runs[tag] = (open(out + "-00001.hdr", "rb").read(), r.stdout)
    assert runs["host"][0] == runs["device"][0]
    line = [l for l in runs["device"][1].splitlines() if l.startswith("bvh: ")]
    assert len(line) == 1 and "builder device, 68 items" in line[0] and "depth" in line[0] and " ms" in line[0], runs["device"][1]
    assert not any(l.startswith("bvh: ") for l in runs["host"][1].splitlines())
    bad = subprocess.run([BLING, path, "--bvh", "gpu"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--bvh takes host or device" in bad.stderr
