"""The device derivation (bling_scene_upload_with, BLING_UPLOAD_DERIVE_DEVICE; csrc/core/bvh_derive.hip): the BVH4,
the leaf records and the threaded list it leaves on the device against the host derivation of the same BVH2, byte
for byte, for both BVH builders; and everything downstream -- plans, hits, radiance, films, the CLI's files --
against the same scene uploaded with the host derivation.

Scenes come from tests/plan_scenes.py and tests/derive_scenes.py (no two triangles share an edge or a plane, so
exact ties have measure zero); the arrays are equal, so zero mismatches are required everywhere.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bling_amd  # noqa: E402
import plan_scenes  # noqa: E402
from bling_amd import _ffi  # noqa: E402
from bling_amd.render import BlingError, Context, host_camera_samples  # noqa: E402
from bling_amd.scene import load_config, parse_job  # noqa: E402
from derive_scenes import tree_scene  # noqa: E402
from plan_scenes import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 0x0B11A6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLING = os.path.join(ROOT, "bling_amd", "_lib", "bling")
f32 = np.float32
ARRAYS = ("nodes4", "leaf_geo", "pkt")


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("bvh_derive")


def same_derived(a, b):
    return all(same_bits(a[k].view(np.uint32), b[k].view(np.uint32)) for k in ARRAYS)


# ------------------------------------------------------------------ 1. / 2. the arrays
TREES = ["soup_3", "soup_5", "soup_12", "soup_40", "soup_64", "soup_65", "soup_257", "chain_24", "cell_200", "soup_20000"]


@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("name", TREES)
def test_device_derivation_equals_the_host_derivation(ctx, scene_dir, name, builder):
    """One BVH4 level (7 items), a frontier inside one wave, one across blocks (20 004 items), the deepest chain,
    Morton ties (200 items in one cell), SAH trees with one-item leaves and Morton trees."""
    job = parse_job(tree_scene(scene_dir, name))
    ctx.upload(job, bvh=builder, derive="host")
    assert ctx.bvh_build_info()["used"] == builder
    ih = ctx.derive_info()
    assert (ih["requested"], ih["used"], ih["fallback"]) == ("host", "host", "none")
    want, tree, plan = ctx.derived(), ctx.bvh(), ctx.scene_info()
    ctx.upload(job, bvh=builder, derive="device")
    assert ctx.bvh_build_info()["used"] == builder
    info = ctx.derive_info()
    assert (info["requested"], info["used"], info["fallback"]) == ("device", "device", "none"), info
    got, tree_d = ctx.derived(), ctx.bvh()
    print(f"derive[{name}, {builder}] n2={len(tree[0])} n4={info['bvh4_nodes']} depth4={info['bvh4_depth']} "
          f"stack={info['stack_need']} levels={info['level_launches']} ms_device={info['ms_derive_device']:.3f} "
          f"ms_plan_host={info['ms_plan_host']:.3f} host path ms={ih['ms_plan_host']:.3f}")
    for k in ARRAYS:
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        assert same_bits(got[k].view(np.uint32), want[k].view(np.uint32)), k
    assert same_bits(tree[0].view(np.uint32), tree_d[0].view(np.uint32)) and same_bits(tree[1], tree_d[1])
    assert ctx.scene_info() == plan
    assert {k: info[k] for k in ("bvh4_nodes", "bvh4_depth", "stack_need")} == {k: ih[k] for k in ("bvh4_nodes", "bvh4_depth", "stack_need")}
    assert len(got["leaf_geo"]) == 3 * (len(tree[1]) + 1) and len(got["nodes4"]) == plan["bvh4_nodes"]
    n4, i4 = bling_amd.host_bvh4(tree_d[0])
    assert same_bits(got["nodes4"].view(np.uint32), n4.view(np.uint32))
    assert (i4["depth"], max(1, i4["stack_need"])) == (plan["bvh4_depth"], plan["stack4_need"])
    if plan["pkt_n"]:
        assert same_bits(got["pkt"].view(np.uint32), bling_amd.host_threaded(tree_d[0]).view(np.uint32))
    # 2. reproducible: a second upload gives the same bytes
    ctx.upload(job, bvh=builder, derive="device")
    assert same_derived(ctx.derived(), got)


# ------------------------------------------------------------------ 3. same hits and radiance
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


@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("plan,n_tris,brute", [("brute", 12, None), ("packet", 5, "0"), ("lds_all4", 40, None),
                                               ("global", 257, None)])
def test_same_hits_and_radiance_on_both_derivations(ctx, scene_dir, monkeypatch, plan, n_tris, brute, builder):
    """Closest and any-hit of the 16 x 16 image's camera rays and 4 096 random rays, sample_li over the image and an
    ordered film: bit-equal between the two derivations, on a scene of each traversal plan.  The arrays are equal
    (above), so this pins the upload's wiring: pointers, sizes, plans."""
    if brute is not None:
        monkeypatch.setenv("BLING_BRUTE", brute)
    job = parse_job(plan_scenes.soup(scene_dir, n_tris, 4), "image=16,16")
    rays = all_rays(job)
    x0, x1, y0, y1 = job.extent()
    smp = np.array([(x, y, n) for y in range(y0, y1 + 1) for x in range(x0, x1 + 1) for n in range(job.spp)], np.int32)
    got = {}
    for dv in ("host", "device"):
        ctx.upload(job, bvh=builder, derive=dv)
        assert ctx.derive_info()["used"] == dv
        assert plan_of(ctx.scene_info()) == plan, (dv, ctx.scene_info())
        hits = [ctx.trace(rays, any_hit=a) for a in (False, True)]
        L, _, _ = ctx.sample_li(smp, seed=SEED, pass_index=1)
        film, _ = ctx.render_pass(seed=SEED, pass_index=1, ordered=True)
        got[dv] = (hits, L, film)
    for a in range(2):
        for k, what in enumerate(("t", "prim", "bary")):
            h, d = got["host"][0][a][k], got["device"][0][a][k]
            bad = int((h.view(np.uint32) != d.view(np.uint32)).reshape(len(h), -1).any(1).sum())
            print(f"hits[{plan}, {builder}] any={a} {what}: {bad} of {len(h)} rays differ")
            assert bad == 0
    assert (got["host"][0][0][1] != 0xFFFFFFFF).mean() > 0.3          # the rays do hit the scene
    assert np.isfinite(got["host"][1]).all() and (got["host"][1] != 0).any()
    assert same_bits(got["host"][1].view(np.uint32), got["device"][1].view(np.uint32))
    assert same_bits(got["host"][2].view(np.uint32), got["device"][2].view(np.uint32))


# ------------------------------------------------------------------ 4. standing down
def test_fractal_scene_keeps_the_host_derivation(ctx):
    job = load_config("C5", "image=16,16")
    ctx.upload(job)
    want = ctx.derived()
    ctx.upload(job, derive="device")
    info = ctx.derive_info()
    assert (info["requested"], info["used"], info["fallback"]) == ("device", "host", "fractal")
    assert same_derived(ctx.derived(), want)


def one_add_per_pixel_scene(dirname):
    """soup(65, 4) with the box filter (half a pixel wide) and one stratified sample per pixel: every film pixel
    receives exactly one contribution, so the film of a pass does not depend on the order the float atomics of a
    multi-device pass land in, and two passes over the same device state give the same bits."""
    text = open(plan_scenes.soup(dirname, 65, 4)).read()
    assert "filter mitchell 2 2 0.333333 0.333333" in text and "stratified 2 2" in text
    text = text.replace("filter mitchell 2 2 0.333333 0.333333", "filter box").replace("stratified 2 2", "stratified 1 1")
    return plan_scenes._write(dirname, "soup_65_box_1spp", text)


def test_multi_device_context_keeps_the_host_derivation(scene_dir, monkeypatch):
    """Two contexts on one GPU (bling_create's test hook): the peers receive the host's plan, as before, and the
    pass's film equals the derive="host" film of the same context bit for bit."""
    monkeypatch.setenv("BLING_ALLOW_REPEATED_DEVICES", "1")
    job = parse_job(one_add_per_pixel_scene(scene_dir), "image=16,16")
    multi = Context([0, 0])
    try:
        films, state = {}, {}
        for dv in ("host", "device"):
            multi.upload(job, bvh="device", derive=dv)
            info = multi.derive_info()
            assert (info["requested"], info["used"]) == (dv, "host")
            assert info["fallback"] == ("devices" if dv == "device" else "none")
            state[dv] = (multi.derived(), multi.bvh(), multi.scene_info())
            films[dv], _ = multi.render_pass(seed=SEED, pass_index=2)
    finally:
        multi.close()
    assert same_derived(state["host"][0], state["device"][0]) and state["host"][2] == state["device"][2]
    assert same_bits(state["host"][1][0].view(np.uint32), state["device"][1][0].view(np.uint32))
    assert same_bits(state["host"][1][1], state["device"][1][1])
    assert np.isfinite(films["host"]).all() and (films["host"] != 0).any()
    assert same_bits(films["host"].view(np.uint32), films["device"].view(np.uint32))


# ------------------------------------------------------------------ 5. refusals
def test_unknown_flags_and_small_capacities(ctx, scene_dir):
    job = parse_job(plan_scenes.soup(scene_dir, 5, 4))
    fresh = Context(0)
    try:
        up = _ffi.UploadParams(_ffi.BVH_BUILDERS["device"], 2)
        assert _ffi.hip().bling_scene_upload_with(fresh._h, C.c_void_p(job.desc), C.byref(up)) == -1      # BLING_EINVAL
        up = _ffi.UploadParams(_ffi.BVH_BUILDERS["host"], 3)
        assert _ffi.hip().bling_scene_upload_with(fresh._h, C.c_void_p(job.desc), C.byref(up)) == -1
        with pytest.raises(BlingError):                        # the context keeps no scene
            fresh.derive_info()
        with pytest.raises(BlingError):
            fresh.derived()
    finally:
        fresh.close()
    with pytest.raises(ValueError):
        ctx.upload(job, derive="gpu")
    ctx.upload(job, bvh="device", derive="device")
    d = ctx.derived()
    assert all(len(d[k]) > 0 for k in ARRAYS)
    sizes = [len(d[k]) for k in ARRAYS]
    n = [C.c_size_t(), C.c_size_t(), C.c_size_t()]
    for short in range(3):                                         # one capacity one short, the others exact
        bufs = [np.full((sizes[j], w), 7, f32) for j, w in enumerate((28, 4, 8))]
        caps = [sizes[j] - (1 if j == short else 0) for j in range(3)]
        rc = _ffi.hip().bling_debug_derived(ctx._h, _ffi.f32ptr(bufs[0]), caps[0], _ffi.f32ptr(bufs[1]), caps[1],
                                            _ffi.f32ptr(bufs[2]), caps[2], C.byref(n[0]), C.byref(n[1]), C.byref(n[2]))
        assert rc == -1 and [int(x.value) for x in n] == sizes
        assert all((b == 7).all() for b in bufs)


# ------------------------------------------------------------------ 6. default untouched
def test_default_upload_is_the_host_derivation(ctx, scene_dir):
    job = parse_job(plan_scenes.soup(scene_dir, 65, 4))
    ctx.upload(job)
    a, ia, da = ctx.derived(), ctx.scene_info(), ctx.derive_info()
    ctx.upload(job, derive="host")
    b, ib = ctx.derived(), ctx.scene_info()
    assert same_derived(a, b) and ia == ib
    assert (da["requested"], da["used"], da["fallback"], da["level_launches"]) == ("host", "host", "none", 0)


# ------------------------------------------------------------------ 7. CLI
def test_cli_derive_device(scene_dir, tmp_path):
    path = plan_scenes.soup(scene_dir, 64, 4)
    runs = {}
    for tag, extra in (("host", []), ("device", ["--derive", "device"])):
        out = str(tmp_path / tag)
        r = subprocess.run([BLING, path, "--passes", "1", "--film", "ordered", "--bvh", "device", "--out", out] + extra,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        runs[tag] = (open(out + "-00001.hdr", "rb").read(), open(out + "-00001.png", "rb").read(), r.stdout)
    assert runs["host"][0] == runs["device"][0] and runs["host"][1] == runs["device"][1]
    line = [l for l in runs["device"][2].splitlines() if l.startswith("derive: ")]
    assert len(line) == 1 and line[0].startswith("derive: device, ") and "BVH4 nodes" in line[0], runs["device"][2]
    assert not any(l.startswith("derive: ") for l in runs["host"][2].splitlines())
    bad = subprocess.run([BLING, path, "--derive", "gpu"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--derive takes host or device" in bad.stderr
