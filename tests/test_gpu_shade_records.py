"""The shading kernel's path-state records (wavefront.h PathSet / Est): the BSDF-MIS ray's records
(mdir, mhit, fm) are loaded only by the lanes whose vertex has such a ray (the factored profile,
while the MIS cull is on; eager otherwise), and the factored profile
keeps one scalar record per vertex (fac = s1c, s1, s2, w / pdf) beside the 4-B lobe offset (rtex); the
Russian-roulette pc comes from |dir.w|.  Only where a value is stored changed, so every camera
sample's 16-band spectrum (bling_sample_li) must equal the oracle's bit for bit, and every ray count
exactly, on scenes of 48 x 48 built from the generators of tests/mis_cull_scenes.py:

  open       a one-lamp room of triangles (the factored profile); the lamp hangs just below the
             ceiling, so some BSDF-sampled rays reach it and most are culled: surviving MIS vertices
             share 64-entry chunks with culled ones.  maxDepth 12: Russian roulette (depth > 7) makes
             pc != 1.  Run with the cull on and off (every vertex then takes the VF_MIS path).
  coplanar   the same with the lamp in the plane of the (black) ceiling triangles
  orennayar  Oren-Nayar lobes (sigma > 0: s1 != 1 / pi, s2 != 1), coloured and white reflectances.
             A white matte material (kd 1 1 1) is a texture like any other and gets a real lobe
             offset; the offset ~0u is stored only for a vertex whose BSDF has no lobe, which no
             material of the factored profile produces, so lobe_r's ~0u branch is not reached by any
             scene and is not exercised here either.
  direct     `open` under the directLighting integrator (k_shade_dl / k_resolve)
  plastic    `open` with a plastic block: a spectral profile, whose records are untouched

Checked on the CPU (test_shade_record_scenes_on_the_oracle): the factored scenes resolve to the
factored profile, no sample is dropped, and BSDF-sampled rays reach the lamp of `open` / `coplanar`
(MIS rays that hit it: the vertices the cull must keep).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mis_cull_scenes as mcs  # noqa: E402
from bling_amd.scene import parse_job  # noqa: E402
from oracle_py import Oracle  # noqa: E402
from parity_util import random_samples, report  # noqa: E402

SEED = 0x0B11A6
FT_FACTORED = (1 << 0) | (1 << 6) | (1 << 12)      # matte | area lights | triangles (wavefront.h factored())
K = 4096

WHITE_ON = "material { matte kd { constant rgbR 1 1 1 } sigma { constant 0.4 } }\n"
BLUE_ON = "material { matte kd { constant rgbR 0.15 0.25 0.8 } sigma { constant 0.6 } }\n"
PLASTIC = "material { plastic kd { constant rgbR 0.7 0.2 0.2 } ks { constant rgbR 0.4 0.4 0.4 } rough { constant 0.02 } }\n"
OPEN_LAMP = mcs._lamp("rotateX -90 translate 0 2.99 1", "quad 1.2 0.9")
# a second block on the floor, left of the first
BLOCK2 = (mcs._quad_mesh((-2.6, -1.8, 1.5), (-1.2, -1.8, 2.0), (-1.7, -1.8, 3.3), (-3.1, -1.8, 2.8)) +
          mcs._quad_mesh((-2.6, -3, 1.5), (-1.2, -3, 2.0), (-1.2, -1.8, 2.0), (-2.6, -1.8, 1.5)))
NAMES = ["open", "coplanar", "orennayar", "direct", "plastic"]
FACTORED = {"open", "coplanar", "orennayar", "direct"}


def _text(name):
    head = mcs.HEADER.format(tag="shade_records_" + name, size=48, depth=12)
    if name == "coplanar":
        return head + mcs._room_meshes(mcs.BLACK) + mcs.TIES_LAMP
    if name == "orennayar":
        return head + mcs._room_meshes() + WHITE_ON + BLOCK2 + BLUE_ON + \
            mcs._quad_mesh((-0.5, -2.2, 0), (0.6, -2.2, 0.3), (0.3, -2.2, 1.2), (-0.8, -2.2, 0.9)) + OPEN_LAMP
    if name == "direct":
        return head.replace("path maxDepth 12 sampleDepth 3", "directLighting maxDepth 5") + mcs._room_meshes() + OPEN_LAMP
    if name == "plastic":
        return head + mcs._room_meshes() + PLASTIC + BLOCK2 + OPEN_LAMP
    assert name == "open"
    return head + mcs._room_meshes() + OPEN_LAMP


def build(dirname, name):
    path = os.path.join(str(dirname), f"shade_records_{name}.bling")
    with open(path, "w") as f:
        f.write(_text(name))
    return parse_job(path)


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("shade_record_scenes")


@pytest.fixture(scope="module")
def oracle_runs(built, scene_dir):
    """name -> (job, samples, L, img, stats) of the oracle, computed once."""
    out = {}
    for name in NAMES:
        job = build(scene_dir, name)
        orc = Oracle(job)
        smp = random_samples(orc, job, K, seed=11)
        L, img, st = orc.sample_li_batch(smp, seed=SEED, pass_index=0)
        out[name] = (job, smp, L, img, st)
    return out


def _counts_o(st):
    return (int(st.samples), int(st.rays_camera), int(st.rays_continuation), int(st.rays_mis), int(st.rays_shadow))


def _counts_g(st):
    return (int(st.camera_samples), int(st.rays_camera), int(st.rays_continuation), int(st.rays_mis), int(st.rays_shadow))


def test_shade_record_scenes_on_the_oracle(oracle_runs, scene_dir):
    for name in NAMES:
        job, smp, L, _, st = oracle_runs[name]
        feats = job.counts()["features"]
        assert job.width == 48 and job.height == 48 and job.spp == 4
        assert ((feats & ~FT_FACTORED) == 0) == (name in FACTORED), (name, hex(feats))
        assert job.counts()["lights"] == 1
        # 1 = BLING_INTEGRATOR_DIRECT, 0 = BLING_INTEGRATOR_PATH (include/bling_scene.h)
        assert job.config.integrator == (1 if name == "direct" else 0), (name, job.config.integrator)
        assert job.config.max_depth == (5 if name == "direct" else 12)
        print(f"shade_records[{name}] counts={_counts_o(st)} dropped={st.dropped} lit={(L.sum(1) > 0).mean():.3f}")
        assert st.dropped == 0 and np.isfinite(L).all()
        assert st.rays_mis > 0 and st.rays_shadow > 0 and (L.sum(1) > 0).mean() > 0.5
    # BSDF-sampled rays that reach the lamp: cosine-distributed directions from points of the floor,
    # traced by the oracle; a ray whose closest hit lies on the lamp's rectangle (x in [-1.2, 1.2],
    # z in [0.1, 1.9], nothing else is there) passes the lamp's own test, so its vertex keeps its MIS ray
    for name in ("open", "coplanar"):
        job = oracle_runs[name][0]
        rng = np.random.default_rng(5)
        n = 20000
        o = np.stack([rng.uniform(-3.9, 3.9, n), np.full(n, -2.99), rng.uniform(-6.9, 5.9, n)])
        u1, u2 = rng.uniform(0, 1, n), rng.uniform(0, 2 * np.pi, n)
        d = np.stack([np.sqrt(u1) * np.cos(u2), np.sqrt(1 - u1), np.sqrt(u1) * np.sin(u2)])
        rays = np.concatenate([o, d, np.full((1, n), 1e-3), np.full((1, n), np.inf)]).astype(np.float32)
        t, _, _, _ = Oracle(job).trace(rays)
        hit = (o + d * t).T[np.isfinite(t)]
        reach = int(((hit[:, 1] > 2.98) & (np.abs(hit[:, 0]) < 1.2) & (np.abs(hit[:, 2] - 1.0) < 0.9)).sum())
        print(f"shade_records[{name}] floor rays reaching the lamp: {reach} of {n}")
        assert 0 < reach < n // 2


def _device_vs_oracle(ctx, run, tag):
    job, smp, Lo, img_o, st_o = run
    Lg, img_g, st_g = ctx.sample_li(smp, seed=SEED, pass_index=0)
    words = int((Lg.view(np.uint32) != Lo.view(np.uint32)).sum())
    report(f"shade_records[{tag}]", sample_words_differ=words, counts_gpu=_counts_g(st_g), counts_oracle=_counts_o(st_o),
           dropped_gpu=int(st_g.dropped_samples), dropped_oracle=int(st_o.dropped))
    assert np.array_equal(img_g, img_o)
    assert words == 0
    assert _counts_g(st_g) == _counts_o(st_o)
    assert st_g.dropped_samples == 0 and st_o.dropped == 0
    return Lg


@pytest.fixture(scope="module")
def ctx():
    from bling_amd.render import Context
    return Context(0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["open", "coplanar"])
def test_mixed_waves_cull_on_and_off(ctx, oracle_runs, name):
    """Case 1: surviving and culled MIS vertices in the same chunks; pc != 1 beyond depth 7."""
    job = oracle_runs[name][0]
    ctx.upload(job)
    _, st = ctx.render_pass(seed=SEED, pass_index=0)
    culled = ctx.mis_culled()
    report(f"shade_records[{name}] pass", rays_mis=int(st.rays_mis), culled=culled)
    assert 0 < culled < st.rays_mis                      # both kinds of vertex occur
    L_on = _device_vs_oracle(ctx, oracle_runs[name], name + ",cull on")
    ctx.set_mis_cull(False)
    try:
        L_off = _device_vs_oracle(ctx, oracle_runs[name], name + ",cull off")
    finally:
        ctx.set_mis_cull(True)
    assert np.array_equal(L_on.view(np.uint32), L_off.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["orennayar", "direct", "plastic"])
def test_records_keep_every_sample(ctx, oracle_runs, name):
    """Cases 2-4: field mix-ups in the merged record, the DirectLighting kernels, a spectral profile."""
    ctx.upload(oracle_runs[name][0])
    _device_vs_oracle(ctx, oracle_runs[name], name)
