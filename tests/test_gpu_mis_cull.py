"""The MIS cull on the device (wavefront.h mis_cull_test): a vertex whose sampled light is an area
light answers its BSDF-MIS query itself when that light's own shape rejects the ray.  On every scene
of tests/mis_cull_scenes.py the cull changes no result and no count, the counts are the oracle's, and
both outcomes of the cull occur.

"No result" is checked where results are reproducible.  Two passes of one scene never give
bit-equal films, with or without the cull: the film kernels sum their samples with floating-point
atomics, in an order that differs from run to run (measured on MI355X: two passes with the same
flags differ in 2 077 of cornell's 16 384 film words, by up to 1e-6 relative; before this change
too).  Each sample's radiance is formed by one thread in a fixed order, so the bit-for-bit check is
on every camera sample's 16-band spectrum (bling_sample_li with the context's cull switch off and
on), which says more than the film would; the films are compared to the bound of their summation.

Measured on MI355X (culled / rays_mis): cornell 75 594 / 76 094, ties 28 495 / 28 907, sphere
48 839 / 49 615, two 54 773 / 56 109, env 6 316 / 9 520, brute 22 321 / 24 285, packet 22 549 /
24 325, direct 6 627 / 10 040, shapes2 7 886 / 7 966.

`ties` holds thousands of exact ties of t per pass between a lamp and the coplanar ceiling, which
the device's walks and the oracle's kd-tree decide in different orders; both surfaces are black, so
the winner changes no count (tests/mis_cull_scenes.py), and the counts are held against the oracle's
like every other scene's.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mis_cull_scenes  # noqa: E402
from bling_amd import _ffi  # noqa: E402
from oracle_py import Oracle  # noqa: E402
from parity_util import random_samples, report  # noqa: E402

SEED = 0x0B11A6
PLAN = {"brute": lambda si: si["bf_prims"] == 16,
        "packet": lambda si: si["bf_prims"] == 0 and si["pkt_n"] > 0,
        "cornell": lambda si: si["bf_prims"] == 0 and si["pkt_n"] == 0 and si["lds_all4"] == 1}
# A film word is a sum of at most 100 terms (4 samples of each of the 5 x 5 source pixels whose
# Mitchell window covers it), none larger in magnitude than the largest sample value x weight, which
# the largest film word bounds up to the window's few negative lobes.  Summed in another order it
# moves by at most (n - 1) eps sum|terms| <= 99 x 2^-24 x 100 max|term| = 5.9e-4 max|film|.
FILM_ORDER_BOUND = 99 * 2.0 ** -24 * 100


@pytest.fixture(scope="module")
def ctx():
    from bling_amd.render import Context
    return Context(0)


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("mis_cull_scenes")


def _counts(st):
    return (st.camera_samples, st.rays_camera, st.rays_continuation, st.rays_mis, st.rays_shadow)


@pytest.mark.gpu
@pytest.mark.parametrize("name", mis_cull_scenes.NAMES)
def test_cull_changes_nothing_but_the_queue(ctx, scene_dir, name):
    job = mis_cull_scenes.build(scene_dir, name)
    ctx.upload(job)
    si = ctx.scene_info()
    if name in PLAN:
        assert PLAN[name](si), si
    f_on, st_on = ctx.render_pass(seed=SEED, pass_index=0)
    culled_on = ctx.mis_culled()
    f_off, st_off = ctx.render_pass(seed=SEED, pass_index=0, flags=_ffi.PASS_NO_MIS_CULL)
    culled_off = ctx.mis_culled()
    orc = Oracle(job)
    _, st_o = orc.render(seed=SEED, pass_index=0)
    oracle = (st_o.samples, st_o.rays_camera, st_o.rays_continuation, st_o.rays_mis, st_o.rays_shadow)
    # every band of every sample, bit for bit
    smp = random_samples(orc, job, 4096, seed=11)
    L_on, img_on, _ = ctx.sample_li(smp, seed=SEED, pass_index=0)
    ctx.set_mis_cull(False)
    try:
        L_off, img_off, _ = ctx.sample_li(smp, seed=SEED, pass_index=0)
    finally:
        ctx.set_mis_cull(True)
    words = int((L_on.view(np.uint32) != L_off.view(np.uint32)).sum())
    film_diff = float(np.abs(f_on - f_off).max() / np.abs(f_off).max())
    report(f"mis_cull[{name}]", culled=culled_on, culled_with_flag=culled_off, counts_on=_counts(st_on),
           counts_off=_counts(st_off), counts_oracle=oracle, vertices=(st_on.path_vertices, st_off.path_vertices),
           sample_words_differ=words, film_max_diff_rel=film_diff)
    assert words == 0 and np.array_equal(img_on, img_off)
    assert film_diff <= FILM_ORDER_BOUND
    assert _counts(st_on) == _counts(st_off)
    assert st_on.path_vertices == st_off.path_vertices
    assert culled_off == 0
    assert 0 < culled_on < st_on.rays_mis
    assert _counts(st_on) == oracle
