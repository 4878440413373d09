"""The timed launches of a render pass (BLING_PASS_KERNEL_TIMING: bling_stats' closest_launches,
shade_launches, ms_closest, ms_shade, with ms_bounce and ms_film) for every way core.hip's render()
runs a pass: one wave, several waves, two half-waves on two streams, DirectLighting and the normal map.
bench.py and the tools read these fields; the pass driver's event bookkeeping (core_internal.h
WaveTiming, core.hip wave_done) fills them.

The Path integrator times one closest-hit and one shade launch per depth 0 .. maxDepth of every wave, and
a pipelined pass is two waves' worth.  The scenes are the cornell and `two` rooms of
tests/mis_cull_scenes.py at 40 x 40 (nine tiles, maxDepth 5, 2 x 2 stratified), as in
tests/test_gpu_pipelined_waves.py.
"""
import ctypes as C
import math
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mis_cull_scenes  # noqa: E402
from bling_amd import _ffi  # noqa: E402
from bling_amd.render import Context  # noqa: E402
from bling_amd.scene import load_config, parse_job  # noqa: E402
from parity_util import report  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 0x0B11A6
DEPTH = 5
TIMED = _ffi.PASS_KERNEL_TIMING
TIMES = ("ms_total", "ms_bounce", "ms_film", "ms_closest", "ms_shade")
# Launch counts measured with this file on the commit before the pass driver was taken apart (they pin
# what it did, exactly): X4 at 24 x 18 is one wave whose DirectLighting walk takes 18 steps, each with one
# timed closest-hit launch and no timed shade launch; the normal map's fixture is one wave of one
# closest-hit launch and one k_shade_nm launch.
DIRECT_LAUNCHES = (18, 0)
NORMALS_LAUNCHES = (1, 1)


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    d = tmp_path_factory.mktemp("pass_timing_scenes")
    path = os.path.join(str(d), "timing_two_40.bling")
    with open(path, "w") as f:
        f.write(mis_cull_scenes._text("two", 40, DEPTH))
    return {"cornell": load_config("C1", f"image=40,40;stratified=2,2;path={DEPTH},3"), "two": parse_job(path)}


def _waves(ctx):
    """How bling_debug_pass_results says the last pass ran; it reports the waves also where it keeps no
    per-sample results (more than one wave)."""
    n, waves = C.c_size_t(), C.c_int()
    _ffi.hip().bling_debug_pass_results(ctx._h, None, 0, C.byref(n), C.byref(waves))
    return int(waves.value)


def _pass(ctx, tag, flags, chunk_paths=0):
    _, st = ctx.render_pass(seed=SEED, pass_index=0, flags=flags, chunk_paths=chunk_paths)
    waves = _waves(ctx)
    report(f"pass_timing[{tag}]", waves=waves, **st.as_dict())
    return st, waves


def _launches(st):
    return (st.closest_launches, st.shade_launches)


def _positive(st, names):
    for k in names:
        v = getattr(st, k)
        assert math.isfinite(v) and v > 0, (k, v)


@pytest.mark.parametrize("name", ["cornell", "two"])
def test_path_passes(ctx, jobs, name):
    ctx.upload(jobs[name])
    ctx.set_pipeline(-1)
    # the flag off: nothing timed
    st, waves = _pass(ctx, f"{name}:untimed", _ffi.PASS_NO_PIPELINE)
    assert waves == 1 and st.tiles == 9
    assert (st.ms_closest, st.ms_shade, st.closest_launches, st.shade_launches) == (0, 0, 0, 0)
    # one wave
    one, waves = _pass(ctx, f"{name}:one", TIMED | _ffi.PASS_NO_PIPELINE)
    assert waves == 1
    assert _launches(one) == (DEPTH + 1, DEPTH + 1)
    _positive(one, TIMES)
    # several waves
    st, waves = _pass(ctx, f"{name}:waves", TIMED | _ffi.PASS_NO_PIPELINE, chunk_paths=3072)
    assert waves > 1
    assert _launches(st) == (waves * (DEPTH + 1), waves * (DEPTH + 1))
    _positive(st, TIMES)
    # two half-waves on two streams
    ctx.set_pipeline(1)
    try:
        pair, waves = _pass(ctx, f"{name}:pair", TIMED)
    finally:
        ctx.set_pipeline(-1)
    assert waves == -2
    assert _launches(pair) == (2 * (DEPTH + 1), 2 * (DEPTH + 1))
    _positive(pair, TIMES)
    # pipelined equals single: every field that is not a time; each half-wave makes a wave's launches, so
    # the two timed counts are doubled, and so is bounce_launches (38 and 76 before the refactor as well)
    a, b = pair.as_dict(), one.as_dict()
    for k in a:
        if k in TIMES:
            continue
        doubled = k in ("closest_launches", "shade_launches", "bounce_launches")
        assert a[k] == (2 * b[k] if doubled else b[k]), (k, a[k], b[k])
    assert one.camera_samples > 0 and one.bounce_launches > 0 and one.path_vertices > 0


def test_direct_lighting_pass(ctx):
    ctx.upload(load_config("X4", "image=24,18"))
    st, waves = _pass(ctx, "direct:untimed", 0)
    assert waves == 1 and _launches(st) == (0, 0) and (st.ms_closest, st.ms_shade) == (0, 0)
    st, waves = _pass(ctx, "direct", TIMED)
    assert waves == 1
    assert _launches(st) == DIRECT_LAUNCHES
    _positive(st, ("ms_total", "ms_bounce", "ms_film", "ms_closest"))
    assert st.ms_shade == 0


def test_normal_map_pass(ctx):
    ctx.upload(load_config("N2"))
    st, waves = _pass(ctx, "normals:untimed", 0)
    assert waves == 1 and _launches(st) == (0, 0) and (st.ms_closest, st.ms_shade) == (0, 0)
    st, waves = _pass(ctx, "normals", TIMED)
    assert waves == 1
    assert _launches(st) == NORMALS_LAUNCHES
    _positive(st, TIMES)
