"""The sampler and camera seam on the host (bling_host_camera_samples, include/bling_host.h): the samples and
camera rays of SampleWindows against the oracle's camera_ray and the stream ids, the window algebra, cut calls,
the refusals, the ABI of the new stats struct and the host-only link.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from bling_amd import _ffi
from bling_amd.render import host_camera_samples
from bling_amd.scene import SCENES, load_config, parse_job
from camera_samples_cases import CASES, algebra_windows, block, case_job, counts_of, host, same_bits, window_samples
from oracle_py import Oracle
from surface_li_cases import SEED, bits, c1, camera_rays, stream_ids, windows_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "bling_amd", "_lib")


# ------------------------------------------------------------------ 1. host against the oracle
@pytest.mark.parametrize("name,pass_index", CASES)
def test_host_equals_the_oracle(built, name, pass_index, tmp_path):
    job = case_job(name, tmp_path)
    samples, windows, counts = windows_of(job)
    if name == "c1":
        assert len(samples) == 1764 and job.spp == 4
    if name == "strat32":
        assert job.spp == 6
    got = host(job, windows, pass_index)
    assert np.array_equal(samples, window_samples(windows, job.spp))
    rays, xy = camera_rays(Oracle(job), samples, pass_index=pass_index)
    assert got["rays"].shape == rays.shape and not bits(got["rays"][6]).any()
    assert np.array_equal(bits(got["rays"]), bits(rays))
    assert np.array_equal(bits(got["xy"]), bits(xy))
    assert np.array_equal(got["ids"], stream_ids(job, samples))
    lens = got["lens"]
    assert ((lens >= 0) & (lens < 1)).all() and len(np.unique(lens)) > len(lens)
    # the outputs do not depend on which of them are asked for
    for outs in (("rays",), ("xy", "ids"), ("lens",)):
        part = host(job, windows, pass_index, outputs=outs)
        assert all((part[k] is not None) == (k in outs) for k in part) and same_bits(part, got)


def test_a_pinhole_ignores_the_lens_sample(built):
    """lensRadius 0: the rays are a function of imageX, imageY alone -- fireRay with any lens sample gives them."""
    import oracle_py
    job = c1("image=16,16")
    _, windows, _ = windows_of(job)
    got = host(job, windows)
    orc = Oracle(job)
    o = got["rays"][:3]
    assert (bits(o) == bits(o[:, :1])).all()                   # one origin: the lens sample moved nothing
    r = np.zeros(6, np.float32)
    for i in range(0, len(got["xy"]), 97):
        x, y = (float(v) for v in got["xy"][i])
        for lu, lv in ((0.0, 0.0), (0.9, 0.05), tuple(float(v) for v in got["lens"][i])):
            oracle_py.lib().oracle_fire_ray_probe(orc.h, x, y, lu, lv, r.ctypes.data_as(C.POINTER(C.c_float)))
            assert np.array_equal(bits(r), bits(got["rays"][:6, i])), (i, lu, lv)


# ------------------------------------------------------------------ 2. window algebra
def test_every_windows_block_is_that_window_alone(built):
    job = c1("image=16,16;stratified=3,2")
    windows = algebra_windows(job)
    counts = counts_of(windows, job.spp)
    first = np.concatenate([[0], np.cumsum(counts)])
    n = int(first[-1])
    whole = host(job, windows)
    assert counts.count(0) == 2 and min(c for c in counts if c) == job.spp and len(whole["xy"]) == n
    assert np.array_equal(whole["ids"], stream_ids(job, window_samples(windows, job.spp)))
    alone = {}
    for k, w in enumerate(windows):
        if w not in alone:
            alone[w] = host(job, [w])
        assert same_bits(block(whole, int(first[k]), int(first[k + 1]), n), block(alone[w], 0, counts[k], counts[k])), k


# ------------------------------------------------------------------ 3. cut
@pytest.mark.parametrize("k", [1, 5, 12])
def test_two_calls_give_the_bits_of_one(built, k):
    job = c1("image=16,16")
    windows = algebra_windows(job)
    counts = counts_of(windows, job.spp)
    n, cut = sum(counts), sum(counts[:k])
    whole = host(job, windows)
    xy, ids, lens = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.uint32), np.zeros((n, 2), np.float32)
    ra, rb = np.zeros((7, cut), np.float32), np.zeros((7, n - cut), np.float32)
    host(job, windows[:k], into={"xy": xy[:cut], "ids": ids[:cut], "lens": lens[:cut], "rays": ra})
    host(job, windows[k:], into={"xy": xy[cut:], "ids": ids[cut:], "lens": lens[cut:], "rays": rb})
    assert same_bits(whole, {"xy": xy, "ids": ids, "lens": lens, "rays": np.concatenate([ra, rb], 1)})


# ------------------------------------------------------------------ 4. refusals
def _refused(job, windows, first=None):
    """The call raises and leaves prefilled outputs as they were."""
    n = 4096
    into = {"xy": np.full((n, 2), 7.5, np.float32), "ids": np.full((n, 2), 0xABCD, np.uint32),
            "rays": np.full((7, n), 7.5, np.float32), "lens": np.full((n, 2), 7.5, np.float32)}
    with pytest.raises(ValueError):
        host_camera_samples(job, windows, SEED, 0, first, into=into)
    return all((v == (0xABCD if k == "ids" else 7.5)).all() for k, v in into.items())


def test_refusals_write_nothing(built):
    job = c1("image=16,16")
    ex0, ex1, ey0, ey1 = job.extent()
    good = (ex0, ex0 + 3, ey0, ey0 + 3)
    for w in ((ex0 - 1, ex0 + 3, ey0, ey0 + 3), (ex1 - 3, ex1 + 1, ey0, ey0 + 3), (ex0, ex0 + 3, ey0 - 1, ey0 + 3),
              (ex0, ex0 + 3, ey1 - 3, ey1 + 1)):
        assert _refused(job, [good, w]), w
    c = 16 * job.spp
    assert _refused(job, [good, good], [0, c, 2 * c + 1])            # a first off by one
    assert _refused(job, [good, good], [0, c - 1, 2 * c])
    assert _refused(job, [good, good], [1, c + 1, 2 * c + 1])        # not from 0
    assert _refused(job, [good, good], [0, 2 * c, c])                # descending
    assert _refused(job, [good, (5, 4, 0, 3)], [0, c, c + 1])        # an empty window owns nothing
    for other in (load_config("X5", "image=16,16"), parse_job(os.path.join(SCENES, "light-tracer.bling"), "image=16,16"),
                  load_config("M1", "image=16,16")):
        e = other.extent()
        assert _refused(other, [(e[0], e[0] + 3, e[2], e[2] + 3)])
    # two outputs that overlap
    buf = np.zeros((2 * c, 2), np.float32)
    with pytest.raises(ValueError):
        host_camera_samples(job, [good], SEED, 0, None, outputs=("xy", "lens"), into={"xy": buf[:c], "lens": buf[c // 2:c // 2 + c]})
    assert not buf.any()
    # and what is not refused: no windows at all, and only empty ones
    assert len(host(job, [])["xy"]) == 0 and len(host(job, [(5, 4, 0, 3)])["xy"]) == 0
    assert host(job, [good])["rays"].shape == (7, c)


# ------------------------------------------------------------------ 5. ABI
def test_the_stats_struct_layout_matches_the_c_compiler(tmp_path):
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bling.h"\n#include "bling_host.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu\\n", sizeof(bling_camera_stats), offsetof(bling_camera_stats, samples),\n'
                   '         offsetof(bling_camera_stats, windows), offsetof(bling_camera_stats, ms_total));\n  return 0;\n}\n')
    exe = tmp_path / "lay"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _ffi.CameraStats
    assert got == [C.sizeof(S), S.samples.offset, S.windows.offset, S.ms_total.offset] == [24, 0, 8, 16]


# ------------------------------------------------------------------ 6. the host-only link
def test_the_new_symbols_are_exported_and_link_no_oracle(built):
    hip = os.path.join(LIB, "libbling_hip.so")
    want = {"libbling_host.so": ["bling_host_camera_samples"]}
    if os.path.exists(hip):
        want["libbling_hip.so"] = ["bling_camera_samples_device", "bling_camera_samples"]
        assert all(s in _ffi.HIP_SYMBOLS for s in want["libbling_hip.so"])
    for name, syms in want.items():
        out = subprocess.run(["nm", "-D", os.path.join(LIB, name)], check=True, capture_output=True, text=True).stdout
        defined = {l.split()[-1] for l in out.splitlines() if " T " in l}
        assert all(s in defined for s in syms), name
        assert "oracle" not in out, name
