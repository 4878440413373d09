"""The yardstick of the ordered splat films, without a device: the CPU restatements' binary32 splat images
are the sequential add of their splats in key order -- (photon, depth) for the light tracer, (chain,
mutation, current before proposal) for Metropolis -- which is what tests/test_gpu_splat_ordered.py pins the
device's ordered images on.

The light tracer's restatement returns its records with their XYZ, so its image is rebuilt from them record
by record.  The Metropolis restatement's records carry no XYZ; its image is shown to be one fixed order's
sum instead: the same bits whatever the number of host threads that walk the chains, nothing where no splat
fell, and the one splat itself where one fell.
"""
import numpy as np
import pytest

from bling_amd.render import SPLAT_REC
from bling_amd.scene import load_config
from lt_ref import LightRef
from mlt_cases import CASES
from mlt_ref import MltRef
from splat_ordered_util import LT_SCENES, ORDER_EXAMPLE, sequential_add

SEED = 0x0B11A6


def _bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def _as_splat_records(rec, width):
    out = np.zeros(len(rec), SPLAT_REC)
    out["pixel"] = rec["sy"].astype(np.int64) * width + rec["sx"]
    out["key"] = (rec["photon"].astype(np.uint64) << np.uint64(32)) | rec["depth"].astype(np.uint64)
    for k in "xyz":
        out[k] = rec[k]
    return out


@pytest.mark.parametrize("name", list(LT_SCENES))
def test_light_tracer_restatement_is_the_sequential_add_of_its_records(name):
    job = LT_SCENES[name]()
    ref = LightRef(job)
    rec, splat, st = ref.run(SEED, 1)
    assert len(rec) == st.splats
    srec = _as_splat_records(rec, job.width)
    assert len(np.unique(np.stack([srec["pixel"].astype(np.uint64), srec["key"]]), axis=1).T) == len(srec)   # keys are unique
    zero = np.zeros(job.width * job.height * 3, np.float32)
    assert np.array_equal(_bits(sequential_add(zero, srec)), _bits(splat))
    shuffled = srec[np.random.default_rng(3).permutation(len(srec))]
    assert np.array_equal(_bits(sequential_add(zero, shuffled)), _bits(splat))
    # a second pass into the first one's image continues its sums
    rec2, both, _ = ref.run(SEED, 2, splat=splat.copy())
    assert np.array_equal(_bits(sequential_add(splat, _as_splat_records(rec2, job.width))), _bits(both))


@pytest.mark.parametrize("name", list(CASES))
def test_metropolis_restatement_adds_in_one_fixed_order(name):
    cfg, ov = CASES[name]
    job = load_config(cfg, ov)
    ref = MltRef(job)
    _, _, s64, s32, st = ref.run(SEED, 1)
    _, _, _, one_thread, st1 = ref.run(SEED, 1, threads=1)
    assert np.array_equal(_bits(s32), _bits(one_thread)) and st.counts() == st1.counts()
    assert int(ref.count.sum()) == st.splats
    untouched = np.repeat(ref.count == 0, 3)
    assert not s32[untouched].any()
    # a pixel with one splat holds that splat exactly: the binary32 image there is the float64 one, rounded
    single = np.repeat(ref.count == 1, 3)
    assert np.array_equal(_bits(s32[single]), _bits(s64[single].astype(np.float32)))


def test_the_order_example_differs():
    vals = np.tile(np.array(ORDER_EXAMPLE, np.float32), 3)
    rec = np.zeros(len(vals), SPLAT_REC)
    rec["key"] = np.arange(len(vals))
    for k in "xyz":
        rec[k] = vals
    up = sequential_add(np.zeros(3, np.float32), rec)
    rec["key"] = len(vals) - rec["key"]
    down = sequential_add(np.zeros(3, np.float32), rec)
    assert up[0] == 1.0 and down[0] == 0.0
    assert not np.array_equal(_bits(up), _bits(down))
