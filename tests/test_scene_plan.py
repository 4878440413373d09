"""bling_debug_scene_plan (bling_amd.scene_plan): the kernel plan of a scene description from the host-only
stages of csrc/core/scene_plan.cpp -- validate, items, the host SAH, derive -- with no context and no GPU.

The goldens (tests/golden/scene_plans.json, tests/golden/make_scene_plans.py) are Context.scene_info() of every
shipped configuration as uploads reported them on an MI355X before the plan had a unit of its own."""
import ctypes as C
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bling_amd  # noqa: E402
from bling_amd import _ffi  # noqa: E402
from bling_amd.render import BlingError  # noqa: E402
from bling_amd.scene import CONFIGS, FEATURE_SCENES, load_config  # noqa: E402
from scene_desc import desc  # noqa: E402

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_plans.json")))


def test_the_goldens_cover_every_shipped_configuration():
    assert sorted(GOLDEN) == sorted(list(CONFIGS) + list(FEATURE_SCENES))


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_plan_equals_the_recorded_upload(name, monkeypatch):
    monkeypatch.delenv("BLING_BRUTE", raising=False)
    plan = bling_amd.scene_plan(load_config(name))
    assert sorted(plan) == sorted(GOLDEN[name])
    for key, want in GOLDEN[name].items():
        assert plan[key] == want, (name, key)


def test_brute_limit_is_read_at_planning(monkeypatch):
    job = load_config("C1")                                   # cornell-box
    prims = job.counts()["prims"]
    assert 16 < prims <= 64
    monkeypatch.setenv("BLING_BRUTE", "0")
    assert bling_amd.scene_plan(job)["bf_prims"] == 0
    monkeypatch.setenv("BLING_BRUTE", "64")
    assert bling_amd.scene_plan(job)["bf_prims"] == prims
    monkeypatch.delenv("BLING_BRUTE")
    assert bling_amd.scene_plan(job)["bf_prims"] == GOLDEN["C1"]["bf_prims"]


def _bad_texture_graph():
    job = load_config("X11")                                  # blend / gradient / checker textures
    d = desc(job)
    k = next(k for k in range(d.num_textures) if d.textures[k].kind == 4)   # BLING_TEX_CHECKER
    d.textures[k].tex1 = -1
    return job


def _bad_sppm_depth():
    job = load_config("X5")                                   # SPPM as shipped
    assert desc(job).config.renderer == 2                     # BLING_RENDERER_SPPM
    desc(job).config.max_depth = 99
    return job


@pytest.mark.parametrize("make,reason", [(_bad_texture_graph, "malformed or nested computed texture"),
                                         (_bad_sppm_depth, "sppm maxDepth outside [1, ")])
def test_plan_refuses_what_validation_refuses(make, reason):
    job = make()
    hip = _ffi.hip()
    rc = hip.bling_scene_validate(C.c_void_p(job.desc))
    text = hip.bling_last_error().decode()
    assert rc != 0 and reason in text
    with pytest.raises(BlingError) as e:
        bling_amd.scene_plan(job)
    assert e.value.rc == rc
    assert hip.bling_last_error().decode() == text and text in str(e.value)


def test_a_null_description_is_an_error():
    hip = _ffi.hip()
    buf = C.create_string_buffer(64)
    assert hip.bling_debug_scene_plan(None, buf, len(buf), None) != 0
    assert hip.bling_last_error().decode() == "null argument"


def test_the_text_call_reports_the_full_length():
    job = load_config("C1")
    hip = _ffi.hip()
    n = C.c_size_t()
    full, small = C.create_string_buffer(1024), C.create_string_buffer(8)
    assert hip.bling_debug_scene_plan(C.c_void_p(job.desc), full, len(full), None) == 0
    assert hip.bling_debug_scene_plan(C.c_void_p(job.desc), small, len(small), C.byref(n)) == 0
    assert n.value == len(full.value) and small.value == full.value[:7]
