"""Textured material parameters, host side (include/bling_scene.h "materials"): every slot parses with a
non-constant texture, sets PROCTEX and validates; a broken encoding is refused; scenes without such slots
keep the feature mask and the material records they had before (tests/golden/material_records.json);
and the constant scenes the device's two-valued test compares against do tell a wrong value apart."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle_py
import param_texture_scenes as pts
from bling_amd import _ffi
from bling_amd.scene import CONFIGS, FEATURE_SCENES, load_config, parse_job
from scene_desc import Material, desc

PROCTEX = 1 << 18
RAW = 1                                                   # BLING_SLOT_RAW
T_CONST, T_CHECKER = 0, 4
TRANSMATTE, SHINYMETAL, SUBSTRATE = 6, 7, 8
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "material_records.json")


def _validate(job):
    hip = _ffi.hip()
    rc = hip.bling_scene_validate(C.c_void_p(job.desc))
    return rc, hip.bling_last_error().decode()


def _tested(job):
    """The material under test: the ground's (the first one parsed after the default material)."""
    return desc(job).materials[1]


@pytest.mark.parametrize("slot,mat", pts.SLOTS, ids=[s for s, _ in pts.SLOTS])
def test_every_slot_takes_a_texture(slot, mat, tmp_path):
    job = parse_job(pts.write_scene(str(tmp_path), "slot", mat))
    assert job.counts()["features"] & PROCTEX, slot
    rc, err = _validate(job)
    assert rc == 0, err
    d, m = desc(job), _tested(job)
    kind, name = slot.split(".")
    if name in ("sigma", "rough", "ior") or slot == "transMatte.ks":      # a scalar slot: stex[0], scalar[0] unused
        assert m.stex[0] >= 0 and d.scalar_textures[m.stex[0]].kind == 1 and m.scalar[0] == 0.0
        assert (kind in ("transMatte", "shinyMetal")) == (m.kind in (TRANSMATTE, SHINYMETAL))
        assert list(m.stex[1:3]) == [-1, -1]               # its spectra stay folded
        assert all(d.textures[m.tex[j]].kind == T_CONST for j in range(4) if m.tex[j] >= 0)
    elif kind == "transMatte":                             # t needs r: both raw, whichever varies
        assert m.stex[1] == RAW and m.stex[0] == -1
        kinds = [d.textures[m.tex[j]].kind for j in range(2)]
        assert kinds == ([T_CHECKER, T_CONST] if name == "kr" else [T_CONST, T_CHECKER])
    elif kind == "shinyMetal":
        j = 0 if name == "ks" else 2
        assert m.stex[1 if name == "ks" else 2] == RAW and m.stex[2 if name == "ks" else 1] == -1
        assert m.tex[j] == m.tex[j + 1] and d.textures[m.tex[j]].kind == T_CHECKER
        assert m.tex[2 - j] != m.tex[3 - j] and d.textures[m.tex[2 - j]].kind == d.textures[m.tex[3 - j]].kind == T_CONST
    else:                                                  # substrate: told by the texture's kind
        j = ("kd", "ks", "ka").index(name)
        assert [d.textures[m.tex[i]].kind for i in range(3)] == [T_CHECKER if i == j else T_CONST for i in range(3)]
        assert list(m.stex[:3]) == [-1, -1, -1]


def test_bump_map_around_a_textured_scalar(tmp_path):
    mat = "bumpMap bump { scale 0 0.05 tex { %s } } %s" % (pts.PERLIN, dict(pts.SLOTS)["plastic.rough"])
    job = parse_job(pts.write_scene(str(tmp_path), "bump", mat))
    m = _tested(job)
    assert m.stex[0] >= 0 and m.stex[3] >= 0 and m.stex[3] != m.stex[0]
    assert job.counts()["features"] & PROCTEX and job.counts()["features"] & (1 << 17)
    assert _validate(job)[0] == 0


def test_constant_slots_fold_as_before(tmp_path):
    """The same material written with constants only: no flag, no stex, no PROCTEX, spectra folded."""
    for case in ("transmatte", "shinymetal", "substrate", "plastic_rough"):
        job = parse_job(pts.write_scene(str(tmp_path), case, pts.material(case, "const")))
        m, d = _tested(job), desc(job)
        assert not job.counts()["features"] & PROCTEX, case
        assert list(m.stex) == [-1, -1, -1, -1]
        assert all(d.textures[m.tex[j]].kind == T_CONST for j in range(4) if m.tex[j] >= 0)
        assert _validate(job)[0] == 0


def test_the_wide_spectra_exercise_the_clamps(tmp_path):
    """WIDE and WIDE2 have bands above 1 and bands at 0: sClamp 0 1 and sClamp 0 0.999 both bite."""
    job = parse_job(pts.write_scene(str(tmp_path), "w", pts.material("substrate", "ident")))
    d = desc(job)
    vals = [np.array(d.textures[i].value[:], np.float32) for i in range(d.num_textures) if d.textures[i].kind == T_CONST]
    wide = [v for v in vals if v.max() > 1]
    assert len(wide) >= 4 and all(v.min() == 0 for v in wide)              # both children of the two checkers


def _broken(tmp_path, mat, breaker):
    job = parse_job(pts.write_scene(str(tmp_path), "b", mat))
    assert _validate(job)[0] == 0
    breaker(desc(job), _tested(job))
    rc, err = _validate(job)
    return rc, err


def test_broken_encodings_are_refused(tmp_path):
    slots = dict(pts.SLOTS)

    def tex_out_of_range(d, m):
        m.tex[0] = d.num_textures
    def stex_out_of_range(d, m):
        m.stex[0] = d.num_scalar_textures
    def bad_flag(d, m):
        m.stex[1] = 7
    def folded_but_computed(d, m):                          # the flag says folded, the texture is a checker
        m.stex[1] = -1
    def nested(d, m):                                       # a raw checker whose child is itself a checker
        t = d.textures[m.tex[0]]
        assert t.kind == T_CHECKER
        t.tex1 = m.tex[0]
    def raw_pair_split(d, m):                               # shinyMetal's raw ks must sit in both slots
        m.tex[1] = 0
    cases = [("substrate.kd", tex_out_of_range), ("matte.sigma", stex_out_of_range), ("transMatte.kr", bad_flag),
             ("transMatte.kr", folded_but_computed), ("substrate.kd", nested), ("shinyMetal.ks", nested),
             ("shinyMetal.ks", raw_pair_split), ("shinyMetal.ks", folded_but_computed)]
    for k, (slot, breaker) in enumerate(cases):
        rc, err = _broken(tmp_path / str(k), slots[slot], breaker)
        assert rc == -1 and err, (slot, breaker.__name__)                  # BLING_EINVAL


# ---------------------------------------------------------------- no behaviour change
@pytest.mark.parametrize("name", list(CONFIGS) + list(FEATURE_SCENES))
def test_fixture_scenes_keep_their_features_and_material_records(name):
    """Every benchmark config and feature scene: the feature mask and the bling_material records, byte
    for byte, as recorded before materials took textured parameters."""
    want = json.load(open(GOLDEN))[name]
    job = load_config(name)
    d = desc(job)
    assert job.counts()["features"] == want["features"]
    assert d.num_materials == want["num_materials"]
    raw = C.string_at(C.addressof(d.materials.contents), C.sizeof(Material) * d.num_materials)
    assert raw.hex() == want["materials"]


# ---------------------------------------------------------------- the two-valued device test's inputs
@pytest.mark.parametrize("case", pts.TWO_VALUED_CASES)
def test_two_valued_inputs_tell_a_wrong_value_apart(case, tmp_path):
    """From the oracle alone, on the constant scenes A and B at `path maxDepth 1`: the classes of the
    first-hit points leave out at most 2 % of the samples, each class holds at least 10 %, and within
    each class the radiance under A differs from the one under B on at least half of the samples -- so
    a device that took the wrong value at a hit would fail tests/test_gpu_param_textures.py."""
    L, vtx = [], []
    for how in (0, 1):
        mat, _ = pts.two_valued(case, how)
        job = parse_job(pts.write_scene(str(tmp_path / str(how)), case, mat), "path=1,1")
        assert not job.counts()["features"] & PROCTEX
        s = pts.all_samples(job)
        Lk, vk = oracle_py.Oracle(job).sample_li_vertices(s)
        L.append(Lk)
        vtx.append(vk)
    p = vtx[0][:, 0, 7:10]
    assert np.array_equal(p.view(np.uint32), vtx[1][:, 0, 7:10].view(np.uint32))   # the same first hits
    by_image = pts.two_valued(case, "tex")[1] is not None
    cls = pts.classify(p, by_image)
    n = len(cls)
    differ = (L[0].view(np.uint32) != L[1].view(np.uint32)).any(1)
    shares = [float((cls == k).sum()) / n for k in (0, 1)]
    tell = [float(differ[cls == k].mean()) for k in (0, 1)]
    print(f"{case}: n {n} left out {(cls < 0).sum()} class shares {shares} differing {tell}")
    assert (cls < 0).sum() <= 0.02 * n
    assert min(shares) >= 0.10
    assert min(tell) >= 0.5
    # the two-valued scene itself parses to values that are the constant scenes' bit for bit
    mat, img = pts.two_valued(case, "tex")
    job = parse_job(pts.write_scene(str(tmp_path / "t"), case, mat, img), "path=1,1")
    assert job.counts()["features"] & PROCTEX and _validate(job)[0] == 0
    if img is not None:
        d = desc(job)
        tex = sorted({float(d.images[0].texels[i]) for i in range(4)})
        assert tex == sorted({float(pts.byte_value(b)) for b in img})
