"""The case table and scene text of the sampler / filter / camera / image shape tests
(tests/test_gpu_render_shapes.py: its CPU tests and its device tests).

Scenes are the text of fixtures/scenes/shapes-materials.bling (X1) and fixtures/scenes/envmap.bling
(X15) with their single `filter ...` and `camera { ... }` lines replaced, written into a directory of
the caller's (pytest's tmp_path) and loaded with bling_amd.scene.parse_job plus the usual overrides;
cornell-box (C1, the all-LDS profile, pixel-major slots) and sun-sky (C4, the packet kernels,
sample-major slots) are loaded as they are, with overrides only.  Nothing here is a committed
fixture.

What the shapes are for:
  * a non-power-of-two spp re-enters the cycle walk of the sampler's permutation and takes the
    FastDiv reciprocals off their power-of-two divisors (dev_shade.h permute_spp, k_raygen);
  * nu != nv makes `quotRem i nu` (trap T5) reach strata past nu - 1, so the min(ALMOST_ONE, ...)
    clamps fire for the pixel offset, the lens sample and every 2D dimension; an offset of ALMOST_ONE
    rounds ix + ox to ix + 1, the edge of the window k_film_gather gives a source pixel;
  * fractional filter widths move K = 2 floor(0.5 + fw) + 1 between the film kernels, non-square
    ones take the per-sample kernel with trap T12 (the row index scales by 1 / fw), 0.4 makes the
    tile image narrower than its tile, 15 is the widest filter upload accepts (a 30-pixel tile image
    in the 32-pixel LDS tile) and 15.5 the first it refuses.
"""
import os
from dataclasses import dataclass

from bling_amd.scene import SCENES, parse_job

_BASE = {"X1": "shapes-materials.bling", "X15": "envmap.bling"}
# C1 / C4 without their sampler and image size (a `random=` override would win over `stratified=`)
_CONFIG = {"C1": ("cornell-box.bling", "path=15,3;force_path=1"), "C4": ("sun-sky.bling", "path=7,4;force_path=1")}
_LINES = {"X1": ("filter mitchell 2 2 0.333333 0.333333", "camera { perspective fov 50 lensRadius 0 focalDistance 10 }"),
          "X15": ("filter mitchell 2 2 0.333333 0.333333", "camera { perspective fov 45 lensRadius 0 focalDistance 10 }")}

# X1's camera sits 13 units from the point it looks at: a lens of radius 0.3 focused there blurs the
# rest of the scene, so the (shuffled, stratified) lens sample reaches the radiance
LENS = "camera { perspective fov 50 lensRadius 0.3 focalDistance 13 }"
ENVIRONMENT = "camera { environment }"
MITCHELL = "0.333333 0.333333"


@dataclass(frozen=True)
class Case:
    tag: str
    base: str                 # X1 / X15: scene text with replaced lines; C1 / C4: the fixture, overrides only
    over: str                 # overrides
    filter: str = None        # the scene's `filter ...` line (X1 / X15 only)
    camera: str = None        # the scene's `camera { ... }` line (X1 / X15 only)
    pass_index: int = 0       # the pass of the counter RNG's key

    def __str__(self):
        return self.tag


def scene_text(base, filter=None, camera=None):
    text = open(os.path.join(SCENES, _BASE[base])).read()
    for old, new in zip(_LINES[base], (filter, camera)):
        assert text.count(old + "\n") == 1, old
        if new is not None:
            text = text.replace(old + "\n", new + "\n")
    # files the scene names lie next to the fixture, not next to the generated text
    return text.replace('file "', 'file "' + SCENES + "/")


def load(case, dirname):
    """The case's Job; dirname: where its scene text is written (X1 / X15)."""
    if case.base in _BASE:
        path = os.path.join(str(dirname), case.tag.replace(" ", "_").replace("/", "_") + ".bling")
        with open(path, "w") as f:
            f.write(scene_text(case.base, case.filter, case.camera))
        return parse_job(path, case.over)
    assert case.filter is None and case.camera is None
    scene, rest = _CONFIG[case.base]
    return parse_job(os.path.join(SCENES, scene), case.over + ";" + rest)


# ---- (a) per-sample parity across sampler shapes: dimensions below and above n1d = 8 / n2d = 6
SAMPLERS = ["stratified=3,2", "stratified=2,3", "stratified=1,5", "stratified=5,1", "stratified=3,3",
            "stratified=1,1", "random=1", "random=5", "random=7"]
SAMPLE_CASES = [Case(f"X1 lens {s}", "X1", f"image=24,16;path=5,2;{s}", camera=LENS) for s in SAMPLERS]
# C1 at stratified 3 2 renders pass 1.  In pass 0 three of its 3 654 samples -- (5, 1, 5), (17, 8, 0), (18, 12, 2) --
# hold an exact traversal tie (tests/test_gpu_render_shapes.py
# test_c1_pass0_shadow_rays_end_exactly_on_the_light): a stratum clamped to ALMOST_ONE sends the path grazing
# into a corner of the box, where the ray epsilon (3e-6) falls below the ulp of the distance to the light, so
# the shadow ray's tmax is the light quad's own hit distance bit for bit.  The oracle's kd-tree prunes the
# quad's cell there (unoccluded), the device's BVH and exhaustive walks test the quad (occluded).  24 x 24 and
# 48 x 32 hold such paths too; pass 1 at 24 x 16 holds none.
C1_32 = Case("C1 stratified=3,2", "C1", "image=24,16;stratified=3,2", pass_index=1)
C1_32_PASS0 = Case("C1 stratified=3,2 pass 0", "C1", "image=24,16;stratified=3,2")
SAMPLE_CASES += [C1_32,
                 Case("C4 random=5", "C4", "image=24,16;random=5")]
PINHOLE = Case("X1 pinhole stratified=3,2", "X1", "image=24,16;path=5,2;stratified=3,2")
CLAMPED = ["stratified=2,3", "stratified=1,5"]             # nv > nu: the pixel offset's u stratum passes nu - 1

# ---- (c) film cases
_F = "image=24,16;path=5,2;stratified=3,2"
FILTER_CASES = [
    Case("mitchell 1.5 1.5", "X1", _F, filter=f"filter mitchell 1.5 1.5 {MITCHELL}"),     # K = 5, fractional
    Case("triangle 2.4 2.4", "X1", _F, filter="filter triangle 2.4 2.4"),                 # K = 5, fractional
    Case("mitchell 2.5 2.5", "X1", _F, filter=f"filter mitchell 2.5 2.5 {MITCHELL}"),     # K = 7, fractional
    Case("triangle 3 3", "X1", _F, filter="filter triangle 3 3"),                         # K = 7
    Case("box", "X1", _F, filter="filter box"),                                           # width 0.5: K = 3, generic
    Case("triangle 2 3", "X1", _F, filter="filter triangle 2 3"),                         # generic, T12
    Case("triangle 3 2", "X1", _F, filter="filter triangle 3 2"),                         # generic, T12
    Case("gauss 2 2 1", "X1", _F, filter="filter gauss 2 2 1"),                           # K = 5
    Case("triangle 0.4 0.4", "X1", _F, filter="filter triangle 0.4 0.4"),                 # floor(0.5 + fw) = 0
    Case("triangle 15 15", "X1", "image=20,12;path=5,2;stratified=1,1", filter="filter triangle 15 15"),
]
SLOT_CASES = [C1_32] + [Case(f"{b} {s}", b, f"image=24,16;{s}")
                       for b, s in (("C1", "random=5"), ("C4", "stratified=3,2"), ("C4", "random=5"))]
SIZE_CASES = [Case(f"image {w}x{h}", "X1", f"image={w},{h};path=5,2;stratified=3,2")
              for w, h in ((1, 1), (17, 1), (1, 33), (33, 17))]
ENV_CASE = Case("X15 environment", "X15", "image=32,16;stratified=3,2", camera=ENVIRONMENT)
FILM_CASES = FILTER_CASES + SLOT_CASES + SIZE_CASES + [ENV_CASE]

# ---- (d) tile images, (f) the refusal
TILE_CASES = [FILTER_CASES[5], FILTER_CASES[2]]           # generic kernel, K = 7
REFUSED = Case("triangle 15.5 15.5", "X1", "image=20,12;path=5,2;stratified=1,1", filter="filter triangle 15.5 15.5")
