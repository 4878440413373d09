"""Scenes of the derivation tests (tests/test_bvh4_host.py, tests/test_gpu_bvh_derive.py): the generated scenes of
tests/plan_scenes.py by name, and the recipe of 200 small triangles whose centres share one Morton cell."""
import numpy as np

import plan_scenes


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
    """soup_<n>: plan_scenes.soup(n, 4); chain_<n>: plan_scenes.chain(n); cell_200: cell_scene."""
    kind, n = name.split("_")
    if kind == "soup":
        return plan_scenes.soup(dirname, int(n), 4)
    if kind == "chain":
        return plan_scenes.chain(dirname, int(n))
    assert name == "cell_200"
    return cell_scene(dirname)
