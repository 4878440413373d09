"""bling_host_bvh4 and bling_host_threaded (include/bling.h): the host's derivation of the BVH4 and of the threaded
list from a BVH2, against an independent numpy restatement.  No GPU.  The device derivation
(csrc/core/bvh_derive.hip) is pinned to the host's bit for bit (tests/test_gpu_bvh_derive.py), so this keeps the
device, the host and the shared header (csrc/common/bvh4.h) honest against one more statement.

The restatement is written from the rules alone and shares no code or shape with the library: it collapses
top-down and recursively into nested Python nodes, and only then numbers them level by level; the library opens
nodes from a queue.

  open     the non-empty BVH2 children (an empty child's link is ~0); then, while an inner child fits
           (size - 1 + its own non-empty children <= 4), the inner child of strictly largest area -- the lowest
           slot on a tie -- is replaced in place by its non-empty children, child 0 first
  area     2 (d0 d1 + d0 d2 + d1 d2), d = max(0, hi - lo), every operation rounded to binary32
  number   breadth-first from the root, a node's inner slots in slot order
  stack    pushes = max(0, children - 1); the bound is the largest sum of pushes over a root-to-node chain
  unused   lo = +inf, hi = -inf, link 0x80000000
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bling_amd  # noqa: E402
import plan_scenes  # noqa: E402
from derive_scenes import tree_scene  # noqa: E402
from plan_scenes import same_bits  # noqa: E402

f32 = np.float32
EMPTY2, EMPTY4 = -1, -0x80000000


# ------------------------------------------------------------------ the independent restatement
def area(lo, hi):
    d = np.maximum(f32(0), (hi - lo).astype(f32)).astype(f32)
    return f32(f32(2) * f32(f32(f32(d[0] * d[1]) + f32(d[0] * d[2])) + f32(d[1] * d[2])))


def children2(nodes, node):
    """[(lo, hi, link)] of the non-empty children of a BVH2 node."""
    links = nodes.view(np.int32)
    out = []
    for c in range(2):
        link = int(links[node, 12 + c])
        if link != EMPTY2:
            out.append((nodes[node, 6 * c:6 * c + 3].copy(), nodes[node, 6 * c + 3:6 * c + 6].copy(), link))
    return out


def opened(nodes, node):
    v = children2(nodes, node)
    while True:
        best, best_area = None, None
        for k, (lo, hi, link) in enumerate(v):
            if link < 0 or len(v) - 1 + len(children2(nodes, link)) > 4:
                continue
            a = area(lo, hi)
            if best is None or a > best_area:
                best, best_area = k, a
        if best is None:
            return v
        v[best:best + 1] = children2(nodes, v[best][2])


def collapse(nodes, node, above=0):
    """The BVH4 node opened from BVH2 node `node`, nested: slots of (lo, hi, leaf code | nested node)."""
    v = opened(nodes, node)
    pushes = max(0, len(v) - 1)
    slots = [(lo, hi, link if link < 0 else collapse(nodes, link, above + pushes)) for lo, hi, link in v]
    inner = [s[2] for s in slots if not isinstance(s[2], int)]
    return {"slots": slots, "depth": 1 + max([c["depth"] for c in inner], default=0),
            "need": max([above + pushes] + [c["need"] for c in inner])}


def ref_bvh4(nodes):
    """(nodes4 (m, 28) float32, depth, stack_need) of a BVH2 (n, 16) float32."""
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(10000)
    try:
        root = collapse(np.asarray(nodes, f32), 0)
    finally:
        sys.setrecursionlimit(old)
    order, ids = [root], {id(root): 0}
    for nd in order:                                 # breadth-first: a node's inner slots in slot order
        for _, _, what in nd["slots"]:
            if not isinstance(what, int):
                ids[id(what)] = len(order)
                order.append(what)
    out = np.zeros((len(order), 28), f32)
    links = out.view(np.int32)
    for q, nd in enumerate(order):
        for k in range(4):
            if k < len(nd["slots"]):
                lo, hi, what = nd["slots"][k]
                links[q, 24 + k] = what if isinstance(what, int) else ids[id(what)]
            else:
                lo, hi = np.full(3, np.inf, f32), np.full(3, -np.inf, f32)
                links[q, 24 + k] = EMPTY4
            for a in range(3):
                out[q, 4 * a + k], out[q, 4 * (3 + a) + k] = lo[a], hi[a]
    return out, root["depth"], root["need"]


def ref_threaded(nodes):
    """The depth-first entry list: lo, hi, leaf code or -1, the index of the entry behind the subtree."""
    nodes = np.asarray(nodes, f32)
    rows = []

    def walk(node):
        for lo, hi, link in children2(nodes, node):
            e = len(rows)
            rows.append([lo, hi, link if link < 0 else -1, 0])
            if link >= 0:
                walk(link)
            rows[e][3] = len(rows)

    walk(0)
    out = np.zeros((len(rows), 8), f32)
    for e, (lo, hi, code, skip) in enumerate(rows):
        out[e, 0:3], out[e, 3:6] = lo, hi
        out.view(np.int32)[e, 6:8] = code, skip
    return out


def check(nodes):
    got, info = bling_amd.host_bvh4(nodes)
    want, depth, need = ref_bvh4(nodes)
    assert same_bits(got.view(np.uint32), want.view(np.uint32))
    assert (info["depth"], info["stack_need"]) == (depth, need)
    assert same_bits(bling_amd.host_threaded(nodes).view(np.uint32), ref_threaded(nodes).view(np.uint32))
    return got, info


# ------------------------------------------------------------------ the trees of generated scenes
@pytest.mark.parametrize("name", ["soup_5", "soup_65", "chain_24", "cell_200"])
def test_host_bvh4_equals_the_restatement(tmp_path, name):
    from bling_amd.scene import parse_job
    job = parse_job(tree_scene(tmp_path, name))
    nodes, _, info = bling_amd.host_lbvh(*plan_scenes.items(job))
    got, i4 = check(nodes)
    assert 1 <= len(got) <= len(nodes) and 1 <= i4["depth"] <= info["depth"]
    # every slot is used, a leaf or names a later node exactly once
    links = got.view(np.int32)[:, 24:28]
    inner = links[links >= 0]
    assert sorted(inner.tolist()) == list(range(1, len(got)))


# ------------------------------------------------------------------ a tie, by hand
def leaf(first, count):
    return ~((first << 8) | count)


def node2(box0, link0, box1, link1):
    n = np.zeros(16, f32)
    n[0:6], n[6:12] = box0, box1
    n.view(np.int32)[12:14] = link0, link1
    return n


def test_the_lowest_slot_opens_on_an_area_tie():
    """root = (A, leaf); A = (a0, a1), both inner, of bit-equal area (the same extents on other axes).  Once A is
    open there is room for one of them only: a0, the lower slot, opens; a1 stays a node of its own."""
    a0 = [0, 0, 0, 1, 2, 3]
    a1 = [5, 0, 0, 7, 1, 3]
    nodes = np.stack([
        node2([0, 0, 0, 7, 2, 3], 1, [9, 9, 9, 10, 10, 10], leaf(8, 1)),
        node2(a0, 2, a1, 3),
        node2([0, 0, 0, 1, 1, 3], leaf(0, 2), [0, 1, 0, 1, 2, 3], leaf(2, 2)),
        node2([5, 0, 0, 6, 1, 3], leaf(4, 2), [6, 0, 0, 7, 1, 3], leaf(6, 2))]).astype(f32)
    ar = [area(np.array(b[:3], f32), np.array(b[3:], f32)) for b in (a0, a1)]
    assert ar[0].tobytes() == ar[1].tobytes() and ar[0] > 0          # the case really has the tie
    got, info = check(nodes)
    links = got.view(np.int32)[:, 24:28]
    assert links[0].tolist() == [leaf(0, 2), leaf(2, 2), 1, leaf(8, 1)]
    assert links[1].tolist() == [leaf(4, 2), leaf(6, 2), EMPTY4, EMPTY4]
    assert (info["depth"], info["stack_need"]) == (2, 4)
    assert np.isposinf(got[1, 2]) and np.isneginf(got[1, 12 + 2])      # an unused slot: lo = +inf, hi = -inf


def test_host_bvh4_refuses_what_is_no_tree():
    from bling_amd.render import BlingError
    ok = node2([0, 0, 0, 1, 1, 1], leaf(0, 1), [1, 0, 0, 2, 1, 1], leaf(1, 1))
    for bad_link in (0, 1, 7):                       # the root, the node itself, no node
        nodes = np.stack([node2([0, 0, 0, 1, 1, 1], 1, [1, 0, 0, 2, 1, 1], leaf(0, 1)),
                          node2([0, 0, 0, 1, 1, 1], bad_link, [1, 0, 0, 2, 1, 1], leaf(1, 1))]).astype(f32)
        with pytest.raises(BlingError):
            bling_amd.host_bvh4(nodes)
    check(np.stack([ok]).astype(f32))
