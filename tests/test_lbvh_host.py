"""bling_host_lbvh (include/bling_host.h), the CPU statement of the device BVH builder's algorithm
(csrc/common/lbvh.h), against an independent numpy restatement and against properties that do not
need the algorithm at all.  No GPU.

The restatement below shares no code and no search with the library: it sorts the keys with numpy and
builds the hierarchy top-down -- a range splits behind the last key whose highest differing bit (between
the range's first and last key) is 0 -- where the library finds every node's range bottom-up from
common-prefix lengths (Karras 2012).  A node's index follows from its parent's split: the left child of
a split behind position g is node g, the right one node g + 1, the root node 0.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bling_amd  # noqa: E402

f32 = np.float32
SIZES = [3, 4, 5, 63, 64, 65, 257]


# ------------------------------------------------------------------ the independent restatement
def _spread(v):
    out = 0
    for b in range(10):
        out |= ((int(v) >> b) & 1) << (3 * b)
    return out


def ref_keys(boxes):
    """The n keys in item order: Morton code of the quantised centre << 32 | index, in binary32."""
    b = np.asarray(boxes, f32).reshape(-1, 2, 3)
    c = (b[:, 0] + (b[:, 1] - b[:, 0]) * f32(0.5)).astype(f32)
    cmin, cmax = c.min(0), c.max(0)
    keys = []
    with np.errstate(all="ignore"):
        for i in range(len(b)):
            q = []
            for a in range(3):
                ext = f32(cmax[a] - cmin[a])
                if not ext > 0:
                    q.append(0)
                    continue
                f = f32(f32(c[i, a] - cmin[a]) * f32(f32(1024) / ext))
                q.append(int(f) if f < f32(1023) else 1023)
            m = (_spread(q[0]) << 2) | (_spread(q[1]) << 1) | _spread(q[2])
            keys.append((m << 32) | i)
    return keys


def _pad(lo, hi):
    m = f32(max(np.abs(lo).max(), np.abs(hi).max()))
    e = f32(f32(m * f32(2e-6)) + f32(1e-30))
    return (lo - e).astype(f32), (hi + e).astype(f32)


def ref_lbvh(boxes, refs):
    """(sorted keys, nodes (m, 16) float32, refs in sorted order, depth, leaves, max_leaf)."""
    b = np.asarray(boxes, f32).reshape(-1, 2, 3)
    keys = sorted(ref_keys(b))
    order = [k & 0xFFFFFFFF for k in keys]
    n = len(keys)
    sb = b[order]
    split_of, range_of = {}, {}

    def descend(i, first, last):                     # internal node i covers [first, last], last > first
        hb = (keys[first] ^ keys[last]).bit_length() - 1
        g = max(p for p in range(first, last + 1) if not (keys[p] >> hb) & 1)
        split_of[i], range_of[i] = g, (first, last)
        if g > first:
            descend(g, first, g)
        if last > g + 1:
            descend(g + 1, g + 1, last)

    descend(0, 0, n - 1)
    survive = sorted(i for i, (f, l) in range_of.items() if l - f >= 2)
    number = {i: k for k, i in enumerate(survive)}
    nodes = np.zeros((len(survive), 16), f32)
    links = nodes.view(np.int32)
    stat = {"leaves": 0, "max_leaf": 0}

    def depth_of(i):
        f, l = range_of[i]
        if l - f < 2:
            return 0
        g = split_of[i]
        return 1 + max(depth_of(g) if g > f else 0, depth_of(g + 1) if l > g + 1 else 0)

    for i in survive:
        f, l = range_of[i]
        g = split_of[i]
        for c, (cf, cl) in enumerate([(f, g), (g + 1, l)]):
            lo, hi = _pad(sb[cf:cl + 1, 0].min(0), sb[cf:cl + 1, 1].max(0))
            nodes[number[i], 6 * c:6 * c + 3], nodes[number[i], 6 * c + 3:6 * c + 6] = lo, hi
            if cl - cf < 2:
                links[number[i], 12 + c] = ~((cf << 8) | (cl - cf + 1))
                stat["leaves"] += 1
                stat["max_leaf"] = max(stat["max_leaf"], cl - cf + 1)
            else:
                links[number[i], 12 + c] = number[g if c == 0 else g + 1]
    return (np.asarray(keys, np.uint64), nodes, np.asarray(refs, np.uint32)[order], depth_of(0), stat["leaves"],
            stat["max_leaf"])


def random_boxes(n, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-10, 10, (n, 3))
    h = rng.uniform(0.01, 1.5, (n, 3))
    return np.stack([c - h, c + h], 1).astype(f32)


def some_refs(n, seed=5):
    return np.random.default_rng(seed).permutation(n).astype(np.uint32) | np.uint32(1 << 30)


# ------------------------------------------------------------------ property checks without the algorithm
def check_structure(boxes, refs, nodes, refs_out, info, cap=31):
    """Every ref once; every child box holds its items' boxes; leaves of 1 or 2; root = node 0 (every other
    node is reached from it exactly once); depth as reported and at most the cap."""
    b = np.asarray(boxes, f32).reshape(-1, 2, 3)
    n = len(b)
    assert sorted(refs_out.tolist()) == sorted(np.asarray(refs).tolist())
    by_ref = {int(r): k for k, r in enumerate(np.asarray(refs).tolist())}
    assert len(by_ref) == n
    links = nodes.view(np.int32)
    seen_nodes, seen_slots, leaves = [], [], []

    def walk(i, level):
        seen_nodes.append(i)
        deepest = level
        lo_all, hi_all = np.full(3, np.inf, f32), np.full(3, -np.inf, f32)
        for c in range(2):
            lo, hi = nodes[i, 6 * c:6 * c + 3], nodes[i, 6 * c + 3:6 * c + 6]
            link = int(links[i, 12 + c])
            if link < 0:
                code = ~link
                first, cnt = code >> 8, code & 0xFF
                assert cnt in (1, 2)
                leaves.append(cnt)
                slots = list(range(first, first + cnt))
                seen_slots.extend(slots)
                ilo = np.min([b[by_ref[int(refs_out[s])], 0] for s in slots], 0)
                ihi = np.max([b[by_ref[int(refs_out[s])], 1] for s in slots], 0)
            else:
                ilo, ihi, d = walk(link, level + 1)
                deepest = max(deepest, d)
            assert (lo <= ilo).all() and (hi >= ihi).all()
            lo_all, hi_all = np.minimum(lo_all, ilo), np.maximum(hi_all, ihi)
        return lo_all, hi_all, deepest

    _, _, deepest = walk(0, 1)
    assert sorted(seen_nodes) == list(range(len(nodes)))
    assert sorted(seen_slots) == list(range(n))
    assert (nodes[:, 14:] == 0).all()
    assert deepest == info["depth"] <= cap
    assert (info["nodes"], info["leaves"], info["max_leaf"], info["items"]) == (len(nodes), len(leaves), max(leaves), n)
    return deepest


# ------------------------------------------------------------------ 1. restatement
@pytest.mark.parametrize("n", SIZES)
def test_host_lbvh_equals_the_numpy_restatement(n):
    boxes, refs = random_boxes(n, 100 + n), some_refs(n)
    nodes, refs_out, info, keys = bling_amd.host_lbvh(boxes, refs, with_keys=True)
    rkeys, rnodes, rrefs, rdepth, rleaves, rmax = ref_lbvh(boxes, refs)
    assert (keys == rkeys).all()
    assert (refs_out == rrefs).all()
    assert nodes.shape == rnodes.shape and (nodes.view(np.uint32) == rnodes.view(np.uint32)).all()
    assert (info["depth"], info["leaves"], info["max_leaf"]) == (rdepth, rleaves, rmax)


# ------------------------------------------------------------------ 2. structure
@pytest.mark.parametrize("n", SIZES + [1000])
def test_host_lbvh_structure(n):
    boxes, refs = random_boxes(n, 7 * n + 1), some_refs(n)
    nodes, refs_out, info = bling_amd.host_lbvh(boxes, refs)
    check_structure(boxes, refs, nodes, refs_out, info)


# ------------------------------------------------------------------ 3. degenerate inputs
def degenerate_cases():
    rng = np.random.default_rng(3)
    same = np.tile(np.array([[[1, 2, 3], [2, 3, 5]]], f32), (37, 1, 1))
    t = rng.uniform(0, 1, 50)
    line = np.stack([np.stack([t * 7 - 1, np.full(50, 2.0) - 1, np.full(50, -3.0) - 1], 1),
                     np.stack([t * 7 + 1, np.full(50, 2.0) + 1, np.full(50, -3.0) + 1], 1)], 1).astype(f32)
    huge = random_boxes(40, 9)
    huge[17] = [[-1e6, -1e6, -1e6], [2e6, 3e6, 1e6]]
    # 200 items whose centres differ by far less than a cell (two far corner items set the 1024^3 grid)
    c = f32(0.25) + rng.uniform(0, 1e-4, (200, 3))
    h = rng.uniform(0.01, 0.02, (200, 3))
    cell = np.concatenate([np.stack([c - h, c + h], 1), [[[-100] * 3, [-99] * 3]], [[[99] * 3, [100] * 3]]]).astype(f32)
    return {"identical": same, "line": line, "huge": huge, "cell": cell}


@pytest.mark.parametrize("name", ["identical", "line", "huge", "cell"])
def test_host_lbvh_degenerate_inputs(name):
    boxes = degenerate_cases()[name]
    n = len(boxes)
    refs = some_refs(n)
    nodes, refs_out, info, keys = bling_amd.host_lbvh(boxes, refs, with_keys=True)
    depth = check_structure(boxes, refs, nodes, refs_out, info)
    rkeys, rnodes, rrefs, rdepth, _, _ = ref_lbvh(boxes, refs)
    assert (keys == rkeys).all() and (refs_out == rrefs).all()
    assert (nodes.view(np.uint32) == rnodes.view(np.uint32)).all()
    codes = (keys >> np.uint64(32)).astype(np.int64)
    if name == "identical":
        # one Morton code: the split is on the index bits alone, a balanced tree over 37 items in order
        assert len(set(codes.tolist())) == 1 and (keys & np.uint64(0xFFFFFFFF) == np.arange(n)).all()
        assert depth == int(np.ceil(np.log2(n))) - 1
    if name == "line":
        assert all(_spread(1023) << 1 & int(m) == 0 and _spread(1023) & int(m) == 0 for m in codes)   # y and z quantise to 0
    if name == "cell":
        cnt = np.bincount(np.unique(codes, return_inverse=True)[1])
        assert cnt.max() == 200
        assert depth <= 2 + int(np.ceil(np.log2(200)))


# ------------------------------------------------------------------ 4. depth cap
def test_host_lbvh_reports_a_tree_deeper_than_the_cap(tmp_path):
    import plan_scenes
    from bling_amd.scene import parse_job
    job = parse_job(plan_scenes.chain(tmp_path, 24))
    boxes = plan_scenes.prim_boxes(job)
    refs = np.arange(len(boxes), dtype=np.uint32)
    nodes, refs_out, info = bling_amd.host_lbvh(boxes, refs)
    check_structure(boxes, refs, nodes, refs_out, info)
    assert info["depth"] >= 3
    cap = info["depth"] - 1
    with pytest.raises(bling_amd.LbvhDepthError) as e:
        bling_amd.host_lbvh(boxes, refs, depth_cap=cap)
    assert e.value.depth == info["depth"]
    nodes2, _, info2 = bling_amd.host_lbvh(boxes, refs, depth_cap=info["depth"])      # at the cap: a tree
    assert info2 == info and (nodes2.view(np.uint32) == nodes.view(np.uint32)).all()


def test_host_lbvh_refuses_bad_arguments():
    boxes, refs = random_boxes(2, 1), some_refs(2)
    with pytest.raises(ValueError):
        bling_amd.host_lbvh(boxes, refs)
    with pytest.raises(ValueError):
        bling_amd.host_lbvh(random_boxes(5, 1), some_refs(5), depth_cap=32)
