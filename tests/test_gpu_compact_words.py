"""The queue compaction between two path vertices (wavefront.h k_compact_count / _scan / _scatter),
driven alone through bling_debug_compact against a numpy reference: the kernels read the flag bytes as
16-byte words (a lane's 16 entries, a wave's 1024, a block's 4096) and scan only the live blocks, and
the queues they build must be the reference's element for element.

Queue lengths sit on every one of those boundaries, and one spans three compaction blocks; each runs
over its own capacity and over a capacity of five blocks (the blocks past the queue exit early and
their rows are never read).  The flags past the queue's end are all set and the output queues are
poisoned by the entry point, so an entry read or written out of place shows.
"""
import numpy as np
import pytest

QF_RESOLVE, QF_ANY, QF_MIS, QF_CONT, QF_MISCULL = 1, 2, 4, 8, 16
POISON = 0xEEEEEEEE
LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 2 * 4096 + 1500]


@pytest.fixture(scope="module")
def ctx():
    from bling_amd.render import Context
    return Context(0)


def reference(flags, queue_in, fused):
    """(queues, qcount) as the device lays them out: order-preserving, the closest-hit queue = every
    MIS entry, then every continuation entry."""
    n = flags.size
    ids = np.arange(n, dtype=np.uint32) if fused else queue_in.astype(np.uint32)
    pick = {b: ids[(flags & b) != 0] for b in (QF_RESOLVE, QF_ANY, QF_MIS, QF_CONT)}
    closest = np.concatenate([pick[QF_MIS] << 1 | 1, pick[QF_CONT] << 1])
    q = {"any": pick[QF_ANY], "closest": closest}
    if fused:        # the next shade input (queue 1) is the resolve list; Q_RESOLVE's counter = continuations
        q["shade1"] = pick[QF_RESOLVE]
        qc = [n, pick[QF_RESOLVE].size, closest.size, pick[QF_ANY].size, pick[QF_CONT].size]
    else:
        q["resolve"] = pick[QF_RESOLVE]
        q["shade1"] = pick[QF_CONT]
        qc = [n, pick[QF_CONT].size, closest.size, pick[QF_ANY].size, pick[QF_RESOLVE].size]
    qc.append(int(((flags & QF_MISCULL) != 0).sum()))
    return q, np.array(qc, np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False])
def test_compacted_queues_equal_reference(ctx, fused):
    rng = np.random.default_rng(20240607)
    for n in LENGTHS:
        for cap in sorted({max(n, 1), 5 * 4096}):
            if cap < n:
                continue
            # dense (most paths survive), sparse and full flags, over all five counted bits
            for density in (0.85, 0.1, 1.0):
                flags = (rng.random((n, 5)) < density).astype(np.uint8) @ np.array([1, 2, 4, 8, 16], np.uint8)
                flags = flags.astype(np.uint8)
                queue_in = rng.permutation(max(n, 1)).astype(np.uint32)[:n]
                got, qc = ctx.compact(flags, queue_in, capacity=cap, fused=fused)
                want, qc_want = reference(flags, queue_in, fused)
                assert np.array_equal(qc, qc_want), (n, cap, density, qc, qc_want)
                for name, w in want.items():
                    g = got[name]
                    assert np.array_equal(g[:w.size], w), (n, cap, density, name)
                    assert (g[w.size:] == POISON).all(), (n, cap, density, name, "written past its length")
