"""The restatement of the ordered film (tests/film_ordered_ref.py) is the oracle's order: fed the oracle's
own per-sample results it gives the oracle's film, its tile images and its accumulated film bit for bit,
and it does not depend on the slot order its samples come in.  No tolerance anywhere.  CPU only."""
import numpy as np
import pytest

import shape_scenes as sc
from film_ordered_ref import film_ordered
from film_ref import pass_samples, pass_tiles, spectra_to_results
from oracle_py import Oracle

SEED = 0x0B11A6
SHARDS = [(0, 1), (0, 2), (1, 2)]
_cache = {}


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("film_ordered_scenes")


def oracle_samples(case, scene_dir, pass_index=None):
    """(job, oracle, results, img) of every sample of the case's pass in the oracle's (pixel-major) order,
    computed once."""
    p = case.pass_index if pass_index is None else pass_index
    if (case.tag, p) not in _cache:
        if ("job", case.tag) not in _cache:
            job = sc.load(case, scene_dir)
            _cache["job", case.tag] = (job, Oracle(job))
        job, orc = _cache["job", case.tag]
        L, img, _ = orc.sample_li_batch(pass_samples(job, 0), seed=SEED, pass_index=p)
        _cache[case.tag, p] = (job, orc, spectra_to_results(L), img)
    return _cache[case.tag, p]


def restate(job, res, img, shard=(0, 1), stride=1, **kw):
    """film_ordered of a shard of the whole pass's pixel-major samples."""
    if shard != (0, 1) or stride != 1:
        # the shard's samples out of the whole pass's: tile k of the pass holds a consecutive run
        runs, off = [], 0
        keep = set(pass_tiles(job, shard, stride))
        for t in pass_tiles(job):
            cnt = (t[1] - t[0] + 1) * (t[3] - t[2] + 1) * job.spp
            if t in keep:
                runs.append(np.arange(off, off + cnt))
            off += cnt
        sel = np.concatenate(runs) if runs else np.zeros(0, np.int64)
        res, img = res[sel], img[sel]
    return film_ordered(res, img, job.filter_table(), job.filter_size, job.width, job.height,
                        pass_tiles(job, shard, stride), job.spp, **kw)


@pytest.mark.parametrize("case", sc.FILM_CASES, ids=str)
def test_restatement_is_the_oracles_film(case, scene_dir):
    job, orc, res, img = oracle_samples(case, scene_dir)
    film, st = orc.render(seed=SEED, pass_index=case.pass_index)
    assert st.samples == len(res) and st.dropped == 0 and (film.reshape(-1, 4)[:, 1:] > 0).any()
    assert np.array_equal(restate(job, res, img), film)


@pytest.mark.parametrize("case", sc.TILE_CASES + [sc.C1_32, sc.FILTER_CASES[9]], ids=str)
@pytest.mark.parametrize("shard", SHARDS, ids=str)
def test_restatement_is_the_oracles_tile_images(case, shard, scene_dir):
    job, orc, res, img = oracle_samples(case, scene_dir)
    tiles, org, _ = orc.render_tiles(seed=SEED, pass_index=case.pass_index, shard=shard)
    mine = restate(job, res, img, shard=shard, tiles_only=True)
    assert mine.shape == tiles.shape and len(org) == len(pass_tiles(job, shard))
    assert np.array_equal(mine, tiles)
    assert (tiles[..., 0] > 0).any()


@pytest.mark.parametrize("case", [sc.C1_32_PASS0, sc.FILTER_CASES[5]], ids=str)
def test_accumulated_passes(case, scene_dir):
    """Two passes into one film: film0 is the first operand of every pixel's sum."""
    job, orc, res0, img0 = oracle_samples(case, scene_dir, 0)
    _, _, res1, img1 = oracle_samples(case, scene_dir, 1)
    film, _ = orc.render(seed=SEED, pass_index=0)
    first = film.copy()
    film, _ = orc.render(seed=SEED, pass_index=1, film=film)
    mine0 = restate(job, res0, img0)
    assert np.array_equal(mine0, first)
    assert np.array_equal(restate(job, res1, img1, film0=mine0), film)
    assert not np.array_equal(restate(job, res1, img1), film)


@pytest.mark.parametrize("case", [sc.C1_32, sc.FILTER_CASES[3], sc.FILTER_CASES[5]], ids=str)
def test_slot_order_does_not_matter(case, scene_dir):
    """The same samples permuted into sample-major slots, with sample_major=1: the same bits."""
    job, orc, res, img = oracle_samples(case, scene_dir)
    minor, major = pass_samples(job, 0), pass_samples(job, 1)
    index = {tuple(s): i for i, s in enumerate(minor.tolist())}
    perm = np.array([index[tuple(s)] for s in major.tolist()])
    assert not np.array_equal(perm, np.arange(len(perm))) and np.array_equal(minor[perm], major)
    a = restate(job, res, img)
    b = restate(job, res[perm], img[perm], sample_major=1)
    assert np.array_equal(a, b)
    ta = restate(job, res, img, tiles_only=True)
    tb = restate(job, res[perm], img[perm], sample_major=1, tiles_only=True)
    assert np.array_equal(ta, tb)
