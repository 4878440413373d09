"""The chain a caller-made renderer runs -- caller's camera rays -> surfaceLi -> addSample per window -> addTile --
pinned on the CPU before the device relies on it (tests/test_gpu_surface_li.py, case 8): fed the oracle's
spectra of the oracle's camera rays, window by window in prender's order, the image API's windowed film
(host_add_windowed) IS the sampler renderer's film of the pass, bit for bit, also accumulated over two passes.
CPU only; no tolerance."""
import numpy as np
import pytest

from bling_amd.image import host_add_windowed, image_desc
from oracle_py import Oracle
from surface_li_cases import SEED, c1, camera_rays, job_desc, windows_of


@pytest.fixture(scope="module")
def chain(built):
    job = c1("image=33,17")
    assert job.spp == 4 and (job.width, job.height) == (33, 17)
    return job, Oracle(job)


def test_the_jobs_filter_is_the_image_apis(chain):
    job, _ = chain
    mine, made = job_desc(job), image_desc(("mitchell", 2, 2, 0.333333, 0.333333), job.width, job.height)
    assert (mine.filter.width, mine.filter.height) == (made.filter.width, made.filter.height) == (2.0, 2.0)
    assert np.array_equal(np.array(mine.filter.table[:], np.float32), np.array(made.filter.table[:], np.float32))


def test_windowed_film_of_the_oracles_spectra_is_the_oracles_film(chain):
    job, orc = chain
    samples, windows, counts = windows_of(job)
    assert len(windows) == 6 and sum(counts) == len(samples) == job.camera_samples()
    film_o, film = None, None
    for p in (0, 1):                                                          # the second pass accumulates on both sides
        film_o, st = orc.render(seed=SEED, pass_index=p, film=film_o)
        assert st.samples == len(samples) and st.dropped == 0                 # the cap: the NaN filter drops none of them
        L, img, _ = orc.sample_li_batch(samples, seed=SEED, pass_index=p)
        rays, xy = camera_rays(orc, samples, pass_index=p)
        assert np.array_equal(xy, img) and np.isfinite(rays).all() and np.isfinite(L).all()
        film, _ = host_add_windowed(job_desc(job), None, None, windows, counts, xy, L, "add", film=film, splat=False)
        assert (film[..., 1:] > 0).any()
        assert np.array_equal(film.reshape(-1), film_o), p
