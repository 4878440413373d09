"""Shared helpers of the sampler-and-camera-seam tests (tests/test_camera_samples.py,
tests/test_gpu_camera_samples.py): the case groups, the window lists, a window list's samples in the seam's slot
order, and the host library's outputs as the yardstick of the device's."""
import numpy as np

from bling_amd.render import CAMERA_OUTPUTS, host_camera_samples
from surface_li_cases import SEED, bits, c1, c1_with_camera, windows_of

# (name, pass): the five case groups -- C1 stratified 2 x 2 at two passes, the two other cameras, an spp that is
# no power of two (the fd_spp / fd_nu divisions), and the random sampler
CASES = [("c1", 0), ("c1", 3), ("lens", 0), ("environment", 0), ("strat32", 0), ("random3", 0)]


def case_job(name, tmp):
    if name == "c1":
        return c1("image=16,16")
    if name in ("lens", "environment"):
        return c1_with_camera(name, tmp, "image=16,16")
    if name == "strat32":
        return c1("image=16,16;stratified=3,2")
    if name == "random3":
        return c1("image=16,16;random=3")
    raise KeyError(name)


def window_samples(windows, spp):
    """(k, 3) int32 of (x, y, n): every window's pixels y outer, x inner, n innermost, window after window."""
    out = [np.zeros((0, 3), np.int64)]
    for x0, x1, y0, y1 in windows:
        if x1 < x0 or y1 < y0:
            continue
        ys, xs, ns = np.meshgrid(np.arange(y0, y1 + 1), np.arange(x0, x1 + 1), np.arange(spp), indexing="ij")
        out.append(np.stack([xs.ravel(), ys.ravel(), ns.ravel()], 1))
    return np.concatenate(out).astype(np.int32)


def counts_of(windows, spp):
    return [max(0, x1 - x0 + 1) * max(0, y1 - y0 + 1) * spp for x0, x1, y0, y1 in windows]


def algebra_windows(job):
    """Window algebra: a permutation of splitWindow's tiles, one tile twice, a 1 x 1 window, a window nested in
    another, and two empty windows (x1 = x0 - 1, and y1 < y0)."""
    _, tiles, _ = windows_of(job)
    ex0, ex1, ey0, ey1 = job.extent()
    perm = [tiles[i] for i in np.random.default_rng(7).permutation(len(tiles))]
    return perm + [tiles[1], tiles[1], (ex0 + 3, ex0 + 3, ey1, ey1), (ex0 + 1, ex0 + 9, ey0 + 2, ey0 + 7),
                   (ex0 + 4, ex0 + 6, ey0 + 3, ey0 + 4), (5, 4, 0, 3), (0, 3, 7, 2), tiles[0]]


def one_pixel_windows(job, count=300, seed=11):
    """`count` one-pixel windows of the extent in scrambled order."""
    ex0, ex1, ey0, ey1 = job.extent()
    w = ex1 - ex0 + 1
    px = np.random.default_rng(seed).permutation(w * (ey1 - ey0 + 1))[:count]
    return [(ex0 + int(p % w), ex0 + int(p % w), ey0 + int(p // w), ey0 + int(p // w)) for p in px]


def host(job, windows, pass_index=0, first=None, outputs=CAMERA_OUTPUTS, into=None):
    """The host library's (xy, ids, rays, lens) as a dict."""
    return dict(zip(CAMERA_OUTPUTS, host_camera_samples(job, windows, SEED, pass_index, first, outputs, into)))


def same_bits(a, b):
    """Two output dicts agree bit for bit in every output both hold; ids as integers."""
    ok = True
    for k in CAMERA_OUTPUTS:
        if a.get(k) is None or b.get(k) is None:
            continue
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if k == "ids":
            ok = ok and np.array_equal(x.astype(np.uint32), y.astype(np.uint32))
        else:
            ok = ok and x.shape == y.shape and np.array_equal(bits(x), bits(y))
    return ok


def block(out, lo, hi, n):
    """Slots lo .. hi-1 of an output dict over n slots."""
    return {k: (None if v is None else (np.asarray(v).reshape(7, n)[:, lo:hi] if k == "rays" else np.asarray(v)[lo:hi]))
            for k, v in out.items()}


__all__ = ["CASES", "case_job", "window_samples", "counts_of", "algebra_windows", "one_pixel_windows", "host", "same_bits", "block"]
