"""The cases of the windowed image API tests (test_image_windowed.py on the CPU, test_gpu_image_windowed.py on
the device).  The image is 40 x 24 unless a case says otherwise: a partial 16 x 16 destination tile on both
axes.  Positions are multiples of 1/8; spectra are positive and span 1e-3 .. 1e4, so the order of a binary32 sum
shows in its last bits.  A case is (filter, width, height, windows, first, xy, spectra), window = (x0, x1, y0,
y1) inclusive, first = the n_windows + 1 sample offsets.
"""
import numpy as np

import image_cases

f32 = np.float32
MITCHELL = image_cases.MITCHELL
W, H = 40, 24
EXTENT = (-3, 43, -3, 27)                       # sampleExtent of 40 x 24 under a 3 x 3 filter
OPS = ("add", "add_unfiltered", "splat")


def spectra(rng, n):
    return (10.0 ** rng.uniform(-3.0, 4.0, (n, 1)) * rng.uniform(0.5, 1.5, (n, 16))).astype(f32)


def inside(rng, n, wnd, m=0.0):
    """n positions over the window's pixels and a margin m around them."""
    x0, x1, y0, y1 = wnd
    return image_cases.positions(rng, n, (x0 - m, y0 - m), (x1 + 1 + m, y1 + 1 + m))


def build(rng, flt, w, h, parts):
    """parts: (window, positions) in order."""
    windows = [p[0] for p in parts]
    first = np.concatenate([[0], np.cumsum([len(p[1]) for p in parts])]).astype(np.uint64)
    xy = np.concatenate([p[1] for p in parts]).astype(f32).reshape(-1, 2)
    return flt, w, h, windows, first, xy, spectra(rng, len(xy))


def cases():
    rng = np.random.default_rng(20261021)
    out = {}
    # the extent in a 2 x 2 split, each window's samples on its own pixels: the filter carries them across the cuts
    quads = [(-3, 20, -3, 12), (21, 43, -3, 12), (-3, 20, 13, 27), (21, 43, 13, 27)]
    out["split_2x2"] = build(rng, MITCHELL, W, H, [(q, inside(rng, 500, q)) for q in quads])
    # overlapping and nested windows, one of them twice
    nest = [(0, 39, 0, 23), (5, 20, 4, 15), (10, 12, 8, 9), (5, 20, 4, 15), (15, 35, 10, 22), (-3, 8, -3, 6)]
    out["nested"] = build(rng, MITCHELL, W, H, [(q, inside(rng, 150, q, 2.0)) for q in nest])
    # windows hanging off every edge and corner, one that keeps a single column, two wholly outside
    off = [(-10, 3, 2, 10), (35, 50, 5, 12), (8, 20, -9, 2), (10, 25, 20, 40), (-8, 2, -8, 2), (36, 45, 20, 30), (-20, -2, 0, 5),
           (50, 60, 5, 10), (5, 10, 30, 40)]
    out["off_edges"] = build(rng, MITCHELL, W, H, [(q, inside(rng, 120, q, 3.0)) for q in off])
    # an empty window between two full ones: its tile still covers pixels
    out["empty_between"] = build(rng, MITCHELL, W, H, [((2, 18, 2, 12), inside(rng, 300, (2, 18, 2, 12), 1.0)),
                                                       ((12, 30, 6, 20), np.zeros((0, 2), f32)),
                                                       ((14, 36, 8, 22), inside(rng, 300, (14, 36, 8, 22), 1.0))])
    # samples all over the extent, most of them outside their own window's tile: clipped
    out["outside_own_tile"] = build(rng, MITCHELL, W, H, [((10, 15, 5, 9), inside(rng, 600, EXTENT)), ((20, 33, 12, 20), inside(rng, 600, EXTENT))])
    # box filter, one-pixel windows in any order, some twice, some past the right and lower edge
    px = np.stack([rng.integers(0, 42, 300), rng.integers(0, 26, 300)], 1)
    out["box_one_pixel"] = build(rng, ("box",), W, H, [((x, x, y, y), inside(rng, 3, (x, x, y, y))) for x, y in px])
    # one window, one full and one one-pixel destination tile on both axes
    out["one_window_17x17"] = build(rng, MITCHELL, 17, 17, [((-3, 20, -3, 20), inside(rng, 1500, (-3, 20, -3, 20)))])
    return out


def drop_case():
    """split_2x2's windows with NaN and infinite bands and non-finite and huge positions among the samples, in and
    outside their windows' tiles.  Returns the case and (dropped for the spectrum, dropped for the position)."""
    rng = np.random.default_rng(11)
    quads = [(-3, 20, -3, 12), (21, 43, -3, 12), (-3, 20, 13, 27), (21, 43, 13, 27)]
    flt, w, h, windows, first, xy, sp = build(rng, MITCHELL, W, H, [(q, inside(rng, 100, q)) for q in quads])
    sp[5, 2] = np.nan
    sp[130, 15] = np.inf
    sp[250, 0] = -np.inf
    xy[260] = (39.0, 1.0); sp[260, 7] = np.nan          # outside its own window's tile, counted all the same
    xy[40, 0] = np.nan
    xy[170, 1] = np.inf
    xy[310, 0] = 2.0 ** 21
    xy[390] = (np.nan, 3.0); sp[390, 1] = np.nan        # the position is tested first
    return (flt, w, h, windows, first, xy, sp), (4, 4)
