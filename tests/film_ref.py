"""A float64 restatement of the film for given per-sample inputs (oracle.cpp add_sample / make_tile /
oracle_render_shard's addTile, core.hip pass_tiles, wavefront.h k_film / k_film_gather / film_flush).

Everything that decides WHERE a splat lands is kept in binary32 operations in the kernels' order: the
tile-image clipping (ox = max(0, x0), w = x1 - ox + floor(0.5 + fw)), the pixel ranges
(ceil(dx - fw) .. floor(dx + fw)) and the table indices (min(floor(|(float)x - dx| * (1 / fw) * 16),
15), with trap T12: the row index scales by 1 / fw too).  Only the accumulation is float64.

Per pixel and channel (W, X, Y, Z) film_ref returns
  F64  the float64 sum of the exact products value * weight (a product of two binary32 is exact in
       binary64),
  A64  the float64 sum of their absolute values,
  n    the number of splats that reached the pixel.

The bound is derived, not measured.  A film kernel rounds each product once (or not at all, where
the compiler contracts the multiply-add) and adds the n products in some order -- registers per
source pixel, LDS atomics per tile, global atomics per film pixel on the device; sequentially per
tile image and then tile by tile in the oracle.  Every order is a summation tree of depth at most
n - 1, so to first order in u = 2^-24 the result differs from the exact sum by at most
(1 + n - 1) u A64 <= (n + 2) u A64.  bound() is 1.01 (n + 2) u A64 (the 1 % covers the higher-order
terms: n u < 1e-4 for every case of the table) plus the smallest subnormal as an absolute floor.
Two films that both meet it differ by at most twice that (pair_bound).
"""
import os
import re

import numpy as np

f32 = np.float32
U = 2.0 ** -24
TINY = float(np.finfo(np.float32).smallest_subnormal)


def _table(name):
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bling_amd", "csrc", "common",
                             "spectral_data.h")).read()
    body = re.search(name + r"\[[^=]*=\s*\{(.*?)\};", text, re.S).group(1)
    vals = [float.fromhex(x.rstrip("f")) for x in re.findall(r"-?0x[0-9a-fA-F.]+p[+-]?\d+f?", body)]
    ysum = float.fromhex(re.search(r"BLING_CIE_Y_SUM = (-?0x[0-9a-fA-F.]+p[+-]?\d+)f", text).group(1))
    return np.array(vals, f32), f32(ysum)


def spectra_to_results(L):
    """The film's per-sample record of a (k, 16) array of spectra, as add_sample forms it: to_xyz
    (ocore.h: three sequential binary32 sums of band * value, each divided by BLING_CIE_Y_SUM) and the
    flag -- 0 for a sample with a NaN or an infinite band, which the film drops.  (k, 4) float32
    (X, Y, Z, flag), the layout of bling_debug_pass_results."""
    L = np.ascontiguousarray(L, f32)
    out = np.zeros((len(L), 4), f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c, name in enumerate(("BLING_CIE_X_BANDS", "BLING_CIE_Y_BANDS", "BLING_CIE_Z_BANDS")):
            bands, ysum = _table(name)
            acc = np.zeros(len(L), f32)
            for i in range(16):
                acc = acc + bands[i] * L[:, i]
            out[:, c] = acc / ysum
    out[:, 3] = np.isfinite(L).all(1)
    return out


def pass_tiles(job, shard=(0, 1), stride=1):
    """splitWindow over the sample extent (16 x 16 windows, rows first), every stride-th tile, dealt
    round-robin to the shard: [(x0, x1, y0, y1)] in the pass's tile order (core.hip pass_tiles)."""
    ex0, ex1, ey0, ey1 = job.extent()
    out, k = [], 0
    for y in range(ey0, ey1 + 1, 16):
        for x in range(ex0, ex1 + 1, 16):
            if k % stride == 0 and (k // stride) % shard[1] == shard[0]:
                out.append((x, min(x + 15, ex1), y, min(y + 15, ey1)))
            k += 1
    return out


def pass_samples(job, sample_major, shard=(0, 1), stride=1):
    """The (x, y, n) camera samples of a pass in its slot order: the shard's tiles in order, within a
    tile k_raygen's order (pixel-major: slot = pixel * spp + n; sample-major: n * pixels + pixel;
    pixels row by row).  The oracle's render_tile order is the pixel-major one."""
    spp, out = job.spp, []
    for x0, x1, y0, y1 in pass_tiles(job, shard, stride):
        tw, th = x1 - x0 + 1, y1 - y0 + 1
        j = np.arange(tw * th * spp)
        pt, n = (j % (tw * th), j // (tw * th)) if sample_major else (j // spp, j % spp)
        out.append(np.stack([x0 + pt % tw, y0 + pt // tw, n], 1))
    return np.concatenate(out).astype(np.int32)


def _axis(d, lo, hi, fwid, inv):
    """One axis of add_sample for a tile's samples: pixel coordinates (k, span) int64, table indices
    and validity.  d = position - 0.5 (binary32), [lo, hi] the tile image's pixel range."""
    a = np.maximum(lo, np.ceil(d - fwid).astype(np.int64))
    b = np.minimum(hi, np.floor(d + fwid).astype(np.int64))
    span = int(max(0, (b - a).max(initial=-1) + 1))
    p = a[:, None] + np.arange(span)[None, :]
    ok = p <= b[:, None]
    t = np.abs((p.astype(f32) - d[:, None]) * inv * f32(16))               # ((float)x - dx) * ifw * 16.f
    idx = np.minimum(np.floor(t).astype(np.int64), 15)
    return p, idx, ok


def film_ref(results, img, table, fsize, width, height, tiles, spp):
    """results (k, 4) float32 (X, Y, Z, flag) and img (k, 2) float32 image positions of a pass's
    samples in tile order (tile t holds pixels * spp consecutive samples), table the job's 16 x 16
    filter table, fsize (fw, fh), tiles [(x0, x1, y0, y1)].  Returns F64, A64 (height, width, 4) and n
    (height, width)."""
    results, img = np.ascontiguousarray(results, f32), np.ascontiguousarray(img, f32)
    table = np.ascontiguousarray(table, f32).reshape(16, 16)
    fw, fh = f32(fsize[0]), f32(fsize[1])
    ifw = f32(1) / fw
    ifh = f32(1) / fw                                                       # trap T12
    rx, ry = int(np.floor(f32(0.5) + fw)), int(np.floor(f32(0.5) + fh))
    npx = width * height
    F, A, N = np.zeros((4, npx)), np.zeros((4, npx)), np.zeros(npx, np.int64)
    off = 0
    for x0, x1, y0, y1 in tiles:
        cnt = (x1 - x0 + 1) * (y1 - y0 + 1) * spp
        r, im = results[off:off + cnt], img[off:off + cnt]
        off += cnt
        ox, oy = max(0, x0), max(0, y0)
        w, h = x1 - ox + rx, y1 - oy + ry                                    # mkImageTile
        if w <= 0 or h <= 0:
            continue
        keep = r[:, 3] != 0
        r, im = r[keep], im[keep]
        if not len(r):
            continue
        px, ix, okx = _axis(im[:, 0] - f32(0.5), ox, ox + w - 1, fw, ifw)
        py, iy, oky = _axis(im[:, 1] - f32(0.5), oy, oy + h - 1, fh, ifh)
        okx &= px < width                                                    # addTile: pixels past the film are skipped
        oky &= py < height
        ok = oky[:, :, None] & okx[:, None, :]                               # (k, span_y, span_x)
        if not ok.any():
            continue
        wgt = table[iy[:, :, None], ix[:, None, :]].astype(np.float64)[ok]
        pix = (py[:, :, None] * width + px[:, None, :])[ok]
        s = np.nonzero(ok)[0]
        N += np.bincount(pix, minlength=npx)
        for c in range(4):
            v = wgt if c == 0 else wgt * r[s, c - 1].astype(np.float64)
            F[c] += np.bincount(pix, v, minlength=npx)
            A[c] += np.bincount(pix, np.abs(v), minlength=npx)
    assert off == len(results) == len(img), (off, len(results), len(img))
    return (F.T.reshape(height, width, 4).copy(), A.T.reshape(height, width, 4).copy(), N.reshape(height, width))


def bound(A64, n):
    """|film - F64| of one binary32 film, per pixel and channel."""
    return 1.01 * (n[..., None] + 2) * U * A64 + TINY


def pair_bound(A64, n):
    """|film a - film b| of two binary32 films of the same splats."""
    return 2.02 * (n[..., None] + 2) * U * A64 + TINY


def worst_ratio(film, F64, A64, n, pair=False):
    """max over pixels and channels of |film - F64| / bound (NaN in the film counts as infinite)."""
    film = np.asarray(film, np.float64).reshape(F64.shape)
    q = np.abs(film - F64) / (pair_bound(A64, n) if pair else bound(A64, n))
    return float(np.where(np.isnan(q), np.inf, q).max())
