"""A binary32 sequential restatement of the ordered film (include/bling.h BLING_PASS_ORDERED_FILM;
oracle.cpp add_sample / render_tile / oracle_render_shard's addTile; wavefront.h k_film_ordered /
k_film_add_ordered).

Tile images: every pixel and channel of a tile's mkImageTile image starts from +0 and takes the tile's
contributing samples one at a time in the reference's (iy, ix, n) order -- a = a + w for W, a = a +
(v * w) for X, Y, Z, the product rounded to binary32 before the add -- whatever slot order the samples
come in.  Film: film = film + tile_k per channel for every tile whose image covers the pixel, in the
order of `tiles` (ascending tile index), zero values included; film0 is the first operand.

Where a splat lands is film_ref's index arithmetic (_axis: pixel ranges, table indices, trap T12).  A
sample touches every pixel of its footprint at most once, so adding one sample's whole footprint with
one numpy binary32 operation is the sequential rule.
"""
import numpy as np

from film_ref import _axis, f32


def film_ordered(results, img, table, fsize, width, height, tiles, spp, film0=None, sample_major=0, tiles_only=False):
    """results (k, 4) float32 (X, Y, Z, flag) and img (k, 2) float32 image positions of a pass's samples
    in its slot order (tile t holds pixels * spp consecutive samples; within a tile pixel-major, or
    sample-major with sample_major=1), table the job's 16 x 16 filter table, fsize (fw, fh), tiles
    [(x0, x1, y0, y1)] in tile order.  Returns the film (height * width * 4,) float32, accumulated onto
    film0 (zeros if None); with tiles_only=True the tile images instead, (n, slot_h, slot_w, 4) in the
    slot layout of a BLING_PASS_TILE_IMAGES pass (zero padded, pixels past the film zero)."""
    results, img = np.ascontiguousarray(results, f32), np.ascontiguousarray(img, f32)
    table = np.ascontiguousarray(table, f32).reshape(16, 16)
    fw, fh = f32(fsize[0]), f32(fsize[1])
    ifw = f32(1) / fw
    ifh = f32(1) / fw                                                       # trap T12
    rx, ry = int(np.floor(f32(0.5) + fw)), int(np.floor(f32(0.5) + fh))
    sw, sh = 15 + rx, 15 + ry
    slots = np.zeros((len(tiles), sh, sw, 4), f32)
    off = 0
    for t, (x0, x1, y0, y1) in enumerate(tiles):
        npix = (x1 - x0 + 1) * (y1 - y0 + 1)
        cnt = npix * spp
        r, im = results[off:off + cnt], img[off:off + cnt]
        off += cnt
        ox, oy = max(0, x0), max(0, y0)
        w, h = x1 - ox + rx, y1 - oy + ry                                    # mkImageTile
        if w <= 0 or h <= 0:
            continue
        # the reference's order: pixel by pixel (y outer, x inner), then sample by sample
        pt, n = np.divmod(np.arange(cnt), spp)
        order = n * npix + pt if sample_major else np.arange(cnt)
        r, im = r[order], im[order]
        px, ix, okx = _axis(im[:, 0] - f32(0.5), ox, ox + w - 1, fw, ifw)
        py, iy, oky = _axis(im[:, 1] - f32(0.5), oy, oy + h - 1, fh, ifh)
        T = np.zeros((h, w, 4), f32)
        for s in np.nonzero(r[:, 3] != 0)[0]:
            xs, ys = px[s][okx[s]] - ox, py[s][oky[s]] - oy
            if not len(xs) or not len(ys):
                continue
            wt = table[np.ix_(iy[s][oky[s]], ix[s][okx[s]])]
            at = np.ix_(ys, xs)
            T[..., 0][at] = T[..., 0][at] + wt
            for c in range(3):
                T[..., c + 1][at] = T[..., c + 1][at] + r[s, c] * wt          # binary32 product, then binary32 add
        assert T.dtype == f32
        vh, vw = min(h, sh, max(0, height - oy)), min(w, sw, max(0, width - ox))   # pixels past the film stay zero
        slots[t, :vh, :vw] = T[:vh, :vw]
    assert off == len(results) == len(img), (off, len(results), len(img))
    if tiles_only:
        return slots
    film = np.zeros((height, width, 4), f32) if film0 is None else np.array(film0, f32).reshape(height, width, 4)
    for t, (x0, x1, y0, y1) in enumerate(tiles):
        ox, oy = max(0, x0), max(0, y0)
        vh, vw = min(y1 - oy + ry, height - oy), min(x1 - ox + rx, width - ox)
        if vh <= 0 or vw <= 0:
            continue
        film[oy:oy + vh, ox:ox + vw] = film[oy:oy + vh, ox:ox + vw] + slots[t, :vh, :vw]
    return film.reshape(-1)
