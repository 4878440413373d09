"""An independent numpy restatement of a renderer's use of its film, written from Image.hs of the reference:
mkImageTile (:108-120), sampleExtent (:162-168), addTile (:178-199), the three sample ops with a tile offset
(:201-299) and scaleSplats (:93-106).  Per SampleWindow, in order, a zeroed tile image of the literal size w x h
(pixels and splats) takes the window's samples one at a time, and addTile then adds the whole tile onto the film
and the splat image.  Everything is binary32 and sequential.  XYZ and the drop rules come from image_ref (itself
independent of the product code); nothing here is shared with common/image_sample.h.
"""
import numpy as np

import image_ref

f32 = np.float32


def mk_image_tile(window, fw, fh):
    """mkImageTile: (px, py, w, h) of the SampleWindow (x0, x1, y0, y1)."""
    x0, x1, y0, y1 = (int(v) for v in window)
    px, py = max(0, x0), max(0, y0)
    w = x1 - px + int(np.floor(f32(0.5) + f32(fw)))
    h = y1 - py + int(np.floor(f32(0.5) + f32(fh)))
    return px, py, w, h


def tile_extent(px, py, w, h, fw, fh):
    """sampleExtent of an image of size w x h at offset (px, py)."""
    fw, fh = f32(fw), f32(fh)
    return (px + int(np.floor(f32(0.5) - fw)), px + int(np.floor(f32(0.5) + f32(w) + fw)),
            py + int(np.floor(f32(0.5) - fh)), py + int(np.floor(f32(0.5) + f32(h) + fh)))


def _add_sample(tile, ox, oy, table, fw, fh, sx, sy, v):
    h, w = tile.shape[:2]
    ifw = f32(1) / fw
    ifh = f32(1) / fw                                   # Image.hs:263 divides by fw here too
    dx, dy = sx - f32(0.5), sy - f32(0.5)
    x0, x1 = max(ox, int(np.ceil(dx - fw))), min(ox + w - 1, int(np.floor(dx + fw)))
    y0, y1 = max(oy, int(np.ceil(dy - fh))), min(oy + h - 1, int(np.floor(dy + fh)))
    if x1 - x0 < 0 or y1 - y0 < 0:
        return
    for y in range(y0, y1 + 1):
        fy = min(int(np.floor(np.abs((f32(y) - dy) * ifh * f32(16)))), 15)
        for x in range(x0, x1 + 1):
            fx = min(int(np.floor(np.abs((f32(x) - dx) * ifw * f32(16)))), 15)
            fltw = table[fy * 16 + fx]
            p = tile[y - oy, x - ox]
            p[0] = p[0] + fltw
            p[1] = p[1] + v[0] * fltw
            p[2] = p[2] + v[1] * fltw
            p[3] = p[3] + v[2] * fltw


def add_windowed(table, fsize, width, height, windows, first, xy, spectra, op="add", film=None, splat=None):
    """film (height x width x 4) and splat (height x width x 3) after the windows, in order; an image given as
    None is left out.  The arrays are changed in place and returned."""
    table = np.ascontiguousarray(table, f32).reshape(256)
    fw, fh = f32(fsize[0]), f32(fsize[1])
    xy = np.ascontiguousarray(xy, f32).reshape(-1, 2)
    xyz = image_ref.spectrum_to_xyz(spectra)
    pos, spec = image_ref.dropped(xy, spectra)
    assert first[0] == 0 and first[-1] == len(xy) and len(first) == len(windows) + 1
    for k, wnd in enumerate(windows):
        ox, oy, w, h = mk_image_tile(wnd, fw, fh)
        if w < 1 or h < 1:
            raise ValueError(f"window {k}: MV.replicate of a negative length")
        pixels, splats = np.zeros((h, w, 4), f32), np.zeros((h, w, 3), f32)
        for i in range(int(first[k]), int(first[k + 1])):
            if pos[i] or spec[i]:
                continue
            sx, sy = xy[i]
            v = xyz[i]
            if op == "add":
                _add_sample(pixels, ox, oy, table, fw, fh, sx, sy, v)
                continue
            px, py = int(np.floor(sx)) - ox, int(np.floor(sy)) - oy
            if px >= w or py >= h or px < 0 or py < 0:
                continue
            if op == "splat":
                splats[py, px, :] = splats[py, px, :] + v
            else:
                pixels[py, px, 0] = pixels[py, px, 0] + f32(1)
                pixels[py, px, 1:] = pixels[py, px, 1:] + v
        # addTile onto an image at offset (0, 0): every tile pixel with y + dy < height and x + dx < width
        hh, ww = min(h, height - oy), min(w, width - ox)
        if hh < 1 or ww < 1:
            continue
        if splat is not None:
            splat[oy:oy + hh, ox:ox + ww] = splat[oy:oy + hh, ox:ox + ww] + splats[:hh, :ww]
        if film is not None:
            film[oy:oy + hh, ox:ox + ww] = film[oy:oy + hh, ox:ox + ww] + pixels[:hh, :ww]
    return film, splat


def scale_splats(splat, factors_or_scalar):
    """scaleSplats: v * s per value, s per pixel or one scalar."""
    s = np.asarray(factors_or_scalar, f32)
    if s.ndim:
        s = s.reshape(splat.shape[0], splat.shape[1], 1)
    return (splat * s).astype(f32)
