"""An independent numpy restatement of the image monad's three ops, written from Image.hs:201-299 of the
reference: addSample, addUnfilteredSample and splatSample applied to samples 0 .. n-1 in that order, every
accumulation sequential in binary32 (a = a + w, a = a + (v * w) with the product rounded first).  XYZ is
spectrumToXYZ: three left folds over the 16 bands from 0, each divided by the Y sum.  The drop rules are the
ABI's (include/bling.h): a position that is not finite or beyond 2^20 is dropped, then a spectrum with a NaN
or infinite band.  Nothing here is shared with the product code or with film_ref.
"""
import os
import re

import numpy as np

f32 = np.float32


def _bands():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bling_amd", "csrc", "common", "spectral_data.h")
    text = open(path).read()
    out = []
    for name in ("BLING_CIE_X_BANDS", "BLING_CIE_Y_BANDS", "BLING_CIE_Z_BANDS"):
        body = re.search(name + r"\[[^=]*=\s*\{(.*?)\};", text, re.S).group(1)
        out.append(np.array([float.fromhex(x.rstrip("f")) for x in re.findall(r"-?0x[0-9a-fA-F.]+p[+-]?\d+f?", body)], f32))
    ysum = f32(float.fromhex(re.search(r"BLING_CIE_Y_SUM = (-?0x[0-9a-fA-F.]+p[+-]?\d+)f", text).group(1)))
    return out, ysum


def spectrum_to_xyz(spectra):
    """(n, 16) float32 -> (n, 3) float32."""
    bands, ysum = _bands()
    spectra = np.ascontiguousarray(spectra, f32).reshape(-1, 16)
    out = np.zeros((len(spectra), 3), f32)
    with np.errstate(all="ignore"):
        for c in range(3):
            acc = np.zeros(len(spectra), f32)
            for i in range(16):
                acc = acc + bands[c][i] * spectra[:, i]
            out[:, c] = acc / ysum
    return out


def dropped(xy, spectra):
    """(position dropped, spectrum dropped) boolean arrays; a sample counts in the first that applies."""
    xy = np.asarray(xy, f32).reshape(-1, 2)
    spectra = np.asarray(spectra, f32).reshape(-1, 16)
    with np.errstate(invalid="ignore"):
        pos = ~(np.isfinite(xy).all(1) & (np.abs(xy) <= f32(2.0 ** 20)).all(1))
    spec = ~pos & ~np.isfinite(spectra).all(1)
    return pos, spec


def extent(width, height, fw, fh):
    """sampleExtent (Image.hs:162-168) at offset (0, 0)."""
    fw, fh = f32(fw), f32(fh)
    return (int(np.floor(f32(0.5) - fw)), int(np.floor(f32(0.5) + f32(width) + fw)),
            int(np.floor(f32(0.5) - fh)), int(np.floor(f32(0.5) + f32(height) + fh)))


def add_samples(table, fsize, width, height, xy, spectra, op="add", target=None):
    """The target (height x width x 4 float32; x 3 for "splat") after the op on every sample in order."""
    table = np.ascontiguousarray(table, f32).reshape(256)
    fw, fh = f32(fsize[0]), f32(fsize[1])
    xy = np.ascontiguousarray(xy, f32).reshape(-1, 2)
    xyz = spectrum_to_xyz(spectra)
    pos, spec = dropped(xy, spectra)
    per = 3 if op == "splat" else 4
    img = np.zeros((height, width, per), f32) if target is None else np.array(target, f32).reshape(height, width, per)
    ifw = f32(1) / fw
    ifh = f32(1) / fw                                   # Image.hs:263 divides by fw here too
    for k in range(len(xy)):
        if pos[k] or spec[k]:
            continue
        sx, sy = xy[k]
        v = xyz[k]
        if op != "add":
            px, py = int(np.floor(sx)), int(np.floor(sy))
            if px >= width or py >= height or px < 0 or py < 0:
                continue
            if op == "splat":
                img[py, px, :] = img[py, px, :] + v
            else:
                img[py, px, 0] = img[py, px, 0] + f32(1)
                img[py, px, 1:] = img[py, px, 1:] + v
            continue
        dx, dy = sx - f32(0.5), sy - f32(0.5)
        x0, x1 = max(0, int(np.ceil(dx - fw))), min(width - 1, int(np.floor(dx + fw)))
        y0, y1 = max(0, int(np.ceil(dy - fh))), min(height - 1, int(np.floor(dy + fh)))
        if x1 - x0 < 0 or y1 - y0 < 0:
            continue
        xs, ys = np.arange(x0, x1 + 1), np.arange(y0, y1 + 1)
        ifx = np.minimum(np.floor(np.abs((xs.astype(f32) - dx) * ifw * f32(16))).astype(np.int64), 15)
        ify = np.minimum(np.floor(np.abs((ys.astype(f32) - dy) * ifh * f32(16))).astype(np.int64), 15)
        w = table[ify[:, None] * 16 + ifx[None, :]]                      # (rows, cols)
        win = img[y0:y1 + 1, x0:x1 + 1]
        win[:, :, 0] = win[:, :, 0] + w
        for c in range(3):
            win[:, :, c + 1] = win[:, :, c + 1] + v[c] * w               # the product is a float32 array: rounded first
    return img
