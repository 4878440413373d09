"""Film output of a pass: the reference's tonemap and image writers over the host library.

Reference (src/lib/Graphics/Bling):
  * ``getPixel`` / ``xyzToRgb`` (Image.hs:302-315, Spectrum.hs:162-168)  -> :func:`to_rgb`
  * ``rgbPixels`` (gamma 2.2, clamp, round; Image.hs:317-331)            -> :func:`rgb_pixels`
  * ``writePng`` / ``writeRgbe`` (IO/Bitmap.hs:37-41)                     -> :func:`write_png`, :func:`write_hdr`
  * ``progressWriter`` (IO/Progress.hs:23-36): ``<base>-NNNNN.png`` and ``.hdr`` at every PassDone
    -> :func:`progress_writer`
  * pixels that are already developed, e.g. on the device by ``Context.develop``
    -> :func:`write_png_rgb8`, :func:`write_hdr_rgbe`; the table its 8-bit bytes are looked up in
    -> :func:`gamma_thresholds`
The film is the (W, X, Y, Z) array a pass accumulates (``bling_render_pass``), shape (h * w * 4,).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi


def _film(film, w, h):
    f = np.ascontiguousarray(film, np.float32).reshape(-1)
    if f.size != w * h * 4:
        raise ValueError(f"film has {f.size} floats, expected {w} x {h} x 4")
    return f


def to_rgb(film, w: int, h: int) -> np.ndarray:
    """Linear RGB (h, w, 3) float32: XYZ / W, then xyzToRgb."""
    f = _film(film, w, h)
    rgb = np.zeros(w * h * 3, np.float32)
    _ffi.host().bling_host_film_to_rgb(_ffi.f32ptr(f), w, h, _ffi.f32ptr(rgb))
    return rgb.reshape(h, w, 3)


def rgb_pixels(film, w: int, h: int) -> np.ndarray:
    """8-bit display pixels (h, w, 3) uint8 of rgbPixels."""
    f = _film(film, w, h)
    out = np.zeros(w * h * 3, np.uint8)
    _ffi.host().bling_host_rgb_pixels(_ffi.f32ptr(f), w, h, out.ctypes.data_as(C.POINTER(C.c_uint8)))
    return out.reshape(h, w, 3)


def write_png(path: str, film, w: int, h: int) -> None:
    f = _film(film, w, h)
    if _ffi.host().bling_host_write_png(path.encode(), _ffi.f32ptr(f), w, h) != 0:
        raise OSError(_ffi.host().bling_host_last_error().decode())


def write_hdr(path: str, film, w: int, h: int) -> None:
    rgb = np.ascontiguousarray(to_rgb(film, w, h).reshape(-1))
    if _ffi.host().bling_host_write_hdr(path.encode(), _ffi.f32ptr(rgb), w, h) != 0:
        raise OSError(_ffi.host().bling_host_last_error().decode())


def gamma_thresholds() -> np.ndarray:
    """bling_host_gamma_thresholds: rgbPixels' float -> byte step as 255 ascending float32 thresholds;
    the byte of a linear channel v is the count of thresholds <= v (the table Context.develop's
    "rgb8" looks up on the device)."""
    t = np.zeros(255, np.float32)
    _ffi.host().bling_host_gamma_thresholds(_ffi.f32ptr(t))
    return t


def _pixels(px, w, h, per):
    p = np.ascontiguousarray(px, np.uint8).reshape(-1)
    if p.size != w * h * per:
        raise ValueError(f"image has {p.size} bytes, expected {w} x {h} x {per}")
    return p


def write_png_rgb8(path: str, rgb8, w: int, h: int) -> None:
    """The PNG of write_png for pixels that are already developed (Context.develop's "rgb8")."""
    p = _pixels(rgb8, w, h, 3)
    if _ffi.host().bling_host_write_png_rgb8(path.encode(), p.ctypes.data_as(C.POINTER(C.c_uint8)), w, h) != 0:
        raise OSError(_ffi.host().bling_host_last_error().decode())


def write_hdr_rgbe(path: str, rgbe, w: int, h: int) -> None:
    """The Radiance file of write_hdr for RGBE bytes that are already made (Context.develop's "rgbe")."""
    p = _pixels(rgbe, w, h, 4)
    if _ffi.host().bling_host_write_hdr_rgbe(path.encode(), p.ctypes.data_as(C.POINTER(C.c_uint8)), w, h) != 0:
        raise OSError(_ffi.host().bling_host_last_error().decode())


def mlt_bnext(p: int, b, b_new) -> np.float32:
    """bnext = lerp (1 / p) b bNew (Metropolis.hs:115, Math.hs:108-110) in binary32; b starts at 1."""
    t = np.float32(1) / np.float32(p)
    return np.float32(np.float32((np.float32(1) - t) * np.float32(b)) + np.float32(t * np.float32(b_new)))


def mlt_image(splat, bs, w: int, h: int) -> np.ndarray:
    """The Metropolis renderer's image after pass p = len(bs) (Metropolis.hs:117): getPixel of an empty
    film with the accumulated splat image (h * w * 3 XYZ) and the splat weight bnext / p, where bnext
    runs over the passes' b' values bs; linear RGB (h, w, 3)."""
    from .scene import film_splat_to_rgb
    b = np.float32(1)
    for p, bn in enumerate(bs, 1):
        b = mlt_bnext(p, b, bn)
    return film_splat_to_rgb(None, splat, np.float32(b / np.float32(len(bs))), w, h)


def progress_writer(base: str, w: int, h: int):
    """progressWriter: a ProgressReporter (bling_amd.render.Progress -> bool) that writes every
    completed pass to ``<base>-NNNNN.png`` and ``.hdr`` and asks to continue."""
    def report(pr) -> bool:
        if pr.kind == "PassDone" and pr.film is not None:
            name = f"{base}-{pr.pass_num:05d}"
            print(f"\nWriting {name}...")
            write_png(name + ".png", pr.film, w, h)
            write_hdr(name + ".hdr", pr.film, w, h)
        return True
    return report
