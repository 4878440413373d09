"""The image API (include/bling.h, "the image API on the device"): the reference's image monad -- mkImage,
addSample', addUnfilteredSample', splatSample, sampleExtent', execImageT (Image.hs) -- for samples the
caller computed, on a film that lives on the device.

    img = Image(("mitchell", 3, 3, 1 / 3, 1 / 3), 480, 270)
    x0, x1, y0, y1 = img.extent()
    img.add_samples(xy, spectra)              # numpy arrays, or torch device tensors (no host copy)
    rgb8 = img.develop("rgb8")

The film after add_samples is, bit for bit, what the reference's one thread makes of it by applying the op
to the samples in order; host_add_samples is that sequential restatement on the CPU.  No scene is needed.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi
from .render import BlingError, Context, _check


def make_filter(spec) -> _ffi.Filter:
    """bling_host_make_filter: ("box",), ("gauss", w, h, alpha), ("sinc", w, h, tau), ("mitchell", w, h, B, C)
    or ("triangle", w, h) -- a scene file's `filter` line -- as a bling_filter."""
    if isinstance(spec, _ffi.Filter):
        return spec
    if isinstance(spec, str):
        spec = (spec,)
    name, params = spec[0], np.asarray([np.float32(v) for v in spec[1:]], np.float32)
    if name not in _ffi.FILTER_KINDS:
        raise ValueError(f"unknown pixel filter {name!r}")
    out = _ffi.Filter()
    if _ffi.host().bling_host_make_filter(_ffi.FILTER_KINDS[name], _ffi.f32ptr(params), len(params), C.byref(out)) != 0:
        raise ValueError(f"filter {name}: {_ffi.host().bling_host_last_error().decode()}")
    return out


def eval_filter(spec, x: float, y: float) -> np.float32:
    """bling_host_eval_filter: evalFilter (Filter.hs) of the filter at (x, y)."""
    if isinstance(spec, str):
        spec = (spec,)
    params = np.asarray([np.float32(v) for v in spec[1:]], np.float32)
    return np.float32(_ffi.host().bling_host_eval_filter(_ffi.FILTER_KINDS[spec[0]], _ffi.f32ptr(params), float(np.float32(x)),
                                                         float(np.float32(y))))


def image_desc(filter, width: int, height: int) -> _ffi.ImageDesc:
    return _ffi.ImageDesc(int(width), int(height), make_filter(filter))


def image_extent(desc: _ffi.ImageDesc):
    """bling_host_image_extent: sampleExtent, (x0, x1, y0, y1) inclusive."""
    out = (C.c_int32 * 4)()
    _ffi.host().bling_host_image_extent(C.byref(desc), out)
    return tuple(int(v) for v in out)


def rgb_to_spectrum_illum(rgb) -> np.ndarray:
    """bling_host_rgb_to_spectrum_illum for an (..., 3) array: (..., 16) float32."""
    rgb = np.ascontiguousarray(rgb, np.float32)
    flat = rgb.reshape(-1, 3)
    out = np.zeros((len(flat), 16), np.float32)
    fn = _ffi.host().bling_host_rgb_to_spectrum_illum
    for i in range(len(flat)):
        fn(_ffi.f32ptr(flat[i]), _ffi.f32ptr(out[i]))
    return out.reshape(rgb.shape[:-1] + (16,))


def _op(op) -> int:
    if op not in _ffi.IMAGE_OPS:
        raise ValueError(f"unknown image op {op!r} (add, add_unfiltered, splat)")
    return _ffi.IMAGE_OPS[op]


def _samples(xy, spectra):
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    spectra = np.ascontiguousarray(spectra, np.float32).reshape(-1, 16)
    if len(xy) != len(spectra):
        raise ValueError(f"{len(xy)} positions but {len(spectra)} spectra")
    return xy, spectra


def host_add_samples(filter, width, height, xy, spectra, op="add", target=None) -> np.ndarray:
    """bling_host_image_add_samples: the op applied to the samples in order on the CPU, accumulated into target
    (a float32 array of height x width x 4, or x 3 for "splat"; zeros if None), which is returned."""
    desc = filter if isinstance(filter, _ffi.ImageDesc) else image_desc(filter, width, height)
    code = _op(op)
    per = 3 if op == "splat" else 4
    xy, spectra = _samples(xy, spectra)
    if target is None:
        target = np.zeros((desc.height, desc.width, per), np.float32)
    elif not (isinstance(target, np.ndarray) and target.dtype == np.float32 and target.flags.c_contiguous
              and target.size == desc.width * desc.height * per):
        raise ValueError(f"target must be a C-contiguous float32 array of {desc.width * desc.height * per} elements")
    lib = _ffi.host()
    if lib.bling_host_image_add_samples(C.byref(desc), code, _ffi.f32ptr(xy), _ffi.f32ptr(spectra), len(xy), _ffi.f32ptr(target)) != 0:
        raise ValueError(lib.bling_host_last_error().decode())
    return target


class Image:
    """A film (W, X, Y, Z) and a splat image (X, Y, Z) on the device, written by the caller's samples.
    ``.film`` (height x width x 4) and ``.splat`` (height x width x 3) are torch float32 device tensors,
    zero at first (mkImage).  ``context`` shares an existing Context (its scene, if any, is left alone)."""

    _DEVELOP = Context._DEVELOP

    def __init__(self, filter, width: int, height: int, device: int = 0, context: Context | None = None):
        import torch
        self.desc = image_desc(filter, width, height)
        self.width, self.height = self.desc.width, self.desc.height
        self.ctx = context if context is not None else Context(device)
        self._dev = f"cuda:{self.ctx.device}"
        self.film = torch.zeros((self.height, self.width, 4), dtype=torch.float32, device=self._dev)
        self.splat = torch.zeros((self.height, self.width, 3), dtype=torch.float32, device=self._dev)
        self.last_stats: _ffi.ImageStats | None = None
        torch.cuda.synchronize(self.ctx.device)   # the zeros are written before the context's own stream adds to them

    def extent(self):
        """sampleExtent': (x0, x1, y0, y1), inclusive."""
        return image_extent(self.desc)

    def set_budget(self, max_tile_pairs: int = 0):
        """bling_debug_set_image_budget (0: the default)."""
        _check(_ffi.hip().bling_debug_set_image_budget(self.ctx._h, int(max_tile_pairs)))

    def add_samples(self, xy, spectra, op="add") -> _ffi.ImageStats:
        """bling_image_add_samples_device: op "add" (addSample) or "add_unfiltered" into ``.film``, "splat"
        into ``.splat``, the samples in order.  xy (n x 2) and spectra (n x 16) are numpy arrays, or torch
        float32 tensors on this image's device, which are read in place.  The call runs on the context's own
        stream and returns after completion: work of another stream on the tensors must have finished."""
        import torch
        code = _op(op)
        target = self.splat if op == "splat" else self.film
        if isinstance(xy, torch.Tensor) or isinstance(spectra, torch.Tensor):
            for t, what, per in ((xy, "xy", 2), (spectra, "spectra", 16)):
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == self.ctx.device and t.dtype == torch.float32
                        and t.is_contiguous() and t.numel() % per == 0):
                    raise ValueError(f"add_samples: {what} must be a contiguous float32 tensor on {self._dev}")
            n = xy.numel() // 2
            if spectra.numel() // 16 != n:
                raise ValueError(f"{n} positions but {spectra.numel() // 16} spectra")
            torch.cuda.synchronize(self.ctx.device)
        else:
            hx, hs = _samples(xy, spectra)
            n = len(hx)
            xy, spectra = torch.from_numpy(hx).to(self._dev), torch.from_numpy(hs).to(self._dev)
            torch.cuda.synchronize(self.ctx.device)
        st = _ffi.ImageStats()
        _check(_ffi.hip().bling_image_add_samples_device(self.ctx._h, C.byref(self.desc), code, C.c_void_p(xy.data_ptr() if n else None),
                                                         C.c_void_p(spectra.data_ptr() if n else None), n,
                                                         C.c_void_p(target.data_ptr()), C.byref(st)))
        self.last_stats = st
        return st

    def develop(self, fmt="rgb8", window=None, splat_weight=1.0, out=None):
        """bling_image_develop_device of ``.film`` and ``.splat`` (weighted by splat_weight): a torch device
        tensor, "rgb_f32" (float32 h x w x 3), "rgb8" (uint8 h x w x 3) or "rgbe" (uint8 h x w x 4); window =
        (x0, x1, y0, y1), inclusive, develops those pixels only and leaves the rest of out as it was."""
        import torch
        if fmt not in self._DEVELOP:
            raise ValueError(f"develop: unknown format {fmt!r} (rgb_f32, rgb8, rgbe)")
        code, dtype, per = self._DEVELOP[fmt]
        w, h = self.width, self.height
        win = (0, w - 1, 0, h - 1) if window is None else tuple(int(v) for v in window)
        if len(win) != 4:
            raise ValueError("develop: window is (x0, x1, y0, y1)")
        if out is None:
            out = torch.zeros((h, w, per), dtype=getattr(torch, dtype), device=self._dev)
            torch.cuda.synchronize(self.ctx.device)
        op = Context._develop_tensor(out, "out", dtype, w * h * per)
        dp = _ffi.DevelopParams(code, float(np.float32(splat_weight)), (C.c_int32 * 4)(*win))
        _check(_ffi.hip().bling_image_develop_device(self.ctx._h, C.byref(self.desc), C.byref(dp), C.c_void_p(self.film.data_ptr()),
                                                     C.c_void_p(self.splat.data_ptr()), C.c_void_p(op)))
        return out


__all__ = ["Image", "host_add_samples", "make_filter", "eval_filter", "image_desc", "image_extent", "rgb_to_spectrum_illum",
           "BlingError"]
