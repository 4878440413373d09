"""The image API (include/bling.h, "the image API on the device"): the reference's image monad -- mkImage,
addSample', addUnfilteredSample', splatSample, sampleExtent', execImageT (Image.hs) -- for samples the
caller computed, on a film that lives on the device.

    img = Image(("mitchell", 3, 3, 1 / 3, 1 / 3), 480, 270)
    x0, x1, y0, y1 = img.extent()
    img.add_samples(xy, spectra)              # numpy arrays, or torch device tensors (no host copy)
    rgb8 = img.develop("rgb8")

The film after add_samples is, bit for bit, what the reference's one thread makes of it by applying the op
to the samples in order; host_add_samples is that sequential restatement on the CPU.  No scene is needed.

A renderer that computes its samples in parallel windows uses its film as the reference's renderers do -- one
mkImageTile image per SampleWindow, addTile in window order:

    img.tile((0, 15, 0, 15))                  # the tile image's offset, size and sample extent
    img.add_windowed(windows, counts, xy, spectra)   # window k owns counts[k] consecutive samples
    img.scale_splats(1 / passes)              # scaleSplats; a zeroed tensor serves splitMImage

host_add_windowed is the sequential restatement of add_windowed; the device equals it bit for bit.
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


def image_tile(desc: _ffi.ImageDesc, window) -> dict:
    """bling_host_image_tile: mkImageTile of the SampleWindow (x0, x1, y0, y1), ends inclusive -- the tile image's
    offset ``px, py``, size ``w, h`` and its own sampleExtent ``extent``.  ValueError for a tile below 1 x 1."""
    wnd, out = _ffi.ImageWindow(*(int(v) for v in window)), _ffi.ImageTile()
    lib = _ffi.host()
    if lib.bling_host_image_tile(C.byref(desc), C.byref(wnd), C.byref(out)) != 0:
        raise ValueError(lib.bling_host_last_error().decode())
    return {"px": out.px, "py": out.py, "w": out.w, "h": out.h, "extent": tuple(int(v) for v in out.extent)}


def _windows(windows, counts_or_first, n):
    """The ctypes window array and the n_windows + 1 ascending offsets; counts_or_first holds either the windows'
    sample counts or those offsets."""
    wl = [tuple(int(v) for v in w) for w in windows]
    if any(len(w) != 4 for w in wl):
        raise ValueError("a window is (x0, x1, y0, y1)")
    c = np.asarray(counts_or_first, np.int64).reshape(-1)
    if len(c) == len(wl):
        if (c < 0).any():
            raise ValueError("a window's sample count is negative")
        first = np.concatenate([[0], np.cumsum(c)])
    elif len(c) == len(wl) + 1:
        first = c
    else:
        raise ValueError(f"{len(wl)} windows need {len(wl)} counts or {len(wl) + 1} offsets, not {len(c)}")
    if (first < 0).any():
        raise ValueError("a sample offset is negative")
    arr = (_ffi.ImageWindow * max(1, len(wl)))(*(_ffi.ImageWindow(*w) for w in wl))
    return arr, np.ascontiguousarray(first, np.uint64), len(wl)


def _host_target(t, desc, per, what):
    if not (isinstance(t, np.ndarray) and t.dtype == np.float32 and t.flags.c_contiguous and t.size == desc.width * desc.height * per):
        raise ValueError(f"{what} must be a C-contiguous float32 array of {desc.width * desc.height * per} elements")
    return t


def host_add_windowed(filter, width, height, windows, counts_or_first, xy, spectra, op="add", film=None, splat=None, stats=None):
    """bling_host_image_add_windowed: per window, in order, a zeroed mkImageTile image takes the op of the window's
    samples and addTile adds it onto film (height x width x 4) and splat (height x width x 3), float32 arrays
    accumulated into (zeros if None; pass False for an image that is to be left out, i.e. NULL).  Returns
    (film, splat); stats, an _ffi.ImageStats, receives the counters."""
    desc = filter if isinstance(filter, _ffi.ImageDesc) else image_desc(filter, width, height)
    code = _op(op)
    xy, spectra = _samples(xy, spectra)
    arr, first, nw = _windows(windows, counts_or_first, len(xy))
    if film is None:
        film = np.zeros((desc.height, desc.width, 4), np.float32)
    if splat is None:
        splat = np.zeros((desc.height, desc.width, 3), np.float32)
    fp = _ffi.f32ptr(_host_target(film, desc, 4, "film")) if film is not False else None
    sp = _ffi.f32ptr(_host_target(splat, desc, 3, "splat")) if splat is not False else None
    lib = _ffi.host()
    st = stats if stats is not None else _ffi.ImageStats()
    if lib.bling_host_image_add_windowed(C.byref(desc), code, arr, first.ctypes.data_as(C.POINTER(C.c_uint64)), nw, _ffi.f32ptr(xy),
                                         _ffi.f32ptr(spectra), len(xy), fp, sp, C.byref(st)) != 0:
        raise ValueError(lib.bling_host_last_error().decode())
    return (None if film is False else film), (None if splat is False else splat)


def host_scale_splats(desc: _ffi.ImageDesc, splat: np.ndarray, factors_or_scalar) -> np.ndarray:
    """bling_host_image_scale_splats (scaleSplats) of a float32 height x width x 3 array, in place: a per-pixel
    float32 array of factors, or one scalar."""
    _host_target(splat, desc, 3, "splat")
    lib = _ffi.host()
    if np.ndim(factors_or_scalar) == 0:
        rc = lib.bling_host_image_scale_splats(C.byref(desc), _ffi.f32ptr(splat), None, float(np.float32(factors_or_scalar)))
    else:
        f = np.ascontiguousarray(factors_or_scalar, np.float32)
        if f.size != desc.width * desc.height:
            raise ValueError(f"factors must hold {desc.width * desc.height} values")
        rc = lib.bling_host_image_scale_splats(C.byref(desc), _ffi.f32ptr(splat), _ffi.f32ptr(f), 0.0)
    if rc != 0:
        raise ValueError(lib.bling_host_last_error().decode())
    return splat


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

    def _device_samples(self, xy, spectra):
        """xy and spectra as float32 tensors on this image's device (torch tensors are taken as they are, numpy
        arrays are copied over) and the number of samples; the device has finished with them on return."""
        import torch
        if isinstance(xy, torch.Tensor) or isinstance(spectra, torch.Tensor):
            for t, what, per in ((xy, "xy", 2), (spectra, "spectra", 16)):
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == self.ctx.device and t.dtype == torch.float32
                        and t.is_contiguous() and t.numel() % per == 0):
                    raise ValueError(f"add_samples: {what} must be a contiguous float32 tensor on {self._dev}")
            n = xy.numel() // 2
            if spectra.numel() // 16 != n:
                raise ValueError(f"{n} positions but {spectra.numel() // 16} spectra")
        else:
            hx, hs = _samples(xy, spectra)
            n = len(hx)
            xy, spectra = torch.from_numpy(hx).to(self._dev), torch.from_numpy(hs).to(self._dev)
        torch.cuda.synchronize(self.ctx.device)
        return xy, spectra, n

    def tile(self, window) -> dict:
        """mkImageTile of the SampleWindow (x0, x1, y0, y1): see image_tile."""
        return image_tile(self.desc, window)

    def add_windowed(self, windows, counts_or_first, xy, spectra, op="add") -> _ffi.ImageStats:
        """bling_image_add_windowed_device: what a renderer does with its film -- per window (x0, x1, y0, y1), in
        order, a zeroed tile image takes the op of the window's samples, and addTile adds it onto ``.film`` and
        ``.splat``.  counts_or_first: the windows' sample counts, or the n_windows + 1 ascending offsets into the
        sample list.  xy and spectra as for add_samples.  The result equals host_add_windowed bit for bit."""
        code = _op(op)
        xy, spectra, n = self._device_samples(xy, spectra)
        arr, first, nw = _windows(windows, counts_or_first, n)
        st = _ffi.ImageStats()
        _check(_ffi.hip().bling_image_add_windowed_device(self.ctx._h, C.byref(self.desc), code, arr,
                                                          first.ctypes.data_as(C.POINTER(C.c_uint64)), nw,
                                                          C.c_void_p(xy.data_ptr() if n else None),
                                                          C.c_void_p(spectra.data_ptr() if n else None), n,
                                                          C.c_void_p(self.film.data_ptr()), C.c_void_p(self.splat.data_ptr()), C.byref(st)))
        self.last_stats = st
        return st

    def scale_splats(self, factors_or_scalar):
        """bling_image_scale_splats_device (scaleSplats): every pixel's three ``.splat`` values times its factor --
        a height x width array (numpy, or a float32 tensor on this image's device) -- or times one scalar."""
        import torch
        if np.ndim(factors_or_scalar) == 0 and not isinstance(factors_or_scalar, torch.Tensor):
            f, scalar = None, float(np.float32(factors_or_scalar))
        else:
            f, scalar = factors_or_scalar, 0.0
            if not isinstance(f, torch.Tensor):
                f = torch.from_numpy(np.ascontiguousarray(f, np.float32)).to(self._dev)
            if not (f.is_cuda and f.device.index == self.ctx.device and f.dtype == torch.float32 and f.is_contiguous()
                    and f.numel() == self.width * self.height):
                raise ValueError(f"scale_splats: factors must be {self.width * self.height} contiguous float32 values on {self._dev}")
        torch.cuda.synchronize(self.ctx.device)
        _check(_ffi.hip().bling_image_scale_splats_device(self.ctx._h, C.byref(self.desc), C.c_void_p(self.splat.data_ptr()),
                                                          C.c_void_p(f.data_ptr() if f is not None else None), scalar))

    def add_samples(self, xy, spectra, op="add") -> _ffi.ImageStats:
        """bling_image_add_samples_device: op "add" (addSample) or "add_unfiltered" into ``.film``, "splat"
        into ``.splat``, the samples in order.  xy (n x 2) and spectra (n x 16) are numpy arrays, or torch
        float32 tensors on this image's device, which are read in place.  The call runs on the context's own
        stream and returns after completion: work of another stream on the tensors must have finished."""
        code = _op(op)
        target = self.splat if op == "splat" else self.film
        xy, spectra, n = self._device_samples(xy, spectra)
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


__all__ = ["Image", "host_add_samples", "host_add_windowed", "host_scale_splats", "image_tile","make_filter", "eval_filter", "image_desc", "image_extent", "rgb_to_spectrum_illum",
           "BlingError"]
