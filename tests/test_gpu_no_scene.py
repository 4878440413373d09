"""How the entry points of the three light-path renderers, and two of the pass driver's, refuse: BLING_ENOSCENE
with "no scene uploaded" on a context that holds no scene, and BLING_EINVAL with the renderer's own text once
the cornell box is uploaded with the sampler renderer.  Straight through the C ABI (the Python wrappers check for
a scene themselves); no pass is rendered."""
import ctypes as C

import numpy as np
import pytest
import torch

from bling_amd import _ffi
from bling_amd.render import SPLAT_REC, Context
from bling_amd.scene import load_config

pytestmark = pytest.mark.gpu
ENOSCENE, EINVAL = -4, -1
W = H = 8


def _calls(lib, ctx, dev):
    """name -> a call with valid, tiny arguments: host images of W x H pixels, `dev` as the device image."""
    h = ctx._h
    film, splat = np.zeros(W * H * 4, np.float32), np.zeros(W * H * 3, np.float32)
    dptr = C.c_void_p(dev.data_ptr())
    pp = _ffi.PassParams(1, 0, 0, 1, 1, 0, 0)
    rays = np.zeros(8, np.float32)
    prim = np.zeros(1, np.uint32)
    rec = np.zeros(1, SPLAT_REC)
    n = C.c_size_t()
    return {
        "bling_sppm_pass": lambda: lib.bling_sppm_pass(h, 1, 1, _ffi.f32ptr(film), _ffi.f32ptr(splat), None),
        "bling_sppm_pass_device": lambda: lib.bling_sppm_pass_device(h, 1, 1, 0, dptr, None, None),
        "bling_sppm_pixel_stats": lambda: lib.bling_sppm_pixel_stats(h, None, None, C.byref(n)),
        "bling_light_pass": lambda: lib.bling_light_pass(h, 1, 1, _ffi.f32ptr(splat), None),
        "bling_light_pass_device": lambda: lib.bling_light_pass_device(h, 1, 1, 0, dptr, None),
        "bling_mlt_pass": lambda: lib.bling_mlt_pass(h, 1, 1, _ffi.f32ptr(splat), None),
        "bling_mlt_pass_device": lambda: lib.bling_mlt_pass_device(h, 1, 1, 0, dptr, None),
        "bling_debug_splat_merge": lambda: lib.bling_debug_splat_merge(h, C.c_void_p(rec.ctypes.data), 1, dptr),
        "bling_render_pass": lambda: lib.bling_render_pass(h, C.byref(pp), _ffi.f32ptr(film), None),
        "bling_trace": lambda: lib.bling_trace(h, _ffi.f32ptr(rays), 1, 0, None, _ffi.u32ptr(prim), None),
    }


def test_refusals_without_a_scene_and_with_another_renderer():
    lib = _ffi.hip()
    dev = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ctx = Context(0)
    for name, call in _calls(lib, ctx, dev).items():
        assert call() == ENOSCENE, name
        assert lib.bling_last_error() == b"no scene uploaded", name

    ctx.upload(load_config("C1", f"image={W},{H}"))                  # cornell-box.bling, sampler renderer
    calls = _calls(lib, ctx, dev)
    not_mine = {
        "bling_sppm_pass": b"the uploaded scene's renderer is not sppm",
        "bling_sppm_pass_device": b"the uploaded scene's renderer is not sppm",
        "bling_sppm_pixel_stats": b"the uploaded scene's renderer is not sppm",
        "bling_light_pass": b"the uploaded scene's renderer is not the light tracer",
        "bling_light_pass_device": b"the uploaded scene's renderer is not the light tracer",
        "bling_mlt_pass": b"the uploaded scene's renderer is not metropolis",
        "bling_mlt_pass_device": b"the uploaded scene's renderer is not metropolis",
    }
    for name, text in not_mine.items():
        assert calls[name]() == EINVAL, name
        assert lib.bling_last_error() == text, name
    assert not dev.any().item()                                     # nothing was rendered into the device image
    ctx.close()
