"""Tiny scenes for the textured material parameters (tests/test_param_textures.py on the CPU,
tests/test_gpu_param_textures.py on the device): one ground quad and one sphere that share the material
under test, a quad area light and a constant infinite light, 24 x 24 pixels, `stratified 2 2`.

Three ways to write each parameter:

  * constant                     -- what the oracle renders
  * identity-textured            -- the same value c through a non-constant kind that evaluates to exactly
                                    c: a scalar as `scale c 0 tex { perlin }` = c + 0 * t (Texture.hs:185-186),
                                    a spectrum as a checker whose two children are both the constant c
  * two-valued                   -- the value varies in space between A and B: a scalar through a 2 x 2 Y8
                                    image on a planar mapping, a spectrum through a checker of two constants

and the numpy binary32 restatements of the two lookups that tell a hit point's class (0 = A, 1 = B).
"""
import os
import struct
import zlib

import numpy as np

f32 = np.float32

HEAD = """imageSize 24 24
renderer {
   sampler
   sampled {
      sampler { stratified 2 2 }
      integrator { path maxDepth 5 sampleDepth 3 }
   }
}
transform { lookAt { pos 0 4 -5 look 0 0.5 0 up 0 1 0 } }
camera { perspective fov 50 lensRadius 0 focalDistance 10 }
light { infinite { rotateX -90 } l { constant rgbI 0.4 0.4 0.5 } }
"""
BODY = """newTransform { rotateX -90 }
material { %s }
prim { shape { quad 20 20 } }
newTransform { translate 0 1 0 }
prim { shape { sphere radius 1 } }
newTransform { rotateX -90 translate 0 6 0 }
material { matte kd { constant rgbR 0 0 0 } sigma { constant 0 } }
emission { rgbI 8 8 8 }
prim { shape { quad 3 3 } }
"""
PERLIN = "perlin map { identity { scale 3 3 3 } }"
IMAGE = "ab.png"
# spectra: plain ones, and two with bands above 1 and bands at 0 (tests/test_param_textures.py checks it)
GREY, WARM, COOL = "rgbR 0.5 0.5 0.5", "rgbR 0.7 0.5 0.3", "rgbR 0.3 0.4 0.5"
WIDE = "spd { 380 0 , 450 0 , 520 1.8 , 600 0.6 , 680 0 , 720 0 }"
WIDE2 = "spd { 380 1.4 , 460 0.2 , 540 0 , 600 0 , 660 1.2 , 720 0.9 }"


def num(v) -> str:
    """A binary32 value in decimal digits that parse back to it."""
    return np.format_float_positional(f32(v), unique=True, trim="-")


def scalar(c, how):
    """A scalar parameter's texture block body: how = "const" | "ident"."""
    return f"constant {num(c)}" if how == "const" else f"scale {num(c)} 0 tex {{ {PERLIN} }}"


def spectrum(c, how):
    return f"constant {c}" if how == "const" else f"checker 1 1 1 tex1 {{ constant {c} }} tex2 {{ constant {c} }}"


def byte_value(b):
    """getPixelScalar's value of a Y8 byte (the loader's byte / 255)."""
    return f32(f32(b) / f32(255))


def image_scalar(pre=""):
    """The two-valued scalar: texel (floor x mod 2, floor (-z) mod 2) of the 2 x 2 image."""
    img = f"image {{ file \"{IMAGE}\" map {{ planar 0.5 0 0 0 0 0.5 0 0 }} }}"
    return f"{pre} tex {{ {img} }}" if pre else img


def checker2(a, b):
    """The two-valued spectrum: unit cells in x and z (the ground lies in y = 0, so y takes no part)."""
    return f"checker 1 0 1 tex1 {{ constant {a} }} tex2 {{ constant {b} }}"


def write_png_y8(path, rows):
    """An 8-bit greyscale PNG of the given rows of bytes (top row first)."""
    h, w = len(rows), len(rows[0])

    def chunk(typ, body):
        return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body) & 0xFFFFFFFF)
    raw = b"".join(b"\0" + bytes(r) for r in rows)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def write_scene(dirpath, name, material, bytes_ab=None):
    """Write <name>.bling (and the image [[A, B], [B, A]] when bytes_ab is given); returns its path."""
    os.makedirs(dirpath, exist_ok=True)
    if bytes_ab is not None:
        a, b = bytes_ab
        write_png_y8(os.path.join(dirpath, IMAGE), [[a, b], [b, a]])
    p = os.path.join(dirpath, name + ".bling")
    with open(p, "w") as f:
        f.write(HEAD + BODY % material)
    return p


# ---------------------------------------------------------------- the thirteen slots
def _mat(kind, **slots):
    return kind + " " + " ".join(f"{k} {{ {v} }}" for k, v in slots.items())


def material(case, how):
    """The material text of an identity case with its parameters constant (how = "const") or
    identity-textured (how = "ident"); cases that texture only some slots keep the others constant."""
    s = lambda c: scalar(c, how)
    k = lambda c: spectrum(c, how)
    kc = lambda c: spectrum(c, "const")
    if case == "matte_sigma0":
        return _mat("matte", kd=kc(WARM), sigma=s(0))
    if case == "matte_sigma":
        return _mat("matte", kd=kc(WARM), sigma=s(0.5))
    if case == "plastic_rough":                        # 1 / rough = 20 000: fixExponent caps it
        return _mat("plastic", kd=kc(WARM), ks=kc(GREY), rough=s(0.00005))
    if case == "glass_ior":
        return _mat("glass", ior=s(1.5), kr=kc("rgbR 1 1 1"), kt=kc("rgbR 0.9 1 0.9"))
    if case == "metal_rough":
        return _mat("metal", eta=kc("rgbR 0.2 0.4 1.4"), k=kc("rgbR 3 2.5 2"), rough=s(0.00008))
    if case == "transmatte":                           # ks, kr and kt
        return _mat("transMatte", kr=k(WIDE), kt=k(WIDE2), ks=s(0.3))
    if case == "transmatte_kt":                        # raw with a constant kr; sigma 0: Lambertian lobes
        return _mat("transMatte", kr=kc(COOL), kt=k(WIDE), ks=scalar(0, "const"))
    if case == "shinymetal":                           # rough, kr and ks
        return _mat("shinyMetal", kr=k(WIDE), ks=k(WIDE2), rough=s(0.05))
    if case == "shinymetal_ks":                        # ks raw, kr folded
        return _mat("shinyMetal", kr=kc(WARM), ks=k(WIDE), rough=scalar(0.00002, "const"))
    if case == "substrate":                            # kd, ks and ka
        return _mat("substrate", kd=k(WIDE), ks=k(WIDE2), ka=k(WARM), urough=scalar(0.1, "const"),
                    vrough=scalar(0.2, "const"), depth=scalar(0.5, "const"))
    raise KeyError(case)


IDENTITY_CASES = ["matte_sigma0", "matte_sigma", "plastic_rough", "glass_ior", "metal_rough", "transmatte",
                  "transmatte_kt", "shinymetal", "shinymetal_ks", "substrate"]

# one material per slot with only that slot textured: (name, material text)
SLOTS = [
    ("matte.sigma", _mat("matte", kd=spectrum(WARM, "const"), sigma=scalar(0.5, "ident"))),
    ("plastic.rough", _mat("plastic", kd=spectrum(WARM, "const"), ks=spectrum(GREY, "const"), rough=scalar(0.1, "ident"))),
    ("glass.ior", _mat("glass", ior=scalar(1.5, "ident"), kr=spectrum(GREY, "const"), kt=spectrum(GREY, "const"))),
    ("metal.rough", _mat("metal", eta=spectrum(GREY, "const"), k=spectrum(WARM, "const"), rough=scalar(0.1, "ident"))),
    ("transMatte.ks", _mat("transMatte", kr=spectrum(COOL, "const"), kt=spectrum(GREY, "const"), ks=scalar(0.3, "ident"))),
    ("transMatte.kr", _mat("transMatte", kr=spectrum(COOL, "ident"), kt=spectrum(GREY, "const"), ks=scalar(0.3, "const"))),
    ("transMatte.kt", _mat("transMatte", kr=spectrum(COOL, "const"), kt=spectrum(GREY, "ident"), ks=scalar(0.3, "const"))),
    ("shinyMetal.rough", _mat("shinyMetal", kr=spectrum(WARM, "const"), ks=spectrum(GREY, "const"), rough=scalar(0.05, "ident"))),
    ("shinyMetal.kr", _mat("shinyMetal", kr=spectrum(WARM, "ident"), ks=spectrum(GREY, "const"), rough=scalar(0.05, "const"))),
    ("shinyMetal.ks", _mat("shinyMetal", kr=spectrum(WARM, "const"), ks=spectrum(GREY, "ident"), rough=scalar(0.05, "const"))),
] + [("substrate." + slot, _mat("substrate", **{s: spectrum(WARM, "ident" if s == slot else "const") for s in ("kd", "ks", "ka")},
                                urough=scalar(0.1, "const"), vrough=scalar(0.2, "const"), depth=scalar(0.5, "const")))
     for slot in ("kd", "ks", "ka")]


# ---------------------------------------------------------------- two-valued cases
def _two(kind, how, **slots):
    """slots: name -> a constant text, or ("s", byteA, byteB[, pre]) / ("k", A, B) for the varying ones.
    how = 0 / 1: the constant scene of class A / B; how = "tex": the two-valued scene."""
    out, img = {}, None
    for name, v in slots.items():
        if isinstance(v, tuple) and v[0] == "s":
            pre = v[3] if len(v) > 3 else ""
            if how == "tex":
                out[name], img = image_scalar(pre), (v[1], v[2])
            else:
                t = byte_value(v[1 + how])
                if pre:                                       # scale a s: a + s * t
                    a, s = (f32(x) for x in pre.split()[1:3])
                    t = f32(a + f32(s * t))
                out[name] = scalar(t, "const")
        elif isinstance(v, tuple) and v[0] == "k":
            out[name] = checker2(v[1], v[2]) if how == "tex" else spectrum(v[1 + how], "const")
        elif isinstance(v, tuple) and v[0] == "i":            # identity-textured in the two-valued scene only
            out[name] = scalar(v[1], "ident" if how == "tex" else "const")
        else:
            out[name] = v
    return _mat(kind, **out), img


def two_valued(case, how):
    """(material text, image bytes (A, B) or None) of a two-valued case."""
    kc = lambda c: spectrum(c, "const")
    if case == "matte_sigma":                          # 0 -> Lambertian, 153 / 255 = 0.6 -> Oren-Nayar
        return _two("matte", how, kd=kc(WARM), sigma=("s", 0, 153))
    if case == "plastic_rough":
        return _two("plastic", how, kd=kc(COOL), ks=kc(GREY), rough=("s", 51, 13))
    if case == "metal_rough":
        return _two("metal", how, eta=kc("rgbR 0.2 0.4 1.4"), k=kc("rgbR 3 2.5 2"), rough=("s", 51, 13))
    if case == "glass_ior":                            # 1 + t: 1.2 and 1.6
        return _two("glass", how, ior=("s", 51, 153, "scale 1 1"), kr=kc("rgbR 1 1 1"), kt=kc("rgbR 0.9 1 0.9"))
    if case == "transmatte_kr":
        return _two("transMatte", how, kr=("k", COOL, WIDE), kt=kc(GREY), ks=("i", 0.3))
    if case == "shinymetal":
        return _two("shinyMetal", how, kr=("k", WARM, WIDE), ks=("k", GREY, WIDE2), rough=scalar(0.05, "const"))
    if case == "substrate_kd":
        return _two("substrate", how, kd=("k", WARM, WIDE), ks=kc(GREY), ka=kc(COOL), urough=scalar(0.1, "const"),
                    vrough=scalar(0.2, "const"), depth=scalar(0.5, "const"))
    raise KeyError(case)


TWO_VALUED_CASES = ["matte_sigma", "plastic_rough", "metal_rough", "glass_ior", "transmatte_kr", "shinymetal",
                    "substrate_kd"]
BOUNDARY = f32(1e-3)       # hit points within this of a cell border are left out


def classify(p, by_image):
    """Class (0 = A, 1 = B, -1 = left out) of the hit points p (n, 3), in binary32 as the device forms it.

    image:   planarMapping (0.5, 0, 0) (0, 0, 0.5) (0, 0): s = (px 0.5 + py 0 + pz 0) + 0, t likewise with
             pz; getPixelScalar's pixel x = floor (s w) mod w, y = floor (-t h) mod h (Texture.hs:96-108),
             w = h = 2; the image is [[A, B], [B, A]].
    checker: checkerBoard (1, 0, 1) (Texture.hs:209-219): floor (px 1) + floor (py 0) + floor (pz 1), even -> A.
    A point without a hit (NaN) or near a border is left out."""
    p = np.asarray(p, f32)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore"):
        if by_image:
            s = ((px * f32(0.5) + py * f32(0)) + pz * f32(0)) + f32(0)
            t = ((px * f32(0) + py * f32(0)) + pz * f32(0.5)) + f32(0)
            cx, cy = s * f32(2), -t * f32(2)
        else:
            cx, cy = px * f32(1), pz * f32(1)
        ix, iy = np.floor(cx), np.floor(cy)
        cls = ((ix + iy) % 2).astype(np.int64)         # [[A, B], [B, A]] and the checker: parity of the cell
        near = (np.abs(cx - np.round(cx)) < BOUNDARY) | (np.abs(cy - np.round(cy)) < BOUNDARY)
        bad = near | ~np.isfinite(cx) | ~np.isfinite(cy)
    return np.where(bad, -1, np.where(np.isnan(ix + iy), -1, cls)).astype(np.int64)


def all_samples(job):
    """Every (x, y, n) sample of the job's extent."""
    x0, x1, y0, y1 = job.extent()
    xs, ys, ns = np.meshgrid(np.arange(x0, x1 + 1), np.arange(y0, y1 + 1), np.arange(job.spp), indexing="ij")
    return np.stack([xs.ravel(), ys.ravel(), ns.ravel()], 1).astype(np.int32)
