"""A float64 restatement of the reference's analytic shapes under arbitrary affine transforms, written
from the Haskell text alone (one function per reference function, `file:line` cited), vectorised
with numpy over a batch of rays or points.  tests/test_xform_shapes.py measures the binary32 oracle
against it.

Haskell's guards are tried in order and a comparison with a NaN operand is False, so every guard
list is restated as a `_Guards` chain: a lane takes the first guard that holds for it.  `min` / `max`
are GHC's (`min x y = if x <= y then x else y`, `max x y = if x <= y then y else x`), so with a NaN
operand `min` returns its second argument and `max` its first (hmin / hmax).

Every decision also yields its margin: |a - b| / max(|a|, |b|) of the two compared operands, in
float64.  A ray whose smallest margin is below NEAR lies near a boundary; binary32 may decide it the
other way, and the tests leave it out of their equality checks (and bound how many there are).

MUTATIONS names deliberate misreadings; `Ref(mutation=...)` applies one.  They are the negative
controls of test_xform_shapes.py.
"""
import math

import numpy as np

INF = np.inf
TWO_PI = 2.0 * math.pi
NEAR = 1e-4
MUTATIONS = ("normal_forward", "normalized_dir", "world_area", "cyl_sample_phimax", "box_inside_closest")

f32 = np.float32


def r32(x):
    """A scene-file number as the loader reads it: rounded to binary32, then exact in float64."""
    return np.asarray(x, f32).astype(np.float64)


# ------------------------------------------------------------------ Math.hs
def hmin(x, y):
    with np.errstate(invalid="ignore"):
        return np.where(x <= y, x, y)


def hmax(x, y):
    with np.errstate(invalid="ignore"):
        return np.where(x <= y, y, x)


def rel(a, b):
    """Decision margin of comparing a with b; inf where either is not finite or both are exactly 0
    (such a comparison falls the same way in every precision)."""
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    with np.errstate(all="ignore"):
        m = np.abs(a - b) / np.maximum(np.abs(a), np.abs(b))
    return np.where(np.isfinite(a) & np.isfinite(b) & ~((a == 0) & (b == 0)), m, INF)


class _Guards:
    """An ordered guard list over lanes: `take(cond)` returns the lanes that reach this guard and
    satisfy it, and removes them from the undecided."""

    def __init__(self, n):
        self.und = np.ones(n, bool)

    def take(self, cond):
        with np.errstate(invalid="ignore"):
            m = self.und & np.asarray(cond, bool)
        self.und = self.und & ~m
        return m

    def rest(self):
        m, self.und = self.und, np.zeros_like(self.und)
        return m


def dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]     # Math.hs:343


def sq_len(v):
    return dot(v, v)                                                              # Math.hs:330


def cross(u, v):                                                                  # Math.hs:338-339
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], -(u[..., 0] * v[..., 2] - u[..., 2] * v[..., 0]),
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def normalize(v):                                                                 # Math.hs:351-353
    l2 = sq_len(v)
    with np.errstate(all="ignore"):
        out = v * (1.0 / np.sqrt(l2))[..., None]
    up = np.zeros_like(v)
    up[..., 1] = 1.0
    return np.where((l2 != 0)[..., None], out, up)


def atan2p(y, x):                                                                 # Math.hs:71-75
    a = np.arctan2(y, x)
    return np.where(a < 0, a + TWO_PI, a)


def lerp(t, v1, v2):                                                              # Math.hs:110
    return (1 - t) * v1 + t * v2


def clamp(v, lo, hi):                                                             # Math.hs:84-87
    return lo if v < lo else hi if v > hi else v


def radians(x):                                                                   # Math.hs:66
    return x / 180.0 * math.pi


def solve_quadric(a, b, c):
    """solveQuadric (Math.hs:130-139): (has roots, t0, t1, margin of the discriminant's sign)."""
    with np.errstate(all="ignore"):
        discrim = b * b - 4 * a * c
        root = np.sqrt(discrim)
        q = np.where(b < 0, -0.5 * (b - root), -0.5 * (b + root))
        t0, t1 = q / a, c / q
        ok = ~(discrim < 0)
    return ok, hmin(t0, t1), hmax(t0, t1), rel(b * b, 4 * a * c)


def coordinate_system(v):                                                         # Math.hs:415-425
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    with np.errstate(all="ignore"):
        i1 = 1.0 / np.sqrt(x * x + z * z)
        i2 = 1.0 / np.sqrt(y * y + z * z)
    o = np.zeros_like(x)
    v2 = np.where((np.abs(x) > np.abs(y))[..., None], np.stack([-z * i1, o, x * i1], -1), np.stack([o, z * i2, -y * i2], -1))
    return v2, cross(v, v2), v


def uniform_sample_cone(cs, cos_max, u1, u2):                                     # Montecarlo.hs:135-144
    x, y, z = cs
    ct = lerp(u1, cos_max, 1.0)
    st = np.sqrt(1 - ct * ct)
    phi = u2 * TWO_PI
    return x * (np.cos(phi) * st)[..., None] + y * (np.sin(phi) * st)[..., None] + z * ct[..., None]


def uniform_cone_pdf(cos_max):                                                    # Montecarlo.hs:129-131
    with np.errstate(all="ignore"):
        return np.where(cos_max >= 1, 0.0, 1 / (TWO_PI * (1 - cos_max)))


def uniform_sample_sphere(u1, u2):                                                # Montecarlo.hs:183-186
    u = u1 * 2 - 1
    s = np.sqrt(1 - u * u)
    om = u2 * 2 * math.pi
    return np.stack([s * np.cos(om), s * np.sin(om), u], -1)


def concentric_sample_disk(u1, u2):                                              # Montecarlo.hs:160-177
    sx, sy = u1 * 2 - 1, u2 * 2 - 1
    with np.errstate(all="ignore"):
        a = sx >= -sy
        r = np.where(a, np.where(sx > sy, sx, sy), np.where(sx <= sy, -sx, -sy))
        th = np.where(a, np.where(sx > sy, np.where(sy > 0, sy / sx, 8 + sy / sx), 2 - sx / sy),
                      np.where(sx <= sy, 4 - sy / (-sx), 6 + sx / (-sy)))
    th = th * math.pi / 4
    zero = (sx == 0) & (sy == 0)
    return np.where(zero, 0.0, r * np.cos(th)), np.where(zero, 0.0, r * np.sin(th))


def cosine_sample_hemisphere(n, u1, u2):                                         # Montecarlo.hs:152-158, Math.hs:445-449
    x, y = concentric_sample_disk(u1, u2)
    z = np.sqrt(np.maximum(0, 1 - x * x - y * y))
    sn, tn, nn = coordinate_system(n)
    return sn * x[..., None] + tn * y[..., None] + nn * z[..., None]


def remap_rand(segs, u):                                                          # Math.hs:118-121
    seg = np.minimum(segs - 1, np.floor(u * segs).astype(int))
    return seg, (u - seg / segs) * segs


# ------------------------------------------------------------------ Transform.hs
class Transform:
    """MkTransform (Transform.hs:124-127): the matrix and its inverse, carried side by side."""

    def __init__(self, m, i):
        self.m, self.i = np.asarray(m, np.float64), np.asarray(i, np.float64)


def _mul(m1, m2):
    """mul (Transform.hs:102-105): element (i, j) = sum_k m1[k][j] * m2[i][k] -- that is m2 . m1."""
    out = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            out[i, j] = sum(m1[k, j] * m2[i, k] for k in range(4))
    return out


IDENTITY = Transform(np.eye(4), np.eye(4))                                         # Transform.hs:144-145


def concat(t1, t2):                                                               # Transform.hs:241-244
    return Transform(_mul(t1.m, t2.m), _mul(t2.i, t1.i))


def mconcat(ts):
    """mconcat = foldr (<>) mempty (Transform.hs:132-134; IO/TransformParser.hs pTransform)."""
    acc = IDENTITY
    for t in reversed(ts):
        acc = concat(t, acc)
    return acc


def inverse(t):                                                                   # Transform.hs:238-239
    return Transform(t.i, t.m)


def translate(d):                                                                 # Transform.hs:148-160
    m, i = np.eye(4), np.eye(4)
    m[:3, 3], i[:3, 3] = d, -np.asarray(d)
    return Transform(m, i)


def scale(s):                                                                     # Transform.hs:163-175
    return Transform(np.diag([s[0], s[1], s[2], 1.0]), np.diag([1 / s[0], 1 / s[1], 1 / s[2], 1.0]))


def _rot(deg, rows):
    s, c = math.sin(radians(deg)), math.cos(radians(deg))
    m = np.eye(4)
    for (r, k), v in rows(s, c).items():
        m[r, k] = v
    return Transform(m, m.T)


def rotate_x(deg):                                                                # Transform.hs:176-184
    return _rot(deg, lambda s, c: {(1, 1): c, (1, 2): -s, (2, 1): s, (2, 2): c})


def rotate_y(deg):                                                                # Transform.hs:186-194
    return _rot(deg, lambda s, c: {(0, 0): c, (0, 2): s, (2, 0): -s, (2, 2): c})


def rotate_z(deg):                                                                # Transform.hs:196-204
    return _rot(deg, lambda s, c: {(0, 0): c, (0, 1): -s, (1, 0): s, (1, 1): c})


_CTORS = {"scale": scale, "translate": translate, "rotateX": rotate_x, "rotateY": rotate_y, "rotateZ": rotate_z}


def from_spec(spec):
    """A `newTransform { ... }` block given as [(word, arguments), ...] in the file's order."""
    ts = []
    for word, arg in spec:
        a = r32(arg)
        ts.append(_CTORS[word](float(a) if a.ndim == 0 else a))
    return mconcat(ts)


def trans_point(t, p):                                                            # Transform.hs:247-256
    m = t.m
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    with np.errstate(all="ignore"):
        q = np.stack([m[r, 0] * x + m[r, 1] * y + m[r, 2] * z + m[r, 3] for r in range(3)], -1)
        wp = m[3, 0] * x + m[3, 1] * y + m[3, 2] * z + m[3, 3]
        return np.where((wp == 1)[..., None], q, q / wp[..., None])


def trans_vector(t, v):                                                           # Transform.hs:259-264
    m = t.m
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    return np.stack([m[r, 0] * x + m[r, 1] * y + m[r, 2] * z for r in range(3)], -1)


def trans_normal(t, n, mutation=None):                                            # Transform.hs:267-272
    if mutation == "normal_forward":
        return trans_vector(t, n)
    m = t.i
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    return np.stack([m[0, c] * x + m[1, c] * y + m[2, c] * z for c in range(3)], -1)


def trans_box(t, lo, hi):                                                         # Transform.hs:281-292
    pts = np.array([[(hi if c & 4 else lo)[0], (hi if c & 2 else lo)[1], (hi if c & 1 else lo)[2]] for c in range(8)])
    w = trans_point(t, pts)
    return w.min(0), w.max(0)


# ------------------------------------------------------------------ Shape.hs
def mk_shape(kind, **p):
    """mkBox / mkCylinder / mkDisk / mkQuad / mkSphere (Shape.hs:41-78) from a scene file's numbers."""
    p = {k: r32(v) for k, v in p.items()}
    if kind == "box":
        return ("box", np.minimum(p["pmin"], p["pmax"]), np.maximum(p["pmin"], p["pmax"]))
    if kind == "cylinder":
        return ("cylinder", float(p["radius"]), float(min(p["zmin"], p["zmax"])), float(max(p["zmin"], p["zmax"])),
                radians(clamp(float(p["phiMax"]), 0.0, 360.0)))
    if kind == "disk":
        return ("disk", float(p["height"]), float(max(p["radius"], p["innerRadius"])), float(min(p["radius"], p["innerRadius"])),
                radians(clamp(float(p["phiMax"]), 0.0, 360.0)))
    if kind == "quad":
        return ("quad", float(p["sx"]), float(p["sy"]))
    assert kind == "sphere"
    return ("sphere", float(p["radius"]))


def object_bounds(s):                                                             # Shape.hs:299-311
    k = s[0]
    if k == "box":
        return s[1], s[2]
    if k == "cylinder":
        return np.array([-s[1], -s[1], s[2]]), np.array([s[1], s[1], s[3]])
    if k == "disk":
        return np.array([-s[2], -s[2], s[1]]), np.array([s[2], s[2], s[1]])
    if k == "quad":
        return np.array([-s[1], -s[2], 0.0]), np.array([s[1], s[2], 0.0])
    return np.full(3, -s[1]), np.full(3, s[1])


def area(s):                                                                      # Shape.hs:317-328
    k = s[0]
    if k == "box":
        h, w, l = s[2] - s[1]
        return 2 * (h * w + h * l + w * l)
    if k == "cylinder":
        return 2 * math.pi * s[1] * (s[3] - s[2])
    if k == "disk":
        return math.pi * (s[2] * s[2] - s[3] * s[3])
    if k == "quad":
        return 4 * s[1] * s[2]
    return s[1] * s[1] * 4 * math.pi


def _ray_at(o, d, t):                                                             # Math.hs:390
    with np.errstate(all="ignore"):
        return o + d * t[..., None]


def _phi_margin(phi, phimax):
    """phi against phimax and against the 0 / 2 pi seam (which matters only for a partial sweep)."""
    if phimax >= TWO_PI:
        return np.full(phi.shape, INF)
    return np.minimum(np.abs(phi - phimax), np.minimum(phi, TWO_PI - phi)) / TWO_PI


def intersect(s, o, d, tmin, tmax, mutation=None):
    """Shape.intersect (Shape.hs:86-229): (hit, t, p, n, margin) in object space; eps is 5e-4 t."""
    n_rays = o.shape[0]
    k = s[0]
    hit = np.zeros(n_rays, bool)
    t = np.full(n_rays, np.nan)
    nrm = np.zeros((n_rays, 3))
    with np.errstate(all="ignore"):
        if k == "box":                                                            # :86-111
            pmin, pmax = s[1], s[2]
            near, far = np.full(n_rays, -INF), np.full(n_rays, INF)
            axis = np.zeros(n_rays, int)
            alive = np.ones(n_rays, bool)
            marg = np.full(n_rays, INF)
            for dim in range(3):                                                  # testSlabs :104-111
                alive &= ~(near > far)
                dinv = 1 / d[:, dim]
                a1, a2 = (pmax[dim] - o[:, dim]) * dinv, (pmin[dim] - o[:, dim]) * dinv
                sw = a1 > a2
                t1, t2 = np.where(sw, a2, a1), np.where(sw, a1, a2)
                marg = np.minimum(marg, np.minimum(rel(near, t1), rel(far, t2)))
                axis = np.where(near < t1, dim, axis)
                near, far = hmax(near, t1), hmin(far, t2)
            alive &= ~(near > far)                                                # :101-103
            marg = np.minimum(marg, rel(near, far))
            t0, t1 = hmin(near, far), hmax(near, far)
            g = _Guards(n_rays)
            g.take(~alive)
            if mutation == "box_inside_closest":
                g.take(t0 > tmax)
                tt = np.where(t0 < tmin, t1, t0)
            else:
                g.take((t0 > tmax) | (t0 < tmin))                                 # :90
                tt = np.where(t0 < tmin, t1, t0)                                  # :93
            g.take(tt > tmax)                                                     # :91
            hit = g.rest()
            marg = np.minimum(marg, np.minimum(np.minimum(rel(t0, tmax), rel(t0, tmin)), rel(tt, tmax)))
            t = tt
            p = _ray_at(o, d, t)
            pa = np.take_along_axis(p, axis[:, None], 1)[:, 0]
            half = ((pmin + pmax) / 2)[axis]
            marg = np.minimum(marg, np.where(hit, rel(pa, half), INF))
            nrm[np.arange(n_rays), axis] = np.where(pa > half, 1.0, -1.0)          # :96-98
            return hit, t, p, nrm, marg
        if k == "cylinder":                                                       # :113-140
            r, zmin, zmax, phimax = s[1:]
            a = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
            b = 2 * (d[:, 0] * o[:, 0] + d[:, 1] * o[:, 1])
            c = o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1] - r * r
            ok, t0, t1, marg = solve_quadric(a, b, c)
            p0, p1 = _ray_at(o, d, t0), _ray_at(o, d, t1)
            ph0, ph1 = atan2p(p0[:, 1], p0[:, 0]), atan2p(p1[:, 1], p1[:, 0])
            g = _Guards(n_rays)
            g.take(~ok)
            g.take(t0 > tmax)
            g.take(t1 < tmin)
            first = g.take((t0 > tmin) & (p0[:, 2] > zmin) & (p0[:, 2] < zmax) & (ph0 <= phimax))
            second = g.take((t1 <= tmax) & (p1[:, 2] > zmin) & (p1[:, 2] < zmax) & (ph1 <= phimax))
            hit = first | second
            t = np.where(first, t0, t1)
            p = np.where(first[:, None], p0, p1)
            for tk, pk, phk in ((t0, p0, ph0), (t1, p1, ph1)):
                marg = np.minimum(marg, np.minimum(rel(tk, tmin), rel(tk, tmax)))
                inb = np.isfinite(tk)
                marg = np.minimum(marg, np.where(inb, np.minimum(rel(pk[:, 2], zmin), rel(pk[:, 2], zmax)), INF))
                marg = np.minimum(marg, np.where(inb, _phi_margin(phk, phimax), INF))
            dpdu = np.stack([-phimax * p[:, 1], phimax * p[:, 0], np.zeros(n_rays)], -1)      # :138-140
            dpdv = np.zeros((n_rays, 3))
            dpdv[:, 2] = zmax - zmin
            return hit, t, p, normalize(cross(dpdu, dpdv)), marg
        if k in ("disk", "quad"):                                                 # :142-171
            h = s[1] if k == "disk" else 0.0
            t = (h - o[:, 2]) / d[:, 2] if k == "disk" else -(o[:, 2]) / d[:, 2]
            p = _ray_at(o, d, t)
            marg = np.minimum(rel(np.abs(d[:, 2]), 1e-7), np.minimum(rel(t, tmin), rel(t, tmax)))
            g = _Guards(n_rays)
            par = g.take(np.abs(d[:, 2]) < 1e-7)
            g.take((t < tmin) | (t > tmax))
            if k == "disk":
                rad, irad, phimax = s[2:]
                d2 = p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]
                phi = atan2p(p[:, 1], p[:, 0])
                g.take((d2 > rad * rad) | (d2 < irad * irad))
                g.take(phi > phimax)
                m2 = np.minimum(np.minimum(rel(d2, rad * rad), rel(d2, irad * irad) if irad > 0 else INF), _phi_margin(phi, phimax))
                nrm[:, 2] = -1.0                                                  # :155
            else:
                sx, sy = s[1:]
                g.take((np.abs(p[:, 0]) > sx) | (np.abs(p[:, 1]) > sy))
                m2 = np.minimum(rel(np.abs(p[:, 0]), sx), rel(np.abs(p[:, 1]), sy))
                dpdu, dpdv = np.array([sx, 0.0, 0.0]), np.array([0.0, sy, 0.0])   # :168-171, mkDg :50-51
                nrm[:] = normalize(cross(dpdu, dpdv))
            hit = g.rest()
            return hit, t, p, nrm, np.where(par, rel(np.abs(d[:, 2]), 1e-7), np.minimum(marg, m2))
        assert k == "sphere"                                                      # :173-229
        r = s[1]
        a, b, c = sq_len(d), 2 * dot(o, d), sq_len(o) - r * r
        ok, t1, t2, marg = solve_quadric(a, b, c)
        tt = np.where(t1 < tmin, t2, t1)
        g = _Guards(n_rays)
        g.take(~ok)
        g.take(t1 > tmax)
        g.take(t2 < tmin)
        g.take(tt > tmax)
        hit = g.rest()
        marg = np.minimum(marg, np.minimum(np.minimum(rel(t1, tmax), rel(t1, tmin)), np.minimum(rel(t2, tmin), rel(tt, tmax))))
        p = _ray_at(o, d, tt)
        px, py, pz = p[:, 0], p[:, 1], p[:, 2]
        theta = np.arccos(np.clip(pz / r, -1, 1))
        inv = 1 / np.sqrt(px * px + py * py)
        dth = 0.0 - math.pi                                                       # thetaMax - thetaMin :190-191
        dpdu = np.stack([-TWO_PI * py, TWO_PI * px, np.zeros(n_rays)], -1)
        dpdv = np.stack([pz * px * inv, pz * py * inv, -r * np.sin(theta)], -1) * dth
        return hit, tt, p, normalize(cross(dpdu, dpdv)), marg


def intersects(s, o, d, tmin, tmax):
    """Shape.intersects (Shape.hs:231-284): (occluded, margin)."""
    n_rays = o.shape[0]
    k = s[0]
    with np.errstate(all="ignore"):
        if k == "box":                                                            # :233, AABB.hs:81-94
            near, far = np.broadcast_to(tmin, (n_rays,)).astype(float), np.broadcast_to(tmax, (n_rays,)).astype(float)
            alive = np.ones(n_rays, bool)
            marg = np.full(n_rays, INF)
            for dim in range(3):
                alive &= ~(near > far)
                dinv = 1 / d[:, dim]
                tf, tn = (s[2][dim] - o[:, dim]) * dinv, (s[1][dim] - o[:, dim]) * dinv
                sw = tn > tf
                n1, f1 = np.where(sw, tf, tn), np.where(sw, tn, tf)
                near, far = hmax(near, n1), hmin(far, f1)
                marg = np.minimum(marg, rel(near, far))
            return alive & ~(near > far), marg
        if k == "cylinder":                                                       # :235-251
            r, zmin, zmax, phimax = s[1:]
            a = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
            b = 2 * (d[:, 0] * o[:, 0] + d[:, 1] * o[:, 1])
            c = o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1] - r * r
            ok, t0, t1, marg = solve_quadric(a, b, c)
            p0, p1 = _ray_at(o, d, t0), _ray_at(o, d, t1)
            ph0, ph1 = atan2p(p0[:, 1], p0[:, 0]), atan2p(p1[:, 1], p1[:, 0])
            g = _Guards(n_rays)
            g.take(~ok)
            g.take(t0 > tmax)
            g.take(t1 < tmin)
            first = g.take((t0 > tmin) & (p0[:, 2] > zmin) & (p0[:, 2] < zmax) & (ph0 <= phimax))
            second = g.take((t1 < tmax) & (p1[:, 2] > zmin) & (p1[:, 2] < zmax) & (ph1 <= phimax) & (t1 <= tmax))
            for tk, pk, phk in ((t0, p0, ph0), (t1, p1, ph1)):
                marg = np.minimum(marg, np.minimum(rel(tk, tmin), rel(tk, tmax)))
                inb = np.isfinite(tk)
                marg = np.minimum(marg, np.where(inb, np.minimum(rel(pk[:, 2], zmin), rel(pk[:, 2], zmax)), INF))
                marg = np.minimum(marg, np.where(inb, _phi_margin(phk, phimax), INF))
            return first | second, marg
        if k in ("disk", "quad"):                                                 # :253-273
            hit, _, _, _, marg = intersect(s, o, d, tmin, tmax)
            return hit, marg
        r = s[1]                                                                  # :275-284
        ok, t0, t1, marg = solve_quadric(sq_len(d), 2 * dot(o, d), sq_len(o) - r * r)
        g = _Guards(n_rays)
        g.take(~ok)
        g.take((t0 > tmax) | (t1 < tmin))
        second = g.take(t0 < tmin)
        res = np.where(second, t1 < tmax, g.rest())
        marg = np.minimum(marg, np.minimum(np.minimum(rel(t0, tmax), rel(t0, tmin)), np.minimum(rel(t1, tmin), rel(t1, tmax))))
        return res, marg


def inside_sphere(r, p):                                                          # Shape.hs:330-331
    return sq_len(p) - r * r < 1e-4


def general_pdf(s, p, wi, mutation=None, area_scale=1.0):
    """generalPdf (Shape.hs:346-350): (pdf, hit, margin)."""
    n = p.shape[0]
    hit, t, ph, nrm, marg = intersect(s, p, wi, np.full(n, 1e-3), np.full(n, INF))
    with np.errstate(all="ignore"):
        pd = sq_len(p - ph) / (np.abs(dot(nrm, -wi)) * (area(s) * area_scale))
    pd = np.where(np.isinf(pd), 0.0, pd)
    return np.where(hit, pd, 0.0), hit, marg


def shape_pdf(s, p, wi, mutation=None, area_scale=1.0):
    """shapePdf (Shape.hs:333-344): (pdf, took generalPdf, generalPdf hit, margin)."""
    pd, hit, marg = general_pdf(s, p, wi, mutation, area_scale)
    if s[0] != "sphere":
        return pd, np.ones(len(pd), bool), hit, marg
    r = s[1]
    ins = inside_sphere(r, p)
    with np.errstate(all="ignore"):
        cone = uniform_cone_pdf(np.sqrt(np.maximum(0, 1 - r * r / sq_len(p))))
    m_in = rel(sq_len(p), r * r + 1e-4)
    return np.where(ins, pd, cone), ins, hit, np.where(ins, np.minimum(marg, m_in), m_in)


def sample_shape_any(s, u1, u2, mutation=None):
    """sampleShape' (Shape.hs:379-409): (point, normal)."""
    k = s[0]
    n = len(u1)
    if k == "box":                                                                # :384-392
        pmin, pmax = s[1], s[2]
        axis, u1p = remap_rand(3, u1)
        nf, u2p = remap_rand(2, u2)
        oa0, oa1 = (axis + 1) % 3, (axis + 2) % 3
        p = np.where((nf == 0)[:, None], pmin[None], pmax[None]).astype(float)
        idx = np.arange(n)
        p[idx, oa1] = lerp(u2p, pmin[oa1], pmax[oa1])
        p[idx, oa0] = lerp(u1p, pmin[oa0], pmax[oa0])
        nrm = np.zeros((n, 3))
        nrm[idx, axis] = nf * 2 - 1
        return p, nrm
    if k == "cylinder":                                                           # :394-398
        r, z0, z1, phimax = s[1:]
        phi = lerp(u2, 0, phimax if mutation == "cyl_sample_phimax" else TWO_PI)
        p = np.stack([r * np.cos(phi), r * np.sin(phi), lerp(u1, z0, z1)], -1)
        return p, normalize(np.stack([p[:, 0], p[:, 1], np.zeros(n)], -1))
    if k == "disk":                                                               # :400-403
        h, rmax, rmin, phimax = s[1:]
        r, phi = lerp(u1, rmin, rmax), lerp(u2, 0, phimax)
        return np.stack([r * np.cos(phi), r * np.sin(phi), np.full(n, h)], -1), np.tile([0.0, 0.0, -1.0], (n, 1))
    if k == "quad":                                                               # :405-406
        return (np.stack([lerp(u1, -s[1], s[1]), lerp(u2, -s[2], s[2]), np.zeros(n)], -1),
                np.tile([0.0, 0.0, -1.0], (n, 1)))
    q = uniform_sample_sphere(u1, u2)                                             # :408-409
    return q * s[1], q


def sample_shape(s, p, u1, u2, mutation=None):
    """sampleShape (Shape.hs:362-376): (point, normal, margin)."""
    ps, ns = sample_shape_any(s, u1, u2, mutation)
    n = len(u1)
    if s[0] != "sphere":
        return ps, ns, np.full(n, INF)
    r = s[1]
    ins = inside_sphere(r, p)
    with np.errstate(all="ignore"):
        dn = normalize(-p)
        cos_max = np.sqrt(np.maximum(0, 1 - (r * r) / sq_len(p)))
        dd = uniform_sample_cone(coordinate_system(dn), cos_max, u1, u2)
        hit, t, ph, _, marg = intersect(s, p, dd, np.zeros(n), np.full(n, INF))
        pc = np.where(hit[:, None], ph, dn * r)
    marg = np.minimum(marg, rel(sq_len(p), r * r + 1e-4))
    return np.where(ins[:, None], ps, pc), np.where(ins[:, None], ns, normalize(pc)), marg


# ------------------------------------------------------------------ Primitive/Geometry.hs, DifferentialGeometry.hs, Light.hs
class Prim:
    """mkGeom (Primitive/Geometry.hs:22-36): a shape under o2w, and the area light it may carry."""

    def __init__(self, shape, o2w, emissive=False):
        self.shape, self.o2w, self.w2o, self.emissive = shape, o2w, inverse(o2w), emissive

    def world_bounds(self):                                                       # Shape.hs:292
        return trans_box(self.o2w, *object_bounds(self.shape))


class Ref:
    """The scene's primitives, traced one after the other (what the kd-tree computes, ties aside)."""

    def __init__(self, prims, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.prims, self.mutation = prims, mutation

    def _obj_ray(self, pr, o, d):                                                 # transRay, Transform.hs:275-278
        oo, od = trans_point(pr.w2o, o), trans_vector(pr.w2o, d)
        if self.mutation == "normalized_dir":                                      # the transform's stretch taken out
            with np.errstate(all="ignore"):
                od = od * (np.sqrt(sq_len(d)) / np.sqrt(sq_len(od)))[..., None]
        return oo, od

    def closest(self, o, d, tmin, tmax):
        """Primitive.intersect over all primitives: (prim or -1, t, world p, world n, margin)."""
        n = o.shape[0]
        best_t, best = np.full(n, INF), np.full(n, -1)
        bp, bn = np.zeros((n, 3)), np.zeros((n, 3))
        marg = np.full(n, INF)
        ts = []
        for k, pr in enumerate(self.prims):
            oo, od = self._obj_ray(pr, o, d)
            hit, t, p, nrm, m = intersect(pr.shape, oo, od, tmin, tmax, self.mutation)
            marg = np.minimum(marg, m)
            ts.append(np.where(hit, t, INF))
            better = hit & (t < best_t)
            pw = trans_point(pr.o2w, p)                                           # transDg, DifferentialGeometry.hs:74-81
            nw = normalize(trans_normal(pr.o2w, nrm, self.mutation))
            best_t, best = np.where(better, t, best_t), np.where(better, k, best)
            bp, bn = np.where(better[:, None], pw, bp), np.where(better[:, None], nw, bn)
        ts = np.sort(np.stack(ts, 0), 0)
        if len(self.prims) > 1:
            marg = np.minimum(marg, rel(ts[0], ts[1]))                            # which primitive is nearest
        return best, best_t, bp, bn, marg

    def occluded(self, o, d, tmin, tmax):
        n = o.shape[0]
        occ, marg = np.zeros(n, bool), np.full(n, INF)
        for pr in self.prims:
            oo, od = self._obj_ray(pr, o, d)
            h, m = intersects(pr.shape, oo, od, tmin, tmax)
            occ |= h
            marg = np.minimum(marg, m)
        return occ, marg

    def _area_scale(self, pr):
        # the mutation: the lamp's world-space area (exact for the uniform scales it is used on)
        if self.mutation != "world_area":
            return 1.0
        return abs(np.linalg.det(pr.o2w.m[:3, :3])) ** (2.0 / 3.0)

    def light_sample(self, k, pw, eps, u1, u2):
        """Light.sample of primitive k's area light (Light.hs:152-160): a dict of wi (world), pdf, the
        shadow ray (o, d, tmin, tmax), lit (li is not black) and margin."""
        pr = self.prims[k]
        p = trans_point(pr.w2o, pw)
        ps, ns, marg = sample_shape(pr.shape, p, u1, u2, self.mutation)
        wi = normalize(ps - p)
        pd, gen, ghit, m2 = shape_pdf(pr.shape, p, wi, self.mutation, self._area_scale(pr))
        nd = dot(ns, wi)
        return {"wi": trans_vector(pr.o2w, wi), "pdf": pd, "o": trans_point(pr.o2w, p), "tmin": np.full(len(u1), eps),
                "tmax": np.sqrt(sq_len(ps - p)) - eps, "lit": nd < 0, "general": gen, "general_hit": ghit,
                "margin": np.minimum(np.minimum(marg, m2), np.abs(nd))}

    def light_pdf(self, k, pw, wiw):
        """Light.pdf (Light.hs:228): (pdf, took generalPdf, its ray hit, margin)."""
        pr = self.prims[k]
        return shape_pdf(pr.shape, trans_point(pr.w2o, pw), trans_vector(pr.w2o, wiw), self.mutation, self._area_scale(pr))

    def light_emit(self, k, uo1, uo2, ud1, ud2):
        """Light.sample' of primitive k's area light (Light.hs:174-179): ray origin, direction, the
        normal at the light (world space) and the pdf invPi * shapePdf' * |ns . wi| with shapePdf' =
        1 / area (Shape.hs:358); the ray's tmin is 1e-3."""
        pr = self.prims[k]
        org, ns = sample_shape_any(pr.shape, uo1, uo2, self.mutation)
        org, ns = trans_point(pr.o2w, org), normalize(trans_normal(pr.o2w, ns, self.mutation))
        wi = cosine_sample_hemisphere(ns, ud1, ud2)
        pd = (1 / math.pi) * (1.0 / (area(pr.shape) * self._area_scale(pr))) * np.abs(dot(ns, wi))
        return org, wi, ns, pd
