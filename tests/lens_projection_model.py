"""The lens correction of a lens with a projection of its own (include/r2f.h, r2f_lens_correct_projected) restated in NumPy, on top
of tests/lens_model.py and tests/lens_tca_model.py: what the tests compare the device kernels and the CPU program of
tests/lens_projection_check.cpp with, bit for bit.

The definition.  Everything of lens_model's up to r2 = u*u + v*v is unchanged.  Then:
  - r = sqrt(r2), t = r*inv_focal (inv_focal: the float rounded from 1/focal).
  - The projection factor P(t), with tt = t*t, s = sqrt(1 + tt):
      orthographic:  P = 1/s.
      stereographic: P = 2/(1 + s).
      equisolid:     P = 1/(s*sqrt((s + 1)/(2*s))).
      fisheye:       t <= 1: P = p(tt);  t > 1: w = 1/t, P = (pi_2 - w*p(w*w))*w.
                     p(x) = c0 + x*(c1 + ... + x*c9) by Horner from c9 down; the coefficients are ATAN_COEF (include/r2f.h's).
  - u' = u*P, v' = v*P, r2' = u'*u' + v'*v'; the model factor f of r2' as lens_model's of r2.
  - g0 = f*P, g = g0*inv_scale, ox = dx*g, oy = dy*g.
  - From there lens_model's sampling at (cx + ox, cy + oy), or lens_tca_model's per channel with a TCA record.
Every operation is one operation of type T.  With T = float64 (`evaluate`), P is the exact function (np.arctan and the algebraic forms
in double) and the constants are unrounded.  UNPINNED against lensfun, like lens_model.

A projection record here is (type, inv_focal) with type one of TYPES: `record(profile)` makes it from a LensProfile's `projection`.
"""

from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

import lens_model as lm
import lens_tca_model as tm

F = lm.F
TYPES = {"fisheye": 1, "stereographic": 2, "equisolid": 3, "orthographic": 4}
ATAN_COEF = tuple(F(float.fromhex(h)) for h in (
    "0x1p+0", "-0x1.55554p-2", "0x1.999278p-3", "-0x1.242702p-3", "0x1.c0d2e2p-4", "-0x1.58dd68p-4", "0x1.dd11b4p-5", "-0x1.01b21p-5",
    "0x1.6a946ap-7", "-0x1.df068p-10"))
PI_2 = F(float.fromhex("0x1.921fb6p+0"))

# the records of the tests: name -> (type, focal)
PROJECTIONS = {
    "fisheye": ("fisheye", 2.0 / math.pi),  # at scale 1, t runs from 0 to pi/2 on every shape
    "stereographic": ("stereographic", 0.5),
    "equisolid": ("equisolid", 0.55),
    "orthographic": ("orthographic", 1.2),
}
IDENTITY_FOCAL = 2.0 ** 20


def profile(name, projection, tca=None, **changes):
    """lens_model's distortion spec `name` with the projection `projection` (a name of PROJECTIONS or a (type, focal) pair) and the
    TCA spec `tca` (None, a name of lens_tca_model.TCA_SPECS, or a pair)."""
    from raw2film_amd.lens import LensProfile

    spec = dict(lm.PROFILE_SPECS[name], **changes)
    return LensProfile(**spec, projection=PROJECTIONS[projection] if isinstance(projection, str) else projection,
                       tca=tm.TCA_SPECS[tca] if isinstance(tca, str) else tca)


def record(prof, T=F):
    """(type, inv_focal) of a LensProfile's `projection`: inv_focal rounded to float for T = float32, 1/focal in double otherwise."""
    kind, focal = prof.projection
    return kind, F(1.0 / focal) if T is F else 1.0 / focal


def from_params(pp):
    """A raw2film_amd._lib.LensProjectionParams (the planner's result) as a record."""
    return {v: k for k, v in TYPES.items()}[int(pp.type)], F(pp.inv_focal)


def atan_poly(x):
    """p(x) in float32: Horner from c9 down, each product and each sum rounded on its own."""
    acc = np.full_like(x, ATAN_COEF[9])
    for k in range(8, -1, -1):
        acc = acc * x
        acc = ATAN_COEF[k] + acc
    return acc


def factor(kind, t, T=F):
    """P(t): the definition's operations for T = float32, the exact function in double otherwise."""
    one, two = T(1), T(2)
    tt = t * t
    if kind == "fisheye":
        if T is not F:
            with np.errstate(invalid="ignore", divide="ignore"):
                return np.where(t > 0, np.arctan(t) / np.where(t > 0, t, 1.0), 1.0)
        low = atan_poly(tt)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            w = one / t
            ww = w * w
            a = w * atan_poly(ww)
            b = PI_2 - a
            high = b * w
        return np.where(t <= one, low, high)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = np.sqrt(one + tt)
        if kind == "orthographic":
            return one / s
        if kind == "stereographic":
            return two / (one + s)
        if kind == "equisolid":
            n, m = s + one, two * s
            return one / (s * np.sqrt(n / m))
    raise ValueError(kind)


def offsets(c, rec, X, Y, T=F, want_factor=False):
    """(ox, oy, dx, dy) of output pixels X, Y through the projection step; with want_factor also (P, t)."""
    kind, inv_focal = rec
    one = T(1)
    dx, dy = X.astype(T) - T(c.cx), Y.astype(T) - T(c.cy)
    u, v = dx * T(c.q), dy * T(c.q)
    r2 = u * u + v * v
    t = np.sqrt(r2) * T(inv_focal)
    P = factor(kind, t, T)
    up, vp = u * P, v * P
    r2p = up * up + vp * vp
    k = [T(x) for x in c.k]
    if c.model == 1:
        f = T(c.c0) + k[0] * r2p
    elif c.model == 2:
        f = one + r2p * (k[0] + k[1] * r2p)
    elif c.model == 3:
        r = np.sqrt(r2p)
        f = T(c.c0) + r * (k[2] + r * (k[1] + r * k[0]))
    else:
        f = np.ones_like(r2p)
    g = (f * P) * T(c.inv_scale)
    if want_factor:
        return dx * g, dy * g, dx, dy, P, t
    return dx * g, dy * g, dx, dy


def _sample(image, c, coords, dx, dy, T, window_shape, want_bound):
    """lens_tca_model.correct_tca's per-channel sampling at coords[ch] = (sx, sy): the clamp and the gain of (dx, dy) included."""
    H, W = image.shape[:2]
    pad = np.zeros((H + 16, W + 16, 3), dtype=T)
    pad[8:8 + H, 8:8 + W] = image
    tab = lm.phase_table().astype(T)
    den = None
    if c.vignetting:
        a, b = dx * T(c.qv), dy * T(c.qv)
        rv2 = a * a + b * b
        v = [T(x) for x in c.v]
        den = T(1) + rv2 * (v[0] + rv2 * (v[1] + rv2 * v[2]))
    out = np.zeros(window_shape + (3,), dtype=T)
    details = []
    for ch in range(3):
        sx, sy = coords[ch]
        in_x, ix, fx = lm.split_phase(sx, W, T)
        in_y, iy, fy = lm.split_phase(sy, H, T)
        inside = in_x & in_y
        ix, iy, fx, fy = (np.where(inside, a, 0) for a in (ix, iy, fx, fy))
        acc = bound = None
        for k in range(8):
            h = hb = None
            for j in range(8):
                prod = (tab[fy, k] * tab[fx, j]) * pad[iy + 5 + k, ix + 5 + j, ch]
                h = prod if j == 0 else h + prod
                if want_bound:
                    hb = np.abs(prod.astype(np.float64)) if j == 0 else hb + np.abs(prod.astype(np.float64))
            acc = h if k == 0 else acc + h
            if want_bound:
                bound = hb if k == 0 else bound + hb
        o = np.where(acc < 0, T(0), acc)
        if den is not None:
            with np.errstate(invalid="ignore", divide="ignore"):
                o = o / den
        out[..., ch] = np.where(inside, o, T(0))
        details.append(SimpleNamespace(sum_abs=bound, fx=fx, fy=fy, ix=ix, iy=iy, inside=inside, den=den, sx=sx, sy=sy))
    return out, details


def correct(image, c, rec, tca=None, window=None, T=F, want_bound=False):
    """The projected correction of `image` (H, W, 3 | 4) over the window -- default: the whole frame -- as (rows, cols, 3) of type
    T.  c: lens_model's constants (rounded() for float32); rec: the projection record; tca: None or lens_tca_model's record.  Per
    channel the weights, products and sum order are lens_model.correct's (the three channels share them without a TCA record), so
    with P == 1 the result is lens_model.correct's / lens_tca_model.correct_tca's bit for bit.  want_bound: also the per-channel
    details (sum_abs, phases, inside, den, sx, sy)."""
    image = np.asarray(image)[..., :3].astype(T)
    H, W = image.shape[:2]
    r0, c0, nr, nc = (0, 0, H, W) if window is None else window
    Y, X = np.meshgrid(np.arange(r0, r0 + nr), np.arange(c0, c0 + nc), indexing="ij")
    with np.errstate(invalid="ignore", over="ignore"):
        ox, oy, dx, dy = offsets(c, rec, X, Y, T)
        if tca is None:
            green = (T(c.cx) + ox, T(c.cy) + oy)
            coords = [green, green, green]
        else:
            coords = [tm.channel_coords(c, tca, ch, ox, oy, T) for ch in range(3)]
    out, details = _sample(image, c, coords, dx, dy, T, (nr, nc), want_bound)
    return (out, details) if want_bound else out


def coords_plain(c, X, Y, T=F):
    """(sx, sy) of the unprojected map (lens_model.source_coords), for the tests that ask how far the projection moves a coordinate."""
    sx, sy, _, _ = lm.source_coords(c, X, Y, T)
    return sx, sy


def probes_reach(prof, H, W, scale):
    """The planner's eight probes through the projected map in double at `scale` -- P in double, rounded to float as the planner
    rounds it -- with the TCA factor on top when the profile has a record: the largest distance any channel's source coordinate lies
    outside [0, W - 1] x [0, H - 1] (<= 0: all land inside)."""
    c = lm.constants(prof, H, W, scale)
    kind, focal = prof.projection
    channels = [(1.0, 0.0, 0.0)]
    model = None
    if prof.tca is not None:
        model, red, blue = tm.record(prof)
        channels += [red, blue]
    xs, ys = [0.0, (W - 1) / 2.0, float(W - 1)], [0.0, (H - 1) / 2.0, float(H - 1)]
    worst = -math.inf
    for j, y in enumerate(ys):
        for i, x in enumerate(xs):
            if i == 1 and j == 1:
                continue
            dx, dy = x - c.cx, y - c.cy
            u, v = dx * c.q, dy * c.q
            t = math.sqrt(u * u + v * v) / focal
            P = float(F(float(factor(kind, np.float64(t), np.float64))))
            u, v = u * P, v * P
            r2 = u * u + v * v
            if c.model == 1:
                f = c.c0 + c.k[0] * r2
            elif c.model == 2:
                f = 1.0 + r2 * (c.k[0] + c.k[1] * r2)
            elif c.model == 3:
                r = math.sqrt(r2)
                f = c.c0 + r * (c.k[2] + r * (c.k[1] + r * c.k[0]))
            else:
                f = 1.0
            g = f * P * c.inv_scale
            ox, oy = dx * g, dy * g
            ru = math.hypot(ox * c.qv, oy * c.qv)
            for k in channels:
                tf = k[0] + ru * (k[1] + ru * k[2]) if model == "poly3" else k[0]
                sx, sy = c.cx + ox * tf, c.cy + oy * tf
                worst = max(worst, -sx, sx - (W - 1), -sy, sy - (H - 1))
    return worst


# ---- the kernel's staging rule, restated for the host: which route each 64 x 16 tile of a window takes
BOX_TEXELS = 3072
ROUTES = ("whole", "halves", "gather")


def tile_routes(c, rec, tca, H, W, window=None):
    """Per tile of the window (default: the whole frame) the route of r2f_lens.hip's projected kernel: "whole" (the union of the
    two halves' tap extents fits BOX_TEXELS), else per half "halves" (its own box fits) or "gather" (it does not); -> a list of
    (tile row, tile column, routes of its passes).  Extents are over the inside pixels of all sampled channels."""
    r0, c0, nr, nc = (0, 0, H, W) if window is None else window
    out = []
    for ty in range(0, nr, 16):
        for tx in range(0, nc, 64):
            ext = []
            for half in range(2):
                rows = min(8, nr - ty - 8 * half)
                if rows <= 0:
                    ext.append(None)
                    continue
                Y, X = np.meshgrid(np.arange(r0 + ty + 8 * half, r0 + ty + 8 * half + rows), np.arange(c0 + tx, c0 + min(tx + 64, nc)),
                                   indexing="ij")
                with np.errstate(invalid="ignore", over="ignore"):
                    ox, oy, _, _ = offsets(c, rec, X, Y)
                    coords = [(F(c.cx) + ox, F(c.cy) + oy)] if tca is None else [tm.channel_coords(c, tca, ch, ox, oy) for ch in range(3)]
                e = None
                for sx, sy in coords:
                    in_x, ix, _ = lm.split_phase(sx, W)
                    in_y, iy, _ = lm.split_phase(sy, H)
                    inside = in_x & in_y
                    if inside.any():
                        cur = (ix[inside].min(), ix[inside].max(), iy[inside].min(), iy[inside].max())
                        e = cur if e is None else (min(e[0], cur[0]), max(e[1], cur[1]), min(e[2], cur[2]), max(e[3], cur[3]))
                ext.append(e)
            have = [e for e in ext if e is not None]
            if not have:
                out.append((ty // 16, tx // 64, ("whole",)))
                continue
            un = (min(e[0] for e in have), max(e[1] for e in have), min(e[2] for e in have), max(e[3] for e in have))
            if (un[1] - un[0] + 8) * (un[3] - un[2] + 8) <= BOX_TEXELS:
                out.append((ty // 16, tx // 64, ("whole",)))
            else:
                out.append((ty // 16, tx // 64, tuple(
                    "halves" if e is None or (e[1] - e[0] + 8) * (e[3] - e[2] + 8) <= BOX_TEXELS else "gather" for e in ext)))
    return out


# ---- the cases the host and the GPU tests share
def cases(shape):
    """(distortion spec, projection, TCA spec or None, changes) rendered on `shape`: every projection without and with a TCA record;
    the fisheye at scale 0.25 (t up to 6.3; the gather route on 150 x 210); the fisheye and the equisolid record at their auto
    scales (0.71: every tile whole; 0.52: the two-halves route in the middle of 150 x 210) -- not on a one-pixel-wide frame, where
    the planner finds no fitting scale."""
    out = []
    for projection in PROJECTIONS:
        out += [("ptlens", projection, None, {}), ("vignetting", projection, "poly3", {})]
    out += [("none", "fisheye", None, dict(scale=0.25)), ("none", "fisheye", "linear", dict(scale=0.25))]
    if min(shape) > 1:
        out += [("none", "fisheye", None, dict(scale="auto")), ("none", "fisheye", "poly3", dict(scale="auto")),
                ("none", "equisolid", None, dict(scale="auto")), ("off-centre", "equisolid", "edge", dict(scale="auto"))]
    return out


_MODEL = {}


def model(name, projection, tca, shape, window=None, **changes):
    """correct() of lens_model.frame(*shape) for the case, computed once and shared (callers do not write to it).  With
    scale="auto" among the changes the scale is the planner's."""
    key = (name, projection, tca, shape, window, tuple(sorted(changes.items())))
    if key not in _MODEL:
        prof = profile(name, projection, tca, **changes)
        scale = prof.plan_projected(*shape)[0].scale if prof.scale == "auto" else None
        _MODEL[key] = correct(lm.frame(*shape), lm.rounded(lm.constants(prof, *shape, scale)), record(prof),
                              None if tca is None else tm.record(prof, F), window)
        _MODEL[key].setflags(write=False)
    return _MODEL[key]
