"""The lens correction with transverse chromatic aberration (include/r2f.h, r2f_lens_correct_tca) restated in NumPy, on top of
tests/lens_model.py: what the tests compare the device kernel and the CPU program of tests/lens_tca_check.cpp with, bit for bit.

The definition.  Everything of lens_model's up to g = f*inv_scale is unchanged.  Then:
  - ox = dx*g, oy = dy*g.
  - Green: sx = cx + ox, sy = cy + oy (lens_model's values).
  - Red and blue each have constants (v, c, b) and a factor t:
      linear: t = v.
      poly3:  a = ox*qv, e = oy*qv, r2 = a*a + e*e, r = sqrt(r2); t = v + r*(c + r*b), each operation rounded on its own.
    sx_c = cx + ox*t, sy_c = cy + oy*t.
  - Each channel has its own phase split, inside / outside decision and 64-tap sum over its own plane; the clamp and the vignetting
    gain of the output pixel's (dx, dy) follow, the same for all three.  A channel that is outside yields 0 alone.
Every operation is one operation of type T.  UNPINNED against lensfun, like lens_model.

A TCA record here is (model, red, blue) with red, blue = (v, c, b): `record(profile)` makes it from a LensProfile's `tca`.
"""

from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

import lens_model as lm

F = lm.F
TCA_SPECS = {
    "linear": ("linear", (1.03, 0.97)),
    "poly3": ("poly3", (1.002, 0.998, 0.01, -0.008, -0.02, 0.015)),
    "edge": ("linear", (1.06, 0.94)),
    "identity": ("linear", (1.0, 1.0)),
}
CHANNELS = ("red", "green", "blue")


def profile(name, tca):
    """lens_model's distortion spec `name` with the TCA spec `tca` (a name of TCA_SPECS, or a (model, numbers) pair)."""
    from raw2film_amd.lens import LensProfile

    return LensProfile(**lm.PROFILE_SPECS[name], tca=TCA_SPECS[tca] if isinstance(tca, str) else tca)


def record(prof, T=np.float64):
    """(model, red, blue) of a LensProfile's `tca`, red / blue = (v, c, b) in type T (float32: what the planner hands the kernel)."""
    model, values = prof.tca
    n = len(values) // 2
    red, blue = values[0::2] + (0.0,) * (3 - n), values[1::2] + (0.0,) * (3 - n)
    return model, tuple(T(x) for x in red), tuple(T(x) for x in blue)


def from_params(t):
    """A raw2film_amd._lib.LensTcaParams (the planner's result) as a record."""
    return {1: "linear", 2: "poly3"}[int(t.model)], tuple(F(x) for x in t.red), tuple(F(x) for x in t.blue)


def offsets(c, X, Y, T=F):
    """(ox, oy, dx, dy) of output pixels X, Y: lens_model.source_coords up to the point at which the channels part."""
    one = T(1)
    dx, dy = X.astype(T) - T(c.cx), Y.astype(T) - T(c.cy)
    u, v = dx * T(c.q), dy * T(c.q)
    r2 = u * u + v * v
    k = [T(x) for x in c.k]
    if c.model == 1:
        f = T(c.c0) + k[0] * r2
    elif c.model == 2:
        f = one + r2 * (k[0] + k[1] * r2)
    elif c.model == 3:
        r = np.sqrt(r2)
        f = T(c.c0) + r * (k[2] + r * (k[1] + r * k[0]))
    else:
        f = np.ones_like(r2)
    g = f * T(c.inv_scale)
    return dx * g, dy * g, dx, dy


def channel_coords(c, rec, ch, ox, oy, T=F):
    """(sx, sy) at which channel ch (0 red, 1 green, 2 blue) samples."""
    if ch != 1:
        model, red, blue = rec
        v, cc, b = (T(x) for x in (red if ch == 0 else blue))
        if model == "poly3":
            a, e = ox * T(c.qv), oy * T(c.qv)
            r = np.sqrt(a * a + e * e)
            t = v + r * (cc + r * b)
        else:
            t = v
        ox, oy = ox * t, oy * t
    return T(c.cx) + ox, T(c.cy) + oy


def correct_tca(image, c, rec, window=None, T=F, want_bound=False):
    """lens_model.correct with the TCA record `rec`: (rows, cols, 3) of type T; with want_bound also a list of three details
    (sum_abs, fx, fy, ix, iy, inside, den), one per channel, each as lens_model.correct's."""
    image = np.asarray(image)[..., :3].astype(T)
    H, W = image.shape[:2]
    r0, c0, nr, nc = (0, 0, H, W) if window is None else window
    Y, X = np.meshgrid(np.arange(r0, r0 + nr), np.arange(c0, c0 + nc), indexing="ij")
    with np.errstate(invalid="ignore", over="ignore"):
        ox, oy, dx, dy = offsets(c, X, Y, T)
    pad = np.zeros((H + 16, W + 16, 3), dtype=T)  # ix, iy in [-4, n + 2]: taps in [-7, n + 6]
    pad[8:8 + H, 8:8 + W] = image
    tab = lm.phase_table().astype(T)
    den = None
    if c.vignetting:
        a, b = dx * T(c.qv), dy * T(c.qv)
        rv2 = a * a + b * b
        v = [T(x) for x in c.v]
        den = T(1) + rv2 * (v[0] + rv2 * (v[1] + rv2 * v[2]))
    out = np.zeros((nr, nc, 3), dtype=T)
    details = []
    for ch in range(3):
        with np.errstate(invalid="ignore", over="ignore"):
            sx, sy = channel_coords(c, rec, ch, ox, oy, T)
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
        details.append(SimpleNamespace(sum_abs=bound, fx=fx, fy=fy, ix=ix, iy=iy, inside=inside, den=den))
    return (out, details) if want_bound else out


def channel_splits(c, rec, H, W, window=None):
    """Per channel (inside, ix, iy, fx, fy) of the float32 model over the window: what the tests assert the cases' conditions on."""
    r0, c0, nr, nc = (0, 0, H, W) if window is None else window
    Y, X = np.meshgrid(np.arange(r0, r0 + nr), np.arange(c0, c0 + nc), indexing="ij")
    with np.errstate(invalid="ignore", over="ignore"):
        ox, oy, _, _ = offsets(c, X, Y)
    out = []
    for ch in range(3):
        with np.errstate(invalid="ignore", over="ignore"):
            sx, sy = channel_coords(c, rec, ch, ox, oy)
        in_x, ix, fx = lm.split_phase(sx, W)
        in_y, iy, fy = lm.split_phase(sy, H)
        out.append((in_x & in_y, ix, iy, fx, fy))
    return out


def probes_reach(prof, H, W, scale):
    """lens_model.probes_reach over all three channels: the eight probes through the map in double with the TCA factor in double on
    top, the largest distance any channel's source coordinate lies outside [0, W - 1] x [0, H - 1] (<= 0: all land inside)."""
    c = lm.constants(prof, H, W, scale)
    model, red, blue = record(prof)
    xs, ys = [0.0, (W - 1) / 2.0, float(W - 1)], [0.0, (H - 1) / 2.0, float(H - 1)]
    worst = -math.inf
    for j, y in enumerate(ys):
        for i, x in enumerate(xs):
            if i == 1 and j == 1:
                continue
            dx, dy = x - c.cx, y - c.cy
            u, v = dx * c.q, dy * c.q
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
            g = f * c.inv_scale
            ox, oy = dx * g, dy * g
            ru = math.hypot(ox * c.qv, oy * c.qv)
            for k in ((1.0, 0.0, 0.0), red, blue):
                t = k[0] + ru * (k[1] + ru * k[2]) if model == "poly3" else k[0]
                sx, sy = c.cx + ox * t, c.cy + oy * t
                worst = max(worst, -sx, sx - (W - 1), -sy, sy - (H - 1))
    return worst


# ---- the cases the host and the GPU tests share: (distortion spec, TCA spec) over lens_model.SHAPES
RENDERED = ("linear", "poly3", "edge")
_MODEL = {}


def model(name, tca, shape, window=None):
    """correct_tca of lens_model.frame(*shape) for the case, computed once and shared (callers do not write to it)."""
    key = (name, tca, shape, window)
    if key not in _MODEL:
        prof = profile(name, tca)
        _MODEL[key] = correct_tca(lm.frame(*shape), lm.rounded(lm.constants(prof, *shape)), record(prof, F), window)
        _MODEL[key].setflags(write=False)
    return _MODEL[key]
