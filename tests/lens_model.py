"""The lens correction of include/r2f.h (r2f_lens_correct) restated in NumPy: what the tests compare the device kernel and the
CPU program of tests/lens_check.cpp with, bit for bit.

The definition.  Take output pixel (X, Y) of the corrected full frame.
  - The host rounds these constants from double: cx, cy, q = 1/(norm_radius_px*scale), inv_scale = 1/scale, c0,
    qv = 1/norm_radius_px.
  - dx = X - cx, dy = Y - cy.
  - u = dx*q, v = dy*q.
  - r2 = u*u + v*v.
  - The model factor f:
      poly3:  f = c0 + k1*r2, with c0 = 1 - k1.
      poly5:  f = 1 + r2*(k1 + k2*r2).
      ptlens: r = sqrt(r2), f = c0 + r*(c + r*(b + r*a)), with c0 = 1 - a - b - c.
      none:   f = 1.
  - g = f*inv_scale.
  - sx = cx + dx*g, sy = cy + dy*g.
Every operation is one correctly rounded fp32 operation, with no contraction.
Sampling restates cv2.remap(..., INTER_LANCZOS4) with constant border 0 (OpenCV's imgwarp.cpp, INTER_BITS = 5):
  - qx = rint(sx*32), ix = qx >> 5, fx = qx & 31.  The same for y.
  - Taps are rows iy-3 .. iy+4 and columns ix-3 .. ix+4.
  - Tap weight is fl(wy[fy][k] * wx[fx][j]).  The table is 32 x 8 float: interpolateLanczos4(p/32) (oracle.stages.lanczos4_coeffs).
  - A tap outside the frame contributes 0 (its product with the sample 0.0f is added like any other).
  - The sum runs per row left to right, and rows top to bottom, each starting from the first product.
  - Then o = max(sum, 0), evaluated as (sum < 0 ? 0 : sum).
With vignetting:
  - rv2 = (dx*qv)^2 + (dy*qv)^2.
  - o = o / (1 + rv2*(v1 + rv2*(v2 + rv2*v3))), an IEEE division.
Edge cases:
  - A coordinate that is NaN, infinite, or beyond the frame by more than the tap reach yields 0 without indexing anything; that
    decision is made in floats (on rint(sx*32), rint(sy*32)), before any conversion to int.
  - One coordinate serves all three channels (upstream never calls the TCA path).
  - A fourth input channel is ignored.
cx = (W - 1)/2 + center_x*norm_radius_px, cy = (H - 1)/2 + center_y*norm_radius_px.

UNPINNED against real OpenCV / lensfun: neither cv2 nor lensfunpy is installed on any machine this project sees, so this model is
a restatement of their sources (imgwarp.cpp's remapLanczos4 with a zero border, lensfun's poly3 / poly5 / ptlens / "pa" formulas)
that no test has compared with the libraries themselves.  What IS pinned: the device kernel and the shared arithmetic against this
model, bit for bit; and the model's CONVENTIONS -- the direction of the polynomial, which TCA constant is red's, that vignetting
divides, the sign of `center`, the direction of the projection -- against a simulated lens that owes nothing to this file
(tests/camera_sim.py; tests/test_camera_sim_host.py runs it on this model, tests/test_gpu_camera_sim.py on the device).  The
libraries' bytes stay unpinned.

Besides the float32 model: `evaluate64`, the same definition in float64 with unrounded constants (what upstream's float64 frame
would see, the table's float weights aside), and per pixel the running error bound gamma_66 * sum |w v| of the float32 sum (64
products of two roundings each and 63 additions: at most 66 roundings on any path to the result).
"""

from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

from oracle import stages as st

F = np.float32
MODELS = {"none": 0, "poly3": 1, "poly5": 2, "ptlens": 3}
U = 2.0 ** -24


def gamma(n):
    return n * U / (1 - n * U)


_TABLE = None


def phase_table():
    """32 x 8 float32: row p = interpolateLanczos4(p / 32)."""
    global _TABLE
    if _TABLE is None:
        _TABLE = np.stack([st.lanczos4_coeffs(F(p) / F(32)) for p in range(32)]).astype(F)
    return _TABLE


def constants(profile, H, W, scale=None):
    """The definition's constants in double for an H x W frame (profile: raw2film_amd.lens.LensProfile; scale: the resolved one
    when the profile says "auto")."""
    scale = float(profile.scale if scale is None else scale)
    norm = profile.norm_radius_px
    if norm is None:
        norm = math.hypot(W - 1, H - 1) / 2.0 or 1.0
    k = tuple(profile.coefficients) + (0.0,) * (3 - len(profile.coefficients))
    c0 = 1.0
    if profile.distortion == "poly3":
        c0 = 1.0 - k[0]
    if profile.distortion == "ptlens":
        c0 = 1.0 - k[0] - k[1] - k[2]
    return SimpleNamespace(model=MODELS[profile.distortion], vignetting=profile.vignetting is not None,
                           cx=(W - 1) / 2.0 + profile.center[0] * norm, cy=(H - 1) / 2.0 + profile.center[1] * norm,
                           q=1.0 / (norm * scale), inv_scale=1.0 / scale, c0=c0, k=k, qv=1.0 / norm,
                           v=tuple(profile.vignetting or (0.0, 0.0, 0.0)), scale=scale)


def rounded(c):
    """The constants as the kernel gets them: rounded to float32."""
    return SimpleNamespace(model=c.model, vignetting=c.vignetting, cx=F(c.cx), cy=F(c.cy), q=F(c.q), inv_scale=F(c.inv_scale),
                           c0=F(c.c0), k=tuple(F(x) for x in c.k), qv=F(c.qv), v=tuple(F(x) for x in c.v), scale=c.scale)


def from_params(p):
    """A raw2film_amd._lib.LensParams (the planner's result) as the model's constants."""
    return SimpleNamespace(model=int(p.model), vignetting=bool(p.vignetting), cx=F(p.cx), cy=F(p.cy), q=F(p.q), inv_scale=F(p.inv_scale),
                           c0=F(p.c0), k=tuple(F(x) for x in p.k), qv=F(p.qv), v=tuple(F(x) for x in p.v), scale=float(p.scale))


def source_coords(c, X, Y, T=F):
    """(sx, sy, dx, dy) of output pixels X, Y (integer arrays), every operation in type T, in the definition's order."""
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
    return T(c.cx) + dx * g, T(c.cy) + dy * g, dx, dy


def split_phase(s, n, T=F):
    """(inside, i, phase) of one axis: the decision on the float rint(s * 32), the int conversion only where it is inside."""
    with np.errstate(invalid="ignore", over="ignore"):
        qf = np.rint(s * T(32))
        inside = (qf >= T(-128)) & (qf < T(n + 3) * T(32))
    q = np.where(inside, qf, 0).astype(np.int64)
    return inside, q >> 5, q & 31


def correct(image, c, window=None, T=F, want_bound=False):
    """The corrected window (row0, col0, rows, cols) -- default: the whole frame -- of `image` (H, W, 3 | 4) as (rows, cols, 3) of
    type T; constants c (rounded() for the float32 model).  want_bound: also sum |w v| per output sample and the phases
    (fx, fy, inside), for the comparison of the float32 model with the float64 evaluation."""
    image = np.asarray(image)[..., :3].astype(T)
    H, W = image.shape[:2]
    r0, c0, nr, nc = (0, 0, H, W) if window is None else window
    Y, X = np.meshgrid(np.arange(r0, r0 + nr), np.arange(c0, c0 + nc), indexing="ij")
    with np.errstate(invalid="ignore", over="ignore"):
        sx, sy, dx, dy = source_coords(c, X, Y, T)
    in_x, ix, fx = split_phase(sx, W, T)
    in_y, iy, fy = split_phase(sy, H, T)
    inside = in_x & in_y
    ix, iy, fx, fy = (np.where(inside, a, 0) for a in (ix, iy, fx, fy))
    pad = np.zeros((H + 16, W + 16, 3), dtype=T)  # ix, iy in [-4, n + 2]: taps in [-7, n + 6]
    pad[8:8 + H, 8:8 + W] = image
    tab = phase_table().astype(T)
    acc = bound = None
    for k in range(8):
        h = hb = None
        for j in range(8):
            w = (tab[fy, k] * tab[fx, j])[..., None]
            prod = w * pad[iy + 5 + k, ix + 5 + j]
            h = prod if j == 0 else h + prod
            if want_bound:
                hb = np.abs(prod.astype(np.float64)) if j == 0 else hb + np.abs(prod.astype(np.float64))
        acc = h if k == 0 else acc + h
        if want_bound:
            bound = hb if k == 0 else bound + hb
    o = np.where(acc < 0, T(0), acc)
    den = None
    if c.vignetting:
        a, b = dx * T(c.qv), dy * T(c.qv)
        rv2 = a * a + b * b
        v = [T(x) for x in c.v]
        den = T(1) + rv2 * (v[0] + rv2 * (v[1] + rv2 * v[2]))
        with np.errstate(invalid="ignore", divide="ignore"):
            o = o / den[..., None]
    o = np.where(inside[..., None], o, T(0)).astype(T)
    if want_bound:
        return o, SimpleNamespace(sum_abs=bound, fx=fx, fy=fy, ix=ix, iy=iy, inside=inside, den=den)
    return o


def evaluate64(image, c):
    """The definition in float64 with the unrounded constants c (constants()); -> (result, details)."""
    return correct(image, c, T=np.float64, want_bound=True)


def probes_reach(profile, H, W, scale):
    """The eight probes of the auto scale (four corners, four edge midpoints) through the map in double at `scale`: the largest
    distance a source coordinate lies outside [0, W - 1] x [0, H - 1], in pixels (<= 0: every probe lands inside)."""
    c = constants(profile, H, W, scale)
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
            sx, sy = c.cx + dx * g, c.cy + dy * g
            worst = max(worst, -sx, sx - (W - 1), -sy, sy - (H - 1))
    return worst


# ---- the cases the host and the GPU tests share
SHAPES = ((33, 47), (96, 128), (150, 210), (1, 64), (64, 1), (7, 9))
PROFILE_SPECS = {
    "ptlens": dict(distortion="ptlens", coefficients=(0.02, -0.06, 0.01)),
    "poly3": dict(distortion="poly3", coefficients=(-0.05,), scale=1.05),
    "poly5": dict(distortion="poly5", coefficients=(0.03, -0.01), scale=0.97),
    "none": dict(distortion="none"),
    "scale-0.25": dict(distortion="ptlens", coefficients=(0.02, -0.06, 0.01), scale=0.25),  # a footprint four times its tile
    "off-centre": dict(distortion="ptlens", coefficients=(0.02, -0.06, 0.01), center=(0.01, -0.006)),
    "vignetting": dict(distortion="poly3", coefficients=(-0.05,), scale=1.05, vignetting=(-0.3, 0.1, -0.02)),
}


def profile(name):
    from raw2film_amd.lens import LensProfile

    return LensProfile(**PROFILE_SPECS[name])


def frame(H, W, channels=3, seed=0):
    """A uniform [0, 4) float32 frame, the same for every test that asks with the same arguments."""
    return np.random.default_rng([seed, H, W, channels]).uniform(0, 4, (H, W, channels)).astype(F)
