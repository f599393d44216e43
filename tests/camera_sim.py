"""A simulated camera and lens: the oracle of the RAW and lens pre-path that owes nothing to the NumPy restatements of include/r2f.h.

A scene known in closed form is exposed through a sensor and a lens that do the physical inverse of what each profile field claims
to correct; the mosaic goes to a backend with that profile, and the scene must come back.  A profile field read wrongly -- by the
kernel and by its model alike -- does not bring it back.  Written from INTEGRATION.md, the profile classes' docstrings and physics:
this module imports no model, no oracle and nothing of raw2film_amd._lib.  Host only, float64, no torch, no fixtures of pytest's.

  Scene            a seeded sum of sinusoids per channel, evaluated at real coordinates (row Y, column X)
  expose           the sensor: inverse camera matrix, white-balance attenuation, scale to the white level, black per site, the CFA,
                   rounding; options: noise, stuck samples, saturation, a sensor mounted in one of the eight orientations
  Lens             the forward physical lens of a LensProfile: distortion, projection, TCA, vignetting, centre
  misreadings      the named wrong readings of one kind of field
  CHECKS           name -> a function that builds a Case: a source, a correct Reading and its misreadings
  measure          a check on a backend -> the RMS error against the scene of the correct reading and of every misreading

A backend is an object with
  develop(mosaic, profile, half_size=False, denoise=None, repair=None, keep_units=False) -> uint16 (h, w, 3)
      repair, the data maximum and resolve of a deferred profile, denoise, demosaic (the profile's median passes and blend level),
      orientation; keep_units: the denoised mosaic is demosaiced with black 0 and the multipliers WITHOUT their 2^-shift
  lens(picture float32 (H, W, 3), profile) -> float (H, W, 3)
  composed(mosaic, profile, denoise, repair, lens_profile, keywords) -> (float (h, w, 3) in scene units, (row0, col0))
      the whole pre-path with the crop window's origin in the corrected frame
tools/make_camera_sim.py has the one over the NumPy models, tests/test_gpu_camera_sim.py the one over the device."""

from __future__ import annotations

import dataclasses
import functools
import math
from typing import NamedTuple

import numpy as np

from raw2film_amd.lens import LensProfile
from raw2film_amd.raw import HotPixels, RawLevels, RawProfile, WaveletDenoise, XTransProfile

BAYER_SHAPE, XTRANS_SHAPE, LENS_SHAPE = (98, 150), (97, 149), (128, 160)
BAYER_PATTERNS = ("RGGB", "BGGR", "GRBG", "GBRG")
XTRANS = ("GBGGRG", "RGRBGB", "GBGGRG", "GRGGBG", "BGBRGR", "GRGGBG")  # Fujifilm's published layout

WB = (2.0, 1.0, 1.5)
SITE_GAIN = (1.0, 0.8, 1.0, 0.9)  # the sensitivity of a quad's four sites on top of the white balance: the two greens differ
BLACK = (200, 260, 330, 400)
BLACK36 = tuple((200, 260, 330, 400, 230, 370)[(7 * k) % 6] for k in range(36))
WHITE = 16383
SENSOR_WHITE = 13500  # where the sensor of the `adjusted` checks really saturates: between 75 % and 100 % of the nominal maximum
MATRIX = ((0.75, 0.20, 0.05), (0.05, 0.85, 0.10), (0.10, 0.02, 0.88))  # rows are the output channels; clearly not symmetric
IDENTITY = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
RING, LENS_RING = 4, 8  # the border left out of every error: the demosaics' and the 8 x 8 gather's reach
# the scenes' top frequencies in cycles per sample: DETAIL where an interpolation has to show its phase; MEDIUM where a reduced size
# or a repair adds an error of its own that grows with the detail; CENTRES where half a sample (first order) has to stand out of
# what a mean over a cell costs (second order); SMOOTH where a field only scales and the rounding of a sample is the floor
DETAIL, MEDIUM, CENTRES, SMOOTH = 0.06, 0.03, 0.012, 0.006


# ---------------------------------------------------------------------------------------------------------------- the scene
class Scene:
    """scene(Y, X) -> (..., 3): per channel a level plus `terms` sinusoids of frequency at most `top` cycles per sample, within about
    [0.1, 0.6].  Frequencies, directions and phases are drawn per channel from `seed`, so the channels differ and the scene has no
    symmetry under mirroring, transposition or a shift by a sample or two.  gain scales it; patch = (y0, y1, x0, x1, g) scales it
    by g inside that box of the scene's coordinates."""

    def __init__(self, seed=11, top=DETAIL, terms=4, gain=1.0, patch=None):
        rng = np.random.default_rng([seed, 20])
        self.level = np.array([0.33, 0.36, 0.34])
        mag = rng.uniform(0.4, 1.0, (3, terms)) * top
        ang = rng.uniform(0.0, 2 * np.pi, (3, terms))
        self.fy, self.fx = mag * np.sin(ang), mag * np.cos(ang)
        self.amp = rng.uniform(0.6, 1.0, (3, terms)) * (0.25 / terms)
        self.phase = rng.uniform(0.0, 2 * np.pi, (3, terms))
        self.gain, self.patch = float(gain), patch

    def channel(self, c, Y, X):
        Y, X = np.asarray(Y, np.float64), np.asarray(X, np.float64)
        v = np.full(np.broadcast(Y, X).shape, self.level[c])
        for k in range(self.fy.shape[1]):
            v = v + self.amp[c, k] * np.sin(2 * np.pi * (self.fy[c, k] * Y + self.fx[c, k] * X) + self.phase[c, k])
        v = v * self.gain
        if self.patch is not None:
            y0, y1, x0, x1, g = self.patch
            v = np.where((Y >= y0) & (Y < y1) & (X >= x0) & (X < x1), v * g, v)
        return v

    def __call__(self, Y, X):
        return np.stack([self.channel(c, Y, X) for c in range(3)], axis=-1)


class Grey:
    """A scene of one level in all three channels."""

    def __init__(self, level=0.4):
        self.level = float(level)

    def channel(self, c, Y, X):
        return np.full(np.broadcast(np.asarray(Y), np.asarray(X)).shape, self.level)

    def __call__(self, Y, X):
        return np.stack([self.channel(c, Y, X) for c in range(3)], axis=-1)


def grid(shape, step=1.0, offset=0.0, origin=(0, 0)):
    """(Y, X) of a (rows, cols) frame's pixels: origin + step * index + offset along both axes."""
    ys = origin[0] + step * np.arange(shape[0]) + offset
    xs = origin[1] + step * np.arange(shape[1]) + offset
    return np.meshgrid(ys, xs, indexing="ij")


# ---------------------------------------------------------------------------------------------------------------- the sensor
def upright_shape(shape, orientation):
    """The sides of the upright frame of a sensor of `shape` mounted in `orientation`."""
    return (shape[1], shape[0]) if orientation & 4 else tuple(shape)


def upright_coords(shape, orientation, ys, xs):
    """Where the sample at sensor coordinates (ys, xs) of a (rows, cols) sensor lies in the upright frame -> (Y, X).
    The eight values are LibRaw's sizes.flip as the profiles' docstring words them, spelled out one by one: the upright frame is the
    sensor's frame mirrored or turned by the stated motion."""
    Hs, Ws = shape
    ys, xs = np.asarray(ys, np.float64), np.asarray(xs, np.float64)
    return {
        0: lambda: (ys, xs),                    # upright
        1: lambda: (ys, Ws - 1 - xs),           # columns mirrored
        2: lambda: (Hs - 1 - ys, xs),           # rows mirrored
        3: lambda: (Hs - 1 - ys, Ws - 1 - xs),  # a half turn
        4: lambda: (xs, ys),                    # the axes swapped
        5: lambda: (Ws - 1 - xs, ys),           # the sensor's frame turned a quarter counter-clockwise: its right edge comes up
        6: lambda: (xs, Hs - 1 - ys),           # ... a quarter clockwise: its left edge comes up
        7: lambda: (Ws - 1 - xs, Hs - 1 - ys),  # the axes swapped about the other diagonal
    }[int(orientation)]()


def cfa_of(pattern):
    """The rows of a colour filter array: "GBRG" -> ("GB", "RG"): the quad at (0, 0) in reading order; six strings stay."""
    return (pattern[:2], pattern[2:]) if isinstance(pattern, str) else tuple(pattern)


def colour_ids(cfa, shape):
    """(rows, cols) ints: the colour (R, G, B = 0, 1, 2) of every site."""
    P = len(cfa)
    table = np.array([["RGB".index(ch) for ch in row] for row in cfa])
    return table[(np.arange(shape[0]) % P)[:, None], (np.arange(shape[1]) % P)[None, :]]


def per_site(values, shape):
    """(rows, cols): values[(y % P) * P + x % P] of a table of P * P."""
    P = int(round(math.sqrt(len(values))))
    table = np.asarray(values, np.float64).reshape(P, P)
    return table[(np.arange(shape[0]) % P)[:, None], (np.arange(shape[1]) % P)[None, :]]


def expose(picture, shape, pattern, black, wb, white_level, matrix, *, site_gain=None, orientation=0, noise=0.0, stuck=0.0, seed=0,
           dark_edges=False):
    """The uint16 (rows, cols) mosaic a sensor of `shape` records of `picture`, a callable (Y, X) -> (..., 3) in the output colour
    space (a Scene, or Lens.through(scene)), in sensor coordinates.
      - camera colour = inverse(matrix) @ picture;
      - channel c is attenuated by min(wb) / wb[c] (and a site by its `site_gain`);
      - picture value 1.0 is white_level - min(black) above the black level;
      - black[(y % P) * P + x % P] is added per site, Gaussian noise of `noise` raw units ahead of the rounding;
      - the sensor saturates at white_level; a share `stuck` of the sites reads white_level whatever it sees."""
    cfa = cfa_of(pattern)
    ys, xs = grid(shape)
    Y, X = upright_coords(shape, orientation, ys, xs)
    camera = np.einsum("ij,...j->...i", np.linalg.inv(np.asarray(matrix, np.float64)), picture(Y, X))
    # no photosite sees negative light.  dark_edges: the caller knows of places that ask for it (the rim of a bright patch whose
    # channels a lens has pulled apart) and keeps them out of what it measures; they read 0.
    assert dark_edges or camera.min() >= 0, "the scene asks a photosite for a negative exposure: choose a milder matrix or scene"
    camera = np.maximum(camera, 0.0)
    ids = colour_ids(cfa, shape)
    seen = np.take_along_axis(camera, ids[..., None], axis=-1)[..., 0]
    seen = seen * (min(wb) / np.asarray(wb, np.float64))[ids]
    if site_gain is not None:
        seen = seen * per_site(site_gain, shape)
    levels = per_site(black, shape)
    raw = seen * (white_level - min(black)) + levels
    rng = np.random.default_rng([seed, 21])
    if noise:
        raw = raw + rng.normal(0.0, noise, shape)
    raw = np.clip(np.rint(raw), 0, white_level)
    if stuck:
        raw = np.where(rng.random(shape) < stuck, white_level, raw)
    return raw.astype(np.uint16)


def numeric_multipliers(pattern, wb, white_level, black, site_gain=None):
    """What a caller states for `expose`'s sensor as numbers: per site of a quad, or (r, g, b) for a 6 x 6 array: the white balance
    AND the scale to 16 bits."""
    scale = 65535.0 / (white_level - min(black))
    rgb = tuple(v / min(wb) * scale for v in wb)
    if not isinstance(pattern, str):
        return rgb
    gains = site_gain or (1.0,) * 4
    return tuple(rgb["RGB".index(ch)] / g for ch, g in zip(pattern, gains))


# ---------------------------------------------------------------------------------------------------------------- the lens
RESIDUAL_PX = 1e-9


def _solve_radius(factor, target):
    """r with r * factor(r) = target (arrays, r >= 0) by fixed-point iteration r <- target / factor(r), which contracts while the
    factor changes slowly along the radius -> (r, the largest residual |r factor(r) - target|)."""
    r = np.array(target, np.float64)
    for _ in range(200):
        r = target / factor(r)
        if np.max(np.abs(r * factor(r) - target), initial=0.0) < 1e-15:
            break
    return r, float(np.max(np.abs(r * factor(r) - target), initial=0.0))


_PROJECTION_ANGLE = {  # the angle off the axis of a ray that lands at radius r of a lens of focal length f
    "fisheye": lambda r, f: r / f,                                                # equidistant: r = f theta
    "stereographic": lambda r, f: 2 * np.arctan(r / (2 * f)),                     # r = 2 f tan(theta / 2)
    "equisolid": lambda r, f: 2 * np.arcsin(np.clip(r / (2 * f), -1, 1)),         # r = 2 f sin(theta / 2)
    "orthographic": lambda r, f: np.arcsin(np.clip(r / f, -1, 1)),                # r = f sin(theta)
}
_PROJECTION_RADIUS = {
    "fisheye": lambda t, f: f * t,
    "stereographic": lambda t, f: 2 * f * np.tan(t / 2),
    "equisolid": lambda t, f: 2 * f * np.sin(t / 2),
    "orthographic": lambda t, f: f * np.sin(t),
}


class Lens:
    """The physical lens a LensProfile describes, in front of an H x W picture.  Radii are in units of the profile's r (one r is
    norm_radius_px pixels; half the diagonal by default) about the optical centre, the frame's centre plus `center` r (x to the
    right, y down).  A scene point of the ideal rectilinear picture at radius r_u
      - lands at r_p = focal * theta-law(atan(r_u / focal)) with a projection (else r_p = r_u);
      - then at r_d = r_p * f(r_p), f the distortion model's polynomial: green's place in the picture;
      - red and blue land at r_d * t(r_d) with their TCA factors (a constant, or v + c r + b r^2);
      - and the picture is attenuated by V = 1 + k1 r^2 + k2 r^4 + k3 r^6 -- r the radius of the pixel of the CORRECTED frame that
        shows the point, which is where the documented correction (remap first, gain second, as upstream calls lensfun) takes it.
    The picture at a pixel shows the scene at the inverse of that chain, found by fixed-point iteration to RESIDUAL_PX.
    inverse_distortion / inverse_projection: the lens does the opposite map of that step (a misreading's lens)."""

    def __init__(self, profile, H, W, inverse_distortion=False, inverse_projection=False):
        self.profile, self.H, self.W = profile, H, W
        self.norm = profile.norm_radius_px if profile.norm_radius_px is not None else math.hypot(W - 1, H - 1) / 2
        self.cx = (W - 1) / 2 + profile.center[0] * self.norm
        self.cy = (H - 1) / 2 + profile.center[1] * self.norm
        self.inverse_distortion, self.inverse_projection = inverse_distortion, inverse_projection
        self.residual_px = 0.0

    def distortion_factor(self, r):
        k, model = self.profile.coefficients, self.profile.distortion
        if model == "poly3":
            return 1 - k[0] + k[0] * r * r
        if model == "poly5":
            return 1 + k[0] * r ** 2 + k[1] * r ** 4
        if model == "ptlens":
            a, b, c = k
            return a * r ** 3 + b * r ** 2 + c * r + 1 - a - b - c
        return np.ones_like(r)

    def tca_factor(self, channel, r):
        if self.profile.tca is None or channel == 1:
            return np.ones_like(r)
        model, values = self.profile.tca
        i = 0 if channel == 0 else 1
        if model == "linear":
            return np.full_like(r, values[i])
        v, c, b = values[i], values[2 + i], values[4 + i]
        return b * r * r + c * r + v

    def _invert(self, factor, r):
        out, residual = _solve_radius(factor, r)
        self.residual_px = max(self.residual_px, residual * self.norm)
        assert residual * self.norm < RESIDUAL_PX, f"the lens inverse's residual is {residual * self.norm:g} pixels"
        return out

    def scene_coords(self, channel, Y, X):
        """Where in the scene's coordinates the picture's point (Y, X) of `channel` looks."""
        dy, dx = (np.asarray(Y, np.float64) - self.cy) / self.norm, (np.asarray(X, np.float64) - self.cx) / self.norm
        r0 = np.hypot(dy, dx)
        r = self._invert(lambda q: self.tca_factor(channel, q), r0)  # green's radius in the picture
        if self.inverse_distortion:
            r = r * self.distortion_factor(r)
        else:
            r = self._invert(self.distortion_factor, r)
        if self.profile.projection is not None:
            kind, focal = self.profile.projection
            if self.inverse_projection:
                r = _PROJECTION_RADIUS[kind](np.arctan(r / focal), focal)
            else:
                r = focal * np.tan(_PROJECTION_ANGLE[kind](r, focal))
        ratio = np.where(r0 > 0, r / np.where(r0 > 0, r0, 1.0), 1.0)
        return self.cy + dy * ratio * self.norm, self.cx + dx * ratio * self.norm

    def attenuation(self, Ys, Xs):
        """V at the scene's point (Ys, Xs): by the radius of the corrected frame's pixel that shows it (scale s: that pixel lies s
        times as far from the centre as the point)."""
        if self.profile.vignetting is None:
            return 1.0
        s = 1.0 if self.profile.scale == "auto" else self.profile.scale
        r2 = (((Ys - self.cy) ** 2 + (Xs - self.cx) ** 2) * s * s) / self.norm ** 2
        k1, k2, k3 = self.profile.vignetting
        return 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3

    def through(self, scene):
        """The picture as a callable (Y, X) -> (..., 3): analytic, no resampling of its own."""
        def picture(Y, X):
            planes = []
            for c in range(3):
                Ys, Xs = self.scene_coords(c, Y, X)
                planes.append(scene.channel(c, Ys, Xs) * self.attenuation(Ys, Xs))
            return np.stack(planes, axis=-1)
        return picture

    def corrected_coords(self, shape=None, origin=(0, 0)):
        """(Y, X) of the scene that pixels of the corrected frame show: the pixel itself at scale 1, else centre + offset / scale."""
        Y, X = grid(shape or (self.H, self.W), origin=origin)
        s = self.profile.scale
        return self.cy + (Y - self.cy) / s, self.cx + (X - self.cx) / s


# ---------------------------------------------------------------------------------------------------------------- misreadings
def _replace(profile, **changes):
    return profile._replace(**changes) if hasattr(profile, "_replace") else dataclasses.replace(profile, **changes)


def _roll(values, n=1):
    values = tuple(values)
    return values[n:] + values[:n]


def xtrans_shifted(dy, dx, base=XTRANS):
    """The 6 x 6 array of a frame whose (0, 0) is `base`'s (dy, dx)."""
    return tuple("".join(base[(y + dy) % 6][(x + dx) % 6] for x in range(6)) for y in range(6))


def misreadings(kind, profile=None):
    """The named wrong readings of one kind of field, for a correctly exposed frame -> [(name, changes)].  `changes` holds one of
      "profile": the wrong profile the backend runs with;
      "target": a word the check's builder turns into the wrongly placed or scaled scene the result is compared with;
      "lens": keywords of the Lens that does the opposite of what the (unchanged) profile says;
      "run": other keywords of the backend's call."""
    p = profile
    if kind == "bayer_cfa":
        return [(f"pattern_{q}", {"profile": _replace(p, pattern=q, multipliers=p.multipliers)}) for q in BAYER_PATTERNS if q != p.pattern]
    if kind == "xtrans_cfa":
        rows = p.pattern
        return [("shifted_one_row", {"profile": _replace(p, pattern=xtrans_shifted(1, 0, rows))}),
                ("shifted_one_column", {"profile": _replace(p, pattern=xtrans_shifted(0, 1, rows))}),
                ("transposed", {"profile": _replace(p, pattern=tuple("".join(rows[y][x] for y in range(6)) for x in range(6)))})]
    if kind == "colour":
        mul = p.multipliers
        out = [("multipliers_reversed", {"profile": _replace(p, multipliers=mul[::-1])})]
        if isinstance(p, RawProfile):
            red = mul[p.pattern.index("R")]
            green = mul[p.pattern.index("G")]
            swapped = tuple(red if ch == "G" else green if ch == "R" else m for ch, m in zip(p.pattern, mul))
            out.append(("greens_swapped_with_red", {"profile": _replace(p, multipliers=swapped)}))
        out.append(("matrix_transposed", {"profile": _replace(p, matrix=tuple(zip(*p.matrix)))}))
        out.append(("black_rotated_one_site", {"profile": _replace(p, black=_roll(p.black))}))
        return out
    if kind == "orientation":
        return [(f"orientation_{o}", {"profile": _replace(p, orientation=o)}) for o in range(8) if o != p.orientation]
    if kind == "reduced_centres":
        return [("centres_at_cell_origin", {"target": "cell_origin"})]
    if kind == "levels":
        lv = p.multipliers
        return [("maximum_is_white_level", {"profile": _replace(p, multipliers=dataclasses.replace(lv, white_level=lv.white_level + int(min(p.black))))}),
                ("maximum_is_white_less_largest_black", {"profile": _replace(p, multipliers=dataclasses.replace(lv, white_level=lv.white_level - int(max(p.black))))}),
                ("white_balance_reversed", {"profile": _replace(p, multipliers=dataclasses.replace(lv, white_balance=lv.white_balance[::-1]))})]
    if kind == "adjusted":
        lv = p.multipliers
        return [("nominal_white_kept", {"profile": _replace(p, multipliers=dataclasses.replace(lv, adjust_maximum_thr=0.0))})]
    if kind == "unclip":
        return [("normalised_as_clip", {"target": "as_clip"})]
    if kind == "denoise_units":
        return [("without_shift", {"run": {"keep_units": True}})]
    if kind == "repair":
        return [("not_repaired", {"run": {"repair": None}})]
    if kind == "distortion":
        return [("inverse_direction", {"lens": {"inverse_distortion": True}}),
                ("not_corrected", {"profile": dataclasses.replace(p, distortion="none", coefficients=())})]
    if kind == "vignetting":
        return [("coefficients_negated", {"profile": dataclasses.replace(p, vignetting=tuple(-v for v in p.vignetting))})]
    if kind == "center":
        return [("center_negated", {"profile": dataclasses.replace(p, center=tuple(-v for v in p.center))}),
                ("center_axes_swapped", {"profile": dataclasses.replace(p, center=p.center[::-1])})]
    if kind == "tca":
        model, v = p.tca
        swapped = tuple(x for pair in zip(v[1::2], v[0::2]) for x in pair)
        reciprocal = (1 / v[0], 1 / v[1]) + tuple(-x for x in v[2:])  # (1 / (v + c r + b r^2) to first order)
        return [("red_and_blue_swapped", {"profile": dataclasses.replace(p, tca=(model, swapped))}),
                ("reciprocal", {"profile": dataclasses.replace(p, tca=(model, reciprocal))})]
    if kind == "projection":
        name, focal = p.projection
        return ([(f"as_{q}", {"profile": dataclasses.replace(p, projection=(q, focal))}) for q in _PROJECTION_ANGLE if q != name]
                + [("inverse_direction", {"lens": {"inverse_projection": True}}),
                   ("not_projected", {"profile": dataclasses.replace(p, projection=None)})])
    raise ValueError(kind)


# ---------------------------------------------------------------------------------------------------------------- checks
class Reading(NamedTuple):
    name: str
    run: dict  # the backend call's keywords
    target: np.ndarray  # the scene where the result must show it, in scene units
    source: np.ndarray | None = None  # a source of its own (a misreading's lens), else the case's


class Case(NamedTuple):
    kind: str  # "raw" | "lens" | "composed"
    source: np.ndarray
    readings: list  # the correct one first
    ring: int
    mask: np.ndarray | None = None  # where the error is measured (None: everywhere inside the ring)
    extras: dict = {}
    channels: tuple = (0, 1, 2)  # the channels the error is measured on


def rms_error(out, target, ring, mask=None, channels=(0, 1, 2)):
    """The RMS over `channels` of out - target inside a ring of `ring` pixels (and `mask`).  Frames of two shapes (a wrong
    orientation) are compared over the top-left window both have."""
    out, target = np.asarray(out, np.float64), np.asarray(target, np.float64)
    rows, cols = min(out.shape[0], target.shape[0]), min(out.shape[1], target.shape[1])
    d = (out[:rows, :cols] - target[:rows, :cols])[ring:rows - ring, ring:cols - ring][..., list(channels)]
    if mask is not None:
        d = d[mask[:rows, :cols][ring:rows - ring, ring:cols - ring]]
    return float(np.sqrt(np.mean(d * d)))


def bayer_profile(pattern="GBRG", matrix=MATRIX, **changes):
    return RawProfile(pattern, BLACK, numeric_multipliers(pattern, WB, WHITE, BLACK, SITE_GAIN), matrix, **changes)


def xtrans_profile(pattern=None, **changes):
    pattern = pattern or xtrans_shifted(1, 2)
    return XTransProfile(pattern, BLACK36, numeric_multipliers(pattern, WB, WHITE, BLACK36), MATRIX, **changes)


def _expose_for(profile, scene, shape, white_level=WHITE, **kw):
    bayer = isinstance(profile, RawProfile)
    return expose(scene, shape, profile.pattern, profile.black, WB, white_level, profile.matrix, site_gain=SITE_GAIN if bayer and not profile.deferred else None,
                  orientation=profile.orientation, **kw)


def _raw_case(profile, scene, shape, kinds, *, half_size=False, target=None, run=None, expose_kw=None, mask=None, extras=None,
              targets=None, white_level=WHITE, channels=(0, 1, 2)):
    """A "raw" case: the mosaic of `scene` for `profile`, the correct reading and the misreadings of `kinds`."""
    mosaic = _expose_for(profile, scene, shape, white_level, **(expose_kw or {}))
    up = upright_shape(shape, profile.orientation)
    if target is None:
        step = profile.reduction if half_size else 1
        centre = (step - 1) / 2  # a cell's centre: 2y + 0.5 of a quad, 3y + 1 of a 3 x 3 cell
        target = scene(*grid((up[0] // step, up[1] // step), step, centre))
    targets = dict(targets or {})
    if half_size:
        targets["cell_origin"] = scene(*grid(target.shape[:2], profile.reduction, 0.0))
    base = {"profile": profile, "half_size": half_size, **(run or {})}
    readings = [Reading("correct", base, target)]
    for kind in kinds:
        for name, ch in misreadings(kind, profile):
            readings.append(Reading(name, {**base, **({"profile": ch["profile"]} if "profile" in ch else {}), **ch.get("run", {})},
                                    targets[ch["target"]] if "target" in ch else target))
    return Case("raw", mosaic, readings, RING, mask, extras or {}, channels)


def check_bayer_full():
    return _raw_case(bayer_profile(), Scene(), BAYER_SHAPE, ["bayer_cfa"])


def check_bayer_half():
    return _raw_case(bayer_profile(), Scene(top=MEDIUM), BAYER_SHAPE, ["bayer_cfa"], half_size=True)


def check_bayer_half_centres():
    """Where a half-size pixel sits.  A quad's red and blue sites lie half a sample off its centre, each its own way, so only green
    -- the mean of two sites either side of the centre -- can tell 2y + 0.5 from 2y; on a smooth scene, where what the mean over a
    cell costs (second order) stays far below what half a sample costs (first order)."""
    return _raw_case(bayer_profile(matrix=IDENTITY), Scene(top=CENTRES), BAYER_SHAPE, ["reduced_centres"], half_size=True, channels=(1,))


def check_xtrans_full():
    return _raw_case(xtrans_profile(), Scene(), XTRANS_SHAPE, ["xtrans_cfa"])


def check_xtrans_third():
    return _raw_case(xtrans_profile(), Scene(), XTRANS_SHAPE, ["xtrans_cfa"], half_size=True)


def check_xtrans_third_centres():
    """Where a third-size pixel sits: every colour's sites of a 3 x 3 cell balance about its centre, 3y + 1; on a smooth scene."""
    return _raw_case(xtrans_profile(XTRANS), Scene(top=CENTRES), XTRANS_SHAPE, ["reduced_centres"], half_size=True)


def check_bayer_colour():
    return _raw_case(bayer_profile(), Scene(top=SMOOTH), BAYER_SHAPE, ["colour"])


def check_xtrans_colour():
    return _raw_case(xtrans_profile(), Scene(top=SMOOTH), XTRANS_SHAPE, ["colour"])


def _check_orientation(o, xtrans=False):
    if xtrans:
        return _raw_case(xtrans_profile(orientation=o), Scene(), XTRANS_SHAPE, ["orientation"])
    return _raw_case(bayer_profile(orientation=o), Scene(), BAYER_SHAPE, ["orientation"])


def levels_profile(white_level=WHITE, thr=0.0, highlight="clip", cls=RawProfile, **changes):
    pattern, black = ("GBRG", BLACK) if cls is RawProfile else (xtrans_shifted(1, 2), BLACK36)
    return cls(pattern, black, RawLevels(WB, white_level, thr), MATRIX, highlight=highlight, **changes)


def check_levels_nominal():
    return _raw_case(levels_profile(), Scene(top=SMOOTH), BAYER_SHAPE, ["levels"])


BRIGHT_BOX = (40, 52, 60, 80)  # rows, columns of the patch that saturates the sensor


def _outside(shape, box, margin=6):
    y0, y1, x0, x1 = box
    Y, X = grid(shape)
    return ~((Y >= y0 - margin) & (Y < y1 + margin) & (X >= x0 - margin) & (X < x1 + margin))


def check_levels_adjusted():
    """The sensor saturates at SENSOR_WHITE, below the nominal white level the file states; a patch of the scene drives it there.
    LibRaw's rule takes the data maximum for the white, and the scene comes back outside the patch."""
    scene = Scene(top=SMOOTH, patch=(*BRIGHT_BOX, 8.0))
    return _raw_case(levels_profile(WHITE, 0.75), scene, BAYER_SHAPE, ["adjusted"], white_level=SENSOR_WHITE,
                     mask=_outside(BAYER_SHAPE, BRIGHT_BOX))


def _unclip_case(highlight):
    """A bright frame on which no site saturates (so Blend finds nothing above its clip level).  The modes that normalise by the
    LARGEST white-balance factor bring the scene back times min(wb) / max(wb); read as the "clip" normalisation it is twice too dark."""
    scene = Scene(top=SMOOTH, gain=1.3)
    shape = BAYER_SHAPE
    as_clip = scene(*grid(shape))
    return _raw_case(levels_profile(highlight=highlight), scene, shape, ["unclip"], target=as_clip * (min(WB) / max(WB)),
                     targets={"as_clip": as_clip})


def check_unclip():
    return _unclip_case("unclip")


def check_blend_unsaturated():
    return _unclip_case("blend")


def check_blend_patch():
    """A patch that saturates the sensor's green sites alone.  No reading brings the scene back there; the figure of merit is the
    error inside the patch, which Blend must lower against "clip" (the one assertion of this case: extras["patch"])."""
    scene = Scene(top=SMOOTH, patch=(*BRIGHT_BOX, 3.6))  # (green passes the white level there; red and blue, attenuated, do not)
    shape = BAYER_SHAPE
    truth = scene(*grid(shape))
    blend, clip = levels_profile(highlight="blend"), levels_profile(highlight="clip")
    mosaic = _expose_for(blend, scene, shape)
    y0, y1, x0, x1 = BRIGHT_BOX
    inside = np.zeros(shape, bool)
    inside[y0 + 2:y1 - 2, x0 + 2:x1 - 2] = True
    f = min(WB) / max(WB)
    readings = [Reading("blend", {"profile": blend}, truth * f), Reading("clip", {"profile": clip}, truth)]
    return Case("raw", mosaic, readings, RING, inside, {"patch": True, "scales": (f, 1.0)})


def _check_median(n):
    return _raw_case(bayer_profile(median_passes=n), Scene(), BAYER_SHAPE, ["bayer_cfa"])


NOISE_SIGMA, MEDIAN_NOISE_SIGMA = 40.0, 150.0  # raw units; the median's frame is one on which noise outweighs what the filter costs
DENOISE = WaveletDenoise(300.0, WHITE - min(BLACK))  # (matched: of 50 .. 16000 the threshold that leaves the smallest error)


def colour_difference_error(out, target, ring=RING):
    """The RMS error of R - G and B - G: what the median of colour differences works on."""
    out, target = np.asarray(out, np.float64), np.asarray(target, np.float64)
    d = (out[..., [0, 2]] - out[..., [1]]) - (target[..., [0, 2]] - target[..., [1]])
    d = d[ring:-ring, ring:-ring]
    return float(np.sqrt(np.mean(d * d)))


def check_median_noise():
    """A noisy frame under 0, 1 and 4 passes: the colour-difference error must not grow (extras["median_noise"])."""
    scene = Scene(top=MEDIUM)
    mosaic = _expose_for(bayer_profile(), scene, BAYER_SHAPE, noise=MEDIAN_NOISE_SIGMA, seed=3)
    target = scene(*grid(BAYER_SHAPE))
    readings = [Reading(f"passes_{n}", {"profile": bayer_profile(median_passes=n)}, target) for n in (0, 1, 4)]
    return Case("raw", mosaic, readings, RING, None, {"median_noise": True})


def check_denoise():
    """A smooth field with noise and a matched threshold.  readings[1] is the noisy frame without the denoise (extras["noisy"]):
    the denoise must lower the error's RMS and move the mean by less than the bias bound."""
    scene = Scene(top=SMOOTH)
    profile = bayer_profile()
    case = _raw_case(profile, scene, BAYER_SHAPE, ["denoise_units"], run={"denoise": DENOISE}, expose_kw={"noise": NOISE_SIGMA, "seed": 5})
    noisy = Reading("noisy", {"profile": profile, "half_size": False}, case.readings[0].target)
    return case._replace(readings=[case.readings[0], noisy, *case.readings[1:]], extras={"noisy": 1})


STUCK = 0.003
REPAIR = HotPixels(2000, ratio=0.8)


def check_repair_bayer():
    return _raw_case(bayer_profile(), Scene(top=MEDIUM), BAYER_SHAPE, ["repair"], run={"repair": REPAIR}, expose_kw={"stuck": STUCK, "seed": 7})


def check_repair_xtrans():
    return _raw_case(xtrans_profile(), Scene(top=0.02), XTRANS_SHAPE, ["repair"], run={"repair": REPAIR}, expose_kw={"stuck": STUCK, "seed": 9})


# ---- the lens step
LENS_PROFILES = {
    "ptlens": LensProfile("ptlens", (0.03, -0.10, 0.02)),
    "poly3": LensProfile("poly3", (-0.06,), scale=1.04),
    "poly5": LensProfile("poly5", (0.05, -0.02), scale=0.98),
    "vignetting": LensProfile("poly3", (-0.06,), vignetting=(-0.35, 0.12, -0.03)),
    "center": LensProfile("ptlens", (0.03, -0.10, 0.02), center=(0.05, -0.03)),
    "tca_linear": LensProfile("ptlens", (0.03, -0.10, 0.02), tca=("linear", (1.03, 0.97))),
    "tca_poly3": LensProfile("poly3", (-0.06,), tca=("poly3", (1.02, 0.985, 0.012, -0.009, -0.02, 0.016))),
    "fisheye": LensProfile("ptlens", (0.03, -0.10, 0.02), projection=("fisheye", 1.2)),
    "stereographic": LensProfile("poly3", (-0.06,), projection=("stereographic", 1.2)),
    "equisolid": LensProfile("poly5", (0.05, -0.02), projection=("equisolid", 1.2)),
    "orthographic": LensProfile("none", (), projection=("orthographic", 1.5)),
}
LENS_KINDS = {"ptlens": ["distortion"], "poly3": ["distortion"], "poly5": ["distortion"], "vignetting": ["vignetting"], "center": ["center"],
              "tca_linear": ["tca"], "tca_poly3": ["tca"], "fisheye": ["projection"], "stereographic": ["projection"],
              "equisolid": ["projection"], "orthographic": ["projection"]}


def _check_lens(name):
    profile, scene = LENS_PROFILES[name], Scene()
    H, W = LENS_SHAPE
    lens = Lens(profile, H, W)
    picture = lens.through(scene)(*grid(LENS_SHAPE)).astype(np.float32)
    target = scene(*lens.corrected_coords())
    readings = [Reading("correct", {"profile": profile}, target)]
    for kind in LENS_KINDS[name]:
        for label, ch in misreadings(kind, profile):
            source = None
            if "lens" in ch:
                source = Lens(profile, H, W, **ch["lens"]).through(scene)(*grid(LENS_SHAPE)).astype(np.float32)
            readings.append(Reading(label, {"profile": ch.get("profile", profile)}, target, source))
    return Case("lens", picture, readings, LENS_RING, None, {"residual_px": lens.residual_px})


# ---- composed: the whole pre-path
COMPOSED_LENS = LensProfile("ptlens", (0.06, -0.22, 0.05), vignetting=(-0.35, 0.12, -0.03), scale=1.05, tca=("linear", (1.05, 0.95)))
COMPOSED_KEYWORDS = dict(frame_width=36, frame_height=24, zoom=1.0, rotate_times=0, rotation=0.0, half_size=False, exposure=0.0,
                         lens_correction=True, max_scale=None)
COMPOSED_ORIENTATION = 6
COMPOSED_SCENE, COMPOSED_NOISE, COMPOSED_DENOISE = 0.03, 8.0, 60.0  # (the threshold: DENOISE's, in proportion to the noise)


def _check_composed(xtrans):
    """Everything the gates admit at once: noise, stuck samples, a mounted sensor, adjusted levels, one median pass, the denoise
    (Bayer only), and a ptlens profile with TCA and vignetting.  The misreadings change one option each."""
    cls, shape = (XTransProfile, XTRANS_SHAPE) if xtrans else (RawProfile, BAYER_SHAPE)
    profile = levels_profile(WHITE, 0.75, cls=cls, orientation=COMPOSED_ORIENTATION, median_passes=1)
    up = upright_shape(shape, COMPOSED_ORIENTATION)
    lens = Lens(COMPOSED_LENS, *up)
    y0, y1, x0, x1 = BRIGHT_BOX
    scene = Scene(top=COMPOSED_SCENE, patch=(y0, y1, x0 - 30, x1 - 30, 8.0))
    mosaic = _expose_for(profile, lens.through(scene), shape, SENSOR_WHITE, noise=COMPOSED_NOISE, stuck=STUCK, seed=13, dark_edges=True)
    denoise = None if xtrans else WaveletDenoise(COMPOSED_DENOISE)
    target = scene(*lens.corrected_coords())
    base = {"profile": profile, "denoise": denoise, "repair": REPAIR, "lens_profile": COMPOSED_LENS}
    readings = [Reading("correct", base, target)]
    wrong = {
        "cfa": dict(misreadings("xtrans_cfa" if xtrans else "bayer_cfa", profile))["shifted_one_row" if xtrans else "pattern_RGGB"],
        "orientation": dict(misreadings("orientation", profile))["orientation_5"],
        "levels": dict(misreadings("adjusted", profile))["nominal_white_kept"],
        "white_balance": dict(misreadings("levels", profile))["white_balance_reversed"],
        "repair": dict(misreadings("repair"))["not_repaired"],
    }
    numeric = profile._replace(multipliers=(1.0, 1.0, 1.0))  # (the colour misreadings are stated for numbers; only black and matrix are taken)
    colour = dict(misreadings("colour", numeric))
    wrong["black"] = {"profile": _replace(profile, black=colour["black_rotated_one_site"]["profile"].black)}
    wrong["matrix"] = {"profile": _replace(profile, matrix=colour["matrix_transposed"]["profile"].matrix)}
    for name, ch in wrong.items():
        readings.append(Reading(name, {**base, **({"profile": ch["profile"]} if "profile" in ch else {}), **ch.get("run", {})}, target))
    for kind, label in (("distortion", "not_corrected"), ("tca", "red_and_blue_swapped"), ("vignetting", "coefficients_negated")):
        readings.append(Reading(f"lens_{kind}", {**base, "lens_profile": dict(misreadings(kind, COMPOSED_LENS))[label]["profile"]}, target))
    mask = _outside(up, (y0, y1, x0 - 30, x1 - 30), margin=10)
    return Case("composed", mosaic, readings, LENS_RING, mask, {"keywords": COMPOSED_KEYWORDS})


CHECKS = {
    "bayer_full": check_bayer_full, "bayer_half": check_bayer_half, "xtrans_full": check_xtrans_full, "xtrans_third": check_xtrans_third,
    "bayer_half_centres": check_bayer_half_centres, "xtrans_third_centres": check_xtrans_third_centres,
    "bayer_colour": check_bayer_colour, "xtrans_colour": check_xtrans_colour,
    **{f"orientation_{o}": functools.partial(_check_orientation, o) for o in range(8)},
    "xtrans_orientation_5": functools.partial(_check_orientation, 5, True),
    "levels_nominal": check_levels_nominal, "levels_adjusted": check_levels_adjusted,
    "unclip": check_unclip, "blend_unsaturated": check_blend_unsaturated, "blend_patch": check_blend_patch,
    "median_1": functools.partial(_check_median, 1), "median_4": functools.partial(_check_median, 4), "median_noise": check_median_noise,
    "denoise": check_denoise, "repair_bayer": check_repair_bayer, "repair_xtrans": check_repair_xtrans,
    **{f"lens_{name}": functools.partial(_check_lens, name) for name in LENS_PROFILES},
    "composed_bayer": functools.partial(_check_composed, False), "composed_xtrans": functools.partial(_check_composed, True),
}


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    """The case of a check, built once and shared (its arrays are read-only)."""
    c = CHECKS[name]()
    for a in [c.source] + [r.target for r in c.readings] + [r.source for r in c.readings if r.source is not None]:
        a.setflags(write=False)
    return c


def run_reading(c: Case, reading: Reading, backend):
    """One reading on a backend -> the result in scene units, placed like the reading's target."""
    source = c.source if reading.source is None else reading.source
    if c.kind == "raw":
        return backend.develop(source, **reading.run).astype(np.float64) / 65535.0
    if c.kind == "lens":
        return np.asarray(backend.lens(source, **reading.run), np.float64)
    frame, (r0, c0) = backend.composed(source, keywords=c.extras["keywords"], **reading.run)
    return frame, (r0, c0)


def results(name, backend) -> dict:
    """{reading name: (the result in scene units, the target it is compared with, the mask)} of a check on a backend."""
    c = case(name)
    out = {}
    for reading in c.readings:
        result = run_reading(c, reading, backend)
        target, mask = reading.target, c.mask
        if c.kind == "composed":
            result, (r0, c0) = result
            target = target[r0:r0 + result.shape[0], c0:c0 + result.shape[1]]
            mask = None if mask is None else mask[r0:r0 + result.shape[0], c0:c0 + result.shape[1]]
        out[reading.name] = (result, target, mask)
    return out


def errors(name, backend, res=None) -> dict:
    """{reading name: RMS error against the scene} of a check on a backend, the correct reading first."""
    c = case(name)
    return {k: rms_error(result, target, c.ring, mask, c.channels) for k, (result, target, mask) in (res or results(name, backend)).items()}


def measure(name, backend) -> dict:
    """Every figure of a check on a backend: {"correct", "misreadings": {name: error}}; a denoise case adds "noisy" (the error
    without the denoise), "bias" (how far the denoise moves the mean error) and "misread_bias" (the same under the misreading); a
    case whose extras say "patch" or "median_noise" has {"figures": {reading: figure of merit}} instead."""
    c = case(name)
    res = results(name, backend)
    errs = errors(name, backend, res)
    names = list(errs)
    if c.extras.get("median_noise"):
        return {"figures": {k: colour_difference_error(result, target, c.ring) for k, (result, target, _) in res.items()}}
    if c.extras.get("patch"):  # in scene units: a mode's error over the factor its normalisation puts on the scene
        return {"figures": {k: errs[k] / s for k, s in zip(names, c.extras["scales"])}}
    out, skip = {}, 1
    if "noisy" in c.extras:
        ring = c.ring
        mean = {k: float(np.mean((result - target)[ring:-ring, ring:-ring])) for k, (result, target, _) in res.items()}
        out.update(noisy=errs["noisy"], bias=mean["correct"] - mean["noisy"], misread_bias=mean[names[2]] - mean["noisy"])
        skip = 2
    out.update(correct=errs[names[0]], misreadings={k: errs[k] for k in names[skip:]})
    return out


def decibels(ratio):
    return 20.0 * math.log10(ratio)
