"""LensProfile: the numbers of a lens calibration the caller supplies, for the lens correction on the device.

Upstream corrects through lensfunpy (effects.py:22-43): it looks the camera and the lens up in lensfun's database and applies what
it finds.  The lookup is third-party input; this module takes its RESULT -- a distortion model with its coefficients, a vignetting
model, the optical centre, a scale -- and `plan()` turns it into the fp32 constants of one frame size (r2f_lens_plan, which also
resolves scale="auto").  The definition of the correction is in include/r2f.h (r2f_lens_correct).
"""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

from . import _lib

_MODELS = {"none": (_lib.LENS_NONE, 0), "poly3": (_lib.LENS_POLY3, 1), "poly5": (_lib.LENS_POLY5, 2), "ptlens": (_lib.LENS_PTLENS, 3)}


def _floats(name, values, n):
    try:
        out = tuple(float(v) for v in values)
    except TypeError:
        raise ValueError(f"LensProfile.{name} must be {n} number(s), got {values!r}") from None
    if len(out) != n:
        raise ValueError(f"LensProfile.{name} must be {n} number(s), got {len(out)}")
    if not all(math.isfinite(v) for v in out):
        raise ValueError(f"LensProfile.{name} must be finite, got {values!r}")
    return out


@dataclass(frozen=True)
class LensProfile:
    """A frozen, hashable record (part of the image cache key, like `cam` / `lens` upstream).

    distortion: "none" | "poly3" | "poly5" | "ptlens"; coefficients: (), (k1,), (k1, k2), (a, b, c) -- lensfun's models:
    poly3 Rd = Ru (1 - k1 + k1 Ru^2), poly5 Rd = Ru (1 + k1 Ru^2 + k2 Ru^4), ptlens Rd = Ru (a Ru^3 + b Ru^2 + c Ru + 1 - a - b - c).
    vignetting: None or (k1, k2, k3), lensfun's "pa" model: the frame is divided by 1 + k1 r^2 + k2 r^4 + k3 r^6.
    center: (dx, dy) offset of the optical centre from the frame's, in units of r.
    scale: a positive float, or "auto" (the largest view that shows no border: r2f_lens_plan).
    norm_radius_px: the pixel distance at which r = 1; None: half the diagonal, hypot(W - 1, H - 1) / 2."""
    distortion: str = "none"
    coefficients: tuple = ()
    vignetting: tuple | None = None
    center: tuple = (0.0, 0.0)
    scale: float | str = 1.0
    norm_radius_px: float | None = None

    def __post_init__(self):
        if not isinstance(self.distortion, str) or self.distortion not in _MODELS:
            raise ValueError(f"LensProfile.distortion must be one of {sorted(_MODELS)}, got {self.distortion!r}")
        set_ = lambda k, v: object.__setattr__(self, k, v)  # noqa: E731 -- (frozen: normalised to tuples of floats once)
        set_("coefficients", _floats("coefficients", self.coefficients, _MODELS[self.distortion][1]))
        if self.vignetting is not None:
            set_("vignetting", _floats("vignetting", self.vignetting, 3))
        set_("center", _floats("center", self.center, 2))
        if isinstance(self.scale, str):
            if self.scale != "auto":
                raise ValueError(f"LensProfile.scale must be a positive number or 'auto', got {self.scale!r}")
        else:
            (scale,) = _floats("scale", (self.scale,), 1)
            if scale <= 0:
                raise ValueError(f"LensProfile.scale must be positive, got {self.scale!r}")
            set_("scale", scale)
        if self.norm_radius_px is not None:
            (norm,) = _floats("norm_radius_px", (self.norm_radius_px,), 1)
            if norm <= 0:
                raise ValueError(f"LensProfile.norm_radius_px must be positive, got {self.norm_radius_px!r}")
            set_("norm_radius_px", norm)

    def to_c(self) -> _lib.LensProfile:
        model, n = _MODELS[self.distortion]
        p = _lib.LensProfile(model=model, n_coef=n, has_vignetting=int(self.vignetting is not None),
                             auto_scale=int(self.scale == "auto"), scale=1.0 if self.scale == "auto" else self.scale,
                             norm_radius_px=0.0 if self.norm_radius_px is None else self.norm_radius_px)
        p.coef[:n] = self.coefficients
        if self.vignetting is not None:
            p.vignetting[:] = self.vignetting
        p.center[:] = self.center
        return p

    def plan(self, H: int, W: int) -> _lib.LensParams:
        """The r2f_lens_params of an H x W frame (no GPU); ValueError for what the planner refuses (scale="auto" without a
        fitting scale in [1/16, 16], constants that do not fit a float)."""
        out = _lib.LensParams()
        profile = self.to_c()
        if _lib.load().r2f_lens_plan(C.byref(profile), int(H), int(W), C.byref(out)) != _lib.OK:
            raise ValueError(f"r2f_lens_plan refused {self!r} for a {H} x {W} frame")
        return out
