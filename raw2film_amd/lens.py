"""LensProfile: the numbers of a lens calibration the caller supplies, for the lens correction on the device.

Upstream corrects through lensfunpy (effects.py:22-43): it looks the camera and the lens up in lensfun's database and applies what
it finds.  The lookup is third-party input; this module takes its RESULT -- a distortion model with its coefficients, a vignetting
model, the optical centre, a scale, TCA constants, the lens's projection -- and `plan()` / `plan_tca()` / `plan_projected()` turn it
into the fp32 constants of one frame size (r2f_lens_plan, r2f_lens_plan_tca, r2f_lens_plan_projected, which also resolve
scale="auto").  The definition of the correction is in include/r2f.h (r2f_lens_correct, r2f_lens_correct_tca,
r2f_lens_correct_projected).
"""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field

from . import _lib

_MODELS = {"none": (_lib.LENS_NONE, 0), "poly3": (_lib.LENS_POLY3, 1), "poly5": (_lib.LENS_POLY5, 2), "ptlens": (_lib.LENS_PTLENS, 3)}
_TCA_MODELS = {"linear": (_lib.TCA_LINEAR, 1), "poly3": (_lib.TCA_POLY3, 3)}  # (enum, constants per channel)
_PROJECTIONS = {"fisheye": _lib.PROJ_FISHEYE, "stereographic": _lib.PROJ_STEREOGRAPHIC, "equisolid": _lib.PROJ_EQUISOLID,
                "orthographic": _lib.PROJ_ORTHOGRAPHIC}


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
    norm_radius_px: the pixel distance at which r = 1; None: half the diagonal, hypot(W - 1, H - 1) / 2.
    tca: None, ("linear", (kr, kb)) or ("poly3", (vr, vb, cr, cb, br, bb)) -- transverse chromatic aberration, in the order of
    lensfun's XML attributes: red and blue sample at the corrected coordinate's offset from the centre times kr / kb, or times
    b Ru^2 + c Ru + v of their own constants (r2f_lens_correct_tca).
    projection: None, or (type, focal) with type "fisheye" | "stereographic" | "equisolid" | "orthographic" -- lensfun's lens types
    that are not rectilinear -- and focal the focal length in units of r: the frame is taken to the rectilinear projection in front
    of the distortion model (r2f_lens_correct_projected).  It is the last parameter of the constructor and goes by keyword."""
    distortion: str = "none"
    coefficients: tuple = ()
    vignetting: tuple | None = None
    center: tuple = (0.0, 0.0)
    scale: float | str = 1.0
    norm_radius_px: float | None = None
    projection: tuple | None = field(default=None, kw_only=True)  # (a keyword-only field comes last in the constructor)
    tca: tuple | None = None

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
        if self.tca is not None:
            try:
                model, values = self.tca
            except (TypeError, ValueError):
                raise ValueError(f"LensProfile.tca must be (model, numbers), got {self.tca!r}") from None
            if not isinstance(model, str) or model not in _TCA_MODELS:
                raise ValueError(f"LensProfile.tca's model must be one of {sorted(_TCA_MODELS)}, got {model!r}")
            set_("tca", (model, _floats("tca", values, 2 * _TCA_MODELS[model][1])))
        if self.projection is not None:
            try:
                kind, focal = self.projection
            except (TypeError, ValueError):
                raise ValueError(f"LensProfile.projection must be (type, focal), got {self.projection!r}") from None
            if not isinstance(kind, str) or kind not in _PROJECTIONS:
                raise ValueError(f"LensProfile.projection's type must be one of {sorted(_PROJECTIONS)}, got {kind!r}")
            (focal,) = _floats("projection", (focal,), 1)
            if focal <= 0:
                raise ValueError(f"LensProfile.projection's focal length must be positive, got {self.projection!r}")
            set_("projection", (kind, focal))

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

    def to_c_tca(self) -> _lib.LensTca | None:
        """The r2f_lens_tca of `tca` -- (v, c, b) of red and of blue -- or None without one."""
        if self.tca is None:
            return None
        model, values = self.tca
        code, n = _TCA_MODELS[model]
        t = _lib.LensTca(model=code, n_coef=n)
        t.red[:n], t.blue[:n] = values[0::2], values[1::2]
        return t

    def plan_tca(self, H: int, W: int) -> tuple:
        """(r2f_lens_params, r2f_lens_tca_params) of an H x W frame (no GPU; r2f_lens_plan_tca: with scale="auto" no channel may
        show a border); (plan(H, W), None) for a profile without `tca`.  ValueError for what the planner refuses."""
        tca = self.to_c_tca()
        if tca is None:
            return self.plan(H, W), None
        out, out_tca = _lib.LensParams(), _lib.LensTcaParams()
        profile = self.to_c()
        if _lib.load().r2f_lens_plan_tca(C.byref(profile), C.byref(tca), int(H), int(W), C.byref(out), C.byref(out_tca)) != _lib.OK:
            raise ValueError(f"r2f_lens_plan_tca refused {self!r} for a {H} x {W} frame")
        return out, out_tca

    def to_c_projection(self) -> _lib.LensProjection | None:
        """The r2f_lens_projection of `projection`, or None without one."""
        if self.projection is None:
            return None
        kind, focal = self.projection
        return _lib.LensProjection(type=_PROJECTIONS[kind], focal=focal)

    def plan_projected(self, H: int, W: int) -> tuple:
        """(r2f_lens_params, r2f_lens_projection_params, r2f_lens_tca_params or None) of an H x W frame (no GPU;
        r2f_lens_plan_projected: with scale="auto" the probes go through the projection, and through `tca` when there is one);
        (plan_tca(H, W)[0], None, plan_tca(H, W)[1]) for a profile without `projection`.  ValueError for what the planner refuses:
        with scale="auto" also a circular fisheye, whose image circle never reaches the frame's boundary."""
        projection = self.to_c_projection()
        if projection is None:
            params, tca_params = self.plan_tca(H, W)
            return params, None, tca_params
        tca = self.to_c_tca()
        out, out_projection = _lib.LensParams(), _lib.LensProjectionParams()
        out_tca = None if tca is None else _lib.LensTcaParams()
        profile = self.to_c()
        rc = _lib.load().r2f_lens_plan_projected(C.byref(profile), C.byref(projection), None if tca is None else C.byref(tca), int(H), int(W),
                                                 C.byref(out), C.byref(out_projection), None if tca is None else C.byref(out_tca))
        if rc != _lib.OK:
            raise ValueError(f"r2f_lens_plan_projected refused {self!r} for a {H} x {W} frame")
        return out, out_projection, out_tca
