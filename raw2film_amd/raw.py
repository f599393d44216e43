"""RawProfile: what a RAW file's parser knows of a Bayer frame, for the demosaic on the device.

Upstream has LibRaw do everything behind the file parser (raw_conversion.raw_to_linear, raw_conversion.py:33-53): black / scale,
demosaic, camera matrix, 16-bit clip.  The parser is third-party input; this module takes its RESULT -- the CFA pattern, the black
levels, the multipliers, the camera matrix -- and `plan()` turns it into the constants of one frame size (r2f_demosaic_plan).  The
mosaic itself is the `src` of the call.  The definition of the arithmetic is in include/r2f.h (r2f_demosaic_u16).

XTransProfile is the same record for a 6 x 6 array (r2f_xtrans_plan, r2f_demosaic_xtrans_u16).  Each profile states its own
`reduction`: what half_size=True divides a mosaic's sides by.

RawLevels states the sensor's levels instead of finished multipliers: a profile that holds one as its `multipliers` is DEFERRED --
its scale follows LibRaw's adjust_maximum rule from the frame's data maximum, which the device measures (r2f_mosaic_maximum,
r2f_raw_scale_plan; include/r2f.h has the definition, and its parity with LibRaw's bytes is unpinned like the demosaic's).

`highlight` is LibRaw's highlight mode (rawpy's highlight_mode=): "clip" (0, the default), and on a deferred profile "unclip" (1)
and "blend" (2), which normalise by the largest white-balance factor (r2f_raw_scale_plan_highlight); a profile resolved from
"blend" carries ("blend", clip), the level above which the demosaic blends a pixel's chroma (r2f_demosaic_blend_u16).  The rebuild
modes 3 .. 9 are not built.

`median_passes` is LibRaw's med_passes (rawpy's median_filter_passes=, dcraw's -m n): 0 .. 4 passes of the 3 x 3 median of the
colour differences between the interpolation and the highlight blend (include/r2f.h, step M; r2f_demosaic_median_u16).  A keyword
of both profiles, 0 by default; it is part of equality, hash and repr but no dataclass field (`_median_keyword`).

WaveletDenoise is no part of a profile: it is the record of process(raw_denoise=), LibRaw's wavelet denoise of the Bayer mosaic ahead
of its demosaic (rawpy's noise_thr=; r2f_mosaic_denoise_plan, r2f_mosaic_denoise).

HotPixels is the record of process(raw_repair=): the repair of hot pixels of a mosaic, Bayer or X-Trans, ahead of everything else that
reads it -- the project's own rule, not LibRaw's bad_pixels (r2f_mosaic_repair_plan, r2f_mosaic_repair).
"""

from __future__ import annotations

import ctypes as C
import math
import numbers
from dataclasses import dataclass, field, replace

from . import _lib

_HIGHLIGHT_MODES = {"clip": _lib.HIGHLIGHT_CLIP, "unclip": _lib.HIGHLIGHT_UNCLIP, "blend": _lib.HIGHLIGHT_BLEND}
_PATTERNS = {"RGGB": _lib.CFA_RGGB, "BGGR": _lib.CFA_BGGR, "GRBG": _lib.CFA_GRBG, "GBRG": _lib.CFA_GBRG}


def _floats(name, values, counts, who):
    try:
        out = tuple(float(v) for v in values)
    except TypeError:
        raise ValueError(f"{who}.{name} must be {' or '.join(str(n) for n in counts)} numbers, got {values!r}") from None
    if len(out) not in counts:
        raise ValueError(f"{who}.{name} must be {' or '.join(str(n) for n in counts)} numbers, got {len(out)}")
    if not all(math.isfinite(v) for v in out):
        raise ValueError(f"{who}.{name} must be finite, got {values!r}")
    return out


def _matrix(matrix, who):
    try:
        rows = tuple(_floats("matrix", row, (3,), who) for row in matrix)
    except TypeError:
        raise ValueError(f"{who}.matrix must be 3 x 3, got {matrix!r}") from None
    if len(rows) != 3:
        raise ValueError(f"{who}.matrix must be 3 x 3, got {len(rows)} rows")
    if any(abs(v) > 64 for row in rows for v in row):
        raise ValueError(f"{who}.matrix entries must lie in [-64, 64], got {matrix!r}")
    return rows


def _median_passes(who, n) -> int:
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or not 0 <= n <= _lib.MEDIAN_MAX_PASSES:
        raise ValueError(f"{who}.median_passes must be an integer in [0, {_lib.MEDIAN_MAX_PASSES}] (LibRaw's med_passes), got {n!r}")
    return int(n)


def _median_keyword(cls):
    """Give a profile dataclass its `median_passes`: a keyword of the constructor (default 0), validated, part of equality, hash
    and repr (a profile with 0 passes has the hash and the repr of before), and carried by
    dataclasses.replace(profile, ..., median_passes=n) -- but NOT a dataclass field: the six fields, their
    positional order and `orientation` as the last of them are what callers and the cache keys of stored frames were built on, and
    stay.  So plain dataclasses.replace(profile, ...) drops it like any non-field; `_MosaicProfile._replace` carries it."""
    init, eq, hash_, repr_ = cls.__init__, cls.__eq__, cls.__hash__, cls.__repr__

    def __init__(self, *args, median_passes=0, **kwargs):
        object.__setattr__(self, "median_passes", _median_passes(cls.__name__, median_passes))
        init(self, *args, **kwargs)

    def __eq__(self, other):
        same = eq(self, other)
        return same if same is NotImplemented or not same else self.median_passes == other.median_passes

    def __hash__(self):
        return hash((hash_(self), self.median_passes)) if self.median_passes else hash_(self)

    def __repr__(self):
        return f"{repr_(self)[:-1]}, median_passes={self.median_passes})" if self.median_passes else repr_(self)

    for fn in (__init__, __eq__, __hash__, __repr__):
        fn.__qualname__ = f"{cls.__qualname__}.{fn.__name__}"
        setattr(cls, fn.__name__, fn)
    return cls


@dataclass(frozen=True)
class RawLevels:
    """The sensor's levels, in place of a profile's numeric `multipliers`: a frozen, hashable record.

    white_balance: (r, g, b), finite and > 0 (only their ratios count: the smallest becomes 1).
    white_level: the nominal white level, an integer in [1, 65535], before the black level is subtracted.
    adjust_maximum_thr: LibRaw's parameter of the same name, in [0, 1]; 0.75 is its default, which upstream's raw.postprocess call
        leaves alone; 0 never adjusts.
    A profile holding one scales a frame by 65535 / (white_level - min(black)), or by 65535 / d when the frame's largest
    black-subtracted sample d lies between the threshold's share and the whole of that maximum (include/r2f.h: the Scale steps)."""
    white_balance: tuple
    white_level: int
    adjust_maximum_thr: float = 0.75

    def __post_init__(self):
        wb = _floats("white_balance", self.white_balance, (3,), "RawLevels")
        if any(not v > 0 for v in wb):
            raise ValueError(f"RawLevels.white_balance must be three positive numbers, got {self.white_balance!r}")
        level = self.white_level
        if isinstance(level, bool) or not isinstance(level, numbers.Integral) or not 1 <= level <= 65535:
            raise ValueError(f"RawLevels.white_level must be an integer in [1, 65535], got {level!r}")
        thr = self.adjust_maximum_thr
        if isinstance(thr, bool) or not isinstance(thr, numbers.Real) or not 0 <= thr <= 1:  # (a NaN fails the comparison)
            raise ValueError(f"RawLevels.adjust_maximum_thr must be a number in [0, 1], got {thr!r}")
        for name, value in (("white_balance", wb), ("white_level", int(level)), ("adjust_maximum_thr", float(thr))):
            object.__setattr__(self, name, value)

    def to_c(self) -> _lib.RawLevels:
        c = _lib.RawLevels(white_level=self.white_level, adjust_maximum_thr=self.adjust_maximum_thr)
        c.white_balance[:] = self.white_balance
        return c

    def scale(self, black, data_maximum: int = 0) -> _lib.RawScale:
        """r2f_raw_scale_plan of these levels, a profile's black table (4 or 36 levels) and a data maximum (0: the nominal scale);
        ValueError for what the planner refuses (a white level that is not above the smallest black level, a maximum above 65535)."""
        d = data_maximum
        if isinstance(d, bool) or not isinstance(d, numbers.Integral) or not 0 <= d <= 65535:
            raise ValueError(f"the data maximum must be an integer in [0, 65535], got {data_maximum!r}")
        out = _lib.RawScale()
        table = (C.c_double * len(black))(*black)
        if _lib.load().r2f_raw_scale_plan(C.byref(self.to_c()), table, len(black), int(d), C.byref(out)) != _lib.OK:
            raise ValueError(f"r2f_raw_scale_plan refused {self!r} with black levels {tuple(black)!r} and a data maximum of {d}")
        return out

    def scale_highlight(self, black, data_maximum: int = 0, highlight: str = "clip") -> tuple:
        """r2f_raw_scale_plan_highlight: `scale` with LibRaw's highlight mode "clip", "unclip" or "blend" -> (the r2f_raw_scale, the
        r2f_highlight: mode and, for "blend", the clip level).  "clip" is `scale` itself.  ValueError for what `scale` refuses, and
        for a "blend" whose clip level would fall below 1."""
        if highlight not in _HIGHLIGHT_MODES:
            raise ValueError(f"the highlight mode must be one of {sorted(_HIGHLIGHT_MODES)}, got {highlight!r}")
        if highlight == "clip":
            return self.scale(black, data_maximum), _lib.Highlight()
        d = data_maximum
        if isinstance(d, bool) or not isinstance(d, numbers.Integral) or not 0 <= d <= 65535:
            raise ValueError(f"the data maximum must be an integer in [0, 65535], got {data_maximum!r}")
        out, hl = _lib.RawScale(), _lib.Highlight()
        table = (C.c_double * len(black))(*black)
        if _lib.load().r2f_raw_scale_plan_highlight(C.byref(self.to_c()), table, len(black), int(d), _HIGHLIGHT_MODES[highlight],
                                                    C.byref(out), C.byref(hl)) != _lib.OK:
            raise ValueError(f"r2f_raw_scale_plan_highlight refused {self!r} with black levels {tuple(black)!r}, a data maximum of {d} "
                             f"and highlight = {highlight!r}")
        return out, hl


@dataclass(frozen=True)
class WaveletDenoise:
    """The wavelet denoise of a Bayer mosaic ahead of its demosaic (process(raw_denoise=); rawpy's noise_thr=, dcraw's -n): a frozen,
    hashable record (part of the image cache key).  include/r2f.h has the definition (r2f_mosaic_denoise); parity with LibRaw's
    bytes is unpinned.  Not built: the pull of a quad's two greens toward each other (the second half of dcraw's function),
    anything for X-Trans mosaics, streaming in row bands.

    threshold: rawpy's noise_thr, a number in (0, 1e6].
    maximum: the white level less the black level the frame is scaled by, an integer in [1, 65535]; None takes the resolved
        scale's `maximum_used` of a profile with RawLevels (a numeric profile needs the number)."""
    threshold: float
    maximum: int | None = None

    def __post_init__(self):
        t = self.threshold
        if isinstance(t, bool) or not isinstance(t, numbers.Real) or not 0 < t <= 1e6:  # (a NaN fails the comparison)
            raise ValueError(f"WaveletDenoise.threshold must be a number in (0, 1e6], got {t!r}")
        object.__setattr__(self, "threshold", float(t))
        if self.maximum is not None:
            object.__setattr__(self, "maximum", self._maximum(self.maximum))

    @staticmethod
    def _maximum(m) -> int:
        if isinstance(m, bool) or not isinstance(m, numbers.Integral) or not 1 <= m <= 65535:
            raise ValueError(f"WaveletDenoise.maximum must be an integer in [1, 65535], got {m!r}")
        return int(m)

    def plan(self, black, H: int, W: int, maximum=None) -> _lib.DenoiseParams:
        """The r2f_denoise_params of an H x W mosaic (no GPU: r2f_mosaic_denoise_plan).  black: the four levels per site of the
        quad; maximum: in place of the record's own (one of them is required).  ValueError for what the planner refuses (an odd
        side or a side below 64, a black level outside [0, 65535], a threshold that rounds to 0 as a float)."""
        m = self._maximum(self.maximum if maximum is None else maximum) if (maximum is not None or self.maximum is not None) else None
        if m is None:
            raise ValueError(f"{self!r} has no maximum and none was given: a numeric profile needs WaveletDenoise(threshold, maximum)")
        black = _floats("black", black, (4,), "WaveletDenoise.plan")
        out = _lib.DenoiseParams()
        if _lib.load().r2f_mosaic_denoise_plan(self.threshold, m, (C.c_double * 4)(*black), int(H), int(W), C.byref(out)) != _lib.OK:
            raise ValueError(f"r2f_mosaic_denoise_plan refused {self!r} with black levels {black!r} and a maximum of {m} for a {H} x {W} "
                             "mosaic (both sides must be even and at least 64)")
        return out

    def shift(self, maximum=None) -> int:
        """s of include/r2f.h: the largest shift with (maximum << s) < 65536.  The denoised mosaic is in units of t << s."""
        return int(self.plan((0, 0, 0, 0), 64, 64, maximum).shift)

    @staticmethod
    def shifted(profile, shift: int):
        """The numeric RawProfile the demosaic behind the denoise runs with: black 0 and every multiplier times 2^-shift (exact);
        all else is the profile's, a blend clip level included."""
        return profile._replace(black=(0.0,) * 4, multipliers=tuple(m * 2.0 ** -int(shift) for m in profile.multipliers))


@dataclass(frozen=True)
class HotPixels:
    """The repair of hot pixels of a mosaic ahead of everything else that reads it (process(raw_repair=)): a frozen, hashable record
    (part of the image cache key).  include/r2f.h has the definition (r2f_mosaic_repair): the project's own rule, NOT LibRaw's
    bad_pixels (a caller's coordinate list, sequential and in place: not built).  A sample is hot when it stands more than
    `threshold` above its black level and at least `min_neighbours` of its four neighbours of the same colour lie below `ratio`
    times it; it takes the largest of those neighbours.  For a Bayer or an X-Trans mosaic.

    threshold: an integer in [0, 65535], in black-subtracted raw units.
    ratio: a number whose q = round(ratio * 256) lies in [1, 255]; 0.125 (q = 32) by default.
    min_neighbours: 3 or 4."""
    threshold: int
    ratio: float = 0.125
    min_neighbours: int = 4

    def __post_init__(self):
        t = self.threshold
        if isinstance(t, bool) or not isinstance(t, numbers.Integral) or not 0 <= t <= 65535:
            raise ValueError(f"HotPixels.threshold must be an integer in [0, 65535], got {t!r}")
        r = self.ratio
        if isinstance(r, bool) or not isinstance(r, numbers.Real) or not math.isfinite(r) or not 1 <= round(r * 256) <= 255:
            raise ValueError(f"HotPixels.ratio must be a number whose round(ratio * 256) lies in [1, 255], got {r!r}")
        n = self.min_neighbours
        if isinstance(n, bool) or not isinstance(n, numbers.Integral) or n not in (3, 4):
            raise ValueError(f"HotPixels.min_neighbours must be 3 or 4, got {n!r}")
        for name, value in (("threshold", int(t)), ("ratio", float(r)), ("min_neighbours", int(n))):
            object.__setattr__(self, name, value)

    @property
    def q(self) -> int:
        """The ratio in 1/256ths, as the device compares with it: q * t_centre > 256 * t_neighbour."""
        return int(round(self.ratio * 256))

    def plan(self, profile, H: int, W: int) -> _lib.RepairParams:
        """The r2f_repair_params of an H x W mosaic of `profile` (a RawProfile or an XTransProfile; no GPU: r2f_mosaic_repair_plan).
        ValueError for another kind of profile and for what the planner refuses (a side below 6, an X-Trans pattern with a phase
        and quadrant that has no neighbour of its colour inside ring 2)."""
        if isinstance(profile, RawProfile):
            period, cfa = 2, None
        elif isinstance(profile, XTransProfile):
            period, cfa = 6, (C.c_int32 * 36)(*["RGB".index(c) for row in profile.pattern for c in row])
        else:
            raise ValueError(f"HotPixels.plan needs a RawProfile or an XTransProfile, got {type(profile).__name__}")
        out = _lib.RepairParams()
        black = (C.c_double * len(profile.black))(*profile.black)
        if _lib.load().r2f_mosaic_repair_plan(period, cfa, black, self.threshold, self.q, self.min_neighbours, int(H), int(W),
                                              C.byref(out)) != _lib.OK:
            raise ValueError(f"r2f_mosaic_repair_plan refused {self!r} with {profile!r} for a {H} x {W} mosaic (both sides must be at "
                             "least 6)")
        return out


class _MosaicProfile:
    """What the two profiles share: the normalisation of black, multipliers, matrix and orientation, `oriented_shape()` and `plan()`.  A profile class states
    `_sites` (black levels per period of its array), `_multiplier_counts`, its params type, its planner's name and `to_c` (the C
    profile).
    With a RawLevels as its `multipliers` a profile is deferred (`deferred`): the numbers come from the frame (`resolve`)."""

    def _normalise(self):
        """black, multipliers and matrix as tuples of floats and the orientation as an int, checked (frozen: set once, from
        __post_init__)."""
        who = type(self).__name__
        black = self.black
        if isinstance(black, numbers.Real) and not isinstance(black, bool):
            black = (black,) * self._sites
        black = _floats("black", black, (self._sites,), who)
        if any(b < 0 or b > 65535 or b != math.floor(b) for b in black):
            raise ValueError(f"{who}.black must be integers in [0, 65535], got {self.black!r}")
        mul = self.multipliers
        if not isinstance(mul, RawLevels):  # (a deferred profile keeps the record: part of equality and hash like the numbers)
            mul = _floats("multipliers", mul, self._multiplier_counts, who)
            if any(not 0 < m <= 1024 for m in mul):
                raise ValueError(f"{who}.multipliers must lie in (0, 1024], got {self.multipliers!r}")
        for name, value in (("black", black), ("multipliers", mul), ("matrix", _matrix(self.matrix, who))):
            object.__setattr__(self, name, value)
        o = self.orientation
        if isinstance(o, bool) or not isinstance(o, numbers.Integral) or not 0 <= o <= 7:
            raise ValueError(f"{who}.orientation must be an integer 0 .. 7 (LibRaw's sizes.flip bits), got {o!r}")
        object.__setattr__(self, "orientation", int(o))
        object.__setattr__(self, "highlight", self._highlight(who, isinstance(mul, RawLevels)))

    def _highlight(self, who, deferred):
        """The `highlight` field, checked: a mode's name on a deferred profile; "clip" or ("blend", clip) on a numeric one."""
        h = self.highlight
        if isinstance(h, list):
            h = tuple(h)
        rebuild = isinstance(h, numbers.Integral) and not isinstance(h, bool) and 3 <= h <= 9
        if rebuild or h == "rebuild" or (isinstance(h, tuple) and h[:1] == ("rebuild",)):
            raise ValueError(f"{who}.highlight = {self.highlight!r}: LibRaw's rebuild modes (3 .. 9) are not built; "
                             "\"clip\", \"unclip\" and \"blend\" are")
        if deferred:
            if not isinstance(h, str) or h not in _HIGHLIGHT_MODES:
                raise ValueError(f"{who}.highlight of a profile with RawLevels must be \"clip\", \"unclip\" or \"blend\", got {self.highlight!r}")
            return h
        if isinstance(h, str) and h in ("unclip", "blend"):
            raise ValueError(f"{who}.highlight = {h!r} needs the sensor's levels: numeric multipliers already fix the normalisation; "
                             "give a RawLevels as `multipliers` (or (\"blend\", clip) with the level a resolved profile carries)")
        if isinstance(h, str) and h == "clip":
            return h
        if (isinstance(h, tuple) and len(h) == 2 and h[0] == "blend" and isinstance(h[1], numbers.Integral)
                and not isinstance(h[1], bool) and 1 <= h[1] <= 65535):
            return ("blend", int(h[1]))
        raise ValueError(f"{who}.highlight must be \"clip\" or (\"blend\", clip) with clip an integer in [1, 65535], got {self.highlight!r}")

    def _replace(self, **changes):
        """dataclasses.replace that carries `median_passes`, which is no field (`_median_keyword`)."""
        return replace(self, **{"median_passes": self.median_passes, **changes})

    @property
    def blend_clip(self):
        """The clip level of a numeric ("blend", clip) profile, which the demosaic blends above (r2f_demosaic_blend_u16); else None."""
        return self.highlight[1] if isinstance(self.highlight, tuple) else None

    def oriented_shape(self, H: int, W: int, half_size: bool = False) -> tuple:
        """(rows, cols) of the frame the demosaic of an H x W mosaic yields with this profile's orientation: the demosaiced frame's
        sides (the mosaic's, divided by `reduction` and rounded down with half_size), swapped where bit 4 is set."""
        rows, cols = (int(H) // self.reduction, int(W) // self.reduction) if half_size else (int(H), int(W))
        return (cols, rows) if self.orientation & 4 else (rows, cols)

    @property
    def deferred(self) -> bool:
        """The multipliers are a RawLevels: the scale is derived from the frame's data maximum (`resolve`)."""
        return isinstance(self.multipliers, RawLevels)

    def resolve(self, data_maximum: int):
        """This profile with numeric multipliers: r2f_raw_scale_plan of its levels, its black table and the frame's data maximum
        (HipContext.mosaic_maximum measures it; 0 is the nominal scale).  A numeric profile is returned as it is.  ValueError for
        what the planner refuses, and for a scale outside (0, 1024].  The highlight mode goes into the numbers
        (r2f_raw_scale_plan_highlight): "unclip" resolves to a profile with highlight="clip" -- its multipliers are normalised by the
        largest white-balance factor, and nothing else differs --, "blend" to one with ("blend", clip)."""
        return self.resolve_scale(data_maximum)[0]

    def resolve_scale(self, data_maximum: int) -> tuple:
        """(resolve(data_maximum), the r2f_raw_scale it was resolved with: mul, maximum_used, adjusted) from one run of the planner;
        (the profile itself, None) for a numeric profile."""
        if not self.deferred:
            return self, None
        scale, hl = self.multipliers.scale_highlight(self.black, data_maximum, self.highlight)
        highlight = ("blend", int(hl.clip)) if hl.mode == _lib.HIGHLIGHT_BLEND else "clip"
        return self._replace(multipliers=tuple(scale.mul), highlight=highlight), scale

    def _c_multipliers(self) -> tuple:
        """The multipliers `to_c` states, per site or colour as the profile keeps them: a deferred profile's are those of the
        NOMINAL scale (resolve(0)'s, unchecked: the planner refuses what is out of range)."""
        if not self.deferred:
            return self.multipliers
        mul = tuple(self.multipliers.scale_highlight(self.black, 0, self.highlight)[0].mul)
        return self._spread(mul)

    def _spread(self, mul):  # (r, g, b) as the profile keeps its multipliers
        return mul

    def plan(self, H: int, W: int, half_size: bool = False):
        """The params of an H x W mosaic (no GPU: r2f_demosaic_params / r2f_xtrans_params); ValueError for what the planner refuses
        (a frame below the array's 2 x 2 / 6 x 6, an odd side with half_size of a Bayer frame, an X-Trans pattern that is not
        admissible -- for the reduced size, with half_size --, a multiplier that rounds to 0 as a float).
        A deferred profile (`to_c` as well) plans its NOMINAL scale, resolve(0)'s: phase 1 needs out_h / out_w and the tables
        without a GPU, and the frame's own scale is planned once the device has measured its maximum (`resolve`)."""
        out = self._c_params()
        profile = self.to_c(half_size)
        if getattr(_lib.load(), self._planner)(C.byref(profile), int(H), int(W), C.byref(out)) != _lib.OK:
            raise ValueError(f"{self._planner} refused {self!r} for a {H} x {W} mosaic (half_size={bool(half_size)})")
        return out


@_median_keyword
@dataclass(frozen=True)
class RawProfile(_MosaicProfile):
    """A frozen, hashable record (part of the image cache key, like LensProfile).

    pattern: "RGGB" | "BGGR" | "GRBG" | "GBRG", the colours of the quad at (0, 0) in reading order.
    black: one level for every site, or 4 per site of the quad (k = (y & 1) * 2 + (x & 1)); integers in [0, 65535].
    multipliers: (r, g, b), or 4 per site; each in (0, 1024].  They hold the white balance AND the scale to 16 bits.  Or a
        RawLevels: the profile is then deferred, and its (r, g, b) are derived from each frame's data maximum (`resolve`).
    matrix: 3 x 3, rows are the output channels; |entries| <= 64.
    orientation: 0 .. 7, how the sensor was held, as LibRaw's sizes.flip bits (4 swaps the axes, 2 mirrors rows, 1 mirrors
        columns: 0 upright, 3 180 degrees, 5 90 degrees counter-clockwise, 6 90 degrees clockwise).  The demosaic writes the frame
        that way round (r2f_demosaic_oriented_u16), and everything behind it -- crops, statistic, lens step, turns -- sees that
        frame, as upstream's does.  (Not `flip`: process(flip=) is the aspect's.)
    highlight: LibRaw's highlight mode (rawpy's highlight_mode=).  With a RawLevels: "clip" (0), "unclip" (1: normalised by the
        largest white-balance factor, so nothing is cut below the sensor's saturation) or "blend" (2: unclip, and pixels with a
        channel above the clip level take the chroma of their clipped version).  With numeric multipliers: "clip", or ("blend",
        clip) as `resolve` of a "blend" profile yields it (`blend_clip`).  The rebuild modes 3 .. 9 are not built.
    median_passes (keyword): LibRaw's med_passes, an int in 0 .. 4 (0: none): that many passes of the 3 x 3 median of R - G and
        B - G over the demosaiced frame, between the interpolation and the highlight blend (r2f_demosaic_median_u16)."""
    pattern: str = "RGGB"
    black: tuple | float = 0
    multipliers: tuple | RawLevels = (1.0, 1.0, 1.0)
    matrix: tuple = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
    # keyword-only, and stated ahead of `orientation`: the positional order (..., matrix, orientation) and the last field stay as they were
    highlight: str | tuple = field(default="clip", kw_only=True)
    orientation: int = 0

    reduction = 2  # what half_size=True divides a mosaic's sides by (no dataclass field: not part of equality, hash or repr)
    _sites, _multiplier_counts = 4, (3, 4)
    _c_params, _planner = _lib.DemosaicParams, "r2f_demosaic_plan"

    def __post_init__(self):
        if not isinstance(self.pattern, str) or self.pattern not in _PATTERNS:
            raise ValueError(f"RawProfile.pattern must be one of {sorted(_PATTERNS)}, got {self.pattern!r}")
        self._normalise()
        if not self.deferred and len(self.multipliers) == 3:
            object.__setattr__(self, "multipliers", self._spread(self.multipliers))

    def _spread(self, mul):  # (r, g, b) -> per site of the quad
        return tuple(mul["RGB".index(c)] for c in self.pattern)

    def to_c(self, half_size: bool = False) -> _lib.RawProfile:
        p = _lib.RawProfile(pattern=_PATTERNS[self.pattern], half_size=int(bool(half_size)))
        p.black[:] = self.black
        p.mul[:] = self._c_multipliers()
        p.matrix[:] = [v for row in self.matrix for v in row]
        return p


XTRANS = ("GBGGRG", "RGRBGB", "GBGGRG", "GRGGBG", "BGBRGR", "GRGGBG")  # the canonical layout; a camera's is one of its 36 cyclic shifts


@_median_keyword
@dataclass(frozen=True)
class XTransProfile(_MosaicProfile):
    """What a RAW file's parser knows of a frame with a 6 x 6 colour filter array (Fujifilm's X-Trans), for the demosaic on the
    device: r2f_demosaic_xtrans_u16 of include/r2f.h -- the project's own interpolation, not LibRaw's (Markesteijn's); parity with
    LibRaw's bytes is unpinned.  A frozen, hashable record (part of the image cache key, like RawProfile).

    pattern: six strings of six letters from "RGB" (the rows of the array at (0, 0)), or one string of 36.  Which patterns are
        admissible is the planner's to say (`plan`): green within 2 samples on both sides of every other site along rows and
        columns, both other colours in every centred 3 x 3.
    black: one level for every site, or 36 per phase ((y % 6) * 6 + x % 6); integers in [0, 65535].
    multipliers: (r, g, b); each in (0, 1024].  They hold the white balance AND the scale to 16 bits.  Or a RawLevels, as
        RawProfile's (a deferred profile).
    matrix: 3 x 3, rows are the output channels; |entries| <= 64.
    orientation: 0 .. 7, LibRaw's sizes.flip bits, as RawProfile's (r2f_demosaic_xtrans_oriented_u16).
    highlight: LibRaw's highlight mode, as RawProfile's (r2f_demosaic_xtrans_blend_u16).
    median_passes (keyword): LibRaw's med_passes, as RawProfile's (r2f_demosaic_xtrans_median_u16).
    half_size=True yields A THIRD of the mosaic's sides (the 3 x 3 cells of the array), not a half: `reduction`."""
    pattern: tuple | str = XTRANS
    black: tuple | float = 0
    multipliers: tuple | RawLevels = (1.0, 1.0, 1.0)
    matrix: tuple = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
    # keyword-only, and stated ahead of `orientation`: the positional order (..., matrix, orientation) and the last field stay as they were
    highlight: str | tuple = field(default="clip", kw_only=True)
    orientation: int = 0

    reduction = 3
    _sites, _multiplier_counts = 36, (3,)
    _c_params, _planner = _lib.XTransParams, "r2f_xtrans_plan"

    def __post_init__(self):
        pattern = self.pattern
        if isinstance(pattern, str):
            pattern = tuple(pattern[i:i + 6] for i in range(0, 36, 6)) if len(pattern) == 36 else (pattern,)
        try:
            pattern = tuple(pattern)
        except TypeError:
            pattern = ()
        if len(pattern) != 6 or not all(isinstance(r, str) and len(r) == 6 and set(r) <= set("RGB") for r in pattern):
            raise ValueError(f"XTransProfile.pattern must be six strings of six letters from 'RGB' (or one of 36), got {self.pattern!r}")
        if set("".join(pattern)) != set("RGB"):
            raise ValueError(f"XTransProfile.pattern must hold each of R, G and B, got {self.pattern!r}")
        object.__setattr__(self, "pattern", pattern)
        self._normalise()

    def to_c(self, half_size: bool = False) -> _lib.XTransProfile:
        p = _lib.XTransProfile(reduced=int(bool(half_size)))
        p.pattern[:] = ["RGB".index(c) for row in self.pattern for c in row]
        p.black[:] = self.black
        p.mul[:] = self._c_multipliers()
        p.matrix[:] = [v for row in self.matrix for v in row]
        return p
