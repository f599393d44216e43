"""The projected lens correction, host half, without a GPU: r2f_lens_plan_projected and the shared arithmetic (r2f_lens_math.h:
projection_factor, the projected source_offset, correct_pixel / correct_pixel_tca) in a stand-alone program under AddressSanitizer /
UBSan (tests/lens_projection_check.cpp), the NumPy model (tests/lens_projection_model.py), LensProfile.projection, the payload of
phase 1 and the ABI structs.

The cases are only worth anything if the projection really moves the coordinates, takes both branches of the stated atan and reaches
every staging route of the kernel, so those conditions are asserted from the model first."""

import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import lens_model as lm
import lens_projection_model as pm
import lens_tca_model as tm
from raw2film_amd import _lib
from raw2film_amd.hip_processor import HipProcessor
from raw2film_amd.lens import LensProfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raw2film_amd", "csrc")
F = np.float32
FISHEYE = pm.PROJECTIONS["fisheye"]
BIG = [s for s in lm.SHAPES if s[0] >= 33 and s[1] >= 47]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("lens_projection_check") / "lens_projection_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
           "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "lens_projection_check.cpp"), os.path.join(CSRC, "r2f_lens_plan.cpp"),
           os.path.join(CSRC, "r2f_plan.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _header_atan_bounds():
    text = open(os.path.join(ROOT, "include", "r2f.h")).read()
    low = re.search(r"largest error of P for t in \[2\^-13, 1\]: ([0-9.]+) ulp", text)
    high = re.search(r"largest error of P for t in \(1, 64\]: ([0-9.]+) ulp", text)
    return float(low.group(1)), float(high.group(1))


def _grid(shape, window=None):
    H, W = shape
    r0, c0, nr, nc = (0, 0, H, W) if window is None else window
    return np.meshgrid(np.arange(r0, r0 + nr), np.arange(c0, c0 + nc), indexing="ij")


# ---- the conditions the cases were chosen for
@pytest.mark.parametrize("shape", [(96, 128), (150, 210)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_fisheye_record_takes_both_branches_of_the_stated_atan(shape):
    prof = pm.profile("none", "fisheye")
    Y, X = _grid(shape)
    *_, t = pm.offsets(lm.rounded(lm.constants(prof, *shape)), pm.record(prof), X, Y, want_factor=True)
    print(f"{shape}: t from {t.min():.4f} to {t.max():.4f}; {(t <= 1).mean():.3f} of the pixels on the first branch")
    assert (t <= 1).any() and (t > 1).any() and t.max() > 1.5
    for scale, least in ((0.25, 6.0),):
        *_, t = pm.offsets(lm.rounded(lm.constants(pm.profile("none", "fisheye", scale=scale), *shape)), pm.record(prof), X, Y, want_factor=True)
        assert t.max() > least


def test_the_factor_is_continuous_across_the_seam_to_the_recorded_bound():
    """P at t = 1 comes from p(1), P just above from the reciprocal branch.  Both lie within their recorded error of atan(t)/t, whose
    own change over one float step at 1 is below a tenth of a unit: the two values differ by no more than the sum of the bounds."""
    low, high = _header_atan_bounds()
    one, above = F(1), np.nextafter(F(1), F(2))
    p0, p1 = pm.factor("fisheye", np.array([one]))[0], pm.factor("fisheye", np.array([above]))[0]
    ulp = 2.0 ** -24  # (of values in [0.5, 1): atan(1) = 0.785)
    step = abs(math.atan(1.0) - math.atan(float(above)) / float(above))
    print(f"P(1) = {p0!r}, P(1+) = {p1!r}: {abs(float(p0) - float(p1)) / ulp:.2f} ulp apart, the exact step is {step / ulp:.3f} ulp")
    assert abs(float(p0) - float(p1)) <= (low + high) * ulp + step
    assert abs(float(p0) - math.atan(1.0)) <= low * ulp and abs(float(p1) - math.atan(float(above)) / float(above)) <= high * ulp


def test_below_two_to_the_minus_13_the_fisheye_factor_is_exactly_one_within_half_a_unit():
    t = np.array([0.0, 1e-30, 2.0 ** -20, np.nextafter(F(2.0 ** -13), F(0))], dtype=F)
    assert (pm.factor("fisheye", t) == F(1)).all()
    assert 1.0 - math.atan(float(t[-1])) / float(t[-1]) < 2.0 ** -25
    for kind in pm.TYPES:
        assert (pm.factor(kind, t[:3]) == F(1)).all(), kind


@pytest.mark.parametrize("shape", BIG, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_projection_moves_the_source_coordinate_by_more_than_a_pixel(shape):
    Y, X = _grid(shape)
    for projection in pm.PROJECTIONS:
        for name in ("none", "ptlens"):
            prof = pm.profile(name, projection)
            c = lm.rounded(lm.constants(prof, *shape))
            ox, oy, _, _ = pm.offsets(c, pm.record(prof), X, Y)
            sx, sy = pm.coords_plain(c, X, Y)
            moved = np.hypot((F(c.cx) + ox) - sx, (F(c.cy) + oy) - sy).max()
            print(f"{projection} {name} {shape}: the coordinate moves by up to {moved:.2f} px")
            assert moved > 1.0, (projection, name, shape, moved)


@pytest.mark.parametrize("shape", lm.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_identity_records_are_the_unprojected_models_bit_for_bit(shape):
    image = lm.frame(*shape)
    for name in ("ptlens", "poly3", "poly5", "none", "off-centre", "vignetting"):
        plain = lm.correct(image, lm.rounded(lm.constants(lm.profile(name), *shape)))
        for kind in pm.TYPES:
            prof = pm.profile(name, (kind, pm.IDENTITY_FOCAL))
            c = lm.rounded(lm.constants(prof, *shape))
            assert np.array_equal(_bits(pm.correct(image, c, pm.record(prof))), _bits(plain)), (name, kind)
        for kind in ("fisheye", "equisolid"):
            prof = pm.profile(name, (kind, pm.IDENTITY_FOCAL), "poly3")
            c, rec = lm.rounded(lm.constants(prof, *shape)), tm.record(prof, F)
            assert np.array_equal(_bits(pm.correct(image, c, pm.record(prof), rec)), _bits(tm.correct_tca(image, c, rec))), (name, kind)


# ---- the float32 map against the float64 evaluation, under a running bound
U = 2.0 ** -24


class Run:
    """A float64 value with a running bound on how far the float32 evaluation of the same operations can lie from it: every
    operation propagates its operands' bounds and adds one unit roundoff of its own result (taken of |value| + bound, so that the
    unit is the float32 result's); a constant the host rounds from double starts with one unit."""

    def __init__(self, val, err=0.0):
        self.val, self.err = np.asarray(val, dtype=np.float64), np.asarray(err, dtype=np.float64)

    @staticmethod
    def const(v):
        return Run(v, U * abs(v))

    def _done(self, val, err):
        return Run(val, err + U * (np.abs(val) + err))

    def __add__(self, o):
        return self._done(self.val + o.val, self.err + o.err)

    def __sub__(self, o):
        return self._done(self.val - o.val, self.err + o.err)

    def __mul__(self, o):
        return self._done(self.val * o.val, np.abs(self.val) * o.err + np.abs(o.val) * self.err + self.err * o.err)

    def __truediv__(self, o):  # (o stays away from 0 by more than its bound in every use below)
        q = self.val / o.val
        return self._done(q, (self.err + np.abs(q) * o.err) / (np.abs(o.val) - o.err))

    def sqrt(self):  # (concave: the lower side deviates further)
        r = np.sqrt(self.val)
        return self._done(r, r - np.sqrt(np.maximum(self.val - self.err, 0.0)))


def _factor_run(kind, t, atan_ulp):
    one, two = Run(1.0), Run(2.0)
    if kind == "fisheye":
        # the exact function at t, moved by t's bound (P falls with t: the ends of [t - e, t + e] bound the move), plus the recorded
        # error of the stated polynomial as a term of its own: atan_ulp units of the last place, each at most 2^-23 of the value
        P = pm.factor(kind, t.val, np.float64)
        lo, hi = pm.factor(kind, np.maximum(t.val - t.err, 0.0), np.float64), pm.factor(kind, t.val + t.err, np.float64)
        return Run(P, np.maximum(np.abs(lo - P), np.abs(hi - P)) + atan_ulp * 2.0 ** -23 * P)
    s = (one + t * t).sqrt()
    if kind == "orthographic":
        return one / s
    if kind == "stereographic":
        return two / (one + s)
    return one / (s * ((s + one) / (two * s)).sqrt())


def _coords_run(c, kind, focal, X, Y, atan_ulp):
    """(sx, sy) of the projected map as Run values: the float64 evaluation with unrounded constants, and its running bound."""
    cx, cy, q, inv_scale = Run.const(c.cx), Run.const(c.cy), Run.const(c.q), Run.const(c.inv_scale)
    k = [Run.const(v) for v in c.k]
    dx, dy = Run(X.astype(np.float64)) - cx, Run(Y.astype(np.float64)) - cy
    u, v = dx * q, dy * q
    t = (u * u + v * v).sqrt() * Run.const(1.0 / focal)
    P = _factor_run(kind, t, atan_ulp)
    up, vp = u * P, v * P
    r2 = up * up + vp * vp
    if c.model == 1:
        f = Run.const(c.c0) + k[0] * r2
    elif c.model == 2:
        f = Run(1.0) + r2 * (k[0] + k[1] * r2)
    elif c.model == 3:
        r = r2.sqrt()
        f = Run.const(c.c0) + r * (k[2] + r * (k[1] + r * k[0]))
    else:
        f = Run(np.ones_like(r2.val))
    g = (f * P) * inv_scale
    return cx + dx * g, cy + dy * g


@pytest.mark.parametrize("shape", BIG, ids=lambda s: f"{s[0]}x{s[1]}")
def test_float32_map_against_the_float64_evaluation(shape):
    """The float32 source coordinate lies within the running bound of the float64 evaluation with unrounded constants: one unit
    roundoff per operation on the path, the recorded error of the stated atan as its own term (the larger of the two ranges'
    figures in include/r2f.h).  No fixed pixel figure: the bound is printed beside the error it holds."""
    atan_ulp = max(_header_atan_bounds())
    Y, X = _grid(shape)
    for projection, (kind, focal) in pm.PROJECTIONS.items():
        for name, changes in (("none", {}), ("ptlens", {}), ("poly5", {}), ("off-centre", {}), ("vignetting", {}), ("none", dict(scale=0.25))):
            if changes and kind != "fisheye":
                continue
            prof = pm.profile(name, projection, **changes)
            c64 = lm.constants(prof, *shape)
            ox, oy, _, _ = pm.offsets(lm.rounded(c64), pm.record(prof), X, Y)
            sx32, sy32 = (F(c64.cx) + ox).astype(np.float64), (F(c64.cy) + oy).astype(np.float64)
            sx, sy = _coords_run(c64, kind, focal, X, Y, atan_ulp)
            # the Run values are the float64 evaluation: the model's own float64 path gives the same coordinates
            ox64, oy64, _, _ = pm.offsets(c64, pm.record(prof, np.float64), X, Y, np.float64)
            assert np.allclose(c64.cx + ox64, sx.val, rtol=0, atol=1e-9) and np.allclose(c64.cy + oy64, sy.val, rtol=0, atol=1e-9)
            ex, ey = np.abs(sx32 - sx.val), np.abs(sy32 - sy.val)
            print(f"{projection} {name} {changes} {shape}: error up to {max(ex.max(), ey.max()):.3e} px under a bound of up to "
                  f"{max(sx.err.max(), sy.err.max()):.3e} px; largest error / bound {max((ex / sx.err).max(), (ey / sy.err).max()):.3f}")
            assert bool((ex <= sx.err).all() and (ey <= sy.err).all()), (projection, name, shape)


# ---- the CPU program
@pytest.mark.parametrize("seed", [1, 2, 20261020])
def test_planner_and_decision_are_clean_under_the_sanitizers(check, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([check, "fuzz", str(seed), "20000"], capture_output=True, text=True, env=env, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    assert "cases ok" in res.stdout


def test_the_stated_atan_stays_within_the_error_recorded_in_the_header(check):
    """Every float32 t in [2^-13, 1] and in (1, 64] through the shared arithmetic's fisheye factor, against atan in double."""
    res = subprocess.run([check, "atan"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    m = re.search(r"atan max ulp: low ([0-9.]+) high ([0-9.]+)", res.stdout)
    assert m, res.stdout
    low, high = _header_atan_bounds()
    print(f"measured {m.group(1)} / {m.group(2)} ulp; include/r2f.h records {low} / {high}")
    assert float(m.group(1)) <= low and float(m.group(2)) <= high
    assert low < 2.0 and high < 4.0  # (the record itself is not a blank cheque: the fit reached this)


def _render(binary, tmp_path, image, profile, window=None):
    H, W, C = image.shape
    r0, c0, nr, nc = (0, 0, H, W) if window is None else window
    job, out = str(tmp_path / "job.bin"), str(tmp_path / "out.bin")
    tca = profile.to_c_tca()
    with open(job, "wb") as f:
        f.write(np.array([H, W, C, r0, c0, nr, nc, int(tca is not None)], dtype=np.int32).tobytes())
        f.write(bytes(profile.to_c()))
        f.write(bytes(profile.to_c_projection()))
        f.write(bytes(tca if tca is not None else _lib.LensTca()))
        f.write(np.ascontiguousarray(image, dtype=np.float32).tobytes())
    res = subprocess.run([binary, "render", job, out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    raw = open(out, "rb").read()
    n0, n1, n2 = ctypes.sizeof(_lib.LensParams), ctypes.sizeof(_lib.LensProjectionParams), ctypes.sizeof(_lib.LensTcaParams)
    params = _lib.LensParams.from_buffer_copy(raw[:n0])
    proj = _lib.LensProjectionParams.from_buffer_copy(raw[n0:n0 + n1])
    return params, proj, np.frombuffer(raw[n0 + n1 + n2:], dtype=np.float32).reshape(nr, nc, 3)


RENDER_NAMES = ("ptlens", "poly5", "off-centre", "vignetting")


@pytest.mark.parametrize("shape", lm.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shared_arithmetic_renders_the_model_bit_for_bit(check, tmp_path, shape):
    H, W = shape
    cases = [(name, projection, tca, {}) for name in RENDER_NAMES for projection in pm.PROJECTIONS for tca in (None, "poly3")]
    cases += [("none", "fisheye", tca, dict(scale=0.25)) for tca in (None, "linear")]
    if min(shape) > 1:
        cases += [("none", "fisheye", tca, dict(scale="auto")) for tca in (None, "poly3")]
    for name, projection, tca, changes in cases:
        prof = pm.profile(name, projection, tca, **changes)
        image = lm.frame(H, W)
        if name == "poly5":  # (a fourth channel is ignored)
            image = np.concatenate([image, np.full((H, W, 1), 7.0, F)], -1)
        params, proj, got = _render(check, tmp_path, image, prof)
        scale = params.scale if changes.get("scale") == "auto" else None
        want_c, have_c = lm.rounded(lm.constants(prof, H, W, scale)), lm.from_params(params)
        for field in ("cx", "cy", "q", "inv_scale", "c0", "qv"):
            assert _bits(getattr(want_c, field)) == _bits(getattr(have_c, field)), (name, field)
        assert pm.from_params(proj)[0] == prof.projection[0] and _bits(pm.from_params(proj)[1]) == _bits(pm.record(prof)[1])
        want = pm.model(name, projection, tca, shape, **changes)
        assert np.array_equal(_bits(got), _bits(want)), (name, projection, tca, changes, shape, int((_bits(got) != _bits(want)).sum()))
    # a window that straddles every edge, and one wholly outside the frame
    image = lm.frame(H, W)
    for projection, tca in (("fisheye", None), ("stereographic", "edge")):
        prof = pm.profile("off-centre", projection, tca)
        for window in ((-5, -6, H + 11, W + 9), (H + 40, -W - 50, 5, 7)):
            _, _, got = _render(check, tmp_path, image, prof, window)
            assert np.array_equal(_bits(got), _bits(pm.model("off-centre", projection, tca, shape, window))), (projection, tca, window)


# ---- auto scale
# (a one-pixel-wide frame is no case here: the fisheye record's image circle ends exactly at such a frame's ends, so no finite scale
# puts a probe on them, and the planner refuses it like a circular fisheye)
AUTO_SHAPES = ((33, 47), (150, 210), (4000, 6000), (7, 9))


@pytest.mark.parametrize("shape", AUTO_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_auto_scale_puts_every_probe_of_every_channel_on_or_inside_the_boundary(shape):
    """At the resolved scale every probe of every channel lands inside to 1e-9 px (the model restates the planner's double
    arithmetic; 1e-9 px is what two such restatements may differ by).  One ulp of scale lower the furthest probe is no longer
    inside by that measure, and a millionth lower it is outside outright."""
    H, W = shape
    for name in ("none", "ptlens", "off-centre"):
        for tca in (None, "linear", "poly3"):
            prof = pm.profile(name, "fisheye", tca, scale="auto")
            params, proj, tca_params = prof.plan_projected(H, W)
            scale = params.scale
            assert 1 / 16 < scale < 16 and (tca_params is None) == (tca is None)
            assert pm.probes_reach(prof, H, W, scale) <= 1e-9
            assert pm.probes_reach(prof, H, W, np.nextafter(scale, 0.0)) > -1e-9
            assert pm.probes_reach(prof, H, W, scale * (1 - 1e-6)) > 0
            if tca is not None:
                assert scale >= pm.profile(name, "fisheye", scale="auto").plan_projected(H, W)[0].scale  # (green alone needs no more)
            want, have = lm.rounded(lm.constants(prof, H, W, scale)), lm.from_params(params)
            assert (_bits(want.q), _bits(want.inv_scale)) == (_bits(have.q), _bits(have.inv_scale))


def test_auto_scale_of_the_full_frame_fisheye_is_decided_by_the_long_edges():
    """A 180-degree-diagonal fisheye (focal 2/pi) on a 3:2 frame: about 0.70 -- well below 1, which is what sends the centre tiles'
    boxes past the size a block stages whole."""
    scale = LensProfile(scale="auto", projection=FISHEYE).plan_projected(2001, 3001)[0].scale
    print(f"auto scale of the fisheye record on 2001 x 3001: {scale:.4f}")
    assert 0.65 < scale < 0.75
    r = (2000 / 2) / (math.hypot(2000, 3000) / 2)  # a long edge's midpoint, in units of the normalisation radius
    assert abs(FISHEYE[1] * math.atan(r / scale / FISHEYE[1]) - r) < 1e-6  # it lands on the boundary: r_source = focal * atan(r / focal)


def test_auto_scale_of_an_identity_record_is_the_plain_one_to_the_bit():
    for kind in pm.TYPES:
        for name in ("ptlens", "poly3", "poly5", "off-centre"):
            for H, W in ((33, 47), (150, 210), (4000, 6000)):
                prof = pm.profile(name, (kind, pm.IDENTITY_FOCAL), scale="auto")
                assert bytes(prof.plan_projected(H, W)[0]) == bytes(prof.plan(H, W)), (kind, name, H, W)
                prof = pm.profile(name, (kind, pm.IDENTITY_FOCAL), "poly3", scale="auto")
                assert bytes(prof.plan_projected(H, W)[0]) == bytes(prof.plan_tca(H, W)[0]), (kind, name, H, W)


def test_without_auto_scale_the_params_are_the_plain_planners_byte_for_byte():
    for name in lm.PROFILE_SPECS:
        for projection in pm.PROJECTIONS:
            for tca in (None, "linear", "poly3"):
                prof = pm.profile(name, projection, tca)
                params, proj, tca_params = prof.plan_projected(150, 210)
                assert bytes(params) == bytes(lm.profile(name).plan(150, 210))
                assert proj.type == pm.TYPES[projection] and _bits(proj.inv_focal) == _bits(F(1.0 / pm.PROJECTIONS[projection][1]))
                if tca is not None:
                    assert bytes(tca_params) == bytes(prof.plan_tca(150, 210)[1])


def test_a_circular_fisheye_is_refused_by_the_auto_scale():
    with pytest.raises(ValueError, match="r2f_lens_plan_projected"):
        LensProfile(scale="auto", projection=("fisheye", 0.2)).plan_projected(96, 128)
    LensProfile(scale=1.0, projection=("fisheye", 0.2)).plan_projected(96, 128)  # (with a scale given it is planned like any other)
    assert LensProfile(scale="auto", projection=FISHEYE).plan_projected(1, 1)[0].scale == 1.0


# ---- the kernel's staging routes
def _routes(prof, shape, scale=None):
    tca = None if prof.tca is None else tm.record(prof, F)
    return pm.tile_routes(lm.rounded(lm.constants(prof, *shape, scale)), pm.record(prof), tca, *shape)


def test_which_tiles_take_which_staging_route():
    """150 x 210 is 10 x 4 tiles of 64 x 16.  A tile's taps span 63 / scale + 8 by 15 / scale + 8 texels in the magnified middle:
      - at the fisheye record's auto scale (0.706) that is 98 x 30 = 2940 of the 3072 texels a box holds: every tile still stages
        whole (the estimate of 102 x 33 that started this work counted 64 and 16 steps and a scale of 0.70);
      - at the equisolid record's auto scale (0.52) the middle tiles no longer fit and take the two-halves route, while the border
        tiles' boxes shrink and stay whole; nothing there has to gather;
      - at scale 0.25 a half's box does not fit either: the gather route.
    Every route the kernel has is reached by a case the GPU tests render on this shape."""
    shape = (150, 210)
    seen = {}
    for projection, tca in (("fisheye", None), ("fisheye", "poly3"), ("equisolid", None), ("equisolid", "poly3")):
        prof = pm.profile("none", projection, tca, scale="auto")
        scale = prof.plan_projected(*shape)[0].scale
        routes = _routes(prof, shape, scale)
        assert len(routes) == 40
        seen[projection, tca] = routes
        print(projection, tca, f"{scale:.4f}", {k: sum(k in p for _, _, p in routes) for k in pm.ROUTES})
        assert all(p == ("whole",) for ty, tx, p in routes if tx == 3)  # (the last column is 18 pixels wide)
    for tca in (None, "poly3"):
        assert {r for _, _, p in seen["fisheye", tca] for r in p} == {"whole"}
        assert {r for _, _, p in seen["equisolid", tca] for r in p} == {"whole", "halves"}
        middle = [p for ty, tx, p in seen["equisolid", tca] if ty in (4, 5) and tx == 1]  # (the tiles that hold the centre)
        assert len(middle) == 2 and all(p == ("halves", "halves") for p in middle)
    quarter = _routes(pm.profile("none", "fisheye", scale=0.25), shape)
    assert any(p == ("gather", "gather") for _, _, p in quarter)
    assert {r for rs in list(seen.values()) + [quarter] for _, _, p in rs for r in p} == set(pm.ROUTES)


# ---- LensProfile
def test_profile_with_a_projection_is_frozen_hashable_and_normalised():
    a = LensProfile("ptlens", [0.02, -0.06, 0.01], projection=["fisheye", 1])
    b = LensProfile("ptlens", (0.02, -0.06, 0.01), projection=("fisheye", 1.0))
    assert a.projection == ("fisheye", 1.0) and type(a.projection[1]) is float and type(a.projection) is tuple
    assert a == b and hash(a) == hash(b) and {a: 1}[b] == 1
    assert a != LensProfile("ptlens", (0.02, -0.06, 0.01), projection=("fisheye", 1.5))
    assert a != LensProfile("ptlens", (0.02, -0.06, 0.01), projection=("equisolid", 1.0))
    assert a != LensProfile("ptlens", (0.02, -0.06, 0.01))
    with pytest.raises(Exception):
        a.projection = None
    plain = LensProfile(tca=("linear", (1.03, 0.97)))
    assert plain.projection is None and plain.to_c_projection() is None
    params, proj, tca = plain.plan_projected(40, 60)
    assert proj is None and bytes(params) == bytes(plain.plan_tca(40, 60)[0]) and bytes(tca) == bytes(plain.plan_tca(40, 60)[1])
    assert LensProfile().plan_projected(40, 60)[1:] == (None, None)
    import inspect

    assert list(inspect.signature(LensProfile).parameters)[-1] == "projection"  # the constructor's last parameter


@pytest.mark.parametrize("projection", [
    ("thoby", 1.0), ("rectilinear", 1.0), ("panoramic", 1.0), (1, 1.0), ("fisheye",), "fisheye", 1.0, ("fisheye", 1.0, 2.0),
    ("fisheye", 0.0), ("fisheye", -1.0), ("fisheye", float("nan")), ("fisheye", float("inf")), ("fisheye", "wide"), ("fisheye", None),
    ("fisheye", (1.0, 2.0)),
])
def test_projection_validation_raises_before_any_work(projection):
    with pytest.raises(ValueError):
        LensProfile(projection=projection)


def test_to_c_projection_and_the_planners_refusals():
    p = LensProfile(projection=("equisolid", 0.55)).to_c_projection()
    assert (p.type, p.focal) == (_lib.PROJ_EQUISOLID, 0.55)
    assert [LensProfile(projection=(k, 1.0)).to_c_projection().type for k in ("fisheye", "stereographic", "equisolid", "orthographic")] == [1, 2, 3, 4]
    lib = _lib.load()
    out, out_proj, out_tca = _lib.LensParams(), _lib.LensProjectionParams(), _lib.LensTcaParams()
    prof = LensProfile("poly5", (0.03, -0.01)).to_c()
    tca = LensProfile(tca=("linear", (1.0, 1.0))).to_c_tca()

    def plan(type=1, focal=0.6, profile=prof, with_tca=False):
        proj = _lib.LensProjection(type=type, focal=focal)
        return lib.r2f_lens_plan_projected(ctypes.byref(profile), ctypes.byref(proj), ctypes.byref(tca) if with_tca else None, 40, 60,
                                           ctypes.byref(out), ctypes.byref(out_proj), ctypes.byref(out_tca) if with_tca else None)

    assert plan() == _lib.OK and (out_proj.type, _bits(out_proj.inv_focal)) == (1, _bits(F(1 / 0.6)))
    assert plan(with_tca=True) == _lib.OK and out_tca.model == _lib.TCA_LINEAR
    nan, inf = float("nan"), float("inf")
    for bad in (dict(type=0), dict(type=5), dict(type=-1), dict(focal=0.0), dict(focal=-0.6), dict(focal=nan), dict(focal=inf),
                dict(focal=1e-39), dict(focal=5e-324)):
        assert plan(**bad) == _lib.EINVAL, bad
    assert plan(focal=1e300) == _lib.OK and out_proj.inv_focal == 0.0  # (its reciprocal fits a float: 0, the identity)
    bad_profile = LensProfile().to_c()
    bad_profile.scale = -1.0
    assert plan(profile=bad_profile) == _lib.EINVAL
    tca.model = _lib.TCA_NONE
    assert plan(with_tca=True) == _lib.EINVAL


# ---- ABI
def test_struct_layouts_match_the_header():
    P, R = _lib.LensProjection, _lib.LensProjectionParams
    assert ctypes.sizeof(P) == 16 and [getattr(P, f).offset for f in ("type", "focal")] == [0, 8]
    assert ctypes.sizeof(R) == 8 and [getattr(R, f).offset for f in ("type", "inv_focal")] == [0, 4]
    assert (ctypes.sizeof(_lib.LensProfile), ctypes.sizeof(_lib.LensParams), ctypes.sizeof(_lib.LensTca), ctypes.sizeof(_lib.LensTcaParams)) \
        == (96, 64, 56, 28)
    text = open(os.path.join(ROOT, "include", "r2f.h")).read()
    body = text[text.index("typedef struct r2f_lens_projection {"):text.index("} r2f_lens_projection;")]
    order = [body.index(w) for w in ("int32_t type;", "double focal;")]
    assert order == sorted(order)
    body = text[text.index("typedef struct r2f_lens_projection_params {"):text.index("} r2f_lens_projection_params;")]
    order = [body.index(w) for w in ("int32_t type;", "float inv_focal;")]
    assert order == sorted(order)
    enum = text[text.index("R2F_PROJ_NONE = 0"):]
    enum = enum[:enum.index("}")]
    assert re.sub(r"\s+", " ", enum).strip() == ("R2F_PROJ_NONE = 0, R2F_PROJ_FISHEYE = 1, R2F_PROJ_STEREOGRAPHIC = 2, R2F_PROJ_EQUISOLID = 3, "
                                                  "R2F_PROJ_ORTHOGRAPHIC = 4")
    assert (_lib.PROJ_NONE, _lib.PROJ_FISHEYE, _lib.PROJ_STEREOGRAPHIC, _lib.PROJ_EQUISOLID, _lib.PROJ_ORTHOGRAPHIC) == (0, 1, 2, 3, 4)
    # the stated coefficients are the model's and the shared arithmetic's
    for h in ("0x1p+0f", "-0x1.55554p-2f", "0x1.999278p-3f", "-0x1.242702p-3f", "0x1.c0d2e2p-4f", "-0x1.58dd68p-4f", "0x1.dd11b4p-5f",
              "-0x1.01b21p-5f", "0x1.6a946ap-7f", "-0x1.df068p-10f", "0x1.921fb6p+0f"):
        assert h in text and h in open(os.path.join(CSRC, "r2f_lens_math.h")).read(), h
    assert [float(x).hex() for x in pm.ATAN_COEF][0] == "0x1.0000000000000p+0"


# ---- phase 1 of the processor
@pytest.fixture
def proc():
    p = HipProcessor.__new__(HipProcessor)
    p.cameras = p.lenses = None
    p.payload_alpha = True
    return p


BASE = dict(distortion="ptlens", coefficients=(0.02, -0.06, 0.01), vignetting=(-0.3, 0.1, -0.02), scale=0.8)
PLAIN = LensProfile(**BASE)
PROJECTED = LensProfile(**BASE, projection=FISHEYE)
PROJECTED_TCA = LensProfile(**BASE, projection=FISHEYE, tca=tm.TCA_SPECS["poly3"])
CROP_KEYS = ("final_resolution", "output_resolution", "canvas_resolution", "pipeline_resolution", "resize_to", "upscale_to", "chroma_nr",
             "u16_factor", "u16_window", "warp")


@pytest.mark.parametrize("kw", [
    dict(), dict(zoom=1.3, rotate_times=1), dict(rotation=3.5, zoom=1.3, rotate_times=1), dict(flip=True, frame_width=36, frame_height=36),
    dict(resolution=(60, 90), canvas_mode="Uniform white", canvas_scale=1.1), dict(rotate_times=3, max_scale=2.0),
])
def test_payload_has_the_projection_key_exactly_with_a_projected_profile(proc, kw):
    img = lm.frame(150, 210)
    plain = proc.extract_image_data_cpu(img, lens_correction=True, lens_profile=PLAIN, **kw)
    pay = proc.extract_image_data_cpu(img, lens_correction=True, lens_profile=PROJECTED, **kw)
    both = proc.extract_image_data_cpu(img, lens_correction=True, lens_profile=PROJECTED_TCA, **kw)
    assert set(pay) == set(plain) == set(both)
    assert set(plain["lens"]) == {"params", "window", "rotate_times"}
    assert set(pay["lens"]) == set(plain["lens"]) | {"projection"} and set(both["lens"]) == set(plain["lens"]) | {"projection", "tca"}
    for p in (pay, both):
        assert isinstance(p["lens"]["projection"], _lib.LensProjectionParams) and pm.from_params(p["lens"]["projection"])[0] == "fisheye"
        assert bytes(p["lens"]["params"]) == bytes(plain["lens"]["params"])
        assert (p["lens"]["window"], p["lens"]["rotate_times"]) == (plain["lens"]["window"], plain["lens"]["rotate_times"])
        assert np.array_equal(p["image_array"], plain["image_array"])
        for k in CROP_KEYS:
            a, b = p[k], plain[k]
            if isinstance(a, dict):
                assert set(a) == set(b) and all(np.array_equal(a[f], b[f]) for f in a), k
            else:
                assert a == b, k
    off = proc.extract_image_data_cpu(img, lens_correction=False, lens_profile=PROJECTED, **kw)
    assert "lens" not in off and set(off) == set(proc.extract_image_data_cpu(img, lens_correction=False, **kw))


def test_uint16_payload_with_a_projection(proc):
    u16 = np.random.default_rng(3).integers(0, 65535, (150, 210, 3), dtype=np.uint16)
    for kw in (dict(exposure=0.5), dict(exposure="device", metadata=None)):
        plain = proc.extract_image_data_cpu(u16, lens_correction=True, lens_profile=PLAIN, zoom=1.3, **kw)
        pay = proc.extract_image_data_cpu(u16, lens_correction=True, lens_profile=PROJECTED, zoom=1.3, **kw)
        assert "projection" in pay["lens"] and "projection" not in plain["lens"] and "tca" not in pay["lens"]
        assert (pay["u16_factor"], pay["u16_window"], pay["lens"]["window"]) == (plain["u16_factor"], plain["u16_window"], plain["lens"]["window"])


def test_a_changed_projection_invalidates_the_image_cache_and_an_equal_one_does_not(proc):
    uploads = []

    def prepare(payload):
        uploads.append(payload.get("lens"))
        proc._texture = ("frame", None, {})
        proc.image_param_dict = None

    proc.prepare_gpu_textures = prepare
    img = lm.frame(40, 60)
    proc.load_image_texture(img, lens_profile=LensProfile("ptlens", (0.02, -0.06, 0.01), projection=("fisheye", 0.7)))
    proc.load_image_texture(img, lens_profile=LensProfile("ptlens", [0.02, -0.06, 0.01], projection=["fisheye", 0.7]))  # equal: the frame stays
    assert len(uploads) == 1 and "projection" in uploads[0]
    proc.load_image_texture(img, lens_profile=LensProfile("ptlens", (0.02, -0.06, 0.01), projection=("fisheye", 0.8)))
    assert len(uploads) == 2 and "projection" in uploads[1]
    proc.load_image_texture(img, lens_profile=LensProfile("ptlens", (0.02, -0.06, 0.01), projection=("stereographic", 0.8)))
    assert len(uploads) == 3
    proc.load_image_texture(img, lens_profile=LensProfile("ptlens", (0.02, -0.06, 0.01)))
    assert len(uploads) == 4 and "projection" not in uploads[3]
    proc.load_image_texture(img, lens_profile=LensProfile("ptlens", (0.02, -0.06, 0.01)))
    assert len(uploads) == 4


def test_a_projected_payload_is_still_refused_by_the_stream_with_the_lens_steps_words(proc):
    from raw2film_amd.payload import stream_rejection

    pay = proc.extract_image_data_cpu(lm.frame(40, 60), lens_profile=PROJECTED)
    plain = proc.extract_image_data_cpu(lm.frame(40, 60), lens_profile=PLAIN)
    why = stream_rejection(pay, (4096, 4096, 4), "torch.float32", False, "gpu")
    assert why is not None and "lens" in why and why == stream_rejection(plain, (4096, 4096, 4), "torch.float32", False, "gpu")
