"""The simulated camera and lens (tests/camera_sim.py) on the project's NumPy models, no GPU: every check reproduces
tests/golden/camera_sim.json, the correct reading passes its threshold and every named misreading fails it -- the proof that the
checks of tests/test_gpu_camera_sim.py discriminate --, the 20 dB condition holds, and the simulator is checked against itself."""

import importlib.util
import json
import math
import os
import re

import numpy as np
import pytest

import camera_sim as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("make_camera_sim", os.path.join(ROOT, "tools", "make_camera_sim.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


mk = _tool()
with open(mk.GOLDEN) as _f:
    GOLDEN = json.load(_f)
_RECORDS = {}


def record(name):
    """A check's entry as the tool makes it from the models today, computed once."""
    if name not in _RECORDS:
        _RECORDS[name] = mk.record(name)
    return _RECORDS[name]


def _numbers(entry, path=""):
    for k, v in entry.items():
        if isinstance(v, dict):
            yield from _numbers(v, f"{path}{k}/")
        else:
            yield f"{path}{k}", v


# ---------------------------------------------------------------------------------------------------------------- the file
def test_the_file_lists_the_checks_and_holds_numbers_and_names_only():
    assert list(GOLDEN["checks"]) == sorted(cs.CHECKS) and set(GOLDEN) == {"comment", "notes", "checks"}
    assert all(isinstance(v, str) for v in GOLDEN["notes"].values())
    for name, entry in GOLDEN["checks"].items():
        for key, value in _numbers(entry):
            assert isinstance(value, (int, float)) and not isinstance(value, bool) and math.isfinite(value), (name, key)
            assert re.fullmatch(r"[A-Za-z0-9_/]+", key), (name, key)


@pytest.mark.parametrize("name", sorted(cs.CHECKS))
def test_the_models_reproduce_the_file(name):
    """Within the rounding of the file's six digits (and of another NumPy's last bits)."""
    got, want = dict(_numbers(record(name))), dict(_numbers(GOLDEN["checks"][name]))
    assert got.keys() == want.keys()
    for key in want:
        if key == "lens_inverse_residual_px":  # (a residual at the floor of float64: only its bound is asserted, below)
            continue
        assert got[key] == pytest.approx(want[key], rel=1e-4, abs=1e-9), key


THRESHOLDED = sorted(n for n, e in GOLDEN["checks"].items() if "threshold" in e)


@pytest.mark.parametrize("name", THRESHOLDED)
def test_the_correct_reading_passes_and_every_misreading_fails(name):
    entry, threshold = record(name), GOLDEN["checks"][name]["threshold"]
    names = [r.name for r in cs.case(name).readings if r.name not in ("correct", "noisy")]
    assert list(entry["misreadings"]) == names and names  # (none dropped)
    assert entry["correct"] < threshold
    for wrong, err in entry["misreadings"].items():
        assert err > threshold, wrong
    # the threshold is the tool's: the geometric mean of the correct error and the smallest misreading's
    assert threshold == pytest.approx(math.sqrt(entry["correct"] * min(entry["misreadings"].values())), rel=1e-4)


def test_every_misreading_lies_20_db_above_the_correct_reading_or_has_its_note():
    assert mk.violations(GOLDEN) == []
    assert mk.violations({**GOLDEN, "checks": {n: record(n) for n in THRESHOLDED}}) == []
    below = {f"{n}/{w}" for n in THRESHOLDED for w, err in GOLDEN["checks"][n]["misreadings"].items()
             if cs.decibels(err / GOLDEN["checks"][n]["correct"]) < mk.MIN_GAP_DB}
    assert below == set(GOLDEN["notes"]) == set(mk.NOTES)  # (no note without its misreading)
    assert all(cs.decibels(err / e["correct"]) >= mk.FLOOR_GAP_DB for e in map(GOLDEN["checks"].get, THRESHOLDED) for err in e["misreadings"].values())


def test_the_tool_refuses_a_gap_without_a_note_and_any_below_the_floor():
    entry = {"correct": 1.0, "misreadings": {"near": 5.0, "far": 100.0}}
    assert len(mk.violations({"notes": {}, "checks": {"x": entry}})) == 1
    assert mk.violations({"notes": {"x/near": "why"}, "checks": {"x": entry}}) == []
    assert len(mk.violations({"notes": {"x/near": "why"}, "checks": {"x": {"correct": 1.0, "misreadings": {"near": 3.0}}}})) == 1


def test_every_misreading_the_oracle_was_built_for_is_named():
    have = {w for n in THRESHOLDED for w in GOLDEN["checks"][n]["misreadings"]}
    want = {"pattern_RGGB", "pattern_BGGR", "pattern_GRBG", "shifted_one_row", "shifted_one_column", "transposed", "multipliers_reversed",
            "greens_swapped_with_red", "matrix_transposed", "black_rotated_one_site", *(f"orientation_{o}" for o in range(8)),
            "centres_at_cell_origin", "red_and_blue_swapped", "reciprocal", "coefficients_negated", "center_negated", "inverse_direction",
            "as_fisheye", "as_stereographic", "as_equisolid", "as_orthographic", "maximum_is_white_level", "nominal_white_kept",
            "without_shift", "not_repaired"}
    assert want <= have
    for o in range(8):  # each orientation against the seven others
        assert set(GOLDEN["checks"][f"orientation_{o}"]["misreadings"]) == {f"orientation_{q}" for q in range(8) if q != o}


def test_the_figures_of_merit_hold_on_the_models():
    patch = record("blend_patch")["figures"]
    assert patch["blend"] < patch["clip"]  # Blend lowers the error inside the saturated patch
    noise = record("median_noise")["figures"]
    assert noise["passes_1"] <= noise["passes_0"] and noise["passes_4"] <= noise["passes_0"]  # the colour-difference error does not grow
    dn = record("denoise")
    assert dn["correct"] < dn["noisy"] and abs(dn["bias"]) < GOLDEN["checks"]["denoise"]["bias_bound"]
    for name in ("repair_bayer", "repair_xtrans"):
        assert set(record(name)["misreadings"]) == {"not_repaired"}


# ---------------------------------------------------------------------------------------------------------------- the simulator
def test_the_simulator_owes_nothing_to_the_models():
    with open(cs.__file__) as f:
        imports = [line for line in f if re.match(r"\s*(import|from)\s", line)]
    assert imports and not any(re.search(r"_model|oracle|_lib|torch|pytest|prepath", line) for line in imports), imports


def test_the_scene_differs_between_channels_and_has_no_symmetry():
    s = cs.Scene()
    Y, X = cs.grid((98, 150))
    v = s(Y, X)
    assert 0.08 < v.min() and v.max() < 0.62
    rms = lambda a, b: float(np.sqrt(np.mean((a - b) ** 2)))  # noqa: E731
    floor = 0.02  # (the largest threshold of a check that leans on this is 0.03; every distance below is above it)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert rms(v[..., a], v[..., b]) > floor
    assert rms(v, v[::-1]) > floor and rms(v, v[:, ::-1]) > floor and rms(v, v[::-1, ::-1]) > floor
    sq = v[:98, :98]
    assert rms(sq, sq.transpose(1, 0, 2)) > floor and rms(sq, sq[::-1, ::-1].transpose(1, 0, 2)) > floor
    for dy, dx in ((1, 0), (0, 1), (2, 0), (0, 2), (1, 1)):
        assert rms(v, s(Y + dy, X + dx)) > 0.005, (dy, dx)  # (a sample's shift: above the demosaic checks' correct error)


def test_a_grey_scene_exposes_to_equal_white_balanced_sites():
    black = cs.BLACK
    for pattern in ("GBRG", cs.xtrans_shifted(1, 2)):
        table = black if isinstance(pattern, str) else cs.BLACK36
        mosaic = cs.expose(cs.Grey(0.4), (24, 36), pattern, table, cs.WB, cs.WHITE, cs.IDENTITY)
        ids = cs.colour_ids(cs.cfa_of(pattern), mosaic.shape)
        balanced = (mosaic - cs.per_site(table, mosaic.shape)) * np.asarray(cs.WB)[ids] / min(cs.WB)
        want = 0.4 * (cs.WHITE - min(table))
        assert np.abs(balanced - want).max() <= max(cs.WB) / min(cs.WB) * 0.5 + 1e-9  # (half a unit of the rounding, times the largest factor)
    # a camera matrix whose rows sum to 1 keeps grey grey
    rows = np.asarray(cs.MATRIX).sum(1)
    assert np.allclose(rows, 1.0)
    numeric = cs.numeric_multipliers("GBRG", cs.WB, cs.WHITE, black, cs.SITE_GAIN)
    mosaic = cs.expose(cs.Grey(0.4), (24, 36), "GBRG", black, cs.WB, cs.WHITE, cs.MATRIX, site_gain=cs.SITE_GAIN)
    scaled = (mosaic - cs.per_site(black, mosaic.shape)) * cs.per_site(numeric, mosaic.shape) / 65535.0
    assert np.abs(scaled - 0.4).max() < 1e-3


def test_orientation_0_is_the_identity_and_the_eight_are_distinct_motions():
    ys, xs = cs.grid((5, 7))
    Y, X = cs.upright_coords((5, 7), 0, ys, xs)
    assert np.array_equal(Y, ys) and np.array_equal(X, xs) and cs.upright_shape((5, 7), 0) == (5, 7)
    scene = cs.Scene()
    a = cs.expose(scene, cs.BAYER_SHAPE, "GBRG", cs.BLACK, cs.WB, cs.WHITE, cs.MATRIX)
    assert np.array_equal(a, cs.expose(scene, cs.BAYER_SHAPE, "GBRG", cs.BLACK, cs.WB, cs.WHITE, cs.MATRIX, orientation=0))
    seen = set()
    for o in range(8):
        Y, X = cs.upright_coords((5, 7), o, ys, xs)
        h, w = cs.upright_shape((5, 7), o)
        assert (h, w) == ((7, 5) if o & 4 else (5, 7))
        assert sorted(zip(Y.ravel(), X.ravel())) == [(y, x) for y in range(h) for x in range(w)]  # a bijection onto the upright frame
        seen.add(tuple(zip(Y.ravel(), X.ravel())))
    assert len(seen) == 8
    # the wording of the docstrings: 3 a half turn, 5 a quarter turn counter-clockwise, 6 a quarter turn clockwise -- of the sensor's
    # frame into the upright one.  The sensor's top-left sample: under 5 it lands bottom-left, under 6 top-right.
    assert [tuple(int(v) for v in np.ravel(cs.upright_coords((5, 7), o, 0, 0))) for o in (3, 5, 6)] == [(4, 6), (6, 0), (0, 4)]


@pytest.mark.parametrize("name", sorted(cs.LENS_PROFILES))
def test_the_lens_inverse_meets_its_residual(name):
    profile = cs.LENS_PROFILES[name]
    lens = cs.Lens(profile, *cs.LENS_SHAPE)
    Y, X = cs.grid(cs.LENS_SHAPE)
    for c in range(3):
        lens.scene_coords(c, Y, X)
    assert lens.residual_px < cs.RESIDUAL_PX
    assert GOLDEN["checks"][f"lens_{name}"]["lens_inverse_residual_px"] < cs.RESIDUAL_PX
    # the forward lens takes the inverse's answer back to the pixel: green, by the chain of Lens's docstring
    Ys, Xs = lens.scene_coords(1, Y, X)
    r = np.hypot(Ys - lens.cy, Xs - lens.cx) / lens.norm
    rp = r
    if profile.projection is not None:
        kind, focal = profile.projection
        rp = cs._PROJECTION_RADIUS[kind](np.arctan(r / focal), focal)
    rd = rp * lens.distortion_factor(rp)
    assert np.abs(rd * lens.norm - np.hypot(Y - lens.cy, X - lens.cx)).max() < 1e-8


def test_a_lens_without_a_model_is_transparent():
    from raw2film_amd.lens import LensProfile

    lens = cs.Lens(LensProfile(), 40, 60)
    Y, X = cs.grid((40, 60))
    for c in range(3):
        Ys, Xs = lens.scene_coords(c, Y, X)
        assert np.abs(Ys - Y).max() < 1e-12 and np.abs(Xs - X).max() < 1e-12
    scene = cs.Scene()
    assert np.abs(lens.through(scene)(Y, X) - scene(Y, X)).max() < 1e-12
