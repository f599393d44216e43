"""tests/golden/noise_extremes.json, without a GPU: the searched (seed, x, y) whose PCG3D hash lands in one of gaussian_noise()'s
special regions -- the clamp max(u, 1e-7), u == 1.0, the fraction wrap of u1 + uy, the zero crossings of the angle -- which a
random frame reaches about once in 1e7 samples and a 100 MP export on every frame (tools/find_noise_extremes.py).  The fixture
is what it says it is, covers every row of the tool's table, and the float32 oracle stays within the field's bound of the
float64 truth at every record, so the GPU tests (tests/test_gpu_noise_extremes.py) can hold the device to both."""

import importlib.util
import json
import os

import numpy as np
import pytest

from oracle import stages as st
from oracle import truth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "noise_extremes.json")
BOUND = 1e-5  # test_gpu_parity.test_gaussian_field's: absolute, |n| < 6

# kind -> components it must be present for (the table of tools/find_noise_extremes.py, restated)
TABLE = {
    "zero": ("vx", "vy", "vz"),
    "clamped": ("vx", "vz"),
    "just-free": ("vx", "vz"),
    "one": ("vx", "vy", "vz"),
    "below-one": ("vx", "vz"),
    "quarter": ("vy",),
    "wrap": ("s12",),
    "edge": ("vx", "vz"),
}
INDEX = {"vx": 0, "vy": 1, "vz": 2}


def load():
    with open(FIXTURE) as f:
        doc = json.load(f)
    return doc["records"], doc["window"]["H"], doc["window"]["W"]


RECORDS, H, W = load()


def record_id(r):
    return f'{r["kind"]}-{r["component"]}-{r["seed"]}'


def of_kind(kind, component=None):
    return [r for r in RECORDS if r["kind"] == kind and component in (None, r["component"])]


def hashes_at(r):
    return tuple(int(v[0, 0]) for v in st.pcg3d(np.array([[r["x"]]]), np.array([[r["y"]]]), r["seed"]))


def test_every_record_hashes_to_its_recorded_value_inside_the_window():
    assert len(RECORDS) == len({(r["kind"], r["component"], r["seed"], r["x"], r["y"]) for r in RECORDS})
    for r in RECORDS:
        assert 0 <= r["x"] < W and 0 <= r["y"] < H and 0 <= r["seed"] < 1 << 32, r
        got = hashes_at(r)
        if r["kind"] == "wrap":
            assert (got[0], got[1]) == (r["hash"], r["hash_y"]), r
        else:
            assert got[INDEX[r["component"]]] == r["hash"], r


def test_every_record_is_of_its_kind():
    f32 = np.float32
    inv = f32(1.0) / f32(0xFFFFFFFF)
    for r in RECORDS:
        v, kind = r["hash"], r["kind"]
        u = f32(v) * inv
        if kind == "zero":
            assert v == 0
        elif kind == "clamped":
            assert 1 <= v <= 429 and u < f32(1e-7)
        elif kind == "just-free":
            assert 430 <= v <= 440 and u >= f32(1e-7)
        elif kind == "one":
            assert v >= 0xFFFFFF80 and u == f32(1.0)
        elif kind == "below-one":
            assert 0xFFFFFE80 <= v <= 0xFFFFFF7F and f32(1.0) - f32(2.0 ** -23) <= u < f32(1.0)
        elif kind == "quarter":
            assert abs(v - (r["quarter"] << 30)) <= 32 and u == f32(0.25 * r["quarter"])
        elif kind == "wrap":
            s12 = np.maximum(u, f32(1e-7)) + f32(r["hash_y"]) * inv
            assert abs(float(s12) - 1.0) <= 2.0 ** -22 and (s12 < f32(1.0)) == (r["side"] == "below"), r
        elif kind == "edge":
            assert (v <= 429 or v >= 0xFFFFFF80) and min(r["x"], W - 1 - r["x"], r["y"], H - 1 - r["y"]) <= 1
        else:
            raise AssertionError(f"unknown kind {kind}")


def test_every_kind_and_component_of_the_table_is_present():
    assert {r["kind"] for r in RECORDS} == set(TABLE)
    for kind, components in TABLE.items():
        for c in components:
            assert of_kind(kind, c), (kind, c)
    for c in ("vx", "vz"):
        assert len(of_kind("clamped", c)) >= 3 and min(r["hash"] for r in of_kind("clamped", c)) <= 3, c
    for side in ("below", "at-or-above"):
        assert sum(r["side"] == side for r in of_kind("wrap")) >= 3, side
    assert {r["quarter"] for r in of_kind("quarter")} == {1, 2, 3}
    # the clamp is not a dead branch of the float32 formula: without it these samples are not finite
    with np.errstate(divide="ignore"):
        assert np.isinf(np.sqrt(np.float32(-2.0) * np.log(np.float32(0.0))))


@pytest.mark.parametrize("mono", [False, True], ids=["colour", "mono"])
def test_the_oracle_is_finite_and_within_the_bound_of_the_truth_at_every_record(mono):
    worst = 0.0
    for r in RECORDS:
        xs, ys = np.array([[r["x"]]]), np.array([[r["y"]]])
        got = st.gaussian_noise(xs, ys, r["seed"], mono)[0, 0]
        exact = truth.gaussian_noise(xs, ys, r["seed"], mono)[0, 0]
        assert got.dtype == np.float32 and np.isfinite(got).all() and np.isfinite(exact).all(), r
        worst = max(worst, float(np.abs(got - exact).max()))
        assert np.abs(got - exact).max() <= BOUND, r
    print(f"oracle against truth at the records ({'mono' if mono else 'colour'}): {worst:.2e}")
    # (measured 2.3e-6: the reference's own share of the bound, mostly the float32 rounding of the angle times r = 5.68)


def test_what_the_special_regions_give():
    """The values the kinds exist for, on the truth: r = sqrt(-2 ln 1e-7) at the clamp and at hash 0, r = 0 at u == 1, a zero
    of the sine or cosine at a quarter turn."""
    r_clamp = float(np.sqrt(-2.0 * np.log(float(np.float32(1e-7)))))
    two_pi = float(np.float32(2.0 * 3.14159265359))
    for r in RECORDS:
        n = truth.gaussian_noise(np.array([[r["x"]]]), np.array([[r["y"]]]), r["seed"])[0, 0]
        hx, hy, hz = hashes_at(r)
        uy = float(np.float32(hy)) * 2.0 ** -32
        if r["kind"] in ("zero", "clamped") and r["component"] == "vx":
            assert abs(np.hypot(n[0], n[1]) - r_clamp) <= 1e-12 and 5.67 < r_clamp < 5.68
        if r["kind"] in ("zero", "clamped") and r["component"] == "vz":
            u1 = max(float(np.float32(hx)) * 2.0 ** -32, float(np.float32(1e-7)))
            assert abs(n[2] - r_clamp * np.cos(two_pi * ((u1 + uy) % 1.0))) <= 1e-9
        if r["kind"] == "one" and r["component"] == "vx":
            assert n[0] == 0.0 and n[1] == 0.0
        if r["kind"] == "one" and r["component"] == "vz":
            assert n[2] == 0.0
        if r["kind"] == "quarter":
            small = n[0] if r["quarter"] in (1, 3) else n[1]
            assert abs(small) <= 6.0 * 2e-7  # the float32 two_pi of the WGSL is 1.7e-7 off a full turn


def test_the_tool_reproduces_the_first_record():
    spec = importlib.util.spec_from_file_location("find_noise_extremes", os.path.join(ROOT, "tools", "find_noise_extremes.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    first = RECORDS[0]
    found = [rec for _, rec in tool.search(max(first["seed"] - 2, 0), first["seed"] + 3)]
    assert first in found
    assert (tool.W, tool.H) == (W, H)
    # and its table is the one this file restates
    kinds = {}
    for kind, c in tool.REQUIRED:
        kind = kind.split("<")[0]
        kinds.setdefault(kind, set()).add("s12" if kind == "wrap" else "vy" if kind == "quarter" else c)
    assert kinds == {k: set(v) for k, v in TABLE.items()}
    # a fixture that lacks a row does not get written
    some = [(key, rec) for key, rec in tool.search(first["seed"], first["seed"] + 1)]
    assert tool.select(some)[1], "select() must name the missing rows"
