"""A mosaic's scale from the sensor's levels, without a GPU: RawLevels' validation, the planner (raw2film_amd/csrc/r2f_levels_plan.cpp)
against the NumPy model of include/r2f.h's Scale steps (tests/levels_model.py) -- through the library and through a stand-alone program
under AddressSanitizer / UBSan (tests/levels_check.cpp) --, deferred profiles (`resolve`, `plan`), the ABI structs, the stream gates
and the payload of phase 1."""

import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import demosaic_model as dm
import levels_model as lm
import xtrans_model as xm
from raw2film_amd import _lib
from raw2film_amd.hip_processor import HipProcessor
from raw2film_amd.payload import host_stream_gate, mosaic_rejection, stream_rejection
from raw2film_amd.raw import RawLevels, RawProfile, XTransProfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raw2film_amd", "csrc")
WB = (2.1, 1.0, 1.6)


# ---- RawLevels
def test_levels_are_frozen_hashable_and_normalised():
    a = RawLevels([2.0, 1, 1.5], np.int64(16383))
    b = RawLevels((2.0, 1.0, 1.5), 16383, 0.75)
    assert a == b and hash(a) == hash(b) and {a: 1}[b] == 1 and a != RawLevels((2.0, 1.0, 1.5), 16383, 0.5)
    assert a.white_balance == (2.0, 1.0, 1.5) and type(a.white_level) is int and a.adjust_maximum_thr == 0.75
    with pytest.raises(Exception):
        a.white_level = 4095
    for thr in (0, 1, 0.0, 1.0):
        assert RawLevels(WB, 1, thr).adjust_maximum_thr == float(thr)
    assert RawLevels(WB, 65535).white_level == 65535


@pytest.mark.parametrize("kw, field", [
    (dict(white_balance=(1.0, 1.0)), "white_balance"), (dict(white_balance=(1.0, 0.0, 1.0)), "white_balance"),
    (dict(white_balance=(1.0, -2.0, 1.0)), "white_balance"), (dict(white_balance=(1.0, float("inf"), 1.0)), "white_balance"),
    (dict(white_balance=(1.0, float("nan"), 1.0)), "white_balance"), (dict(white_balance=2.0), "white_balance"),
    (dict(white_level=0), "white_level"), (dict(white_level=65536), "white_level"), (dict(white_level=4095.0), "white_level"),
    (dict(white_level=True), "white_level"), (dict(white_level="4095"), "white_level"), (dict(white_level=-1), "white_level"),
    (dict(adjust_maximum_thr=-0.1), "adjust_maximum_thr"), (dict(adjust_maximum_thr=1.01), "adjust_maximum_thr"),
    (dict(adjust_maximum_thr=float("nan")), "adjust_maximum_thr"), (dict(adjust_maximum_thr="0.75"), "adjust_maximum_thr"),
    (dict(adjust_maximum_thr=None), "adjust_maximum_thr"),
])
def test_each_refusal_names_its_field(kw, field):
    with pytest.raises(ValueError, match=rf"RawLevels\.{field}"):
        RawLevels(**{**dict(white_balance=WB, white_level=16383), **kw})


# ---- the planner against the model
M_EXACT, M_INEXACT = 15871, 15873  # 15871 * 0.75 = 11903.25 is a float; 15873 * 0.7 is not (nor is 0.7)
THRESHOLDS = (0, 0.000009, 0.00001, 0.5, 0.75, 0.99999, 0.999991, 1)
BLACK4 = (512, 515, 509, 512)  # a distinct minimum: m = white_level - 509
BLACK36 = tuple(1024 + ((7 * i) % 36) - (40 if i == 23 else 0) for i in range(36))  # ... at phase 23: 1024 + 17 - 40


def _maxima(m):
    """d across every branch of the Scale steps for a maximum m: the ends, m's neighbours, and both sides of each threshold product."""
    ds = {0, 1, m - 1, m, m + 1, 65535}
    for thr in THRESHOLDS:
        t = lm.threshold(float(thr))
        if t is not None:
            p = int(np.float32(m) * np.float32(t))
            ds |= {p - 1, p, p + 1, p + 2}
    return sorted(d for d in ds if 0 <= d <= 65535)


def _cases():
    for m, black in ((M_EXACT, BLACK4), (M_INEXACT, BLACK36), (M_INEXACT, (0,) * 4), (1, (65534,) * 4)):
        white = m + min(black)
        for thr in THRESHOLDS + (0.7,):
            for d in _maxima(m):
                yield WB, white, thr, black, d
    yield (1.0, 2.5, 1.75), 4095, 0.75, (64,) * 36, 3500
    yield (3.0, 3.0, 3.0), 65535, 0.75, (0,) * 4, 60000


CASES = list(_cases())


def _plan(wb, white, thr, black, d):
    return RawLevels(wb, white, thr).scale(black, d)


def test_the_grid_crosses_every_branch():
    seen = set()
    for wb, white, thr, black, d in CASES:
        mul, used, adjusted = lm.scale(wb, white, thr, black, d)
        m = white - min(black)
        seen.add(("adjusted" if adjusted else "off" if lm.threshold(float(thr)) is None else "zero" if d == 0 else "above" if d >= m else "below"))
    assert seen == {"adjusted", "off", "zero", "above", "below"}
    # the example of the definition: 15871 * 0.75 = 11903.25
    assert lm.scale(WB, M_EXACT + 509, 0.75, BLACK4, 11903)[1:] == (M_EXACT, False)
    assert lm.scale(WB, M_EXACT + 509, 0.75, BLACK4, 11904)[1:] == (11904, True)
    # a product that is not exact in fp32: the comparison is against the ROUNDED product
    exact, rounded = M_INEXACT * 0.7, float(np.float32(M_INEXACT) * np.float32(0.7))
    assert exact != rounded and float(np.float32(0.7)) != 0.7
    # 0.00001 is a threshold (nearly every frame is adjusted), 0.000009 is none; 0.999991 means 0.75, 0.99999 is itself
    assert lm.scale(WB, 16383, 0.00001, (0,) * 4, 5)[2] and not lm.scale(WB, 16383, 0.000009, (0,) * 4, 5)[2]
    assert lm.scale(WB, 16383, 0.999991, (0,) * 4, 13000)[2] and not lm.scale(WB, 16383, 0.99999, (0,) * 4, 13000)[2]
    assert lm.scale(WB, 16383, 1, (0,) * 4, 13000)[2] and not lm.scale(WB, 16383, 0.99999, (0,) * 4, 16382)[2]  # (16382.84 is the product)


def test_planner_equals_the_model_bit_for_bit():
    for wb, white, thr, black, d in CASES:
        want = lm.scale(wb, white, thr, black, d)
        got = _plan(wb, white, thr, black, d)
        assert (tuple(got.mul), got.maximum_used, bool(got.adjusted)) == want, (wb, white, thr, black, d)
    # the smallest white balance becomes 1: mul of that channel is 65535 / m_eff
    got = _plan(WB, M_EXACT + 509, 0.75, BLACK4, 0)
    assert got.mul[1] == 65535.0 / M_EXACT and got.maximum_used == M_EXACT and not got.adjusted


def test_planner_refusals_leave_the_output_alone():
    lib = _lib.load()

    def plan(wb=WB, white=16383, thr=0.75, black=(512,) * 4, d=0, n=None):
        lv = _lib.RawLevels(white_level=white, adjust_maximum_thr=thr)
        lv.white_balance[:] = wb
        out = _lib.RawScale(maximum_used=-77, adjusted=-88)
        out.mul[:] = (-1.5, -2.5, -3.5)
        rc = lib.r2f_raw_scale_plan(ctypes.byref(lv), (ctypes.c_double * len(black))(*black), len(black) if n is None else n, d, ctypes.byref(out))
        return rc, (tuple(out.mul), out.maximum_used, out.adjusted) == ((-1.5, -2.5, -3.5), -77, -88)

    assert plan() == (_lib.OK, False)
    nan, inf = float("nan"), float("inf")
    bad = [dict(white=512), dict(white=511), dict(white=0), dict(white=65536), dict(white=-5), dict(black=(20000,) * 4, white=1)]
    bad += [dict(wb=(1.0, nan, 1.0)), dict(wb=(inf, 1.0, 1.0)), dict(wb=(1.0, 1.0, 0.0)), dict(wb=(1.0, -1.0, 1.0))]
    bad += [dict(thr=nan), dict(thr=-0.01), dict(thr=1.01), dict(thr=inf), dict(d=65536), dict(d=2 ** 32 - 1)]
    bad += [dict(black=(512,) * 5), dict(black=(512,) * 4, n=0), dict(black=(512,) * 36, n=35), dict(black=(512, 512, 512, 12.5)),
            dict(black=(512, -1, 512, 512)), dict(black=(512, 65536, 512, 512)), dict(black=(512, nan, 512, 512))]
    for b in bad:
        assert plan(**b) == (_lib.EINVAL, True), b
    assert plan(white=513)[0] == _lib.OK  # white_level <= min(black) refused, one above it planned (m = 1)
    out = _lib.RawScale()
    assert lib.r2f_raw_scale_plan(None, (ctypes.c_double * 4)(), 4, 0, ctypes.byref(out)) == _lib.EINVAL
    with pytest.raises(ValueError, match="r2f_raw_scale_plan"):
        RawLevels(WB, 512).scale((512,) * 4)
    with pytest.raises(ValueError, match="data maximum"):
        RawLevels(WB, 16383).scale((512,) * 4, 65536)


# ---- the stand-alone program
@pytest.fixture(scope="module")
def levels_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("levels_check") / "levels_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
           "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "levels_check.cpp"), os.path.join(CSRC, "r2f_levels_plan.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def test_the_program_sweeps_the_grid_to_the_models_numbers(levels_check, tmp_path):
    refused = [(WB, 512, 0.75, (512,) * 4, 0), (WB, 2 ** 40, 0.75, (512,) * 4, 0), ((1.0, float("nan"), 1.0), 16383, 0.75, (512,) * 4, 0),
               (WB, 16383, float("inf"), (512,) * 4, 0), (WB, 16383, 0.75, (512,) * 5, 0), (WB, 16383, 0.75, (512, 1e300, 512, 512), 0),
               (WB, 16383, 0.75, (512,) * 4, 65536)]
    cases = CASES + refused
    job = tmp_path / "job.txt"
    job.write_text("".join(" ".join([*(float(v).hex() for v in wb), str(white), float(thr).hex(), str(d), str(len(black)),
                                     *(float(b).hex() for b in black)]) + "\n" for wb, white, thr, black, d in cases))
    res = subprocess.run([levels_check, "sweep", str(job)], capture_output=True, text=True, env=ENV, timeout=120)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    lines = res.stdout.splitlines()
    assert len(lines) == len(cases)
    for line, case in zip(lines[:len(CASES)], CASES):
        rc, *mul, used, adjusted = line.split()
        want = lm.scale(*case)
        assert int(rc) == _lib.OK and (tuple(float.fromhex(v) for v in mul), int(used), bool(int(adjusted))) == want, case
    assert lines[len(CASES):] == [str(_lib.EINVAL)] * len(refused)


@pytest.mark.parametrize("seed", [1, 20261020])
def test_planner_fuzz_is_clean_under_the_sanitizers(levels_check, seed):
    res = subprocess.run([levels_check, "fuzz", str(seed), "20000"], capture_output=True, text=True, env=ENV, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    assert "cases ok" in res.stdout


# ---- deferred profiles
MATRIX = dm.CAMERA
BAYER = RawProfile("GRBG", black=BLACK4, multipliers=RawLevels(WB, M_EXACT + 509), matrix=MATRIX, orientation=5)
XTRANS = XTransProfile(xm.PATTERNS[1], black=BLACK36, multipliers=RawLevels(WB, M_INEXACT + min(BLACK36), 0.7), matrix=MATRIX)


def _fields(params):
    return {name: bytes(memoryview(getattr(params, name)).cast("B")) if hasattr(getattr(params, name), "_length_") else getattr(params, name)
            for name, _ in params._fields_}


@pytest.mark.parametrize("profile, shape", [(BAYER, (40, 60)), (XTRANS, (42, 66))], ids=["bayer", "xtrans"])
@pytest.mark.parametrize("half", [False, True])
def test_resolve_plans_what_the_models_numbers_plan(profile, shape, half):
    lv = profile.multipliers
    m = lv.white_level - int(min(profile.black))
    assert profile.deferred and not profile.resolve(0).deferred and profile.resolve(0).resolve(5) == profile.resolve(0)
    for d in (0, 1, m // 2, int(m * 0.9), m - 1, m, 65535):
        mul, _, adjusted = lm.scale(lv.white_balance, lv.white_level, lv.adjust_maximum_thr, profile.black, d)
        assert adjusted == (d in (int(m * 0.9), m - 1))
        numeric = type(profile)(profile.pattern, black=profile.black, multipliers=mul, matrix=profile.matrix, orientation=profile.orientation)
        resolved = profile.resolve(d)
        assert resolved == numeric and hash(resolved) == hash(numeric) and resolved != profile
        got, want = _fields(resolved.plan(*shape, half)), _fields(numeric.plan(*shape, half))
        for name in want:
            assert got[name] == want[name], (name, d)
        if d == 0:  # a deferred profile plans its nominal scale, and so does its C form
            nominal = _fields(profile.plan(*shape, half))
            assert nominal == want and bytes(profile.to_c(half)) == bytes(numeric.to_c(half))
    assert profile.oriented_shape(*shape) == profile.resolve(0).oriented_shape(*shape)


def test_deferred_profiles_take_part_in_equality_and_hash():
    lv = RawLevels(WB, 16383)
    a, b = RawProfile("RGGB", black=512, multipliers=lv), RawProfile("RGGB", black=(512,) * 4, multipliers=RawLevels(list(WB), 16383, 0.75))
    assert a == b and hash(a) == hash(b) and a.multipliers is lv
    assert a != RawProfile("RGGB", black=512, multipliers=RawLevels(WB, 16383, 0.5)) and a != a.resolve(0)
    assert RawProfile("RGGB").deferred is False and RawProfile("RGGB").resolve(9) == RawProfile("RGGB")
    x = XTransProfile(black=512, multipliers=lv)
    assert x.deferred and x == XTransProfile(black=512, multipliers=RawLevels(WB, 16383)) and len(x.resolve(0).multipliers) == 3
    assert a.resolve(0).multipliers == tuple(a.resolve(0).multipliers["RGGB".index(c)] for c in "RGGB") and len(a.resolve(0).multipliers) == 4
    resolved, scale = a.resolve_scale(13000)  # one run of the planner: the profile and the record it was resolved with
    assert resolved == a.resolve(13000) and (scale.maximum_used, scale.adjusted) == (13000, 1) and tuple(scale.mul) == lm.scale(WB, 16383, 0.75, a.black, 13000)[0]
    assert resolved.resolve_scale(5) == (resolved, None)
    with pytest.raises(ValueError):
        a.resolve(-1)
    with pytest.raises(ValueError):
        a.resolve(1.5)


def test_a_scale_outside_the_planners_range_is_refused_by_plan():
    """mul = wb / min(wb) * 65535 / m_eff leaves (0, 1024] for a small maximum: m = 32 gives 2047.97."""
    small = RawProfile("RGGB", black=512, multipliers=RawLevels((1.0, 1.0, 1.0), 512 + 32))
    with pytest.raises(ValueError, match="r2f_demosaic_plan"):
        small.plan(8, 8)
    with pytest.raises(ValueError, match=r"\(0, 1024\]"):
        small.resolve(0)
    edge = RawProfile("RGGB", black=512, multipliers=RawLevels((1.0, 1.0, 1.0), 512 + 64))  # 65535 / 64 = 1023.98
    assert edge.plan(8, 8).mul[0] == np.float32(65535.0 / 64)
    with pytest.raises(ValueError, match=r"\(0, 1024\]"):
        edge.resolve(60)  # adjusted to 60 (above 0.75 * 64): 1092.25
    with pytest.raises(ValueError, match="r2f_xtrans_plan"):
        XTransProfile(black=512, multipliers=RawLevels((1.0, 16.5, 1.0), 512 + 1024)).plan(12, 12)  # 16.5 * 65535 / 1024 = 1055.98
    with pytest.raises(ValueError, match="r2f_raw_scale_plan"):
        RawProfile("RGGB", black=512, multipliers=RawLevels(WB, 512)).plan(8, 8)  # white_level <= min(black)


# ---- ABI
def test_struct_layouts_match_the_header():
    L, S = _lib.RawLevels, _lib.RawScale
    assert ctypes.sizeof(L) == 40 and [getattr(L, f).offset for f in ("white_balance", "white_level", "adjust_maximum_thr")] == [0, 24, 32]
    assert ctypes.sizeof(S) == 32 and [getattr(S, f).offset for f in ("mul", "maximum_used", "adjusted")] == [0, 24, 28]
    # the four structs from before this one keep their sizes
    assert [ctypes.sizeof(t) for t in (_lib.RawProfile, _lib.DemosaicParams, _lib.XTransProfile, _lib.XTransParams)] == [144, 96, 536, 900]
    text = open(os.path.join(ROOT, "include", "r2f.h")).read()
    body = text[text.index("typedef struct r2f_raw_levels {"):text.index("} r2f_raw_levels;")]
    order = [body.index(w) for w in ("double white_balance[3];", "int32_t white_level;", "double adjust_maximum_thr;")]
    assert order == sorted(order)
    body = text[text.index("typedef struct r2f_raw_scale {"):text.index("} r2f_raw_scale;")]
    order = [body.index(w) for w in ("double mul[3];", "int32_t maximum_used;", "int32_t adjusted;")]
    assert order == sorted(order)
    assert f"R2F_MOSAIC_MAX_VEC = {_lib.MOSAIC_MAX_VEC}, R2F_MOSAIC_MAX_ROWS = {_lib.MOSAIC_MAX_ROWS}" in text
    assert "UNPINNED" in text[text.index("The scale of a mosaic from the sensor's levels"):text.index("typedef struct r2f_raw_levels")]


# ---- the gates
def test_both_gates_answer_with_the_new_reason_for_a_call_that_otherwise_streams():
    big = np.zeros((1 << 13, 1 << 13), np.uint16)
    samples = 3 << 26
    assert mosaic_rejection(True, 0, False, samples) is None and mosaic_rejection(True, 4, False, samples, levels=False) is None
    why = mosaic_rejection(True, 0, False, samples, levels=True)
    assert why is not None and "demosaic" in why and "RawLevels" in why
    kw = dict(stops=True, rotate_times=0, frame_samples=samples)
    assert host_stream_gate(big, 16, 0.0, 0, "No", 0.0, False, True, **kw) is None
    assert host_stream_gate(big, 16, 0.0, 0, "No", 0.0, False, True, levels=False, **kw) is None
    assert host_stream_gate(big, 16, 0.0, 0, "No", 0.0, False, True, levels=True, **kw) == why
    assert host_stream_gate(np.zeros((1 << 12, 1 << 12, 3), np.uint16), 16, levels=True) is None  # (no mosaic: nothing to defer)
    # the new reason is the last one asked for: every earlier reason keeps its answer with levels=True
    for args in ((False, 0, False, samples), (True, 1, False, samples), (True, 0, True, samples), (True, 0, False, None), (True, 0, False, 99)):
        assert mosaic_rejection(*args, levels=True) == mosaic_rejection(*args) is not None
    assert mosaic_rejection(True, 0, False, samples, True, levels=True) == mosaic_rejection(True, 0, False, samples, True)
    assert mosaic_rejection(True, 0, False, samples, False, 3, levels=True) == mosaic_rejection(True, 0, False, samples, False, 3)
    assert host_stream_gate(big, 1, levels=True, demosaic=True, **kw) == "stream_bands = 1"
    assert host_stream_gate(big, 16, 2.5, demosaic=True, levels=True, **kw) == host_stream_gate(big, 16, 2.5, demosaic=True, **kw) is not None


# ---- phase 1 of the processor
@pytest.fixture
def proc():
    p = HipProcessor.__new__(HipProcessor)
    p.cameras = p.lenses = None
    p.payload_alpha = True
    return p


MOSAIC, NUMERIC = dm.fixture("random", "GRBG", 96, 144)


def test_a_deferred_profiles_payload_carries_the_levels_and_provisional_nominal_params(proc):
    deferred = RawProfile("GRBG", black=NUMERIC.black, multipliers=RawLevels(WB, 16383), matrix=NUMERIC.matrix)
    for kw in (dict(exposure=0.5), dict(exposure=0.5, half_size=False), dict(exposure=None, zoom=1.3)):
        pay = proc.extract_image_data_cpu(MOSAIC, raw_profile=deferred, **kw)
        nominal = proc.extract_image_data_cpu(MOSAIC, raw_profile=deferred.resolve(0), **kw)
        step = pay["demosaic"]
        assert set(step) == {"params", "window", "rotate_times", "levels"} and step["levels"] is deferred
        assert set(pay) == set(nominal) and pay["image_array"] is MOSAIC
        assert _fields(step["params"]) == _fields(nominal["demosaic"]["params"])
        for k in pay:
            if k not in ("demosaic", "image_array", "warp"):
                assert pay[k] == nominal[k], k
        assert {k: v for k, v in step.items() if k not in ("params", "levels")} == {k: v for k, v in nominal["demosaic"].items() if k != "params"}
    x = XTransProfile(black=512, multipliers=RawLevels(WB, 16383), orientation=6)
    step = proc.extract_image_data_cpu(MOSAIC, raw_profile=x, exposure=0.0)["demosaic"]
    assert set(step) == {"params", "window", "rotate_times", "orientation", "levels"} and step["levels"] is x


def test_a_numeric_profiles_payload_is_what_it_was(proc):
    """The key set and the values of the payload of a numeric profile, spelled out: no `levels`, nothing else new."""
    pay = proc.extract_image_data_cpu(MOSAIC, raw_profile=NUMERIC, exposure=0.5)
    params = pay["demosaic"].pop("params")
    assert _fields(params) == _fields(NUMERIC.plan(96, 144, True))
    assert pay.pop("image_array") is MOSAIC
    assert pay.pop("u16_factor") == float(np.float32(2.0 ** 0.5))
    assert pay == {
        "u16_window": None, "exposure_root": None, "exposure_rejected": None, "clip_on_device": False,
        "final_resolution": (48, 72), "output_resolution": (72, 48), "canvas_resolution": None, "pipeline_resolution": (72, 48),
        "chroma_nr": 0, "resize_to": None, "warp": None, "upscale_to": None,
        "demosaic": {"window": (0, 0, 48, 72), "rotate_times": 0},
    }
    oriented = proc.extract_image_data_cpu(MOSAIC, raw_profile=RawProfile("GRBG", orientation=5), exposure=0.5)
    assert set(oriented["demosaic"]) == {"params", "window", "rotate_times", "orientation"}


def test_the_payloads_gate_refuses_a_deferred_profile_last(proc, monkeypatch):
    deferred = RawProfile("GRBG", black=NUMERIC.black, multipliers=RawLevels(WB, 16383), matrix=NUMERIC.matrix)
    pay = proc.extract_image_data_cpu(MOSAIC, raw_profile=deferred, exposure=0.5)
    plain = proc.extract_image_data_cpu(MOSAIC, raw_profile=deferred.resolve(0), exposure=0.5)
    args = ((96, 144), "torch.int16", False, "gpu")
    assert stream_rejection(pay, *args) == stream_rejection(plain, *args) and "below 16.7 M" in stream_rejection(pay, *args)
    monkeypatch.setattr("raw2film_amd.payload.STREAM_MIN_SAMPLES", 1)  # a frame that otherwise streams
    assert stream_rejection(plain, *args) is None
    why = stream_rejection(pay, *args)
    assert why is not None and "demosaic" in why and "RawLevels" in why


def test_a_changed_levels_record_invalidates_the_image_cache_and_an_equal_one_does_not(proc):
    uploads = []

    def prepare(payload):
        uploads.append(payload.get("demosaic"))
        proc._texture = ("frame", None, {})
        proc.image_param_dict = None

    proc.prepare_gpu_textures = prepare
    make = lambda white, thr=0.75: RawProfile("GRBG", black=64, multipliers=RawLevels(WB, white, thr))  # noqa: E731
    proc.load_image_texture(MOSAIC, raw_profile=make(16383), exposure=0.0)
    proc.load_image_texture(MOSAIC, raw_profile=make(16383), exposure=0.0)
    assert len(uploads) == 1 and uploads[0]["levels"] == make(16383)
    proc.load_image_texture(MOSAIC, raw_profile=make(16383, 0.5), exposure=0.0)
    proc.load_image_texture(MOSAIC, raw_profile=make(4095), exposure=0.0)
    proc.load_image_texture(MOSAIC, raw_profile=make(4095).resolve(0), exposure=0.0)
    assert len(uploads) == 4 and "levels" not in uploads[3]
