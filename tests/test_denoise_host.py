"""The wavelet denoise of a Bayer mosaic without a GPU: the planner (r2f_mosaic_denoise_plan) through the library; the text the kernel
compiles (r2f_denoise_math.h) and the planner in a stand-alone program under AddressSanitizer / UBSan (tests/denoise_check.cpp), whose
bytes are held against the NumPy model of include/r2f.h (tests/denoise_model.py) and which walks every index reflection; the
WaveletDenoise record, phase 1's checks and payload, the stream gates and the image cache key; the model's own sanity on flat fields."""

import ctypes
import dataclasses
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import demosaic_model as dm
import denoise_cases as cases
import denoise_model as model
from raw2film_amd import _lib, hip_processor
from raw2film_amd.hip_processor import HipProcessor
from raw2film_amd.payload import host_stream_gate, mosaic_rejection, stream_rejection
from raw2film_amd.raw import RawLevels, RawProfile, WaveletDenoise, XTransProfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raw2film_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
WB = (2.1, 1.0, 1.6)


# ---- the model itself
def test_shift_of_the_headers_maxima():
    assert [model.shift_of(m) for m in (1, 255, 16383 - 512, 32767, 32768, 65535)] == [15, 8, 2, 1, 0, 0]
    assert tuple(model.shift_of(m) for m in cases.MAXIMA) == cases.SHIFTS


def test_a_flat_field_comes_back_as_t_shifted_and_clamps_above_the_range():
    """256 sqrt(v) squared over 65536 is v where sqrt(v) is exact in float32: every level's low pass of a flat field is the field
    (2 F + F + F over 4, exactly), every detail 0."""
    for s, maximum in ((0, 40000), (2, 16383)):
        for t in (0, 1, 4, 3969):
            flat = np.full((64, 72), t + 100, np.uint16)
            out = model.denoise(flat, (100,) * 4, maximum, 100.0)
            assert (out == (t << s)).all(), (t, s)
    out = model.denoise(np.full((64, 64), 65535, np.uint16), (0,) * 4, 16383, 100.0)  # s = 2: 262140 leaves as 65535
    assert (out == 65535).all()


def test_the_threshold_smooths_a_noisy_flat_field():
    rng = np.random.default_rng(5)
    noisy = np.clip(np.rint(12000 + rng.normal(0, 237, (128, 128))), 0, 65535).astype(np.uint16)
    sd = [float(model.denoise(noisy, (0,) * 4, 65535, T).astype(np.float64).std()) for T in (1.0, 100.0, 400.0)]
    assert sd[0] > sd[1] > sd[2] and abs(sd[0] - 237) < 12 and sd[2] < 120


def test_every_tap_of_the_side_bound_stays_inside():
    for n in range(32, 81):
        for c in (1, 2, 4, 8, 16):
            model.taps(n, c)  # (asserts)
    with pytest.raises(AssertionError):
        model.taps(16, 16)  # dcraw's out-of-row index, which the side bound rules out


# ---- the planner through the library
def _plan(threshold, maximum, black, H, W):
    out = _lib.DenoiseParams(shift=-15, threshold=-16.0)
    out.black[:] = (-11, -12, -13, -14)
    table = None if black is None else (ctypes.c_double * len(black))(*black)
    rc = _lib.load().r2f_mosaic_denoise_plan(threshold, maximum, table, H, W, ctypes.byref(out))
    return rc, (tuple(out.black), out.shift, out.threshold)


UNTOUCHED = ((-11, -12, -13, -14), -15, -16.0)


def test_planner_shifts_and_fields():
    for maximum, shift in zip((1, 255, 16383 - 512, 32767, 32768, 65535), (15, 8, 2, 1, 0, 0)):
        rc, got = _plan(0.1, maximum, cases.BLACK, 64, 70)
        assert rc == _lib.OK and got == (cases.BLACK, shift, float(np.float32(0.1)))
    assert _plan(1e6, 1, (0, 65535, 0, 0), 64, 64)[0] == _lib.OK


@pytest.mark.parametrize("args", [
    (0.0, 16383, cases.BLACK, 64, 64), (-3.0, 16383, cases.BLACK, 64, 64), (float("nan"), 16383, cases.BLACK, 64, 64),
    (float("inf"), 16383, cases.BLACK, 64, 64), (1000000.5, 16383, cases.BLACK, 64, 64), (1e-60, 16383, cases.BLACK, 64, 64),
    (100.0, 0, cases.BLACK, 64, 64), (100.0, 65536, cases.BLACK, 64, 64), (100.0, -1, cases.BLACK, 64, 64),
    (100.0, 16383, (512, 512.5, 512, 512), 64, 64), (100.0, 16383, (512, -1, 512, 512), 64, 64),
    (100.0, 16383, (512, 65536, 512, 512), 64, 64), (100.0, 16383, (512, float("nan"), 512, 512), 64, 64),
    (100.0, 16383, cases.BLACK, 62, 64), (100.0, 16383, cases.BLACK, 64, 62), (100.0, 16383, cases.BLACK, 65, 64),
    (100.0, 16383, cases.BLACK, 64, 65), (100.0, 16383, cases.BLACK, 0, 0), (100.0, 16383, cases.BLACK, -64, 64),
    (100.0, 16383, None, 64, 64),
])
def test_planner_refusals_leave_the_output_alone(args):
    rc, got = _plan(*args)
    assert rc == _lib.EINVAL and got == UNTOUCHED


def test_planner_refuses_a_null_output_and_sizes_the_workspace():
    lib = _lib.load()
    assert lib.r2f_mosaic_denoise_plan(100.0, 16383, (ctypes.c_double * 4)(*cases.BLACK), 64, 64, None) == _lib.EINVAL
    for H, W in cases.SHAPES:
        assert lib.r2f_mosaic_denoise_workspace_bytes(H, W) == 12 * H * W
    assert lib.r2f_mosaic_denoise_workspace_bytes(62, 64) == 0 and lib.r2f_mosaic_denoise_workspace_bytes(64, 65) == 0


def test_struct_and_enums_match_the_header():
    assert ctypes.sizeof(_lib.DenoiseParams) == 24 and _lib.DenoiseParams.shift.offset == 16 and _lib.DenoiseParams.threshold.offset == 20
    text = open(os.path.join(ROOT, "include", "r2f.h")).read()
    assert f"R2F_DENOISE_TILE_W = {_lib.DENOISE_TILE_W}, R2F_DENOISE_TILE_H = {_lib.DENOISE_TILE_H}" in text
    section = text[text.index("The wavelet denoise of a Bayer mosaic on the device"):text.index("typedef struct r2f_denoise_params")]
    assert "UNPINNED" in section and "NOT built" in section and "X-Trans" in section and "two greens" in section


# ---- the stand-alone program under the sanitizers
@pytest.fixture(scope="module")
def denoise_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("denoise_check") / "denoise_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall",
           os.path.join(ROOT, "tests", "denoise_check.cpp"), os.path.join(CSRC, "r2f_denoise_plan.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


def test_the_program_walks_every_reflection(denoise_check):
    res = subprocess.run([denoise_check, "reflect"], capture_output=True, text=True, env=ENV, timeout=120)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    assert res.stdout.split()[:2] == ["reflect", "ok"] and int(res.stdout.split()[2]) == 2 * 5 * sum(range(32, 81))


def test_the_programs_planner_refusals_leave_the_output_alone(denoise_check):
    res = subprocess.run([denoise_check, "refuse"], capture_output=True, text=True, env=ENV, timeout=120)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    assert "refusals ok 21" in res.stdout


PROGRAM_CASES = [(shape, name, T, M) for shape in cases.SHAPES
                 for name, T, M in (("edge", 100.0, 16383 - 512), ("edge", 400.0, 255), ("impulses", 1.0, 32768), ("impulses", 1e5, 1),
                                    ("full", 100.0, 32767), ("zeros", 400.0, 1))]


@pytest.mark.parametrize("shape", cases.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_programs_bytes_equal_the_models(denoise_check, tmp_path, shape):
    for _, name, T, M in (c for c in PROGRAM_CASES if c[0] == shape):
        src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
        src.write_bytes(struct.pack("<7id", shape[0], shape[1], M, *cases.BLACK, T) + cases.mosaic(shape, name).tobytes())
        res = subprocess.run([denoise_check, "run", str(src), str(dst)], capture_output=True, text=True, env=ENV, timeout=300)
        assert res.returncode == 0, (name, T, M, (res.stdout + res.stderr)[-4000:])
        got = np.frombuffer(dst.read_bytes(), np.uint16).reshape(shape)
        want = cases.expected(shape, name, T, M)
        assert np.array_equal(got, want), (name, T, M, int((got != want).sum()))


def test_the_inputs_exercise_what_they_are_for():
    """Chosen here, where it is cheap: the black level above some samples, thresholds on both sides of the details, clamped output."""
    edge = cases.mosaic((66, 70), "edge")
    assert (edge[1::2, 1::2] < cases.BLACK[3]).any() and (edge[1::2, 1::2] > cases.BLACK[3]).any()
    outs = [cases.expected((66, 70), "edge", T, 16383 - 512) for T in cases.THRESHOLDS]
    assert all(not np.array_equal(a, b) for a, b in zip(outs, outs[1:]))
    assert (cases.expected((64, 64), "full", 100.0, 255) == 65535).all() and (cases.expected((64, 64), "zeros", 100.0, 255) == 0).all()
    imp = cases.expected((64, 64), "impulses", 1.0, 32768)
    assert imp[0, 0] > 50000 and imp[63, 63] > 50000  # (a threshold of 1 keeps the corner samples)


# ---- the record
def test_the_record_is_frozen_hashable_and_checked():
    a, b = WaveletDenoise(100, 16383), WaveletDenoise(100.0, maximum=16383)
    assert a == b and hash(a) == hash(b) and a != WaveletDenoise(100.0) and a != WaveletDenoise(101.0, 16383)
    assert isinstance(a.threshold, float) and isinstance(a.maximum, int) and WaveletDenoise(5).maximum is None
    assert [f.name for f in dataclasses.fields(WaveletDenoise)] == ["threshold", "maximum"]
    with pytest.raises(dataclasses.FrozenInstanceError):
        a.threshold = 3.0
    for bad in (0, -1.0, float("nan"), float("inf"), 1e6 + 1, True, "100", None):
        with pytest.raises(ValueError, match="threshold"):
            WaveletDenoise(bad)
    for bad in (0, 65536, -3, 1.5, True, "16383"):
        with pytest.raises(ValueError, match="maximum"):
            WaveletDenoise(100.0, bad)


def test_plan_and_shift_of_the_record():
    dn = WaveletDenoise(100.0, 255)
    assert dn.shift() == 8 and dn.shift(32767) == 1 and WaveletDenoise(1.0).shift(1) == 15
    p = dn.plan(cases.BLACK, 66, 70)
    assert (tuple(p.black), p.shift, p.threshold) == (cases.BLACK, 8, 100.0)
    assert dn.plan(cases.BLACK, 66, 70, 16383 - 512).shift == 2
    with pytest.raises(ValueError, match="maximum"):
        WaveletDenoise(100.0).plan(cases.BLACK, 66, 70)
    for H, W in ((62, 70), (66, 71), (63, 64)):
        with pytest.raises(ValueError, match="even and at least 64"):
            dn.plan(cases.BLACK, H, W)
    with pytest.raises(ValueError):
        dn.plan((512, 512, 70000, 512), 66, 70)


def test_the_shifted_profile_has_no_black_and_exactly_scaled_multipliers():
    profile = RawProfile("GRBG", black=cases.BLACK, multipliers=(8.3, 4.1, 6.7), matrix=((1.2, -0.1, -0.1), (0, 1, 0), (0.1, 0.2, 0.7)),
                         highlight=("blend", 40000), orientation=5)
    shifted = WaveletDenoise.shifted(profile, 2)
    assert shifted.black == (0.0,) * 4 and shifted.multipliers == tuple(m / 4 for m in profile.multipliers)
    assert (shifted.pattern, shifted.matrix, shifted.highlight, shifted.orientation) == (profile.pattern, profile.matrix, profile.highlight, 5)
    a, b = profile.plan(96, 144), shifted.plan(96, 144)
    assert tuple(b.black) == (0,) * 4 and [np.float32(m) for m in b.mul] == [np.float32(m) * np.float32(0.25) for m in a.mul]
    assert WaveletDenoise.shifted(profile, 0).multipliers == profile.multipliers


def test_the_profiles_keep_their_six_fields():
    names = ["pattern", "black", "multipliers", "matrix", "highlight", "orientation"]
    assert [f.name for f in dataclasses.fields(RawProfile)] == names and [f.name for f in dataclasses.fields(XTransProfile)] == names


# ---- phase 1 of the processor
@pytest.fixture
def proc():
    p = HipProcessor.__new__(HipProcessor)
    p.cameras = p.lenses = None
    p.payload_alpha = True
    return p


MOSAIC, NUMERIC = dm.fixture("random", "GRBG", 96, 144)
DEFERRED = RawProfile("GRBG", black=NUMERIC.black, multipliers=RawLevels(WB, 16383), matrix=NUMERIC.matrix)


def test_phase_1_names_each_reason_it_refuses_a_denoise_for(proc):
    dn = WaveletDenoise(100.0, 16383)
    with pytest.raises(ValueError, match="needs a raw_profile"):
        proc.extract_image_data_cpu(np.zeros((96, 144, 3), np.uint16), raw_denoise=dn, exposure=0.0)
    with pytest.raises(ValueError, match="not built for X-Trans mosaics"):
        proc.extract_image_data_cpu(MOSAIC, raw_profile=XTransProfile(black=512), raw_denoise=dn, exposure=0.0)
    with pytest.raises(ValueError, match="maximum=None"):
        proc.extract_image_data_cpu(MOSAIC, raw_profile=NUMERIC, raw_denoise=WaveletDenoise(100.0), exposure=0.0)
    for shape in ((62, 144), (96, 62), (97, 144), (96, 145)):
        with pytest.raises(ValueError, match="even and at least 64"):
            proc.extract_image_data_cpu(np.zeros(shape, np.uint16), raw_profile=NUMERIC, raw_denoise=dn, exposure=0.0, half_size=False)
    with pytest.raises(ValueError, match="WaveletDenoise"):
        proc.extract_image_data_cpu(MOSAIC, raw_profile=NUMERIC, raw_denoise=100.0, exposure=0.0)


def test_the_demosaic_step_carries_the_record_and_nothing_else_moves(proc):
    dn = WaveletDenoise(100.0, 16383)
    for profile, extra in ((NUMERIC, set()), (DEFERRED, {"levels"})):
        for record in (dn, WaveletDenoise(100.0)) if profile is DEFERRED else (dn,):
            pay = proc.extract_image_data_cpu(MOSAIC, raw_profile=profile, raw_denoise=record, exposure=0.5)
            plain = proc.extract_image_data_cpu(MOSAIC, raw_profile=profile, exposure=0.5)
            step = pay["demosaic"]
            assert set(step) == {"params", "window", "rotate_times", "denoise", "profile"} | extra
            assert step["denoise"] is record and step["profile"] is profile and "denoise" not in plain["demosaic"]
            assert set(pay) == set(plain) and pay["image_array"] is MOSAIC
            for k in pay:
                if k not in ("demosaic", "image_array"):
                    assert pay[k] == plain[k], k


def test_both_gates_ask_for_the_denoise_last():
    big = np.zeros((1 << 13, 1 << 13), np.uint16)
    samples = 3 << 26
    assert mosaic_rejection(True, 0, False, samples) is None and mosaic_rejection(True, 0, False, samples, denoise=False) is None
    why = mosaic_rejection(True, 0, False, samples, denoise=True)
    assert why is not None and why.startswith("the demosaic step (raw_profile): ") and "raw_denoise" in why
    levels = mosaic_rejection(True, 0, False, samples, levels=True)
    assert mosaic_rejection(True, 0, False, samples, levels=True, denoise=True) == levels != why
    kw = dict(stops=True, rotate_times=0, frame_samples=samples)
    assert host_stream_gate(big, 16, 0.0, 0, "No", 0.0, False, True, **kw) is None
    assert host_stream_gate(big, 16, 0.0, 0, "No", 0.0, False, True, denoise=True, **kw) == why
    assert host_stream_gate(big, 16, 0.0, 0, "No", 0.0, False, True, levels=True, denoise=True, **kw) == levels
    assert host_stream_gate(np.zeros((1 << 12, 1 << 12, 3), np.uint16), 16, denoise=True) is None  # (no mosaic)
    for args in ((False, 0, False, samples), (True, 1, False, samples), (True, 0, True, samples), (True, 0, False, None), (True, 0, False, 99),
                 (True, 0, False, samples, True), (True, 0, False, samples, False, 3)):
        assert mosaic_rejection(*args, denoise=True) == mosaic_rejection(*args) is not None
    assert host_stream_gate(big, 1, denoise=True, demosaic=True, **kw) == "stream_bands = 1"
    assert host_stream_gate(big, 16, 2.5, demosaic=True, denoise=True, **kw) == host_stream_gate(big, 16, 2.5, demosaic=True, **kw) is not None


def test_the_payloads_gate_refuses_a_denoise_last(proc, monkeypatch):
    dn = WaveletDenoise(100.0, 16383)
    pay = proc.extract_image_data_cpu(MOSAIC, raw_profile=NUMERIC, raw_denoise=dn, exposure=0.5)
    plain = proc.extract_image_data_cpu(MOSAIC, raw_profile=NUMERIC, exposure=0.5)
    args = ((96, 144), "torch.int16", False, "gpu")
    assert stream_rejection(pay, *args) == stream_rejection(plain, *args) and "below 16.7 M" in stream_rejection(pay, *args)
    monkeypatch.setattr("raw2film_amd.payload.STREAM_MIN_SAMPLES", 1)  # a frame that otherwise streams
    assert stream_rejection(plain, *args) is None
    why = stream_rejection(pay, *args)
    assert why is not None and why.startswith("the demosaic step (raw_profile): ") and "raw_denoise" in why


def test_the_keyword_is_a_load_keyword_of_every_entry():
    import inspect

    assert "raw_denoise" in hip_processor._LOAD_KEYWORDS
    for name in ("process", "extract_image_data_cpu", "load_image_texture"):
        assert inspect.signature(getattr(HipProcessor, name)).parameters["raw_denoise"].default is None, name


def test_a_changed_record_invalidates_the_image_cache_and_an_equal_one_does_not(proc):
    uploads = []

    def prepare(payload):
        uploads.append(payload.get("demosaic"))
        proc._texture = ("frame", None, {})
        proc.image_param_dict = None

    proc.prepare_gpu_textures = prepare
    proc._texture = proc._texture_src = proc.image_param_dict = None
    proc.profile_stages = False
    proc.load_image_texture(MOSAIC, raw_profile=NUMERIC, raw_denoise=WaveletDenoise(100.0, 16383), exposure=0.0)
    proc.load_image_texture(MOSAIC, raw_profile=NUMERIC, raw_denoise=WaveletDenoise(100, 16383), exposure=0.0)
    assert len(uploads) == 1 and uploads[0]["denoise"] == WaveletDenoise(100.0, 16383)
    proc.load_image_texture(MOSAIC, raw_profile=NUMERIC, raw_denoise=WaveletDenoise(101.0, 16383), exposure=0.0)
    proc.load_image_texture(MOSAIC, raw_profile=NUMERIC, raw_denoise=WaveletDenoise(101.0, 16000), exposure=0.0)
    proc.load_image_texture(MOSAIC, raw_profile=NUMERIC, exposure=0.0)
    assert len(uploads) == 4 and "denoise" not in uploads[3]
