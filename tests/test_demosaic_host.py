"""The Bayer demosaic's host half, without a GPU: the NumPy model of the definition (tests/demosaic_model.py) in its two forms, the
planner (raw2film_amd/csrc/r2f_demosaic_plan.cpp) and the shared arithmetic (r2f_demosaic_math.h) in a stand-alone program under
AddressSanitizer / UBSan (tests/demosaic_check.cpp), RawProfile's validation, the payload of phase 1 and the ABI structs.

The bit-for-bit comparison of the program's renders with the model pins the arithmetic the GPU runs, on this machine: the same
text compiled for the CPU with contraction off.  That the device compiles it to the same bytes is tests/test_gpu_demosaic.py's."""

import ctypes
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import demosaic_model as dm
from raw2film_amd import _lib
from raw2film_amd.hip_processor import HipProcessor
from raw2film_amd.payload import host_stream_gate, stream_rejection
from raw2film_amd.raw import RawProfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raw2film_amd", "csrc")
SMALL = [(2, 2), (3, 5), (6, 6), (7, 7), (8, 9), (13, 18)]


# ---- the model
@pytest.mark.parametrize("pattern", dm.PATTERNS)
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_vectorised_model_equals_the_sequential_one(pattern, shape):
    for kind in dm.KINDS:
        mosaic, prof = dm.fixture(kind, pattern, *shape)
        assert np.array_equal(dm.demosaic(mosaic, prof), dm.demosaic(mosaic, prof, sequential=True)), kind


# (kind -> the counters it is there for; every one must be above zero on a 33 x 130 frame of every pattern)
EXERCISES = {
    "random": ("b1_vertical", "b1_horizontal", "b1_clamp_low", "b1_clamp_high", "a_negative", "a_clip_65535", "c_clip_0", "c_clip_65535"),
    "flat": ("b1_tie", "b3_tie"),
    "checker": ("b23_clip_0", "b23_clip_65535"),
    "black": ("a_negative",),
    "negative-row": ("c_clip_0", "c_clip_65535"),
}


@pytest.mark.parametrize("pattern", dm.PATTERNS)
def test_fixtures_are_not_vacuous(pattern):
    for kind, wanted in EXERCISES.items():
        stats = {}
        mosaic, prof = dm.fixture(kind, pattern, 33, 130)
        out = dm.demosaic(mosaic, prof, stats=stats)
        assert out.shape == (33, 130, 3) and out.dtype == np.uint16
        assert [k for k in wanted if stats.get(k, 0) <= 0] == [], (kind, stats)
    mosaic, prof = dm.fixture("black", pattern, 33, 130)
    assert int(mosaic.max()) < max(prof.black)  # a black level above every sample


def test_step_b_stays_inside_16_bits_before_its_clips_are_needed_on_plain_frames():
    """Near-flat mosaics stay inside [0, 65535] without B2 / B3's clips (the clips are there for the others)."""
    for pattern in dm.PATTERNS:
        stats = {}
        dm.demosaic(*dm.fixture("flat", pattern, 33, 130), stats=stats)
        assert stats["b23_clip_0"] == 0 and stats["b23_clip_65535"] == 0


def test_half_size_is_the_quad_rule():
    mosaic, _ = dm.fixture("random", "GRBG", 6, 8)
    out = dm.demosaic(mosaic, RawProfile("GRBG"), half_size=True)
    m = mosaic.astype(np.int64)
    assert out.shape == (3, 4, 3)
    assert np.array_equal(out[..., 0], m[0::2, 1::2]) and np.array_equal(out[..., 2], m[1::2, 0::2])
    assert np.array_equal(out[..., 1], (m[0::2, 0::2] + m[1::2, 1::2]) >> 1)


# ---- the stand-alone program
@pytest.fixture(scope="module")
def demosaic_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("demosaic_check") / "demosaic_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
           "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "demosaic_check.cpp"), os.path.join(CSRC, "r2f_demosaic_plan.cpp"),
           "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


@pytest.mark.parametrize("seed", [1, 2, 20261019])
def test_planner_fuzz_is_clean_under_the_sanitizers(demosaic_check, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([demosaic_check, "fuzz", str(seed), "20000"], capture_output=True, text=True, env=env, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    assert "cases ok" in res.stdout


def _render(binary, tmp_path, mosaic, profile, half_size):
    H, W = mosaic.shape
    job, out = str(tmp_path / "job.bin"), str(tmp_path / "out.bin")
    with open(job, "wb") as f:
        f.write(np.array([H, W, int(half_size)], dtype=np.int32).tobytes())
        f.write(bytes(profile.to_c()))
        f.write(np.ascontiguousarray(mosaic, dtype=np.uint16).tobytes())
    res = subprocess.run([binary, "render", job, out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    raw = open(out, "rb").read()
    n = ctypes.sizeof(_lib.DemosaicParams)
    params = _lib.DemosaicParams.from_buffer_copy(raw[:n])
    return params, np.frombuffer(raw[n:], dtype=np.uint16).reshape(params.out_h, params.out_w, 3)


def _same_constants(a, b):
    return (a.cfa == b.cfa and np.array_equal(a.black, b.black) and np.array_equal(a.mul.view(np.uint32), b.mul.view(np.uint32))
            and np.array_equal(a.M.view(np.uint32), b.M.view(np.uint32)) and (a.half_size, a.out_h, a.out_w) == (b.half_size, b.out_h, b.out_w))


@pytest.mark.parametrize("pattern", dm.PATTERNS)
def test_shared_arithmetic_renders_the_model_bit_for_bit(demosaic_check, tmp_path, pattern):
    for shape in SMALL + [(33, 130), (65, 67)]:
        for kind in dm.KINDS:
            mosaic, prof = dm.fixture(kind, pattern, *shape)
            params, got = _render(demosaic_check, tmp_path, mosaic, prof, False)
            assert _same_constants(dm.from_params(params), dm.constants(prof, *shape)), (kind, shape)
            assert np.array_equal(got, dm.demosaic(mosaic, prof)), (kind, shape)
    for shape in [(2, 2), (4, 6), (66, 130)]:
        for kind in dm.KINDS:
            mosaic, prof = dm.fixture(kind, pattern, *shape)
            params, got = _render(demosaic_check, tmp_path, mosaic, prof, True)
            assert _same_constants(dm.from_params(params), dm.constants(prof, *shape, half_size=True)), (kind, shape)
            assert np.array_equal(got, dm.demosaic(mosaic, prof, half_size=True)), (kind, shape)


# ---- the planner
def test_planner_refuses_every_item_of_its_list():
    lib = _lib.load()
    out = _lib.DemosaicParams()

    def plan(H=40, W=60, **changes):
        p = RawProfile("GRBG", black=64, multipliers=(2.0, 1.0, 1.5), matrix=dm.CAMERA).to_c()
        for k, v in changes.items():
            if isinstance(v, tuple):
                getattr(p, k)[v[0]] = v[1]
            else:
                setattr(p, k, v)
        return lib.r2f_demosaic_plan(ctypes.byref(p), H, W, ctypes.byref(out))

    assert plan() == _lib.OK and plan(half_size=1) == _lib.OK and plan(2, 2) == _lib.OK
    assert (out.out_h, out.out_w, out.half_size) == (2, 2, 0)
    nan, inf = float("nan"), float("inf")
    bad = [dict(pattern=4), dict(pattern=-1), dict(H=1), dict(W=1), dict(H=0), dict(H=41, half_size=1), dict(W=61, half_size=1),
           dict(black=(0, nan)), dict(black=(3, inf)), dict(black=(1, -1.0)), dict(black=(2, 65536.0)), dict(black=(0, 12.5)),
           dict(mul=(0, nan)), dict(mul=(1, inf)), dict(mul=(2, 0.0)), dict(mul=(3, -1.0)), dict(mul=(0, 1024.5)), dict(mul=(0, 1e-60)),
           dict(matrix=(0, nan)), dict(matrix=(8, -inf)), dict(matrix=(4, 64.5)), dict(matrix=(5, -64.5))]
    for b in bad:
        assert plan(**b) == _lib.EINVAL, b
    for ok in (dict(black=(0, 65535.0)), dict(mul=(0, 1024.0)), dict(matrix=(4, -64.0)), dict(matrix=(0, 64.0))):
        assert plan(**ok) == _lib.OK, ok
    assert lib.r2f_demosaic_plan(None, 40, 60, ctypes.byref(out)) == _lib.EINVAL


def test_the_bounds_keep_every_truncation_inside_int32():
    """Step A: |t * mul| <= 65535 * 1024 < 2^27.  Step C: three products of at most 64 * 65535 each < 2^24 in sum; float32's rounding
    adds at most a few ulps of 2^24 to that."""
    assert 65535 * 1024 < 2 ** 27 and 3 * 64 * 65535 < 2 ** 24
    prof = RawProfile("RGGB", black=0, multipliers=(1024.0,) * 3, matrix=((64.0,) * 3, (-64.0,) * 3, (64.0, -64.0, 64.0)))
    full = np.full((8, 8), 65535, np.uint16)
    out = dm.demosaic(full, prof)
    assert np.array_equal(out[..., 0], np.full((8, 8), 65535)) and not out[..., 1].any()


# ---- ABI
def test_struct_layouts_match_the_header():
    P, R = _lib.RawProfile, _lib.DemosaicParams
    assert ctypes.sizeof(P) == 144
    assert [getattr(P, f).offset for f in ("pattern", "half_size", "black", "mul", "matrix")] == [0, 4, 8, 40, 72]
    assert ctypes.sizeof(R) == 96
    assert [getattr(R, f).offset for f in ("cfa", "black", "mul", "M", "half_size", "out_h", "out_w")] == [0, 16, 32, 48, 84, 88, 92]
    text = open(os.path.join(ROOT, "include", "r2f.h")).read()
    body = text[text.index("typedef struct r2f_demosaic_params {"):text.index("} r2f_demosaic_params;")]
    order = [body.index(w) for w in ("int32_t cfa[4];", "int32_t black[4];", "float mul[4];", "float M[9];", "int32_t half_size, out_h, out_w;")]
    assert order == sorted(order)
    body = text[text.index("typedef struct r2f_raw_profile {"):text.index("} r2f_raw_profile;")]
    order = [body.index(w) for w in ("int32_t pattern, half_size;", "double black[4];", "double mul[4];", "double matrix[9];")]
    assert order == sorted(order)
    assert f"R2F_DEMOSAIC_TILE_W = {dm.TILE_W}, R2F_DEMOSAIC_TILE_H = {dm.TILE_H}" in text
    assert (_lib.DEMOSAIC_TILE_W, _lib.DEMOSAIC_TILE_H) == (dm.TILE_W, dm.TILE_H)
    assert "UNPINNED" in text[text.index("Demosaic of a Bayer frame"):text.index("enum { R2F_CFA_RGGB")]


# ---- RawProfile
def test_profile_is_frozen_and_hashable():
    a = RawProfile("GRBG", black=[64, 64, 64, 64], multipliers=[2.0, 1.0, 1.5], matrix=np.array(dm.CAMERA))
    b = RawProfile("GRBG", black=64, multipliers=(1.0, 2.0, 1.5, 1.0), matrix=dm.CAMERA)  # (per site: G R B G)
    assert a == b and hash(a) == hash(b) and a != RawProfile("GRBG", black=65, multipliers=(2.0, 1.0, 1.5), matrix=dm.CAMERA)
    assert a != RawProfile("RGGB", black=64, multipliers=(2.0, 1.0, 1.5), matrix=dm.CAMERA)
    with pytest.raises(Exception):
        a.pattern = "RGGB"
    assert {a: 1}[b] == 1
    assert RawProfile("BGGR", multipliers=(3.0, 1.0, 2.0)).multipliers == (2.0, 1.0, 1.0, 3.0)


@pytest.mark.parametrize("kw", [
    dict(pattern="XTRANS"), dict(pattern=0), dict(pattern="rggb"), dict(black=-1), dict(black=65536), dict(black=12.5), dict(black=float("nan")),
    dict(black=(1, 2, 3)), dict(black="64"), dict(multipliers=(1.0, 1.0)), dict(multipliers=(1.0, 0.0, 1.0)), dict(multipliers=(1.0, -2.0, 1.0)),
    dict(multipliers=(1.0, 1024.5, 1.0)), dict(multipliers=(1.0, float("inf"), 1.0)), dict(multipliers=2.0),
    dict(matrix=((1, 0, 0), (0, 1, 0))), dict(matrix=((1, 0), (0, 1), (0, 0))), dict(matrix=((1, 0, 0), (0, 65, 0), (0, 0, 1))),
    dict(matrix=((1, 0, 0), (0, float("nan"), 0), (0, 0, 1))), dict(matrix=3.0),
])
def test_profile_validation_raises_before_any_work(kw):
    with pytest.raises(ValueError):
        RawProfile(**kw)


def test_plan_refusals_surface_as_value_errors():
    p = RawProfile("RGGB")
    for H, W, half in ((1, 8, False), (8, 1, False), (7, 8, True), (8, 9, True)):
        with pytest.raises(ValueError, match="r2f_demosaic_plan"):
            p.plan(H, W, half)
    with pytest.raises(ValueError, match="r2f_demosaic_plan"):
        RawProfile("RGGB", multipliers=(1e-60, 1.0, 1.0)).plan(8, 8)  # (rounds to 0 as a float)
    q = p.plan(8, 10, True)
    assert (q.out_h, q.out_w, q.half_size) == (4, 5, 1)


# ---- phase 1 of the processor
@pytest.fixture
def proc():
    p = HipProcessor.__new__(HipProcessor)
    p.cameras = p.lenses = None
    p.payload_alpha = True
    return p


MOSAIC, PROFILE = dm.fixture("random", "GRBG", 96, 144)
CROP_KEYS = ("final_resolution", "output_resolution", "canvas_resolution", "pipeline_resolution", "resize_to", "upscale_to", "chroma_nr",
             "u16_factor", "u16_window", "exposure_root")


@pytest.mark.parametrize("kw", [
    dict(exposure=0.5), dict(exposure=0.5, half_size=False), dict(exposure=-1.0, zoom=1.3, rotate_times=1), dict(exposure=0.0, rotation=3.5, zoom=1.2),
    dict(exposure="device", zoom=1.3), dict(exposure=None), dict(exposure=0.25, flip=True, frame_width=36, frame_height=36),
    dict(exposure=0.5, resolution=(30, 45), canvas_mode="Uniform white", canvas_scale=1.1), dict(exposure=0.5, rotate_times=3, max_scale=1.0),
])
def test_payload_is_the_mosaic_with_the_crop_numbers_of_the_demosaiced_frame(proc, kw):
    half = kw.get("half_size", True)
    rgb = dm.demosaic(MOSAIC, PROFILE, half_size=half)
    pay = proc.extract_image_data_cpu(MOSAIC, raw_profile=PROFILE, **kw)
    plain = proc.extract_image_data_cpu(rgb, **dict(kw, exposure="device" if kw["exposure"] is None else kw["exposure"]))
    assert set(pay) == set(plain) | {"demosaic"} and "demosaic" not in plain
    assert pay["image_array"] is MOSAIC  # 2 bytes per pixel go up, the caller's array itself
    step = pay["demosaic"]
    assert set(step) == {"params", "window", "rotate_times"}
    assert (step["params"].out_h, step["params"].out_w, step["params"].half_size) == (rgb.shape[0], rgb.shape[1], int(half))
    for k in CROP_KEYS:
        assert pay[k] == plain[k], k
    assert (pay["warp"] is None) == (plain["warp"] is None)
    if pay["warp"] is not None:
        assert pay["warp"]["window"] == plain["warp"]["window"] and pay["warp"]["rotate_times"] == plain["warp"]["rotate_times"]
    # window and quarter turns applied to the demosaiced frame give the frame the plain call uploads
    if plain["u16_window"] is None:
        r0, c0, nr, nc = step["window"]
        assert np.array_equal(np.rot90(rgb[r0:r0 + nr, c0:c0 + nc], k=step["rotate_times"]), plain["image_array"])
    else:
        assert step["window"] is None and step["rotate_times"] == 0 and plain["image_array"].shape == rgb.shape


def test_a_mosaic_without_stops_where_the_device_measurement_is_refused_raises(proc):
    for kw in (dict(rotation=2.0), dict(rotate_times=1), dict(exposure="device", rotate_times=2)):
        with pytest.raises(ValueError, match="turned or rotated"):
            proc.extract_image_data_cpu(MOSAIC, raw_profile=PROFILE, **kw)
    proc.extract_image_data_cpu(MOSAIC, raw_profile=PROFILE, exposure=0.0, rotate_times=1, rotation=2.0)


def test_two_dimensions_without_a_profile_and_three_with_one_raise(proc):
    with pytest.raises(ValueError, match=r"\(H, W, 3\|4\)"):
        proc.extract_image_data_cpu(MOSAIC)
    rgb = dm.demosaic(MOSAIC, PROFILE)
    with pytest.raises(ValueError, match="mosaic"):
        proc.extract_image_data_cpu(rgb, raw_profile=PROFILE, exposure=0.0)
    with pytest.raises(ValueError, match="mosaic"):
        proc.extract_image_data_cpu(MOSAIC.astype(np.float32), raw_profile=PROFILE, exposure=0.0)
    with pytest.raises(ValueError, match="raw_profile"):
        proc.extract_image_data_cpu(MOSAIC, raw_profile={"pattern": "RGGB"}, exposure=0.0)
    with pytest.raises(ValueError, match="r2f_demosaic_plan"):
        proc.extract_image_data_cpu(MOSAIC[:95], raw_profile=PROFILE, exposure=0.0)  # an odd frame at half size


def test_both_stream_refusals_name_the_demosaic_step(proc):
    pay = proc.extract_image_data_cpu(MOSAIC, raw_profile=PROFILE, exposure=0.5)
    why = stream_rejection(pay, (8192, 8192), "torch.int16", False, "gpu")
    assert why is not None and "demosaic" in why
    big = np.zeros((1 << 13, 1 << 13), np.uint16)
    why = host_stream_gate(big, 16, 0.0, 0, "No", 0.0, False, True)
    assert why is not None and "demosaic" in why
    assert host_stream_gate(np.zeros((1 << 12, 1 << 12, 3), np.uint16), 16, 0.0, 0, "No", 0.0, False, False) is None


def test_every_settings_forwarder_takes_the_keyword():
    for name in ("process", "extract_image_data_cpu", "load_image_texture"):
        assert inspect.signature(getattr(HipProcessor, name)).parameters["raw_profile"].default is None, name
    for name in ("process_preloaded", "process_preloaded_jpeg", "process_preloaded_tiff", "process_jpeg", "process_tiff", "submit_preloaded"):
        params = inspect.signature(getattr(HipProcessor, name)).parameters.values()
        assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in params), name  # (settings are forwarded whole)
    from raw2film_amd import hip_processor

    assert "raw_profile" in hip_processor._LOAD_KEYWORDS  # (process, process_jpeg and process_tiff hand it to phase 1)


def test_a_changed_profile_invalidates_the_image_cache_and_an_equal_one_does_not(proc):
    uploads = []

    def prepare(payload):
        uploads.append(payload.get("demosaic"))
        proc._texture = ("frame", None, {})
        proc.image_param_dict = None

    proc.prepare_gpu_textures = prepare
    a = RawProfile("GRBG", black=64, multipliers=(2.0, 1.0, 1.5))
    proc.load_image_texture(MOSAIC, raw_profile=a, exposure=0.0)
    proc.load_image_texture(MOSAIC, raw_profile=RawProfile("GRBG", black=[64] * 4, multipliers=[2.0, 1.0, 1.5]), exposure=0.0)
    assert len(uploads) == 1 and uploads[0] is not None
    proc.load_image_texture(MOSAIC, raw_profile=RawProfile("GRBG", black=65, multipliers=(2.0, 1.0, 1.5)), exposure=0.0)
    assert len(uploads) == 2
    proc.load_image_texture(MOSAIC, raw_profile=a, exposure=0.0, half_size=False)
    assert len(uploads) == 3 and uploads[2]["params"].half_size == 0
    proc.load_image_texture(MOSAIC, raw_profile=a, exposure=0.0, half_size=False)
    assert len(uploads) == 3
