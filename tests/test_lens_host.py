"""The lens correction's host half, without a GPU: the planner (raw2film_amd/csrc/r2f_lens_plan.cpp) and the shared arithmetic
(r2f_lens_math.h) in a stand-alone program under AddressSanitizer / UBSan (tests/lens_check.cpp), the NumPy model of the
definition (tests/lens_model.py), LensProfile's validation, the payload of phase 1 and the ABI structs.

The bit-for-bit comparison of the program's renders with the model pins the arithmetic the GPU runs, on this machine: the same
text compiled for the CPU with contraction off.  That the device compiles it to the same roundings is tests/test_gpu_lens.py's."""

import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import lens_model as lm
from raw2film_amd import _lib
from raw2film_amd.hip_processor import HipProcessor
from raw2film_amd.payload import host_stream_gate, stream_rejection
from raw2film_amd.lens import LensProfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raw2film_amd", "csrc")


@pytest.fixture(scope="module")
def lens_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("lens_check") / "lens_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
           "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "lens_check.cpp"), os.path.join(CSRC, "r2f_lens_plan.cpp"),
           os.path.join(CSRC, "r2f_plan.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


@pytest.mark.parametrize("seed", [1, 2, 20261018])
def test_planner_and_decision_are_clean_under_the_sanitizers(lens_check, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([lens_check, "fuzz", str(seed), "20000"], capture_output=True, text=True, env=env, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    assert "cases ok" in res.stdout


def _render(binary, tmp_path, image, profile, window=None):
    H, W, C = image.shape
    r0, c0, nr, nc = (0, 0, H, W) if window is None else window
    job, out = str(tmp_path / "job.bin"), str(tmp_path / "out.bin")
    with open(job, "wb") as f:
        f.write(np.array([H, W, C, r0, c0, nr, nc], dtype=np.int32).tobytes())
        f.write(bytes(profile.to_c()))
        f.write(np.ascontiguousarray(image, dtype=np.float32).tobytes())
    res = subprocess.run([binary, "render", job, out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    raw = open(out, "rb").read()
    params = _lib.LensParams.from_buffer_copy(raw[:ctypes.sizeof(_lib.LensParams)])
    return params, np.frombuffer(raw[ctypes.sizeof(_lib.LensParams):], dtype=np.float32).reshape(nr, nc, 3)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("shape", lm.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shared_arithmetic_renders_the_model_bit_for_bit(lens_check, tmp_path, shape):
    H, W = shape
    for name in lm.PROFILE_SPECS:
        prof = lm.profile(name)
        image = lm.frame(H, W, 4 if name == "poly5" else 3)  # (a fourth channel is ignored)
        params, got = _render(lens_check, tmp_path, image, prof)
        # the planner's constants are the definition's, rounded from double
        want_c, have_c = lm.rounded(lm.constants(prof, H, W)), lm.from_params(params)
        for field in ("cx", "cy", "q", "inv_scale", "c0", "qv"):
            assert _bits(getattr(want_c, field)) == _bits(getattr(have_c, field)), (name, field)
        assert [_bits(x) for x in want_c.k] == [_bits(x) for x in have_c.k] and [_bits(x) for x in want_c.v] == [_bits(x) for x in have_c.v]
        assert (have_c.model, have_c.vignetting, have_c.scale) == (want_c.model, want_c.vignetting, want_c.scale)
        want = lm.correct(image, want_c)
        assert np.array_equal(_bits(got), _bits(want)), (name, shape, int((_bits(got) != _bits(want)).sum()))
    # a window that straddles every edge, and one wholly outside the frame
    prof = lm.profile("off-centre")
    image = lm.frame(H, W)
    c = lm.rounded(lm.constants(prof, H, W))
    for window in ((-5, -6, H + 11, W + 9), (H + 40, -W - 50, 5, 7)):
        _, got = _render(lens_check, tmp_path, image, prof, window)
        assert np.array_equal(_bits(got), _bits(lm.correct(image, c, window))), window


def test_the_none_profile_at_scale_one_is_the_identity():
    image = lm.frame(33, 47)
    out = lm.correct(image, lm.rounded(lm.constants(lm.profile("none"), 33, 47)))
    assert np.array_equal(out, image)  # phase 0 is the unit tap


@pytest.mark.parametrize("shape", [(33, 47), (96, 128), (150, 210)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_float32_model_against_the_float64_evaluation(shape):
    """The float32 model against the same definition in float64 with unrounded constants.  A pixel whose 1/32 phase (or tap
    origin) differs between the two samples another set of weights and is left out; the share of such pixels may not exceed 2e-3.
    Every other sample lies within the running error bound gamma_66 * sum |w v| of its 64-term sum; with vignetting the bound is
    divided by the gain's denominator and gamma_16 |o| is added for the gain itself (qv, three coefficients, five operations
    to rv2, six to the denominator, one division: at most 16 roundings)."""
    H, W = shape
    for name in lm.PROFILE_SPECS:
        prof, image = lm.profile(name), lm.frame(H, W)
        c64 = lm.constants(prof, H, W)
        o32, d32 = lm.correct(image, lm.rounded(c64), want_bound=True)
        o64, d64 = lm.evaluate64(image, c64)
        same = (d32.inside == d64.inside) & (d32.fx == d64.fx) & (d32.fy == d64.fy) & (d32.ix == d64.ix) & (d32.iy == d64.iy)
        share = 1.0 - same.mean()
        print(f"{name} {H}x{W}: phase differs on {share:.2e} of the pixels")
        assert share <= 2e-3, (name, shape, share)
        bound = lm.gamma(66) * d64.sum_abs
        if d64.den is not None:
            bound = bound / np.abs(d64.den)[..., None] + lm.gamma(16) * np.abs(o64)
        err = np.abs(o32.astype(np.float64) - o64)
        ok = err <= bound
        print(f"{name} {H}x{W}: largest error / bound {np.max(np.where(same[..., None] & (bound > 0), err / np.maximum(bound, 1e-300), 0)):.3f}")
        assert bool(ok[same].all()), (name, shape, float((err - bound)[same].max()))


# (an off-centre optical centre lies outside a frame one pixel wide: no scale fits, which the next test covers)
@pytest.mark.parametrize("name,shape", [(n, s) for n in ("ptlens", "poly3", "poly5", "off-centre")
                                        for s in ((33, 47), (150, 210), (4000, 6000), (64, 1)) if (n, s) != ("off-centre", (64, 1))])
def test_auto_scale_puts_every_probe_on_or_inside_the_boundary(name, shape):
    """All eight probes land inside the frame -- to the resolution of a double at frame coordinates, 1e-9 px: the planner's
    bisection ends between neighbouring doubles, this check evaluates the map once more -- and at scale * (1 - 1e-6) one does not."""
    H, W = shape
    spec = dict(lm.PROFILE_SPECS[name], scale="auto")
    prof = LensProfile(**spec)
    scale = prof.plan(H, W).scale
    assert 1 / 16 < scale < 16
    assert lm.probes_reach(prof, H, W, scale) <= 1e-9
    assert lm.probes_reach(prof, H, W, scale * (1 - 1e-6)) > 0
    # the resolved scale is what the constants are made from
    want = lm.rounded(lm.constants(prof, H, W, scale))
    have = lm.from_params(prof.plan(H, W))
    assert (_bits(want.q), _bits(want.inv_scale)) == (_bits(have.q), _bits(have.inv_scale))


def test_auto_scale_without_a_fitting_scale_is_refused():
    with pytest.raises(ValueError, match="r2f_lens_plan"):
        LensProfile("poly3", (-40.0,), scale="auto").plan(100, 150)  # (the view would have to shrink more than 16 times)
    with pytest.raises(ValueError, match="r2f_lens_plan"):
        LensProfile(**dict(lm.PROFILE_SPECS["off-centre"], scale="auto")).plan(64, 1)  # the centre is outside
    assert LensProfile("none", scale="auto").plan(1, 1).scale == 1.0  # nothing can leave a 1 x 1 frame


def test_phase_table_is_the_oracles():
    tab = np.zeros((32, 8), dtype=np.float32)
    assert _lib.load().r2f_lens_phase_table(tab.ctypes.data) == 0
    assert np.array_equal(_bits(tab), _bits(lm.phase_table()))


# ---- LensProfile
def test_profile_is_frozen_and_hashable():
    a = LensProfile("ptlens", [0.02, -0.06, 0.01], vignetting=[-0.3, 0.1, -0.02], center=[0.01, 0])
    b = LensProfile("ptlens", (0.02, -0.06, 0.01), vignetting=(-0.3, 0.1, -0.02), center=(0.01, 0.0))
    assert a == b and hash(a) == hash(b) and a != LensProfile("ptlens", (0.02, -0.06, 0.011))
    with pytest.raises(Exception):
        a.scale = 2.0
    assert {a: 1}[b] == 1


@pytest.mark.parametrize("kw", [
    dict(distortion="fisheye"), dict(distortion=3), dict(distortion="poly3"), dict(distortion="poly3", coefficients=(0.1, 0.2)),
    dict(distortion="none", coefficients=(0.1,)), dict(distortion="ptlens", coefficients=(0.1, 0.2)),
    dict(distortion="poly5", coefficients=(0.1, float("nan"))), dict(distortion="poly3", coefficients=(float("inf"),)),
    dict(vignetting=(0.1, 0.2)), dict(vignetting=(0.1, 0.2, float("nan"))), dict(center=(0.0,)), dict(center=(0.0, float("inf"))),
    dict(scale=0), dict(scale=-1.0), dict(scale=float("nan")), dict(scale="fit"), dict(norm_radius_px=0), dict(norm_radius_px=float("inf")),
    dict(coefficients=3.0, distortion="poly3"),
])
def test_profile_validation_raises_before_any_work(kw):
    with pytest.raises(ValueError):
        LensProfile(**kw)


def test_planner_refuses_what_the_profile_refuses():
    lib = _lib.load()
    out = _lib.LensParams()

    def plan(**changes):
        p = LensProfile("poly5", (0.03, -0.01), vignetting=(-0.3, 0.1, -0.02)).to_c()
        for k, v in changes.items():
            if isinstance(v, tuple):
                getattr(p, k)[:] = v
            else:
                setattr(p, k, v)
        return lib.r2f_lens_plan(ctypes.byref(p), 40, 60, ctypes.byref(out))

    assert plan() == _lib.OK
    nan, inf = float("nan"), float("inf")
    for bad in (dict(model=4), dict(model=-1), dict(n_coef=1), dict(n_coef=3), dict(coef=(0.1, nan, 0.0)), dict(vignetting=(inf, 0.0, 0.0)),
                dict(center=(nan, 0.0)), dict(scale=0.0), dict(scale=-2.0), dict(scale=nan), dict(norm_radius_px=-1.0),
                dict(norm_radius_px=nan)):
        assert plan(**bad) == _lib.EINVAL, bad
    assert plan(scale=nan, auto_scale=1) == _lib.OK  # (the given scale is not read then)
    p = LensProfile().to_c()
    assert lib.r2f_lens_plan(ctypes.byref(p), 0, 60, ctypes.byref(out)) == _lib.EINVAL
    assert lib.r2f_lens_plan(None, 40, 60, ctypes.byref(out)) == _lib.EINVAL


# ---- ABI
def test_struct_layouts_match_the_header():
    P, R = _lib.LensProfile, _lib.LensParams
    assert ctypes.sizeof(P) == 96
    assert [getattr(P, f).offset for f in ("model", "n_coef", "coef", "has_vignetting", "auto_scale", "vignetting", "center", "scale",
                                           "norm_radius_px")] == [0, 4, 8, 32, 36, 40, 64, 80, 88]
    assert ctypes.sizeof(R) == 64
    assert [getattr(R, f).offset for f in ("model", "vignetting", "cx", "cy", "q", "inv_scale", "c0", "k", "qv", "v", "scale")] == [
        0, 4, 8, 12, 16, 20, 24, 28, 40, 44, 56]
    text = open(os.path.join(ROOT, "include", "r2f.h")).read()
    body = text[text.index("typedef struct r2f_lens_params {"):text.index("} r2f_lens_params;")]
    assert [w for w in ("model", "vignetting", "cx", "cy", "q", "inv_scale", "c0", "k[3]", "qv", "v[3]", "scale") if w not in body] == []
    order = [body.index(w) for w in ("int32_t model, vignetting;", "float cx, cy, q, inv_scale, c0;", "float k[3];", "float qv;", "float v[3];",
                                     "double scale;")]
    assert order == sorted(order)


# ---- phase 1 of the processor
@pytest.fixture
def proc():
    p = HipProcessor.__new__(HipProcessor)
    p.cameras = p.lenses = None
    p.payload_alpha = True
    return p


PROFILE = LensProfile("ptlens", (0.02, -0.06, 0.01), vignetting=(-0.3, 0.1, -0.02), scale=1.02)
CROP_KEYS = ("final_resolution", "output_resolution", "canvas_resolution", "pipeline_resolution", "resize_to", "upscale_to", "chroma_nr")


@pytest.mark.parametrize("kw", [
    dict(), dict(zoom=1.3, rotate_times=1), dict(rotation=3.5, zoom=1.3, rotate_times=1), dict(flip=True, frame_width=36, frame_height=36),
    dict(resolution=(60, 90), canvas_mode="Uniform white", canvas_scale=1.1), dict(rotate_times=3, max_scale=2.0),
])
def test_payload_keeps_the_whole_frame_and_the_crop_numbers(proc, kw):
    img = lm.frame(150, 210)
    plain = proc.extract_image_data_cpu(img, lens_correction=True, **kw)
    pay = proc.extract_image_data_cpu(img, lens_correction=True, lens_profile=PROFILE, **kw)
    assert set(pay) == set(plain) | {"lens"} and "lens" not in plain
    assert set(pay["lens"]) == {"params", "window", "rotate_times"}
    assert pay["image_array"].shape[:2] == (150, 210) and np.array_equal(pay["image_array"][..., :3], img)  # upstream corrects before any crop
    for k in CROP_KEYS:
        assert pay[k] == plain[k], k
    have = lm.from_params(pay["lens"]["params"])
    want = lm.rounded(lm.constants(PROFILE, 150, 210))
    assert (_bits(have.cx), _bits(have.cy), _bits(have.q)) == (_bits(want.cx), _bits(want.cy), _bits(want.q))
    # the window is what the aspect crop keeps (and the zoom crop when there is no rotation)
    from raw2film_amd import geometry

    aspect = kw.get("frame_width", 36) / kw.get("frame_height", 24)
    r0, c0, nr, nc = geometry.crop_box(150, 210, 1, aspect, kw.get("flip", False))
    if kw.get("rotation"):
        assert pay["lens"]["window"] == (r0, c0, nr, nc) and pay["lens"]["rotate_times"] == 0
        assert pay["warp"]["window"] == plain["warp"]["window"] and pay["warp"]["rotate_times"] == plain["warp"]["rotate_times"]
    else:
        z = geometry.crop_box(nr, nc, kw.get("zoom", 1.0), aspect, False)
        assert pay["lens"]["window"] == (r0 + z[0], c0 + z[1], z[2], z[3]) and pay["warp"] is None
        assert pay["lens"]["rotate_times"] == kw.get("rotate_times", 0) % 4
        # ... so that the plain call's frame is that window of the uncorrected frame, turned
        w = pay["lens"]["window"]
        assert np.array_equal(np.rot90(img[w[0]:w[0] + w[2], w[1]:w[1] + w[3]], k=pay["lens"]["rotate_times"]), plain["image_array"][..., :3])


def test_uint16_payloads_stay_whole_too(proc):
    u16 = np.random.default_rng(3).integers(0, 65535, (150, 210, 3), dtype=np.uint16)
    for kw in (dict(exposure=0.5), dict(exposure="device", metadata=None)):
        plain = proc.extract_image_data_cpu(u16, lens_correction=True, zoom=1.3, **kw)
        pay = proc.extract_image_data_cpu(u16, lens_correction=True, lens_profile=PROFILE, zoom=1.3, **kw)
        assert pay["image_array"].shape == (150, 210, 3) and pay["image_array"].dtype == np.uint16
        assert pay["u16_factor"] == plain["u16_factor"] and pay["pipeline_resolution"] == plain["pipeline_resolution"]
        if kw["exposure"] == "device":  # decoded whole first; the statistic is whole-frame anyway
            assert pay["u16_window"] == (0, 0, 150, 210) and pay["lens"]["window"] == plain["u16_window"]


def test_lens_correction_false_ignores_the_profile_and_cam_lens_still_raise(proc):
    img = lm.frame(40, 60)
    off = proc.extract_image_data_cpu(img, lens_correction=False, lens_profile=PROFILE)
    assert "lens" not in off and off["image_array"].shape[:2] == (40, 60)
    for extra in (dict(), dict(lens_profile=PROFILE)):
        with pytest.raises(NotImplementedError, match="lens correction"):
            proc.extract_image_data_cpu(img, cam="cam", lens="lens", lens_correction=True, **extra)
    proc.extract_image_data_cpu(img, cam="cam", lens="lens", lens_correction=False, lens_profile=PROFILE)
    with pytest.raises(ValueError, match="lens_profile"):
        proc.extract_image_data_cpu(img, lens_profile={"distortion": "poly3"})
    with pytest.raises(ValueError, match="r2f_lens_plan"):
        proc.extract_image_data_cpu(img, lens_profile=LensProfile("poly3", (-40.0,), scale="auto"))


def test_both_stream_refusals_name_the_lens_step(proc):
    img = lm.frame(40, 60)
    pay = proc.extract_image_data_cpu(img, lens_profile=PROFILE)
    why = stream_rejection(pay, (4096, 4096, 4), "torch.float32", False, "gpu")
    assert why is not None and "lens" in why
    plain = proc.extract_image_data_cpu(img)
    assert stream_rejection(plain, (4096, 4096, 4), "torch.float32", False, "gpu") is None
    big = np.zeros((1 << 12, 1 << 12, 3), np.float32)
    assert host_stream_gate(big, 16) is None
    why = host_stream_gate(big, 16, 0.0, 0, "No", 0.0, True)
    assert why is not None and "lens" in why


def test_every_settings_forwarder_takes_the_keyword():
    import inspect

    for name in ("process", "extract_image_data_cpu", "load_image_texture"):
        assert inspect.signature(getattr(HipProcessor, name)).parameters["lens_profile"].default is None, name
    for name in ("process_preloaded", "process_preloaded_jpeg", "process_preloaded_tiff", "process_jpeg", "process_tiff", "submit_preloaded"):
        params = inspect.signature(getattr(HipProcessor, name)).parameters.values()
        assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in params), name  # (settings are forwarded whole)


def test_a_changed_profile_invalidates_the_image_cache_and_an_equal_one_does_not(proc):
    uploads = []

    def prepare(payload):
        uploads.append(payload.get("lens"))
        proc._texture = ("frame", None, {})
        proc.image_param_dict = None

    proc.prepare_gpu_textures = prepare
    img = lm.frame(40, 60)
    a = LensProfile("ptlens", (0.02, -0.06, 0.01))
    proc.load_image_texture(img, lens_profile=a)
    proc.load_image_texture(img, lens_profile=LensProfile("ptlens", [0.02, -0.06, 0.01]))  # an equal profile: the frame stays
    assert len(uploads) == 1 and uploads[0] is not None
    proc.load_image_texture(img, lens_profile=LensProfile("ptlens", (0.02, -0.06, 0.02)))
    assert len(uploads) == 2
    proc.load_image_texture(img, lens_profile=None)
    assert len(uploads) == 3 and uploads[2] is None
    proc.load_image_texture(img, lens_profile=None)
    assert len(uploads) == 3
