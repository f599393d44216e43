"""The lens correction with TCA, host half, without a GPU: r2f_lens_plan_tca and the shared arithmetic (r2f_lens_math.h:
channel_coord, sample64_channel, correct_pixel_tca) in a stand-alone program under AddressSanitizer / UBSan
(tests/lens_tca_check.cpp), the NumPy model (tests/lens_tca_model.py), LensProfile.tca, the payload of phase 1 and the ABI structs.

The cases are only worth anything if red and blue really sample elsewhere than green, so the conditions the cases were chosen for
are asserted from the model first: a kernel that reused green's coordinates could not pass the comparisons below."""

import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import lens_model as lm
import lens_tca_model as tm
from raw2film_amd import _lib
from raw2film_amd.hip_processor import HipProcessor
from raw2film_amd.lens import LensProfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raw2film_amd", "csrc")


@pytest.fixture(scope="module")
def tca_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("lens_tca_check") / "lens_tca_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
           "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "lens_tca_check.cpp"), os.path.join(CSRC, "r2f_lens_plan.cpp"),
           os.path.join(CSRC, "r2f_plan.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _constants(name, tca, shape):
    prof = tm.profile(name, tca)
    return prof, lm.rounded(lm.constants(prof, *shape)), tm.record(prof, np.float32)


# ---- the conditions the cases were chosen for
@pytest.mark.parametrize("shape", lm.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_red_and_blue_sample_elsewhere_than_green(shape):
    for name in lm.PROFILE_SPECS:
        for tca, least in (("linear", 0.93), ("edge", 0.93), ("poly3", 0.5 if shape != (7, 9) else None)):
            _, c, rec = _constants(name, tca, shape)
            red, green, blue = tm.channel_splits(c, rec, *shape)
            for other in (red, blue):
                differs = np.zeros(green[0].shape, bool)
                for a, b in zip(other[1:], green[1:]):
                    differs |= a != b
                share = differs[green[0]].mean()
                print(f"{name} {tca} {shape}: differs on {share:.3f} of green's inside pixels")
                assert share > 0 if least is None else share >= least, (name, tca, shape, share)


@pytest.mark.parametrize("name,shape,found", [("none", (150, 210), 1308), ("ptlens", (150, 210), 1754), ("ptlens", (96, 128), 158)])
def test_edge_puts_red_or_blue_outside_where_green_is_inside(name, shape, found):
    _, c, rec = _constants(name, "edge", shape)
    red, green, blue = tm.channel_splits(c, rec, *shape)
    count = int((green[0] & ~(red[0] & blue[0])).sum())
    print(f"{name} edge {shape}: {count} pixels (found when the cases were chosen: {found})")
    assert count > 0


def test_the_unstaged_and_the_union_box_cases_are_what_they_are_said_to_be():
    """Of a block's 64 x 16 tile of 150 x 210: at scale 0.25 the union of the channels' tap boxes around the centre exceeds the 3072
    texels a block stages (the unstaged path); with `edge` on ptlens at scale 1 the first tile's fits, and is wider than green's by
    more than the tap reach."""
    def boxes(name, tca, tile):
        _, c, rec = _constants(name, tca, (150, 210))
        per = []
        for inside, ix, iy, _, _ in tm.channel_splits(c, rec, 150, 210, tile + (16, 64)):
            assert inside.any()
            per.append((ix[inside].min(), ix[inside].max(), iy[inside].min(), iy[inside].max()))
        union = (min(p[0] for p in per), max(p[1] for p in per), min(p[2] for p in per), max(p[3] for p in per))
        return per[1], union

    _, union = boxes("scale-0.25", "linear", (64, 64))
    assert (union[1] - union[0] + 8) * (union[3] - union[2] + 8) > 3072
    green, union = boxes("ptlens", "edge", (0, 0))
    assert (union[1] - union[0] + 8) * (union[3] - union[2] + 8) <= 3072
    assert (union[1] - union[0]) - (green[1] - green[0]) > 4  # (taps reach from ix - 3 to ix + 4)


# ---- the CPU program
@pytest.mark.parametrize("seed", [1, 2, 20261020])
def test_planner_and_decision_are_clean_under_the_sanitizers(tca_check, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([tca_check, "fuzz", str(seed), "20000"], capture_output=True, text=True, env=env, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    assert "cases ok" in res.stdout


def _render(binary, tmp_path, image, profile, window=None):
    H, W, C = image.shape
    r0, c0, nr, nc = (0, 0, H, W) if window is None else window
    job, out = str(tmp_path / "job.bin"), str(tmp_path / "out.bin")
    with open(job, "wb") as f:
        f.write(np.array([H, W, C, r0, c0, nr, nc], dtype=np.int32).tobytes())
        f.write(bytes(profile.to_c()))
        f.write(bytes(profile.to_c_tca()))
        f.write(np.ascontiguousarray(image, dtype=np.float32).tobytes())
    res = subprocess.run([binary, "render", job, out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    raw = open(out, "rb").read()
    n0, n1 = ctypes.sizeof(_lib.LensParams), ctypes.sizeof(_lib.LensTcaParams)
    params, tca = _lib.LensParams.from_buffer_copy(raw[:n0]), _lib.LensTcaParams.from_buffer_copy(raw[n0:n0 + n1])
    return params, tca, np.frombuffer(raw[n0 + n1:], dtype=np.float32).reshape(nr, nc, 3)


@pytest.mark.parametrize("shape", lm.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shared_arithmetic_renders_the_model_bit_for_bit(tca_check, tmp_path, shape):
    H, W = shape
    for name in lm.PROFILE_SPECS:
        for tca in tm.RENDERED:
            prof = tm.profile(name, tca)
            image = lm.frame(H, W, 4 if name == "poly5" else 3)  # (a fourth channel is ignored)
            params, tca_params, got = _render(tca_check, tmp_path, image, prof)
            # the planner's constants are the definition's, rounded from double
            want_c, have_c = lm.rounded(lm.constants(prof, H, W)), lm.from_params(params)
            for field in ("cx", "cy", "q", "inv_scale", "c0", "qv"):
                assert _bits(getattr(want_c, field)) == _bits(getattr(have_c, field)), (name, field)
            want_rec, have_rec = tm.record(prof, np.float32), tm.from_params(tca_params)
            assert have_rec[0] == want_rec[0] and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(have_rec[1:], want_rec[1:]))
            want = tm.correct_tca(image, want_c, want_rec)
            assert np.array_equal(_bits(got), _bits(want)), (name, tca, shape, int((_bits(got) != _bits(want)).sum()))
    # a window that straddles every edge, and one wholly outside the frame
    image = lm.frame(H, W)
    for tca in tm.RENDERED:
        prof, c, rec = _constants("off-centre", tca, shape)
        for window in ((-5, -6, H + 11, W + 9), (H + 40, -W - 50, 5, 7)):
            _, _, got = _render(tca_check, tmp_path, image, prof, window)
            assert np.array_equal(_bits(got), _bits(tm.correct_tca(image, c, rec, window))), (tca, window)


# ---- the model's two identities
@pytest.mark.parametrize("shape", lm.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_identity_record_is_the_plain_correction_and_green_always_is(shape):
    image = lm.frame(*shape)
    for name in lm.PROFILE_SPECS:
        plain = lm.correct(image, lm.rounded(lm.constants(lm.profile(name), *shape)))
        for tca in ("identity", ("poly3", (1, 1, 0, 0, 0, 0))):
            _, c, rec = _constants(name, tca, shape)
            assert np.array_equal(_bits(tm.correct_tca(image, c, rec)), _bits(plain)), (name, tca)
        for tca in tm.RENDERED:
            assert np.array_equal(_bits(tm.model(name, tca, shape)[..., 1]), _bits(plain[..., 1])), (name, tca)
            if shape == (150, 210):
                assert not np.array_equal(tm.model(name, tca, shape)[..., 0], plain[..., 0])


@pytest.mark.parametrize("shape", [(33, 47), (96, 128), (150, 210)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_float32_model_against_the_float64_evaluation(shape):
    """tests/test_lens_host.py's criterion, per channel: a pixel whose 1/32 phase (or tap origin) differs between the float32 model
    and the float64 evaluation with unrounded constants is left out, and the share of such pixels may not exceed 2e-3 (found when
    the cases were chosen: at most 1.3e-3; `edge` reaches 1.8e-3 and is not here).  Every other sample lies within
    gamma_66 * sum |w v|; with vignetting the bound is divided by the gain's denominator and gamma_16 |o| is added."""
    H, W = shape
    for name in lm.PROFILE_SPECS:
        for tca in ("linear", "poly3"):
            prof, image = tm.profile(name, tca), lm.frame(H, W)
            c64 = lm.constants(prof, H, W)
            o32, d32 = tm.correct_tca(image, lm.rounded(c64), tm.record(prof, np.float32), want_bound=True)
            o64, d64 = tm.correct_tca(image, c64, tm.record(prof), T=np.float64, want_bound=True)
            for ch in (0, 2):
                a, b = d32[ch], d64[ch]
                same = (a.inside == b.inside) & (a.fx == b.fx) & (a.fy == b.fy) & (a.ix == b.ix) & (a.iy == b.iy)
                share = 1.0 - same.mean()
                print(f"{name} {tca} {H}x{W} {tm.CHANNELS[ch]}: phase differs on {share:.2e} of the pixels")
                assert share <= 2e-3, (name, tca, shape, ch, share)
                bound = lm.gamma(66) * b.sum_abs
                if b.den is not None:
                    bound = bound / np.abs(b.den) + lm.gamma(16) * np.abs(o64[..., ch])
                err = np.abs(o32[..., ch].astype(np.float64) - o64[..., ch])
                assert bool((err <= bound)[same].all()), (name, tca, shape, ch, float((err - bound)[same].max()))


# ---- auto scale
@pytest.mark.parametrize("name,shape", [(n, s) for n in ("ptlens", "poly3", "poly5", "off-centre")
                                        for s in ((33, 47), (150, 210), (4000, 6000), (64, 1)) if (n, s) != ("off-centre", (64, 1))])
def test_auto_scale_puts_every_probe_of_every_channel_on_or_inside_the_boundary(name, shape):
    """tests/test_lens_host.py's check with the three-channel probes: all land inside to 1e-9 px, at scale * (1 - 1e-6) one does not."""
    H, W = shape
    for tca in ("linear", "poly3"):
        prof = LensProfile(**dict(lm.PROFILE_SPECS[name], scale="auto"), tca=tm.TCA_SPECS[tca])
        params, _ = prof.plan_tca(H, W)
        scale = params.scale
        assert 1 / 16 < scale < 16
        assert tm.probes_reach(prof, H, W, scale) <= 1e-9
        assert tm.probes_reach(prof, H, W, scale * (1 - 1e-6)) > 0
        assert scale >= prof.plan(H, W).scale  # (green alone needs no more)
        want = lm.rounded(lm.constants(prof, H, W, scale))
        have = lm.from_params(params)
        assert (_bits(want.q), _bits(want.inv_scale)) == (_bits(have.q), _bits(have.inv_scale))


@pytest.mark.parametrize("tca", ["identity", ("poly3", (1, 1, 0, 0, 0, 0))], ids=["linear", "poly3"])
def test_auto_scale_of_an_identity_record_is_the_plain_one_to_the_bit(tca):
    for name in ("ptlens", "poly3", "poly5", "off-centre"):
        for H, W in ((33, 47), (150, 210), (4000, 6000)):
            prof = LensProfile(**dict(lm.PROFILE_SPECS[name], scale="auto"), tca=tm.TCA_SPECS[tca] if isinstance(tca, str) else tca)
            params, _ = prof.plan_tca(H, W)
            assert bytes(params) == bytes(prof.plan(H, W)), (name, H, W)


def test_without_auto_scale_the_params_are_the_plain_planners_byte_for_byte():
    for name in lm.PROFILE_SPECS:
        for tca in tm.RENDERED:
            prof = tm.profile(name, tca)
            assert bytes(prof.plan_tca(150, 210)[0]) == bytes(prof.plan(150, 210)) == bytes(lm.profile(name).plan(150, 210))


def test_auto_scale_without_a_fitting_scale_is_refused():
    with pytest.raises(ValueError, match="r2f_lens_plan_tca"):
        LensProfile("poly3", (-40.0,), scale="auto", tca=tm.TCA_SPECS["linear"]).plan_tca(100, 150)
    with pytest.raises(ValueError, match="r2f_lens_plan_tca"):  # green fits; red would need a view shrunk more than 16 times
        LensProfile("none", scale="auto", tca=("linear", (20.0, 1.0))).plan_tca(100, 150)
    LensProfile("none", scale="auto").plan(100, 150)
    assert LensProfile("none", scale="auto", tca=tm.TCA_SPECS["linear"]).plan_tca(1, 1)[0].scale == 1.0


# ---- LensProfile
def test_profile_with_tca_is_frozen_hashable_and_normalised():
    a = LensProfile("ptlens", [0.02, -0.06, 0.01], tca=["linear", [1, 0.97]])
    b = LensProfile("ptlens", (0.02, -0.06, 0.01), tca=("linear", (1.0, 0.97)))
    assert a.tca == ("linear", (1.0, 0.97)) and all(type(v) is float for v in a.tca[1])
    assert a == b and hash(a) == hash(b) and {a: 1}[b] == 1
    assert a != LensProfile("ptlens", (0.02, -0.06, 0.01), tca=("linear", (1.0, 0.98)))
    assert a != LensProfile("ptlens", (0.02, -0.06, 0.01))
    with pytest.raises(Exception):
        a.tca = None
    assert LensProfile().tca is None and LensProfile().to_c_tca() is None and LensProfile().plan_tca(40, 60)[1] is None
    assert list(LensProfile.__dataclass_fields__)[-1] == "tca"


@pytest.mark.parametrize("tca", [
    ("cubic", (1.0, 1.0)), (3, (1.0, 1.0)), ("linear", (1.0,)), ("linear", (1.0, 1.0, 0.0)), ("poly3", (1.0, 1.0)),
    ("poly3", (1.0, 1.0, 0.0, 0.0, 0.0)), ("linear", (1.0, float("nan"))), ("poly3", (1.0, 1.0, 0.0, float("inf"), 0.0, 0.0)),
    ("linear",), "linear", 1.0, ("linear", 1.0), ("linear", (1.0, 1.0), 0),
])
def test_tca_validation_raises_before_any_work(tca):
    with pytest.raises(ValueError):
        LensProfile(tca=tca)


def test_to_c_tca_puts_the_xml_order_into_per_channel_constants():
    t = LensProfile(tca=("poly3", (1.002, 0.998, 0.01, -0.008, -0.02, 0.015))).to_c_tca()
    assert (t.model, t.n_coef, list(t.red), list(t.blue)) == (_lib.TCA_POLY3, 3, [1.002, 0.01, -0.02], [0.998, -0.008, 0.015])
    t = LensProfile(tca=("linear", (1.03, 0.97))).to_c_tca()
    assert (t.model, t.n_coef, t.red[0], t.blue[0]) == (_lib.TCA_LINEAR, 1, 1.03, 0.97)


def test_planner_refuses_a_bad_tca_record():
    lib = _lib.load()
    out, out_tca = _lib.LensParams(), _lib.LensTcaParams()
    prof = LensProfile("poly5", (0.03, -0.01)).to_c()

    def plan(**changes):
        t = LensProfile(tca=("poly3", (1.002, 0.998, 0.01, -0.008, -0.02, 0.015))).to_c_tca()
        for k, v in changes.items():
            if isinstance(v, tuple):
                getattr(t, k)[:] = v
            else:
                setattr(t, k, v)
        return lib.r2f_lens_plan_tca(ctypes.byref(prof), ctypes.byref(t), 40, 60, ctypes.byref(out), ctypes.byref(out_tca))

    assert plan() == _lib.OK
    nan, inf = float("nan"), float("inf")
    for bad in (dict(model=0), dict(model=3), dict(model=-1), dict(n_coef=1), dict(n_coef=2), dict(model=1), dict(red=(1.0, nan, 0.0)),
                dict(blue=(inf, 0.0, 0.0)), dict(blue=(1.0, 0.0, 1e39))):
        assert plan(**bad) == _lib.EINVAL, bad
    assert plan(model=1, n_coef=1, red=(1.0, nan, inf)) == _lib.OK  # (constants past n_coef are not read)
    assert (out_tca.model, list(out_tca.red), list(out_tca.blue)[1:]) == (1, [1.0, 0.0, 0.0], [0.0, 0.0])
    bad_profile = LensProfile().to_c()
    bad_profile.scale = -1.0
    t = LensProfile(tca=("linear", (1.0, 1.0))).to_c_tca()
    assert lib.r2f_lens_plan_tca(ctypes.byref(bad_profile), ctypes.byref(t), 40, 60, ctypes.byref(out), ctypes.byref(out_tca)) == _lib.EINVAL


# ---- ABI
def test_struct_layouts_match_the_header():
    T, R = _lib.LensTca, _lib.LensTcaParams
    assert ctypes.sizeof(T) == 56 and [getattr(T, f).offset for f in ("model", "n_coef", "red", "blue")] == [0, 4, 8, 32]
    assert ctypes.sizeof(R) == 28 and [getattr(R, f).offset for f in ("model", "red", "blue")] == [0, 4, 16]
    assert (ctypes.sizeof(_lib.LensProfile), ctypes.sizeof(_lib.LensParams)) == (96, 64)
    text = open(os.path.join(ROOT, "include", "r2f.h")).read()
    body = text[text.index("typedef struct r2f_lens_tca {"):text.index("} r2f_lens_tca;")]
    order = [body.index(w) for w in ("int32_t model, n_coef;", "double red[3], blue[3];")]
    assert order == sorted(order)
    body = text[text.index("typedef struct r2f_lens_tca_params {"):text.index("} r2f_lens_tca_params;")]
    order = [body.index(w) for w in ("int32_t model;", "float red[3], blue[3];")]
    assert order == sorted(order)
    assert "enum { R2F_TCA_NONE = 0, R2F_TCA_LINEAR = 1, R2F_TCA_POLY3 = 2 };" in text
    assert (_lib.TCA_NONE, _lib.TCA_LINEAR, _lib.TCA_POLY3) == (0, 1, 2)


# ---- phase 1 of the processor
@pytest.fixture
def proc():
    p = HipProcessor.__new__(HipProcessor)
    p.cameras = p.lenses = None
    p.payload_alpha = True
    return p


PLAIN = LensProfile("ptlens", (0.02, -0.06, 0.01), vignetting=(-0.3, 0.1, -0.02), scale=1.02)
WITH_TCA = LensProfile("ptlens", (0.02, -0.06, 0.01), vignetting=(-0.3, 0.1, -0.02), scale=1.02, tca=tm.TCA_SPECS["poly3"])
CROP_KEYS = ("final_resolution", "output_resolution", "canvas_resolution", "pipeline_resolution", "resize_to", "upscale_to", "chroma_nr",
             "u16_factor", "u16_window", "warp")


@pytest.mark.parametrize("kw", [
    dict(), dict(zoom=1.3, rotate_times=1), dict(rotation=3.5, zoom=1.3, rotate_times=1), dict(flip=True, frame_width=36, frame_height=36),
    dict(resolution=(60, 90), canvas_mode="Uniform white", canvas_scale=1.1), dict(rotate_times=3, max_scale=2.0),
])
def test_payload_has_the_tca_key_exactly_with_a_tca_profile(proc, kw):
    img = lm.frame(150, 210)
    plain = proc.extract_image_data_cpu(img, lens_correction=True, lens_profile=PLAIN, **kw)
    pay = proc.extract_image_data_cpu(img, lens_correction=True, lens_profile=WITH_TCA, **kw)
    assert set(pay) == set(plain)
    assert set(plain["lens"]) == {"params", "window", "rotate_times"} and set(pay["lens"]) == set(plain["lens"]) | {"tca"}
    assert isinstance(pay["lens"]["tca"], _lib.LensTcaParams) and bytes(pay["lens"]["params"]) == bytes(plain["lens"]["params"])
    assert tm.from_params(pay["lens"]["tca"])[0] == "poly3"
    assert (pay["lens"]["window"], pay["lens"]["rotate_times"]) == (plain["lens"]["window"], plain["lens"]["rotate_times"])
    assert np.array_equal(pay["image_array"], plain["image_array"])
    for k in CROP_KEYS:
        a, b = pay[k], plain[k]
        if isinstance(a, dict):
            assert set(a) == set(b) and all(np.array_equal(a[f], b[f]) for f in a), k
        else:
            assert a == b, k
    off = proc.extract_image_data_cpu(img, lens_correction=False, lens_profile=WITH_TCA, **kw)
    assert "lens" not in off and set(off) == set(proc.extract_image_data_cpu(img, lens_correction=False, **kw))


def test_uint16_payload_with_tca(proc):
    u16 = np.random.default_rng(3).integers(0, 65535, (150, 210, 3), dtype=np.uint16)
    for kw in (dict(exposure=0.5), dict(exposure="device", metadata=None)):
        plain = proc.extract_image_data_cpu(u16, lens_correction=True, lens_profile=PLAIN, zoom=1.3, **kw)
        pay = proc.extract_image_data_cpu(u16, lens_correction=True, lens_profile=WITH_TCA, zoom=1.3, **kw)
        assert "tca" in pay["lens"] and "tca" not in plain["lens"]
        assert (pay["u16_factor"], pay["u16_window"], pay["lens"]["window"]) == (plain["u16_factor"], plain["u16_window"], plain["lens"]["window"])


def test_a_changed_tca_invalidates_the_image_cache_and_an_equal_one_does_not(proc):
    uploads = []

    def prepare(payload):
        uploads.append(payload.get("lens"))
        proc._texture = ("frame", None, {})
        proc.image_param_dict = None

    proc.prepare_gpu_textures = prepare
    img = lm.frame(40, 60)
    proc.load_image_texture(img, lens_profile=LensProfile("ptlens", (0.02, -0.06, 0.01), tca=("linear", (1.03, 0.97))))
    proc.load_image_texture(img, lens_profile=LensProfile("ptlens", [0.02, -0.06, 0.01], tca=["linear", [1.03, 0.97]]))  # equal: the frame stays
    assert len(uploads) == 1 and "tca" in uploads[0]
    proc.load_image_texture(img, lens_profile=LensProfile("ptlens", (0.02, -0.06, 0.01), tca=("linear", (1.03, 0.98))))
    assert len(uploads) == 2 and "tca" in uploads[1]
    proc.load_image_texture(img, lens_profile=LensProfile("ptlens", (0.02, -0.06, 0.01)))
    assert len(uploads) == 3 and "tca" not in uploads[2]
    proc.load_image_texture(img, lens_profile=LensProfile("ptlens", (0.02, -0.06, 0.01)))
    assert len(uploads) == 3


def test_a_tca_payload_is_still_refused_by_the_stream_with_the_lens_steps_words(proc):
    from raw2film_amd.payload import stream_rejection

    pay = proc.extract_image_data_cpu(lm.frame(40, 60), lens_profile=WITH_TCA)
    plain = proc.extract_image_data_cpu(lm.frame(40, 60), lens_profile=PLAIN)
    why = stream_rejection(pay, (4096, 4096, 4), "torch.float32", False, "gpu")
    assert why is not None and "lens" in why and why == stream_rejection(plain, (4096, 4096, 4), "torch.float32", False, "gpu")
