"""Step M (the median filter of the colour differences, LibRaw's med_passes) without a GPU: the NumPy model of include/r2f.h
(tests/median_model.py) against its per-pixel restatement, its composition and its symmetry under the eight orientations; the
selection network and the clamp of raw2film_amd/csrc/r2f_median_math.h in a stand-alone program under AddressSanitizer / UBSan
(tests/median_check.cpp), whose filtered planes the model reproduces; the profiles' `median_passes`, `resolve`, the upload bounds
of a streamed mosaic and phase 1's payload; and the input conditions of the GPU tests' mosaics (tests/test_gpu_median.py), checked
here where they were chosen."""

import dataclasses
import os
import shutil
import subprocess

import numpy as np
import pytest

import demosaic_model as dm
import highlight_model as hm
import median_model as mm
import xtrans_model as xm
from raw2film_amd import _lib
from raw2film_amd.hip_processor import HipProcessor
from raw2film_amd.payload import DEMOSAIC_REACH, mosaic_upload_bounds, stream_rejection
from raw2film_amd.raw import RawLevels, RawProfile, WaveletDenoise, XTransProfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = RawLevels(hm.WB, 16383)
CLAMP_LEVELS = np.array([0, 40, 30000, 65000, 65535], dtype=np.uint16)


def fixture_planes(xtrans, shape, reduced, kind="wb"):
    """I_0 of a GPU test's fixture whose demosaiced frame has `shape`."""
    k = (3 if xtrans else 2) if reduced else 1
    mosaic, prof, clip = (hm.xtrans_case if xtrans else hm.bayer_case)(kind, xm.PATTERNS[1] if xtrans else "GRBG", (k * shape[0], k * shape[1]))
    c = (xm if xtrans else dm).constants(prof, *mosaic.shape, reduced)
    return mosaic, prof, clip, hm.planes(mosaic, c, xtrans)


# ---- the model
@pytest.mark.parametrize("xtrans", [False, True], ids=["bayer", "xtrans"])
def test_the_model_equals_its_per_pixel_restatement(xtrans):
    for shape, reduced in (((14, 19), False), ((9, 11), True), ((3, 3), False), ((3, 9), False), ((8, 3), False)):
        if xtrans and min(shape) < 6 and not reduced:
            continue
        p = fixture_planes(xtrans, shape, reduced)[3]
        for n in (1, 2, 4):
            assert np.array_equal(mm.passes(p, n), mm.passes_slow(p, n)), (shape, reduced, n)
    rng = np.random.default_rng(7)
    p = rng.choice(CLAMP_LEVELS, size=(3, 12, 17)).astype(np.int64)  # both clamps, ties
    for n in (1, 3):
        assert np.array_equal(mm.passes(p, n), mm.passes_slow(p, n))


def test_n_passes_are_one_pass_n_times_and_green_never_changes():
    p = fixture_planes(False, hm.ONE_TILE, False)[3]
    q = p
    for n in range(1, mm.MAX_PASSES + 1):
        q = mm.passes(q, 1)
        assert np.array_equal(mm.passes(p, n), q)
        assert np.array_equal(q[1], p[1]) and not np.array_equal(q[0], p[0]) and not np.array_equal(q[2], p[2])
        # a border pixel is carried over
        for c in (0, 2):
            assert np.array_equal(q[c, 0], p[c, 0]) and np.array_equal(q[c, -1], p[c, -1])
            assert np.array_equal(q[c, :, 0], p[c, :, 0]) and np.array_equal(q[c, :, -1], p[c, :, -1])
    assert np.array_equal(mm.passes(p, 0), p)


@pytest.mark.parametrize("xtrans", [False, True], ids=["bayer", "xtrans"])
def test_the_model_commutes_with_the_eight_orientations(xtrans):
    p = fixture_planes(xtrans, hm.ONE_TILE, False, "equal")[3]
    hwc = lambda planes: np.ascontiguousarray(planes.transpose(1, 2, 0))  # noqa: E731
    for n in (1, 4):
        want = hwc(mm.passes(p, n))
        for o in range(8):
            turned = hm.orient(hwc(p), o).transpose(2, 0, 1)
            assert np.array_equal(hwc(mm.passes(turned, n)), hm.orient(want, o)), (n, o)


def test_a_frame_with_a_side_of_two_is_the_plain_demosaic():
    for shape, half in (((2, 40), False), ((40, 2), False), ((2, 2), False), ((4, 40), True), ((40, 4), True)):
        mosaic, prof, clip = hm.bayer_case("equal", "RGGB", shape)
        for n in (1, 4):
            assert np.array_equal(mm.demosaic(mosaic, prof, n, half_size=half), dm.demosaic(mosaic, prof, half_size=half))
            assert np.array_equal(mm.demosaic(mosaic, prof, n, clip, half_size=half), hm.demosaic(mosaic, prof, clip, half_size=half))
    mosaic, prof, _ = hm.bayer_case("equal", "RGGB", (3, 40))
    assert not np.array_equal(mm.demosaic(mosaic, prof, 1), dm.demosaic(mosaic, prof))


# ---- the fixtures' conditions
@pytest.mark.parametrize("reduced", [False, True], ids=["full", "reduced"])
@pytest.mark.parametrize("xtrans", [False, True], ids=["bayer", "xtrans"])
def test_every_pass_changes_the_fixtures_and_the_result_is_not_the_plain_demosaic(xtrans, reduced):
    shape = hm.XTRANS_FRAME if xtrans else hm.BAYER_FRAME
    for kind in ("equal", "wb"):
        mosaic, prof, _, p = fixture_planes(xtrans, shape, reduced, kind)
        stats = {}
        out = mm.passes(p, 4, stats)
        assert len(stats["changed"]) == 4 and min(stats["changed"]) >= 0.10, stats["changed"]
        want = mm.demosaic(mosaic, prof, 4, half_size=reduced, xtrans=xtrans)
        plain = hm.demosaic(mosaic, prof, None, half_size=reduced, xtrans=xtrans)
        assert np.array_equal(want, (xm if xtrans else dm).colour(out, (xm if xtrans else dm).constants(prof, *mosaic.shape, reduced)))
        assert np.count_nonzero((want != plain).any(axis=-1)) >= 0.50 * shape[0] * shape[1]


def test_both_clamps_engage_on_the_five_level_mosaic():
    rng = np.random.default_rng(1)
    mosaic = rng.choice(CLAMP_LEVELS, size=hm.BAYER_FRAME)
    stats = {}
    mm.demosaic(mosaic, RawProfile("RGGB", matrix=dm.CAMERA), 4, stats=stats)
    assert stats["clamp_low"] >= 0.01 * stats["interior"] and stats["clamp_high"] >= 0.01 * stats["interior"], stats


# ---- the stand-alone program
@pytest.fixture(scope="module")
def median_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("median_check") / "median_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
           os.path.join(ROOT, "tests", "median_check.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def test_the_network_selects_the_median_of_all_zero_one_inputs(median_check):
    res = subprocess.run([median_check, "network"], capture_output=True, text=True, env=ENV, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "512 ok", res.stdout + res.stderr


@pytest.mark.parametrize("seed", [3, 20261020])
def test_the_network_on_random_inputs_with_ties(median_check, seed):
    res = subprocess.run([median_check, "random", str(seed), "200000"], capture_output=True, text=True, env=ENV, timeout=300)
    assert res.returncode == 0 and res.stdout.strip() == "200000 ok", res.stdout + res.stderr


def test_the_clamp_at_both_ends(median_check):
    res = subprocess.run([median_check, "clamp"], capture_output=True, text=True, env=ENV, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "clamp ok", res.stdout + res.stderr


@pytest.mark.parametrize("h, w, n", [(13, 21, 1), (9, 7, 4), (3, 3, 2), (2, 9, 3), (1, 1, 1)])
def test_the_programs_passes_are_the_models(median_check, h, w, n):
    res = subprocess.run([median_check, "planes", str(h), str(w), "11", str(n)], capture_output=True, text=True, env=ENV, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    rows = np.array([[int(v) for v in line.split()] for line in res.stdout.splitlines()], dtype=np.int64)
    assert rows.shape == (2 * h, 3 * w)
    before, after = (rows[k * h:(k + 1) * h].reshape(h, w, 3).transpose(2, 0, 1) for k in (0, 1))
    assert np.array_equal(mm.passes(before, n), after)
    assert h < 3 or w < 3 or not np.array_equal(before, after)


# ---- the profiles' keyword
@pytest.mark.parametrize("cls", [RawProfile, XTransProfile], ids=lambda c: c.__name__)
def test_median_passes_is_a_validated_keyword_of_equality_hash_and_repr(cls):
    assert cls().median_passes == 0 and cls() == cls(median_passes=0) and hash(cls()) == hash(cls(median_passes=0))
    a, b = cls(median_passes=2), cls(median_passes=np.int64(2))
    assert a == b and hash(a) == hash(b) and type(b.median_passes) is int and {a: 1}[b] == 1
    assert a != cls() and a != cls(median_passes=3) and len({cls(median_passes=n) for n in range(5)}) == 5
    assert "median_passes=2" in repr(a) and "median_passes" not in repr(cls())
    with pytest.raises(Exception):
        a.median_passes = 0
    for bad in (-1, 5, 6, 100, 1.0, 2.5, "2", None, True, False, (1,)):
        with pytest.raises(ValueError, match="med_passes"):
            cls(median_passes=bad)
    with pytest.raises(TypeError):  # a keyword: the positional order is what it was
        cls(cls().pattern, 0, (1.0, 1.0, 1.0), cls().matrix, 0, 2)
    assert cls(cls().pattern, 0, (1.0, 1.0, 1.0), cls().matrix, 5, median_passes=4).orientation == 5
    # the six fields and their order stay; a copy with changed fields keeps the passes when it is asked to
    assert [f.name for f in dataclasses.fields(cls)] == ["pattern", "black", "multipliers", "matrix", "highlight", "orientation"]
    assert dataclasses.replace(a, orientation=3, median_passes=a.median_passes) == cls(orientation=3, median_passes=2)
    assert a._replace(orientation=3) == cls(orientation=3, median_passes=2)
    assert bytes(a.to_c()) == bytes(cls().to_c()) and bytes(a.plan(96, 144)) == bytes(cls().plan(96, 144))  # (no part of the params)


@pytest.mark.parametrize("cls", [RawProfile, XTransProfile], ids=lambda c: c.__name__)
def test_resolve_and_the_denoise_profile_carry_the_passes(cls):
    for highlight in ("clip", "unclip", "blend"):
        d = cls(black=512, multipliers=LEVELS, highlight=highlight, orientation=5, median_passes=3)
        r = d.resolve(13000)
        assert not r.deferred and r.median_passes == 3 and r.orientation == 5
        assert r == dataclasses.replace(cls(black=512, multipliers=LEVELS, highlight=highlight, orientation=5).resolve(13000), median_passes=3)
        assert d.resolve_scale(0)[0].median_passes == 3
    numeric = cls(median_passes=1)
    assert numeric.resolve(5) is numeric
    if cls is RawProfile:
        assert WaveletDenoise.shifted(cls(black=64, multipliers=(2.0, 1.0, 1.5), median_passes=4), 2).median_passes == 4


# ---- the upload bounds of a streamed mosaic
def upload_bounds_of_today(bounds, window, Hm, half_size):
    """mosaic_upload_bounds as it stood before `median`."""
    row0, rows = int(window[0]), int(window[2])
    if half_size:
        return [2 * (row0 + int(b)) for b in bounds]
    r = DEMOSAIC_REACH
    return [max(row0 - r, 0)] + [min(row0 + int(b) + r, Hm) for b in bounds[1:-1]] + [min(row0 + rows + r, Hm)]


def test_upload_bounds_cover_every_bands_reach():
    rng = np.random.default_rng(20261020)
    for _ in range(400):
        half = bool(rng.integers(0, 2))
        out_h = int(rng.integers(8, 400))
        Hm = 2 * out_h if half else out_h
        rows = int(rng.integers(1, out_h + 1))
        row0 = int(rng.integers(0, out_h - rows + 1))
        window = (row0, 3, rows, 40)
        cuts = sorted(set(int(v) for v in rng.integers(1, rows, int(rng.integers(0, 6))))) if rows > 1 else []
        bounds = [0] + cuts + [rows]
        assert mosaic_upload_bounds(bounds, window, Hm, half) == upload_bounds_of_today(bounds, window, Hm, half)
        assert mosaic_upload_bounds(bounds, window, Hm, half, 0) == upload_bounds_of_today(bounds, window, Hm, half)
        for n in range(1, 5):
            ub = mosaic_upload_bounds(bounds, window, Hm, half, median=n)
            assert len(ub) == len(bounds) and all(a <= b for a, b in zip(ub, ub[1:])) and 0 <= ub[0] and ub[-1] <= Hm
            for k, (b0, b1) in enumerate(zip(bounds, bounds[1:])):
                lo, hi = mm.source_rows(row0 + b0, row0 + b1, n, out_h, Hm, DEMOSAIC_REACH, 2 if half else 0)
                assert ub[0] <= lo and hi <= ub[k + 1], (half, out_h, window, bounds, n, k)
            # nothing beyond the reach of the window's first and last row travels
            lo, hi = mm.source_rows(row0, row0 + rows, n, out_h, Hm, DEMOSAIC_REACH, 2 if half else 0)
            assert (ub[0], ub[-1]) == (lo, hi)
    assert DEMOSAIC_REACH == 4
    assert mosaic_upload_bounds([0, 10, 20], (8, 0, 20, 9), 100, False, median=2) == [2, 24, 34]
    assert mosaic_upload_bounds([0, 10, 20], (8, 0, 20, 9), 100, True, median=2) == [12, 40, 60]
    assert mosaic_upload_bounds([0, 10, 20], (0, 0, 20, 9), 40, True, median=3) == [0, 26, 40]


# ---- phase 1 of the processor and the gates
@pytest.fixture
def proc():
    p = HipProcessor.__new__(HipProcessor)
    p.cameras = p.lenses = None
    p.payload_alpha = True
    return p


MOSAIC, NUMERIC = dm.fixture("random", "GRBG", 96, 144)


def with_passes(profile, n):
    return dataclasses.replace(profile, median_passes=n)


def test_the_payload_step_names_the_passes_only_when_there_are_some(proc):
    for kw in (dict(exposure=0.5), dict(exposure=0.5, half_size=False), dict(exposure=None, zoom=1.3)):
        plain = proc.extract_image_data_cpu(MOSAIC, raw_profile=NUMERIC, **kw)
        zero = proc.extract_image_data_cpu(MOSAIC, raw_profile=with_passes(NUMERIC, 0), **kw)
        pay = proc.extract_image_data_cpu(MOSAIC, raw_profile=with_passes(NUMERIC, 3), **kw)
        assert "median" not in plain["demosaic"] and "median" not in zero["demosaic"] and set(zero["demosaic"]) == set(plain["demosaic"])
        assert set(pay) == set(plain) and set(pay["demosaic"]) == set(plain["demosaic"]) | {"median"} and pay["demosaic"]["median"] == 3
        assert bytes(pay["demosaic"]["params"]) == bytes(plain["demosaic"]["params"])
        for k in pay:
            if k not in ("demosaic", "image_array", "warp"):
                assert pay[k] == plain[k] == zero[k], k
    x = XTransProfile(black=512, multipliers=(2.0, 1.0, 1.5), highlight=("blend", 500), orientation=6, median_passes=1)
    step = proc.extract_image_data_cpu(MOSAIC, raw_profile=x, exposure=0.0)["demosaic"]
    assert set(step) == {"params", "window", "rotate_times", "orientation", "clip", "median"} and step["median"] == 1
    deferred = RawProfile("GRBG", black=NUMERIC.black, multipliers=LEVELS, matrix=NUMERIC.matrix, highlight="blend", median_passes=4)
    step = proc.extract_image_data_cpu(MOSAIC, raw_profile=deferred, exposure=0.5)["demosaic"]
    assert set(step) == {"params", "window", "rotate_times", "levels", "median"} and step["levels"] is deferred and step["median"] == 4


def test_both_gates_answer_for_a_median_profile_as_for_a_plain_one(proc, monkeypatch):
    settings = dict(rotation=0.0, chroma_nr=0, canvas_mode="No", highlight_burn=0.0, lens_correction=False, lens_profile=None, exposure=0.5,
                    rotate_times=0, half_size=False, frame_width=36, frame_height=24, flip=False, zoom=1.0)
    proc.stream_bands = 16
    big = np.zeros((4096, 6144), np.uint16)
    for src in (MOSAIC, big):
        for extra in ({}, dict(rotate_times=1), dict(exposure=None), dict(rotation=2.5), dict(half_size=True)):
            a = proc._host_stream_gate(src, {**settings, **extra, "raw_profile": with_passes(NUMERIC, 2)})
            b = proc._host_stream_gate(src, {**settings, **extra, "raw_profile": NUMERIC})
            assert a == b, (src.shape, extra)
    assert proc._host_stream_gate(big, {**settings, "raw_profile": with_passes(NUMERIC, 4)}) is None  # a Bayer mosaic streams with it
    x = XTransProfile(median_passes=2)
    assert "X-Trans mosaics do not stream yet" in proc._host_stream_gate(big, {**settings, "raw_profile": x})
    pay = proc.extract_image_data_cpu(MOSAIC, raw_profile=with_passes(NUMERIC, 2), exposure=0.5, half_size=False)
    args = ((96, 144), "torch.int16", False, "gpu")
    assert "below 16.7 M" in stream_rejection(pay, *args)
    monkeypatch.setattr("raw2film_amd.payload.STREAM_MIN_SAMPLES", 1)
    assert stream_rejection(pay, *args) is None


def test_changed_passes_invalidate_the_image_cache_and_equal_ones_do_not(proc):
    uploads = []

    def prepare(payload):
        uploads.append(payload.get("demosaic"))
        proc._texture = ("frame", None, {})
        proc.image_param_dict = None

    proc.prepare_gpu_textures = prepare
    make = lambda n: RawProfile("GRBG", black=64, multipliers=(2.0, 1.0, 1.5), median_passes=n)  # noqa: E731
    proc.load_image_texture(MOSAIC, raw_profile=make(2), exposure=0.0)
    proc.load_image_texture(MOSAIC, raw_profile=make(np.int32(2)), exposure=0.0)
    assert len(uploads) == 1 and uploads[0]["median"] == 2
    proc.load_image_texture(MOSAIC, raw_profile=make(3), exposure=0.0)
    proc.load_image_texture(MOSAIC, raw_profile=make(0), exposure=0.0)
    assert len(uploads) == 3 and uploads[1]["median"] == 3 and "median" not in uploads[2]


# ---- the header, the library and the documents
def test_the_header_states_step_m_and_the_library_exports_it():
    text = open(os.path.join(ROOT, "include", "r2f.h")).read()
    definition = text[text.index("Step M: the median filter"):text.index("R2F_API int r2f_demosaic_median_u16")]
    assert "UNPINNED" in definition and "med_passes" in definition and "NOT a border" in definition and "#define R2F_MEDIAN_MAX_PASSES 4" in definition
    assert _lib.MEDIAN_MAX_PASSES == mm.MAX_PASSES == 4
    lib = _lib.load()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("r2f_demosaic_median_u16", "r2f_demosaic_median_f32", "r2f_demosaic_xtrans_median_u16"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert f"`{name}`" in integration
