"""The hot-pixel repair of a mosaic without a GPU: the NumPy model of include/r2f.h (tests/repair_model.py) on its own; the planner
(r2f_mosaic_repair_plan) through the library; the text the kernel compiles (r2f_repair_math.h) and the planner in a stand-alone
program under AddressSanitizer / UBSan (tests/repair_check.cpp), whose bytes are held against the model's and which walks the
neighbour table of all 36 shifts of the X-Trans pattern; the HotPixels record, phase 1's checks and payload, the rows that travel with
a streamed band, the image cache key."""

import ctypes
import inspect
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import demosaic_model as dm
import repair_model as model
from raw2film_amd import _lib, hip_processor
from raw2film_amd.hip_processor import HipProcessor
from raw2film_amd.payload import REPAIR_REACH, host_stream_gate, mosaic_rejection, mosaic_upload_bounds
from raw2film_amd.raw import HotPixels, RawLevels, RawProfile, XTransProfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raw2film_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
BLACK = (512, 520, 500, 512)
BLACK36 = tuple(400 + 7 * ((5 * i + 3) % 36) for i in range(36))
SHIFTS = [(dy, dx) for dy in range(6) for dx in range(6)]


# ---- the model itself
def test_every_shift_has_four_distinct_neighbours_inside_ring_2_of_the_centres_colour():
    for dy, dx in SHIFTS:
        cfa = model.cfa_ids(model.CANONICAL, dy, dx)
        table = model.neighbour_table(6, cfa)
        for ph, row in enumerate(table):
            assert None not in row and len(set(row)) == 4, (dy, dx, ph)
            for d, (oy, ox) in enumerate(row):
                assert max(abs(oy), abs(ox)) in (1, 2) and cfa[(ph // 6 + oy) % 6, (ph % 6 + ox) % 6] == cfa[ph // 6, ph % 6]
                assert (oy, ox) in model.candidates(d, max(abs(oy), abs(ox)))


def test_the_rings_sites_belong_to_exactly_one_quadrant_each():
    for r, n in ((1, 8), (2, 16)):
        sites = [c for d in range(4) for c in model.candidates(d, r)]
        assert len(sites) == len(set(sites)) == n and all(max(abs(a), abs(b)) == r for a, b in sites)


@pytest.mark.parametrize("shape", [(33, 65), (70, 200)])
def test_the_random_recipe_does_not_pass_vacuously(shape):
    frame = model.field(shape, 11)
    out4, hot4 = model.repair(frame, 2, BLACK, 1000, 32, 4)
    out3, hot3 = model.repair(frame, 2, BLACK, 1000, 32, 3)
    assert hot4.mean() >= 0.02 and hot3.mean() > hot4.mean() and (out3 != out4).any()
    assert ((out4 != frame) == hot4).all() and (out4[hot4] < frame[hot4]).all()  # a replaced sample always differs: it falls
    ring = np.ones(shape, bool)
    ring[2:-2, 2:-2] = False
    assert not hot3[ring].any()


def test_a_lone_hot_sample_takes_its_largest_neighbour_and_a_flat_field_is_left_alone():
    flat = np.full((12, 12), 1000, np.uint16)
    out, hot = model.repair(flat, 2, BLACK, 100, 32, 4)
    assert not hot.any() and (out == flat).all()
    frame = flat.copy()
    frame[5, 6] = 40000
    frame[3, 6], frame[7, 6], frame[5, 4], frame[5, 8] = 1100, 1200, 1300, 1250
    out, hot = model.repair(frame, 2, BLACK, 100, 32, 4)
    assert hot.sum() == 1 and out[5, 6] == 1300 and (out[~hot] == frame[~hot]).all()


# ---- the planner through the library
def _plan(period, cfa, black, threshold, q, mn, H, W):
    out = _lib.RepairParams()
    ctypes.memset(ctypes.byref(out), 0x5A, ctypes.sizeof(out))
    before = bytes(out)
    ids = None if cfa is None else (ctypes.c_int32 * 36)(*[int(v) for v in np.asarray(cfa).ravel()])
    table = None if black is None else (ctypes.c_double * len(black))(*black)
    rc = _lib.load().r2f_mosaic_repair_plan(period, ids, table, threshold, q, mn, H, W, ctypes.byref(out))
    return rc, out, bytes(out) == before


def test_planner_fields_and_tables():
    rc, p, _ = _plan(2, None, BLACK, 1000, 32, 4, 6, 6)
    assert rc == _lib.OK and (p.period, p.threshold, p.q, p.min_neighbours) == (2, 1000, 32, 4)
    assert list(p.black) == [BLACK[(ph // 6 % 2) * 2 + ph % 6 % 2] for ph in range(36)]
    assert all([tuple(p.offset[ph][d]) for d in range(4)] == list(model.BAYER) for ph in range(36))
    for dy, dx in ((0, 0), (1, 2), (5, 3)):
        cfa = model.cfa_ids(model.CANONICAL, dy, dx)
        rc, p, _ = _plan(6, cfa, BLACK36, 0, 255, 3, 37, 70)
        assert rc == _lib.OK and list(p.black) == list(BLACK36)
        assert [[tuple(p.offset[ph][d]) for d in range(4)] for ph in range(36)] == model.neighbour_table(6, cfa)


LONE = [1] * 36
LONE[0], LONE[1] = 0, 2


@pytest.mark.parametrize("args", [
    (4, None, BLACK, 1000, 32, 4, 64, 64), (6, None, BLACK36, 1000, 32, 4, 64, 64), (2, None, None, 1000, 32, 4, 64, 64),
    (2, None, BLACK, -1, 32, 4, 64, 64), (2, None, BLACK, 65536, 32, 4, 64, 64), (2, None, BLACK, 1000, 0, 4, 64, 64),
    (2, None, BLACK, 1000, 256, 4, 64, 64), (2, None, BLACK, 1000, 32, 2, 64, 64), (2, None, BLACK, 1000, 32, 5, 64, 64),
    (2, None, BLACK, 1000, 32, 4, 5, 64), (2, None, BLACK, 1000, 32, 4, 64, 5), (2, None, (512, -1, 500, 512), 1000, 32, 4, 64, 64),
    (2, None, (512, 65536, 500, 512), 1000, 32, 4, 64, 64), (2, None, (512, 512.5, 500, 512), 1000, 32, 4, 64, 64),
    (2, None, (512, float("nan"), 500, 512), 1000, 32, 4, 64, 64), (6, LONE, BLACK36, 1000, 32, 4, 64, 64),
    (6, [3] + [1] * 35, BLACK36, 1000, 32, 4, 64, 64),
])
def test_planner_refusals_leave_the_output_alone(args):
    rc, _, untouched = _plan(*args)
    assert rc == _lib.EINVAL and untouched


def test_struct_and_enums_match_the_header():
    assert ctypes.sizeof(_lib.RepairParams) == 448 and _lib.RepairParams.offset.offset == 148 and _lib.RepairParams.threshold.offset == 436
    text = open(os.path.join(ROOT, "include", "r2f.h")).read()
    assert f"R2F_MOSAIC_REPAIR_VEC = {_lib.MOSAIC_REPAIR_VEC}, R2F_MOSAIC_REPAIR_ROWS = {_lib.MOSAIC_REPAIR_ROWS}" in text
    section = text[text.index("The repair of hot pixels of a mosaic on the device"):text.index("typedef struct r2f_repair_params")]
    assert "NOT LibRaw's bad_pixels" in section and "dark-frame" in section and "fused into the demosaic" in section


# ---- the stand-alone program under the sanitizers
@pytest.fixture(scope="module")
def repair_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("repair_check") / "repair_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
           os.path.join(ROOT, "tests", "repair_check.cpp"), os.path.join(CSRC, "r2f_repair_plan.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


def test_the_programs_neighbour_tables_are_the_models_on_all_36_shifts(repair_check):
    res = subprocess.run([repair_check, "table"], capture_output=True, text=True, env=ENV, timeout=120)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    lines = [[int(v) for v in line.split()] for line in res.stdout.splitlines()]
    assert [tuple(line[:2]) for line in lines] == SHIFTS
    for line in lines:
        want = model.neighbour_table(6, model.cfa_ids(model.CANONICAL, line[0], line[1]))
        assert line[2:] == [v for row in want for off in row for v in off], line[:2]


def test_the_programs_planner_refusals_leave_the_output_alone(repair_check):
    res = subprocess.run([repair_check, "refuse"], capture_output=True, text=True, env=ENV, timeout=120)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    assert "refusals ok 22" in res.stdout


PROGRAM_CASES = [(2, (6, 6), None, 4), (2, (37, 70), None, 3), (2, (70, 200), None, 4), (6, (37, 70), (0, 0), 4), (6, (70, 200), (4, 1), 3),
                 (6, (6, 6), (2, 5), 3)]


@pytest.mark.parametrize("case", PROGRAM_CASES, ids=lambda c: f"p{c[0]}-{c[1][0]}x{c[1][1]}-n{c[3]}")
def test_the_programs_bytes_equal_the_models(repair_check, tmp_path, case):
    P, shape, shift, mn = case
    black = BLACK if P == 2 else BLACK36
    cfa = None if P == 2 else model.cfa_ids(model.CANONICAL, *shift)
    frame = model.field(shape, shape[1] + P)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    head = struct.pack("<6i", shape[0], shape[1], P, 1000, 32, mn) + struct.pack(f"<{P * P}d", *black)
    src.write_bytes(head + (b"" if cfa is None else cfa.astype("<i4").tobytes()) + frame.tobytes())
    res = subprocess.run([repair_check, "run", str(src), str(dst)], capture_output=True, text=True, env=ENV, timeout=300)
    assert res.returncode == 0, (case, (res.stdout + res.stderr)[-4000:])
    blob = dst.read_bytes()
    want, hot = model.repair(frame, P, black, 1000, 32, mn, cfa)
    assert struct.unpack("<I", blob[:4])[0] == int(hot.sum()) and (hot.any() or shape == (6, 6))
    assert (np.frombuffer(blob[4:], np.uint16).reshape(shape) == want).all()


# ---- the record
def test_the_record_is_frozen_hashable_and_normalised():
    r = HotPixels(1000)
    assert (r.threshold, r.ratio, r.min_neighbours, r.q) == (1000, 0.125, 4, 32)
    assert r == HotPixels(np.int64(1000), 0.125, 4) and hash(r) == hash(HotPixels(1000, 1 / 8)) and r != HotPixels(1000, min_neighbours=3)
    with pytest.raises(Exception):
        r.threshold = 5
    assert HotPixels(0, 1 / 256).q == 1 and HotPixels(65535, 255 / 256, 3).q == 255


@pytest.mark.parametrize("kwargs, name", [
    (dict(threshold=-1), "threshold"), (dict(threshold=65536), "threshold"), (dict(threshold=10.0), "threshold"),
    (dict(threshold=True), "threshold"), (dict(threshold=10, ratio=0.0), "ratio"), (dict(threshold=10, ratio=1.0), "ratio"),
    (dict(threshold=10, ratio=0.001), "ratio"), (dict(threshold=10, ratio=float("nan")), "ratio"), (dict(threshold=10, ratio="x"), "ratio"),
    (dict(threshold=10, min_neighbours=2), "min_neighbours"), (dict(threshold=10, min_neighbours=5), "min_neighbours"),
    (dict(threshold=10, min_neighbours=3.0), "min_neighbours"),
])
def test_the_record_names_the_field_it_refuses(kwargs, name):
    with pytest.raises(ValueError, match=f"HotPixels.{name} must be"):
        HotPixels(**kwargs)


def test_the_records_plan_is_the_planners():
    r = HotPixels(1000, min_neighbours=3)
    p = r.plan(RawProfile("GRBG", black=BLACK), 37, 70)
    assert (p.period, p.threshold, p.q, p.min_neighbours, p.black[7]) == (2, 1000, 32, 3, 512)
    x = r.plan(XTransProfile(model.shifted_pattern(1, 2), black=BLACK36), 37, 70)
    assert x.period == 6 and [[tuple(x.offset[ph][d]) for d in range(4)] for ph in range(36)] == model.neighbour_table(6, model.cfa_ids(model.CANONICAL, 1, 2))
    with pytest.raises(ValueError, match="refused"):
        r.plan(RawProfile("GRBG", black=BLACK), 5, 70)
    with pytest.raises(ValueError, match="RawProfile or an XTransProfile"):
        r.plan(None, 37, 70)


# ---- phase 1 of the processor
@pytest.fixture
def proc():
    p = HipProcessor.__new__(HipProcessor)
    p.cameras = p.lenses = None
    p.payload_alpha = True
    return p


MOSAIC, NUMERIC = dm.fixture("random", "GRBG", 96, 144)
DEFERRED = RawProfile("GRBG", black=NUMERIC.black, multipliers=RawLevels((2.1, 1.0, 1.6), 16383), matrix=NUMERIC.matrix)


def test_phase_1_names_each_reason_it_refuses_a_repair_for(proc):
    r = HotPixels(1000)
    with pytest.raises(ValueError, match="raw_repair needs a raw_profile"):
        proc.extract_image_data_cpu(np.zeros((96, 144, 3), np.uint16), raw_repair=r, exposure=0.0)
    with pytest.raises(ValueError, match="raw_repair must be a raw2film_amd.raw.HotPixels"):
        proc.extract_image_data_cpu(MOSAIC, raw_profile=NUMERIC, raw_repair=1000, exposure=0.0)
    with pytest.raises(ValueError, match="at least 6"):
        proc.extract_image_data_cpu(np.zeros((4, 144), np.uint16), raw_profile=NUMERIC, raw_repair=r, exposure=0.0, half_size=False)


def test_the_demosaic_step_carries_the_record_only_when_given(proc):
    r = HotPixels(1000)
    for profile, extra in ((NUMERIC, set()), (DEFERRED, {"levels"}), (XTransProfile(black=512), set())):
        pay = proc.extract_image_data_cpu(MOSAIC, raw_profile=profile, raw_repair=r, exposure=0.5)
        plain = proc.extract_image_data_cpu(MOSAIC, raw_profile=profile, exposure=0.5)
        step = pay["demosaic"]
        assert set(step) == {"params", "window", "rotate_times", "repair", "profile"} | extra
        assert step["repair"] is r and step["profile"] is profile and "repair" not in plain["demosaic"] and "profile" not in plain["demosaic"]
        assert set(pay) == set(plain) and pay["image_array"] is MOSAIC
        for k in pay:
            if k not in ("demosaic", "image_array"):
                assert pay[k] == plain[k], k


def test_the_gates_do_not_know_the_repair():
    assert "repair" not in inspect.signature(mosaic_rejection).parameters and "repair" not in inspect.signature(host_stream_gate).parameters


def test_the_keyword_is_a_load_keyword_of_every_entry():
    assert "raw_repair" in hip_processor._LOAD_KEYWORDS
    for name in ("process", "extract_image_data_cpu", "load_image_texture"):
        assert inspect.signature(getattr(HipProcessor, name)).parameters["raw_repair"].default is None, name
    assert HipProcessor.__new__(HipProcessor).last_raw_repair is None


def test_a_changed_record_invalidates_the_image_cache_and_an_equal_one_does_not(proc):
    uploads = []

    def prepare(payload):
        uploads.append(payload.get("demosaic"))
        proc._texture = ("frame", None, {})
        proc.image_param_dict = None

    proc.prepare_gpu_textures = prepare
    proc._texture = proc._texture_src = proc.image_param_dict = None
    proc.profile_stages = False
    proc.load_image_texture(MOSAIC, raw_profile=NUMERIC, raw_repair=HotPixels(1000), exposure=0.0)
    proc.load_image_texture(MOSAIC, raw_profile=NUMERIC, raw_repair=HotPixels(1000, 0.125, 4), exposure=0.0)
    assert len(uploads) == 1 and uploads[0]["repair"] == HotPixels(1000)
    proc.load_image_texture(MOSAIC, raw_profile=NUMERIC, raw_repair=HotPixels(1001), exposure=0.0)
    proc.load_image_texture(MOSAIC, raw_profile=NUMERIC, raw_repair=HotPixels(1001, min_neighbours=3), exposure=0.0)
    proc.load_image_texture(MOSAIC, raw_profile=NUMERIC, raw_repair=HotPixels(1001, 0.25, 3), exposure=0.0)
    proc.load_image_texture(MOSAIC, raw_profile=NUMERIC, exposure=0.0)
    assert len(uploads) == 5 and "repair" not in uploads[4]


# ---- the rows that travel with a streamed band
def windows(Hd):
    """tests/test_demosaic_stream_host.py's windows: odd and even origins, touching the top, the bottom, both or neither."""
    out = {(0, Hd)}
    for row0 in (0, 1, 2, 3, 5, 8):
        for rows in (1, 2, 7, Hd - row0 - 3, Hd - row0 - 1, Hd - row0):
            if rows >= 1 and row0 + rows <= Hd:
                out.add((row0, rows))
    return sorted(out)


@pytest.mark.parametrize("half", [False, True], ids=["full", "half"])
@pytest.mark.parametrize("median", [0, 2])
def test_every_bands_repaired_rows_lie_inside_what_has_been_uploaded(half, median):
    assert REPAIR_REACH == 2
    cases = 0
    for Hm in range(2, 81):
        if half and Hm % 2:
            continue
        Hd = Hm // 2 if half else Hm
        for row0, rows in windows(Hd):
            for n in range(1, 6):
                if n > rows:
                    continue
                bounds = [rows * i // n for i in range(n + 1)]
                window = (row0, 3, rows, 11)
                rb = mosaic_upload_bounds(bounds, window, Hm, half, median)
                assert rb == mosaic_upload_bounds(bounds, window, Hm, half, median, repair=0)
                ub = mosaic_upload_bounds(bounds, window, Hm, half, median, repair=REPAIR_REACH)
                what = (Hm, window, bounds, rb, ub)
                assert ub == [max(rb[0] - 2, 0)] + [min(b + 2, Hm) for b in rb[1:]], what
                assert all(a <= b for a, b in zip(ub[:-1], ub[1:])) and 0 <= ub[0] and ub[-1] <= Hm, what
                for k in range(n):  # band k repairs rows [rb[k], rb[k + 1]): the repair reads 2 rows either side, clipped to the frame
                    assert ub[0] <= max(rb[k] - 2, 0) and min(rb[k + 1] + 2, Hm) <= ub[k + 1], (what, k)
                cases += 1
    assert cases > 2000
