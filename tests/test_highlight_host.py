"""LibRaw's highlight modes 1 and 2 without a GPU: Scale with a highlight mode (r2f_raw_scale_plan_highlight) against the NumPy
model of include/r2f.h (tests/highlight_model.py) -- through the library and through a stand-alone program under AddressSanitizer /
UBSan (tests/highlight_check.cpp), which also runs mosaic::blend_pixel over a check set whose digest the model reproduces --, the
profiles' `highlight` field, `resolve`, the stream gates and phase 1's payload; the input conditions of the GPU tests' mosaics
(tests/test_gpu_highlight.py), checked here where they were chosen; and what a contracted multiply-add in blend_pixel would change."""

import ctypes
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import demosaic_model as dm
import highlight_model as hm
import levels_model as lm
import xtrans_model as xm
from raw2film_amd import _lib
from raw2film_amd.hip_processor import HipProcessor
from raw2film_amd.payload import stream_rejection
from raw2film_amd.raw import RawLevels, RawProfile, XTransProfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raw2film_amd", "csrc")
WB = hm.WB
BLACK4 = (512, 515, 509, 512)
BLACK36 = tuple(1024 + ((7 * i) % 36) for i in range(36))
MODES = {"clip": hm.CLIP, "unclip": hm.UNCLIP, "blend": hm.BLEND}


# ---- the planner against the model
def _cases():
    whites = ((16383, BLACK4), (4095 + 1024, BLACK36), (65535, (0,) * 4))
    wbs = (WB, (1.0, 1.0, 1.0), (3.0, 3.0, 3.0), (1.0, 2.5, 1.75), (1024.0, 1.0, 512.0), (1.0, 1.0, 1024.0), (0.3, 0.7, 0.11),
           (65535.0, 1.0, 65535.0),   # clip lands on 1: fl(65535 / 65535.0f) = 1
           (32767.4, 1.0, 2.0))       # ... and on 2
    for (white, black), wb, mode in itertools.product(whites, wbs, (0, 1, 2)):
        m = white - min(black)
        for thr, d in ((0.75, 0), (0.75, int(m * 0.9)), (0.0, int(m * 0.9)), (0.75, m)):
            yield wb, white, thr, black, d, mode


CASES = list(_cases())
REFUSED = [(WB, 16383, 0.75, BLACK4, 0, mode) for mode in (-1, 3, 4, 5, 6, 7, 8, 9, 10, 2 ** 31 - 1)]
REFUSED += [((65536.5, 1.0, 2.0), 16383, 0.75, BLACK4, 0, 2),  # clip = 0
            ((1.0, float("nan"), 1.0), 16383, 0.75, BLACK4, 0, 2), ((1.0, float("inf"), 1.0), 16383, 0.75, BLACK4, 0, 1),
            (WB, 509, 0.75, BLACK4, 0, 1), (WB, 16383, float("nan"), BLACK4, 0, 2), (WB, 16383, 0.75, BLACK4, 65536, 2),
            (WB, 16383, 0.75, (512, 512.5, 512, 512), 0, 1), (WB, 16383, 0.75, (512,) * 5, 0, 2)]


def _plan(wb, white, thr, black, d, mode):
    lv = _lib.RawLevels(white_level=white, adjust_maximum_thr=thr)
    lv.white_balance[:] = wb
    out, hl = _lib.RawScale(maximum_used=-77, adjusted=-88), _lib.Highlight(-55, -66)
    out.mul[:] = (-1.5, -2.5, -3.5)
    rc = _lib.load().r2f_raw_scale_plan_highlight(ctypes.byref(lv), (ctypes.c_double * len(black))(*black), len(black), d, mode,
                                                  ctypes.byref(out), ctypes.byref(hl))
    return rc, (tuple(out.mul), out.maximum_used, bool(out.adjusted), hl.clip), hl.mode


UNTOUCHED = ((-1.5, -2.5, -3.5), -77, True, -66)


def test_planner_equals_the_model_bit_for_bit():
    clips = set()
    for case in CASES:
        want = hm.scale(*case)
        rc, got, mode = _plan(*case)
        assert want is not None and rc == _lib.OK and got == want and mode == case[5], case
        clips.add(want[3])
        if case[5]:  # the largest factor becomes 1
            assert max(got[0]) == 65535.0 / got[1]
    assert {0, 1, 65535} <= clips and hm.scale(WB, 16383, 0.75, BLACK4, 0, 2)[3] == 31207
    # an adjusted maximum changes mul and does not change clip
    a, b = hm.scale(WB, 16383, 0.75, BLACK4, 0, 2), hm.scale(WB, 16383, 0.75, BLACK4, 15000, 2)
    assert b[2] and not a[2] and a[0] != b[0] and a[3] == b[3]


def test_mode_0_is_the_plain_planner_and_leaves_no_clip():
    for wb, white, thr, black, d, mode in CASES:
        if mode:
            continue
        plain = RawLevels(wb, white, thr).scale(black, d)
        rc, got, m = _plan(wb, white, thr, black, d, 0)
        assert rc == _lib.OK and m == 0 and got == (tuple(plain.mul), plain.maximum_used, bool(plain.adjusted), 0)
        assert got[:3] == lm.scale(wb, white, thr, black, d)


def test_refusals_leave_both_outputs_alone():
    for case in REFUSED:
        wb, _, thr, black, d, _ = case
        if np.isfinite(wb).all() and np.isfinite(thr) and len(black) == 4 and d <= 65535 and all(b == int(b) for b in black):
            assert hm.scale(*case) is None, case  # (the model states the definition's refusals, not the argument checks)
        rc, got, mode = _plan(*case)
        assert rc == _lib.EINVAL and got == UNTOUCHED and mode == -55, case
    lib, lv = _lib.load(), RawLevels(WB, 16383).to_c()
    black, out, hl = (ctypes.c_double * 4)(*BLACK4), _lib.RawScale(), _lib.Highlight()
    assert lib.r2f_raw_scale_plan_highlight(ctypes.byref(lv), black, 4, 0, 2, None, ctypes.byref(hl)) == _lib.EINVAL
    assert lib.r2f_raw_scale_plan_highlight(ctypes.byref(lv), black, 4, 0, 2, ctypes.byref(out), None) == _lib.EINVAL
    assert lib.r2f_raw_scale_plan_highlight(None, black, 4, 0, 2, ctypes.byref(out), ctypes.byref(hl)) == _lib.EINVAL
    assert lib.r2f_raw_scale_plan_highlight(ctypes.byref(lv), black, 4, 0, 2, ctypes.byref(out), ctypes.byref(hl)) == _lib.OK


def test_struct_layout_and_header_text():
    H = _lib.Highlight
    assert ctypes.sizeof(H) == 8 and (H.mode.offset, H.clip.offset) == (0, 4)
    assert [ctypes.sizeof(t) for t in (_lib.RawProfile, _lib.DemosaicParams, _lib.XTransProfile, _lib.XTransParams)] == [144, 96, 536, 900]
    assert (ctypes.sizeof(_lib.RawLevels), ctypes.sizeof(_lib.RawScale)) == (40, 32)
    text = open(os.path.join(ROOT, "include", "r2f.h")).read()
    part = text[text.index("LibRaw's highlight modes 1 (unclip) and 2 (blend)"):text.index("typedef struct r2f_highlight")]
    for word in ("UNPINNED", "0x1.bb67aep+0f", "0x1.bb67aep-1f", "sum[0] == 0", "rebuild"):
        assert word in part, word
    assert float.fromhex("0x1.bb67aep+0") == float(np.float32(1.7320508)) and float.fromhex("0x1.bb67aep-1") == float(np.float32(0.8660254))
    assert "R2F_HIGHLIGHT_CLIP = 0, R2F_HIGHLIGHT_UNCLIP = 1, R2F_HIGHLIGHT_BLEND = 2" in text
    assert (_lib.HIGHLIGHT_CLIP, _lib.HIGHLIGHT_UNCLIP, _lib.HIGHLIGHT_BLEND) == (0, 1, 2)


# ---- the stand-alone program
@pytest.fixture(scope="module")
def highlight_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("highlight_check") / "highlight_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
           "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "highlight_check.cpp"), os.path.join(CSRC, "r2f_levels_plan.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def test_the_program_plans_the_grid_to_the_models_numbers(highlight_check, tmp_path):
    cases = CASES + REFUSED
    job = tmp_path / "job.txt"
    job.write_text("".join(" ".join([*(float(v).hex() for v in wb), str(white), float(thr).hex(), str(d), str(mode), str(len(black)),
                                     *(float(b).hex() for b in black)]) + "\n" for wb, white, thr, black, d, mode in cases))
    res = subprocess.run([highlight_check, "plan", str(job)], capture_output=True, text=True, env=ENV, timeout=120)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    lines = res.stdout.splitlines()
    assert len(lines) == len(cases)
    for line, case in zip(lines[:len(CASES)], CASES):
        rc, m0, m1, m2, used, adjusted, mode, clip = line.split()
        got = (tuple(float.fromhex(v) for v in (m0, m1, m2)), int(used), bool(int(adjusted)), int(clip))
        assert int(rc) == _lib.OK and got == hm.scale(*case) and int(mode) == case[5], case
    assert lines[len(CASES):] == [str(_lib.EINVAL)] * len(REFUSED)


@pytest.mark.parametrize("seed", [2, 20261020])
def test_planner_fuzz_is_clean_under_the_sanitizers(highlight_check, seed):
    res = subprocess.run([highlight_check, "fuzz", str(seed), "20000"], capture_output=True, text=True, env=ENV, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    assert "cases ok" in res.stdout


CHECK_CLIPS = (1, 2, 255, 4096, 31207, 40000, 65534, 65535)


def check_set(clip):
    """tests/highlight_check.cpp's check set for one clip level: int64 (3, n)."""
    edge = sorted({min(max(v, 0), 65535) for v in (0, 1, clip - 1, clip, clip + 1, clip + 2, clip + clip // 2, 2 * clip, 32768, 65534, 65535)})
    triples = [t for t in itertools.product(edge, repeat=3)]
    x, values = clip, []
    for _ in range(60000):
        x = (x * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        values.append((x >> 33) % 65536)
    for i in range(20000):
        a, b, c = values[3 * i:3 * i + 3]
        triples.append((a, a, a) if i % 4 == 3 else (a, b, c))
    return np.array(triples, dtype=np.int64).T


def digest(o):
    i = np.arange(o.shape[1], dtype=np.uint64)
    u = o.astype(np.uint64)
    with np.errstate(over="ignore"):
        return int(((u[0] + np.uint64(65536) * u[1] + np.uint64(65536 ** 2) * u[2] + np.uint64(1)) * (np.uint64(2) * i + np.uint64(1))).sum(dtype=np.uint64))


def test_the_program_blends_the_check_set_to_the_models_digest(highlight_check):
    res = subprocess.run([highlight_check, "blend"], capture_output=True, text=True, env=ENV, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    lines = [tuple(int(v) for v in line.split()) for line in res.stdout.splitlines()]
    assert [line[0] for line in lines] == list(CHECK_CLIPS)
    for clip, count, changed, got in lines:
        v = check_set(clip)
        o = hm.blend(v, clip)
        assert (count, changed, got) == (v.shape[1], int((o != v).any(axis=0).sum()), digest(o)), clip


def test_the_check_set_holds_the_named_pixels():
    for clip in CHECK_CLIPS:
        triples = set(map(tuple, check_set(clip).T))
        assert (65535, 65535, 65535) in triples and (clip, clip, clip) in triples
        if clip < 65535:
            assert {(clip + 1, clip, clip), (clip, clip + 1, 0), (0, 0, clip + 1), (clip + 1,) * 3, (65535, clip + 1, clip + 1)} <= triples
    # the definition's stated cases, on the model
    assert hm.blend_pixel((31207, 31207, 31207), 31207) == (31207, 31207, 31207) and hm.blend_pixel((5, 31207, 0), 31207) == (5, 31207, 0)
    for v in (40000, 65535, 31208):  # sum[0] == 0: chratio is 1 and the pixel leaves as it came
        assert hm.blend_pixel((v, v, v), 31207) == (v, v, v)
    for clip in (1, 31207, 65535):
        assert hm.blend_pixel((65535, 65535, 65535), clip) == (65535, 65535, 65535)
    assert hm.blend_pixel((65535, 2, 7), 65535) == (65535, 2, 7)  # clip = 65535: nothing is above it
    r, g, b = hm.blend_pixel((65535, 31207, 45000), 31207)  # towards neutral: the chroma shrinks, the sum of the channels stays
    assert max(r, g, b) - min(r, g, b) < 65535 - 31207 and abs(r + g + b - (65535 + 31207 + 45000)) <= 3
    stats = {}
    hm.blend(check_set(31207), 31207, stats)
    assert all(stats[k] > 0 for k in hm.CLASSES), stats


def test_a_contracted_multiply_add_changes_outputs_of_the_check_set_and_of_the_gpu_fixtures():
    """What lets tests/test_gpu_highlight.py notice a kernel built with contraction: the fused restatement of the model differs from
    the separate one on pixels of the check set and on pixels of the very planes the GPU tests blend.  The truncation of acc / 3
    hides most last-bit differences, so the share is small; what is required is that it is not zero (the counts are printed)."""
    differing = 0
    for clip in CHECK_CLIPS:
        v = check_set(clip)
        differing += int((hm.blend(v, clip) != hm.blend(v, clip, fused=True)).any(axis=0).sum())
    print(f"check set: fused != separate on {differing} triples")
    assert differing > 0
    on_fixtures = 0
    for planes, clip in _fixture_planes():
        on_fixtures += int((hm.blend(planes, clip) != hm.blend(planes, clip, fused=True)).any(axis=0).sum())
    print(f"GPU fixtures: fused != separate on {on_fixtures} pixels")
    assert on_fixtures > 0


# ---- the GPU tests' mosaics: conditions on the inputs
def _fixture_planes(kinds=("equal", "wb")):
    for kind in kinds:
        for pattern, shape, half in itertools.product(dm.PATTERNS, (hm.ONE_TILE, hm.BAYER_FRAME), (False, True)):
            mosaic, prof, clip = hm.bayer_case(kind, pattern, shape)
            yield hm.planes(mosaic, dm.constants(prof, *shape, half), False), clip
        for pattern, shape, half in itertools.product(xm.PATTERNS[:2], (hm.ONE_TILE, hm.XTRANS_FRAME), (False, True)):
            mosaic, prof, clip = hm.xtrans_case(kind, pattern, shape)
            yield hm.planes(mosaic, xm.constants(prof, *shape, half), True), clip


def test_the_gpu_fixtures_meet_their_conditions():
    assert hm.ONE_TILE == (38, 70) and hm.BAYER_FRAME == (58, 182) and hm.XTRANS_FRAME == (59, 185)
    assert all(s % 3 for s in hm.ONE_TILE + hm.XTRANS_FRAME) and not any(s % 2 for s in hm.ONE_TILE + hm.BAYER_FRAME)
    for kind in ("equal", "wb"):
        for planes, clip in _fixture_planes((kind,)):
            stats = {}
            hm.blend(planes, clip, stats)
            assert stats["blended"] >= hm.MIN_BLENDED * stats["pixels"], (kind, planes.shape, stats)
            if kind == "equal":
                assert all(stats[k] > 0 for k in hm.CLASSES), (planes.shape, stats)
            else:
                assert stats["above_1"] > 0 and stats["above_2"] > 0, (planes.shape, stats)


# ---- the profiles' field
LEVELS = RawLevels(WB, 16383)


@pytest.mark.parametrize("cls", [RawProfile, XTransProfile])
def test_default_profiles_are_what_they_were(cls):
    a = cls()
    assert a.highlight == "clip" and a.blend_clip is None and a == cls(highlight="clip") and hash(a) == hash(cls(highlight="clip"))
    assert [f for f in cls.__dataclass_fields__] == ["pattern", "black", "multipliers", "matrix", "highlight", "orientation"]
    assert cls(cls().pattern, 0, (1.0, 1.0, 1.0), cls().matrix, 5).orientation == 5  # (the positional order is what it was)
    with pytest.raises(TypeError):
        cls(cls().pattern, 0, (1.0, 1.0, 1.0), cls().matrix, 5, "clip")
    d = cls(black=512, multipliers=LEVELS)
    assert d.highlight == "clip" and d.resolve(0).highlight == "clip"
    assert tuple(d.resolve(13000).multipliers) == tuple(cls(multipliers=lm.scale(WB, 16383, 0.75, d.black, 13000)[0]).multipliers)
    assert bytes(d.to_c()) == bytes(cls(black=512, multipliers=lm.scale(WB, 16383, 0.75, d.black, 0)[0]).to_c())


@pytest.mark.parametrize("cls", [RawProfile, XTransProfile])
def test_the_field_takes_part_in_equality_and_hash(cls):
    a, b = cls(highlight=("blend", 31207)), cls(highlight=["blend", np.int64(31207)])
    assert a == b and hash(a) == hash(b) and a.blend_clip == 31207 and type(a.highlight[1]) is int
    assert a != cls() and a != cls(highlight=("blend", 31206)) and len({a, cls(), cls(highlight=("blend", 1))}) == 3
    d = [cls(black=512, multipliers=LEVELS, highlight=h) for h in ("clip", "unclip", "blend")]
    assert len(set(d)) == 3 and d[1] == cls(black=512, multipliers=RawLevels(WB, 16383), highlight="unclip") and d[1].blend_clip is None
    with pytest.raises(Exception):
        a.highlight = "clip"


@pytest.mark.parametrize("cls", [RawProfile, XTransProfile])
def test_every_refusal_of_the_field(cls):
    for h in ("unclip", "blend"):
        with pytest.raises(ValueError, match=rf"{cls.__name__}\.highlight = '{h}'.*RawLevels"):
            cls(highlight=h)
    for h in ("rebuild", 3, 4, 5, 6, 7, 8, 9, ("rebuild", 5)):
        for kw in ({}, {"multipliers": LEVELS}):
            with pytest.raises(ValueError, match=rf"{cls.__name__}\.highlight.*rebuild modes.*not built"):
                cls(highlight=h, **kw)
    for h in (("blend", 0), ("blend", 65536), ("blend", 5.0), ("blend", True), ("blend",), ("blend", 5, 6), ("clip", 5), "Clip", 0, 1, 2, 10, None,
              True, ("unclip", 5)):
        with pytest.raises(ValueError, match=rf"{cls.__name__}\.highlight must be"):
            cls(highlight=h)
    for h in (("blend", 31207), "Blend", 1, 2, None, 0):
        with pytest.raises(ValueError, match=rf"{cls.__name__}\.highlight of a profile with RawLevels"):
            cls(multipliers=LEVELS, highlight=h)
    assert cls(highlight=("blend", 1)).blend_clip == 1 and cls(highlight=("blend", 65535)).blend_clip == 65535


@pytest.mark.parametrize("cls, black", [(RawProfile, BLACK4), (XTransProfile, BLACK36)])
def test_resolve_round_trip(cls, black):
    for name, d in itertools.product(MODES, (0, 12000, 15000, 65535)):
        deferred = cls(black=black, multipliers=LEVELS, matrix=dm.CAMERA, orientation=5, highlight=name)
        mul, used, adjusted, clip = hm.scale(WB, 16383, 0.75, black, d, MODES[name])
        resolved, scale = deferred.resolve_scale(d)
        numeric = cls(black=black, multipliers=mul, matrix=dm.CAMERA, orientation=5, highlight=("blend", clip) if name == "blend" else "clip")
        assert resolved == numeric == deferred.resolve(d) and hash(resolved) == hash(numeric) and not resolved.deferred
        assert (tuple(scale.mul), scale.maximum_used, bool(scale.adjusted)) == (mul, used, adjusted)
        assert resolved.blend_clip == (clip if name == "blend" else None) and resolved.resolve(7) is resolved
        assert resolved.resolve_scale(7) == (resolved, None)
        if d == 0:  # a deferred profile plans, and states in C, its nominal scale -- that of its mode
            assert bytes(deferred.to_c()) == bytes(numeric.to_c())
            assert bytes(deferred.plan(48, 66)) == bytes(numeric.plan(48, 66))
    unclip = cls(black=black, multipliers=LEVELS, highlight="unclip").resolve(0)
    assert max(unclip.multipliers) == 65535.0 / (16383 - min(black)) and unclip.highlight == "clip"
    with pytest.raises(ValueError, match="r2f_raw_scale_plan_highlight"):
        cls(black=black, multipliers=RawLevels((65536.5, 1.0, 2.0), 16383), highlight="blend").resolve(0)  # clip < 1
    with pytest.raises(ValueError, match="r2f_raw_scale_plan"):
        cls(black=black, multipliers=RawLevels(WB, 100), highlight="unclip").resolve(0)
    with pytest.raises(ValueError, match="data maximum"):
        cls(black=black, multipliers=LEVELS, highlight="blend").resolve(65536)


def test_scale_highlight_of_the_levels():
    scale, hl = LEVELS.scale_highlight(BLACK4, 15000, "blend")
    assert (tuple(scale.mul), scale.maximum_used, bool(scale.adjusted), hl.clip) == hm.scale(WB, 16383, 0.75, BLACK4, 15000, 2) and hl.mode == 2
    scale, hl = LEVELS.scale_highlight(BLACK4, 15000)
    assert tuple(scale.mul) == tuple(LEVELS.scale(BLACK4, 15000).mul) and (hl.mode, hl.clip) == (0, 0)
    with pytest.raises(ValueError, match="highlight mode"):
        LEVELS.scale_highlight(BLACK4, 0, "rebuild")


# ---- the gates and phase 1 of the processor
@pytest.fixture
def proc():
    p = HipProcessor.__new__(HipProcessor)
    p.cameras = p.lenses = None
    p.payload_alpha = True
    return p


MOSAIC, NUMERIC = dm.fixture("random", "GRBG", 96, 144)
BLEND = RawProfile("GRBG", black=NUMERIC.black, multipliers=NUMERIC.multipliers, matrix=NUMERIC.matrix, highlight=("blend", 31207))


def test_a_blend_profiles_payload_adds_the_clip_and_nothing_else(proc):
    for kw in (dict(exposure=0.5), dict(exposure=0.5, half_size=False), dict(exposure=None, zoom=1.3)):
        pay = proc.extract_image_data_cpu(MOSAIC, raw_profile=BLEND, **kw)
        plain = proc.extract_image_data_cpu(MOSAIC, raw_profile=NUMERIC, **kw)
        assert set(pay) == set(plain) and set(pay["demosaic"]) == set(plain["demosaic"]) | {"clip"} and pay["demosaic"]["clip"] == 31207
        assert "clip" not in plain["demosaic"] and bytes(pay["demosaic"]["params"]) == bytes(plain["demosaic"]["params"])
        for k in pay:
            if k not in ("demosaic", "image_array", "warp"):
                assert pay[k] == plain[k], k
    deferred = RawProfile("GRBG", black=NUMERIC.black, multipliers=LEVELS, matrix=NUMERIC.matrix, highlight="blend")
    step = proc.extract_image_data_cpu(MOSAIC, raw_profile=deferred, exposure=0.5)["demosaic"]
    assert set(step) == {"params", "window", "rotate_times", "levels"} and step["levels"] is deferred  # (the clip comes with the scale)
    x = XTransProfile(black=512, multipliers=(2.0, 1.0, 1.5), highlight=("blend", 500), orientation=6)
    step = proc.extract_image_data_cpu(MOSAIC, raw_profile=x, exposure=0.0)["demosaic"]
    assert set(step) == {"params", "window", "rotate_times", "orientation", "clip"} and step["clip"] == 500


def test_both_gates_answer_for_a_blend_profile_as_for_a_plain_one(proc, monkeypatch):
    settings = dict(rotation=0.0, chroma_nr=0, canvas_mode="No", highlight_burn=0.0, lens_correction=False, lens_profile=None, exposure=0.5,
                    rotate_times=0, half_size=False, frame_width=36, frame_height=24, flip=False, zoom=1.0)
    proc.stream_bands = 16
    big = np.zeros((4096, 6144), np.uint16)
    for src in (MOSAIC, big):
        for extra in ({}, dict(rotate_times=1), dict(exposure=None), dict(rotation=2.5)):
            a = proc._host_stream_gate(src, {**settings, **extra, "raw_profile": BLEND})
            b = proc._host_stream_gate(src, {**settings, **extra, "raw_profile": NUMERIC})
            assert a == b, (src.shape, extra)
    assert proc._host_stream_gate(big, {**settings, "raw_profile": BLEND}) is None
    deferred = RawProfile("GRBG", multipliers=LEVELS, highlight="blend")
    assert "RawLevels" in proc._host_stream_gate(big, {**settings, "raw_profile": deferred})
    pay = proc.extract_image_data_cpu(MOSAIC, raw_profile=BLEND, exposure=0.5, half_size=False)
    plain = proc.extract_image_data_cpu(MOSAIC, raw_profile=NUMERIC, exposure=0.5, half_size=False)
    args = ((96, 144), "torch.int16", False, "gpu")
    assert stream_rejection(pay, *args) == stream_rejection(plain, *args) and "below 16.7 M" in stream_rejection(pay, *args)
    monkeypatch.setattr("raw2film_amd.payload.STREAM_MIN_SAMPLES", 1)
    assert stream_rejection(pay, *args) is None and stream_rejection(plain, *args) is None


def test_a_changed_clip_invalidates_the_image_cache_and_an_equal_one_does_not(proc):
    uploads = []

    def prepare(payload):
        uploads.append(payload.get("demosaic"))
        proc._texture = ("frame", None, {})
        proc.image_param_dict = None

    proc.prepare_gpu_textures = prepare
    make = lambda h: RawProfile("GRBG", black=64, multipliers=(2.0, 1.0, 1.5), highlight=h)  # noqa: E731
    proc.load_image_texture(MOSAIC, raw_profile=make(("blend", 31207)), exposure=0.0)
    proc.load_image_texture(MOSAIC, raw_profile=make(["blend", 31207]), exposure=0.0)
    assert len(uploads) == 1 and uploads[0]["clip"] == 31207
    proc.load_image_texture(MOSAIC, raw_profile=make(("blend", 31208)), exposure=0.0)
    proc.load_image_texture(MOSAIC, raw_profile=make("clip"), exposure=0.0)
    assert len(uploads) == 3 and "clip" not in uploads[2]
