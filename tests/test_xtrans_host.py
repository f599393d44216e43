"""The X-Trans demosaic's host half, without a GPU: the NumPy model of the definition (tests/xtrans_model.py) in its two forms, the
planner (raw2film_amd/csrc/r2f_xtrans_plan.cpp) and the shared arithmetic (r2f_xtrans_math.h) in a stand-alone program under
AddressSanitizer / UBSan (tests/xtrans_check.cpp), XTransProfile's validation, the payload of phase 1 and the ABI structs.

The bit-for-bit comparison of the program's renders with the model pins the arithmetic the GPU runs, on this machine: the same
text compiled for the CPU with contraction off.  That the device compiles it to the same bytes is tests/test_gpu_xtrans.py's."""

import ctypes
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import xtrans_model as xm
from raw2film_amd import _lib
from raw2film_amd.hip_processor import HipProcessor
from raw2film_amd.payload import host_stream_gate, mosaic_frame_samples, stream_rejection
from raw2film_amd.raw import XTRANS, RawProfile, XTransProfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raw2film_amd", "csrc")
SMALL = [(6, 6), (7, 7), (9, 11), (13, 20)]
ALL_SHIFTS = [xm.shifted(dy, dx) for dy in range(6) for dx in range(6)]
# admissible arrays that are not Fujifilm's: a few sites of the layout recoloured (weight sums 1 .. 7, the divisor 1 among them),
# and a Bayer quad tiled to 6 x 6 (every gap 1, every weight sum 4)
OTHER_PATTERNS = [("GBGGRG", "RGRBGB", "GBGGRG", "GRGGBB", "GGBRGR", "GRGRBG"), ("GBBGRG", "RGRBGB", "GBGGRG", "BRGGBG", "BGBRGR", "GRGGBB"),
                  ("RGRGRG", "GBGBGB") * 3]


# ---- the model
@pytest.mark.parametrize("pattern", xm.PATTERNS, ids=lambda p: p[0])
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_vectorised_model_equals_the_sequential_one(pattern, shape):
    for kind in xm.KINDS:
        mosaic, prof = xm.fixture(kind, pattern, *shape)
        assert np.array_equal(xm.demosaic(mosaic, prof), xm.demosaic(mosaic, prof, sequential=True)), kind


def test_the_four_patterns_put_every_phase_at_a_tile_origin():
    """Tile sides 4 and 2 modulo 6, three tiles each way: with the four shifts the canonical layout's 36 phases all start a tile."""
    assert (xm.TILE_W % 6, xm.TILE_H % 6) == (4, 2)
    seen = {((ty * xm.TILE_H + dy) % 6, (tx * xm.TILE_W + dx) % 6) for dy, dx in ((0, 0), (1, 0), (0, 1), (1, 1)) for ty in range(3) for tx in range(3)}
    assert len(seen) == 36
    assert xm.PATTERNS[0] == XTRANS and len(set(xm.PATTERNS)) == 4
    # (the layout is its own shift by (3, 3): its 36 cyclic shifts are 18 arrays, each met twice)
    assert len(set(ALL_SHIFTS)) == 18 and xm.shifted(3, 3) == XTRANS


# (kind -> the counters it is there for; every one must be above zero on the largest frame of the GPU tests, for every pattern)
EXERCISES = {
    "random": ("b1_vertical", "b1_horizontal", "a_negative", "a_clip_65535", "c_clip_0", "c_clip_65535"),
    "extremes": ("b2_clip_0", "b2_clip_65535", "b2_negative_numerator", "b2_inexact_negative", "b1_vertical", "b1_horizontal"),
}


@pytest.mark.parametrize("pattern", xm.PATTERNS, ids=lambda p: p[0])
def test_fixtures_are_not_vacuous(pattern):
    """The frame built per colour plane from {0, 65535} drives B2's sum below 0 and above 65535 -- both clamps -- and through floor
    divisions of negative numerators that are not exact; the random one clamps step A and step C at both ends."""
    for kind, wanted in EXERCISES.items():
        for shape in ((9, 11), (3 * xm.TILE_H + 5, 3 * xm.TILE_W + 5)):
            stats = {}
            mosaic, prof = xm.fixture(kind, pattern, *shape)
            out = xm.demosaic(mosaic, prof, stats=stats)
            assert out.shape == shape + (3,) and out.dtype == np.uint16
            if shape[0] > 9:
                assert [k for k in wanted if stats.get(k, 0) <= 0] == [], (kind, stats)
    mosaic, prof = xm.fixture("extremes", pattern, 9, 11)
    assert set(np.unique(mosaic)) == {0, 65535}


@pytest.mark.parametrize("pattern", ALL_SHIFTS[::5], ids=lambda p: p[0] + p[1])
def test_a_flat_colour_field_comes_back_exactly_in_the_interior(pattern):
    prof = XTransProfile(pattern)
    H, W = 19, 23
    flat = np.array([30000, 20000, 10000])
    col = xm.colour_map(xm.constants(prof, H, W), H, W)
    out = xm.demosaic(flat[col].astype(np.uint16), prof)
    assert np.array_equal(out[3:-3, 3:-3], np.broadcast_to(flat, (H - 6, W - 6, 3)))
    third = xm.demosaic(flat[col].astype(np.uint16), prof, half_size=True)
    assert third.shape == (6, 7, 3) and np.array_equal(third, np.broadcast_to(flat, (6, 7, 3)))


@pytest.mark.parametrize("half", [False, True], ids=["full", "third"])
def test_the_model_is_band_invariant(half):
    """Output rows [y0, y1) are a function of the mosaic rows the contract names: whatever lies outside them changes no byte."""
    H, W = 40, 29
    mosaic, prof = xm.fixture("random", xm.PATTERNS[3], H, W)
    want = xm.demosaic(mosaic, prof, half_size=half)
    rng = np.random.default_rng(9)
    cuts = [0, 1, 4, 5, 11, want.shape[0] - 2, want.shape[0]]  # (not multiples of 6 or 3)
    for y0, y1 in zip(cuts[:-1], cuts[1:]):
        lo, hi = xm.source_rows(y0, y1, H, half)
        other = rng.integers(0, 65536, (H, W), dtype=np.uint16)
        other[lo:hi] = mosaic[lo:hi]
        assert np.array_equal(xm.demosaic(other, prof, half_size=half)[y0:y1], want[y0:y1]), (y0, y1)
    # ... and the reach is 3 rows, not 2: for some row phases a row at distance 3 matters, for none a row further away
    reach = set()
    for row in range(18, 24):
        other = mosaic.copy()
        other[row] ^= 0x5555
        changed = np.flatnonzero((xm.demosaic(other, prof, half_size=half) != want).any(axis=(1, 2)))
        reach |= {int(y) - row for y in changed} if not half else {int(y) - row // 3 for y in changed}
    assert reach == ({0} if half else {-3, -2, -1, 0, 1, 2, 3})


def test_reduced_size_is_the_cell_rule_and_drops_the_tail():
    mosaic, prof = xm.fixture("random", XTRANS, 8, 10)
    prof = XTransProfile(XTRANS)
    out = xm.demosaic(mosaic, prof, half_size=True)
    assert out.shape == (2, 3, 3)
    m = mosaic.astype(np.int64)
    cell = m[3:6, 6:9]  # rows 3 .. 5 of the layout, columns 0 .. 2: GRG / BGB / GRG
    assert XTRANS[3][:3] == "GRG" and XTRANS[4][:3] == "BGB"
    assert out[1, 2, 0] == (cell[0, 1] + cell[2, 1]) // 2 and out[1, 2, 2] == (cell[1, 0] + cell[1, 2]) // 2
    assert out[1, 2, 1] == (cell[0, 0] + cell[0, 2] + cell[1, 1] + cell[2, 0] + cell[2, 2]) // 5


# ---- the stand-alone program
@pytest.fixture(scope="module")
def xtrans_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("xtrans_check") / "xtrans_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
           "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "xtrans_check.cpp"), os.path.join(CSRC, "r2f_xtrans_plan.cpp"),
           "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


@pytest.mark.parametrize("seed", [1, 20261019])
def test_planner_fuzz_is_clean_under_the_sanitizers(xtrans_check, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([xtrans_check, "fuzz", str(seed), "10000"], capture_output=True, text=True, env=env, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    assert "cases ok" in res.stdout


def test_floor_divisions_equal_pythons_on_negative_numerators(xtrans_check):
    """floor_div of r2f_xtrans_math.h (bias, then the high word of a multiply) against Python's //: every divisor 1 .. 12, the ends
    of the range |n| <= 12 * 65535, every numerator next to a multiple of the divisor near them and near 0, and random ones."""
    rng = np.random.default_rng(3)
    top = 12 * 65535
    cases = []
    for d in range(1, 13):
        ns = {-top, top, -top + 1, top - 1, 0, -1, 1}
        for base in (-top, -65535 * d, -65535, -d * 1000, 0, d * 1000, 65535, 65535 * d, top):
            q = base // d * d
            ns.update(n for n in range(q - d - 1, q + d + 2) if -top <= n <= top)
        ns.update(int(n) for n in rng.integers(-top, top + 1, 3000))
        ns.update(-int(n) for n in rng.integers(1, 40, 200))
        cases += [(n, d) for n in sorted(ns)]
    assert sum(n < 0 and n % d for n, d in cases) > 10000
    text = "".join(f"{n} {d}\n" for n, d in cases)
    res = subprocess.run([xtrans_check, "div"], input=text, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    got = [int(v) for v in res.stdout.split()]
    assert got == [n // d for n, d in cases]


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
    n = ctypes.sizeof(_lib.XTransParams)
    params = _lib.XTransParams.from_buffer_copy(raw[:n])
    return params, np.frombuffer(raw[n:], dtype=np.uint16).reshape(params.out_h, params.out_w, 3)


def _same_constants(a, b):
    return (np.array_equal(a.cfa, b.cfa) and np.array_equal(a.black, b.black) and np.array_equal(a.mul.view(np.uint32), b.mul.view(np.uint32))
            and np.array_equal(a.M.view(np.uint32), b.M.view(np.uint32)) and (a.reduced, a.out_h, a.out_w) == (b.reduced, b.out_h, b.out_w))


@pytest.mark.parametrize("pattern", xm.PATTERNS, ids=lambda p: p[0])
def test_shared_arithmetic_renders_the_model_bit_for_bit(xtrans_check, tmp_path, pattern):
    for shape in SMALL + [(39, 71)]:
        for kind in xm.KINDS:
            mosaic, prof = xm.fixture(kind, pattern, *shape)
            for half in (False, True):
                params, got = _render(xtrans_check, tmp_path, mosaic, prof, half)
                assert _same_constants(xm.from_params(params), xm.constants(prof, *shape, half_size=half)), (kind, shape, half)
                assert np.array_equal(got, xm.demosaic(mosaic, prof, half_size=half)), (kind, shape, half)


def test_shared_arithmetic_on_a_pattern_that_is_not_fujifilms(xtrans_check, tmp_path):
    """Nothing is special-cased to the canonical layout: an admissible array with other gaps and weight sums renders the model."""
    rng = np.random.default_rng(11)
    for pattern in OTHER_PATTERNS:
        prof = XTransProfile(pattern, black=64, multipliers=(1.9, 1.0, 1.4), matrix=xm.CAMERA)
        for shape in ((13, 20), (39, 41)):
            for mosaic in (rng.integers(0, 65536, shape, dtype=np.uint16), (rng.integers(0, 2, shape) * 65535).astype(np.uint16)):
                for half in (False, True):
                    _, got = _render(xtrans_check, tmp_path, mosaic, prof, half)
                    assert np.array_equal(got, xm.demosaic(mosaic, prof, half_size=half)), (pattern, shape, half)
        assert np.array_equal(xm.demosaic(mosaic[:9, :11], prof), xm.demosaic(mosaic[:9, :11], prof, sequential=True))


def test_the_other_patterns_have_other_tables():
    sums = set()
    for pattern in OTHER_PATTERNS:
        params = XTransProfile(pattern).plan(12, 12, True)
        sums |= {params.wsum[ph][slot] for ph in range(36) for slot in range(2)}
    canonical = XTransProfile().plan(12, 12)
    assert {canonical.wsum[ph][slot] for ph in range(36) for slot in range(2)} < sums and {1, 2, 5, 6, 7} <= sums


# ---- the planner
def _plan(layout=XTRANS, H=40, W=60, reduced=0, **changes):
    p = XTransProfile(black=64, multipliers=(2.0, 1.0, 1.5), matrix=xm.CAMERA).to_c(bool(reduced))
    p.pattern[:] = ["RGB".index(c) for row in layout for c in row]
    for k, v in changes.items():
        getattr(p, k)[v[0]] = v[1]
    out = _lib.XTransParams()
    return _lib.load().r2f_xtrans_plan(ctypes.byref(p), H, W, ctypes.byref(out)), out


def _at(p, y, x):
    return p[y % 6][x % 6]


def _gaps_ok(p):
    return all(_at(p, y + dy, x + dx) == "G" or _at(p, y + 2 * dy, x + 2 * dx) == "G" for y in range(6) for x in range(6) if p[y][x] != "G"
               for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)))


def _centred_ok(p):
    return all(set("RGB") - {p[y][x]} <= {_at(p, y + dy, x + dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx}
               for y in range(6) for x in range(6))


def _cells_ok(p):
    return all(len({p[cy + j][cx + i] for j in range(3) for i in range(3)}) == 3 for cy in (0, 3) for cx in (0, 3))


def test_planner_accepts_all_36_shifts_and_tables_what_the_model_finds():
    for pattern in ALL_SHIFTS:
        assert _gaps_ok(pattern) and _centred_ok(pattern) and _cells_ok(pattern)
        for reduced in (0, 1):
            rc, out = _plan(pattern, reduced=reduced)
            assert rc == _lib.OK, (pattern, reduced)
            assert (out.out_h, out.out_w, out.reduced) == ((13, 20, 1) if reduced else (40, 60, 0))
        for ph in range(36):
            y, x = divmod(ph, 6)
            assert "RGB"[out.cfa[ph]] == pattern[y][x]
            if pattern[y][x] == "G":
                assert list(out.gap[ph]) == [0, 0, 0, 0]
            else:
                want = [next(d for d in (1, 2) if _at(pattern, y + d * dy, x + d * dx) == "G") for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0))]
                assert list(out.gap[ph]) == want
            for slot, c in enumerate("RB"):
                q = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy or dx) and _at(pattern, y + dy, x + dx) == c]
                if c == pattern[y][x]:
                    q = []
                w = sum(2 if dy == 0 or dx == 0 else 1 for dy, dx in q)
                assert out.taps[ph][slot] == sum(1 << ((dy + 1) * 3 + dx + 1) for dy, dx in q) and out.wsum[ph][slot] == w
                assert out.recip[ph][slot] == (2 ** 32 // w + 1 if w > 1 else 0)
        for cell in range(4):
            cy, cx = 3 * (cell >> 1), 3 * (cell & 1)
            assert list(out.cell_count[cell]) == [sum(pattern[cy + j][cx + i] == c for j in range(3) for i in range(3)) for c in "RGB"]


def test_planner_refuses_patterns_that_are_not_admissible():
    assert _plan()[0] == _lib.OK and _plan(reduced=1)[0] == _lib.OK
    no_blue = tuple(row.replace("B", "R") for row in XTRANS)
    assert _gaps_ok(no_blue) and _plan(no_blue)[0] == _lib.EINVAL
    run_of_3 = ("GBGGRG", "RGRBGB", "GBGGRG", "GRGGBG", "BBBRGR", "GRGGBG")  # B B B along a row: the middle one has no green within 2
    assert not _gaps_ok(run_of_3) and _centred_ok(run_of_3) and _plan(run_of_3)[0] == _lib.EINVAL
    assert _plan(tuple("".join(r) for r in zip(*run_of_3)))[0] == _lib.EINVAL  # ... and along a column
    no_red_near = ("GBGGRG", "RGRBGB", "GBGGRG", "GRGGBG", "BGBRGG", "GRGGBG")  # gaps fine, a centred 3 x 3 without red
    assert _gaps_ok(no_red_near) and not _centred_ok(no_red_near) and _plan(no_red_near)[0] == _lib.EINVAL
    rc, out = _plan(run_of_3)
    assert bytes(out) == bytes(_lib.XTransParams())  # a refusal leaves the params alone


def test_an_aligned_cell_lacking_a_colour_is_refused_and_cannot_be_a_full_size_only_case():
    """The reduced size needs all three colours in each aligned 3 x 3 cell.  An aligned cell is the centred 3 x 3 of its middle site,
    which holds the site's colour and (the rule for every size) both others: a pattern that fails the cell rule fails that rule too
    and is refused at both sizes; none is admissible at full size only.  Checked here on arrays a few sites away from the layout."""
    lacking = ("GBGGGG", "BGGBGB", "GBGGRG", "GRGGBG", "BGBRGR", "GRGGBG")  # the first cell has no red
    assert not _cells_ok(lacking) and not _centred_ok(lacking)
    assert _plan(lacking, reduced=1)[0] == _lib.EINVAL and _plan(lacking, reduced=0)[0] == _lib.EINVAL
    rng = np.random.default_rng(2)
    seen = 0
    for _ in range(3000):
        p = [list(r) for r in XTRANS]
        for _k in range(int(rng.integers(1, 5))):
            p[int(rng.integers(6))][int(rng.integers(6))] = "RGB"[int(rng.integers(3))]
        p = tuple("".join(r) for r in p)
        ok = len(set("".join(p))) == 3 and _gaps_ok(p) and _centred_ok(p)
        assert not ok or _cells_ok(p)
        seen += not _cells_ok(p)
        for reduced in (0, 1):
            assert _plan(p, reduced=reduced)[0] == (_lib.OK if ok else _lib.EINVAL), (p, reduced)
    assert seen > 20


def test_planner_refuses_small_frames_and_every_numeric_bound():
    assert _plan(H=6, W=6)[0] == _lib.OK and _plan(H=8, W=7, reduced=1)[1].out_h == 2
    nan, inf = float("nan"), float("inf")
    for H, W in ((5, 60), (40, 5), (0, 60), (-6, 60)):
        assert _plan(H=H, W=W)[0] == _lib.EINVAL and _plan(H=H, W=W, reduced=1)[0] == _lib.EINVAL
    bad = [dict(pattern=(7, 3)), dict(pattern=(0, -1)),
           dict(black=(0, nan)), dict(black=(35, inf)), dict(black=(1, -1.0)), dict(black=(20, 65536.0)), dict(black=(0, 12.5)),
           dict(mul=(0, nan)), dict(mul=(1, inf)), dict(mul=(2, 0.0)), dict(mul=(1, -1.0)), dict(mul=(0, 1024.5)), dict(mul=(0, 1e-60)),
           dict(matrix=(0, nan)), dict(matrix=(8, -inf)), dict(matrix=(4, 64.5)), dict(matrix=(5, -64.5))]
    for b in bad:
        assert _plan(**b)[0] == _lib.EINVAL, b
    for ok in (dict(black=(35, 65535.0)), dict(mul=(0, 1024.0)), dict(matrix=(4, -64.0)), dict(matrix=(0, 64.0))):
        assert _plan(**ok)[0] == _lib.OK, ok
    assert _lib.load().r2f_xtrans_plan(None, 40, 60, ctypes.byref(_lib.XTransParams())) == _lib.EINVAL


def test_the_bounds_keep_every_intermediate_inside_int32():
    """Step A and C as in the Bayer definition; B1's numerator is at most 4 * 65535 + 2, B2's at most 12 * 65535 in magnitude, and
    floor_div's biased numerator below 13 * 2^20 < 2^32 / 12."""
    assert 65535 * 1024 < 2 ** 27 and 3 * 64 * 65535 < 2 ** 24 and 12 * 65535 < 2 ** 20 and 13 * 2 ** 20 < 2 ** 32 // 12
    prof = XTransProfile(black=0, multipliers=(1024.0,) * 3, matrix=((64.0,) * 3, (-64.0,) * 3, (64.0, -64.0, 64.0)))
    out = xm.demosaic(np.full((12, 12), 65535, np.uint16), prof)
    assert np.array_equal(out[..., 0], np.full((12, 12), 65535)) and not out[..., 1].any()


# ---- ABI
def test_struct_layouts_match_the_header():
    P, R = _lib.XTransProfile, _lib.XTransParams
    assert ctypes.sizeof(P) == 536
    assert [getattr(P, f).offset for f in ("pattern", "reduced", "black", "mul", "matrix")] == [0, 144, 152, 440, 464]
    assert ctypes.sizeof(R) == 900
    fields = ("cfa", "gap", "taps", "wsum", "cell_count", "recip", "black", "mul", "M", "reduced", "out_h", "out_w")
    assert [getattr(R, f).offset for f in fields] == [0, 36, 180, 324, 396, 408, 696, 840, 852, 888, 892, 896]
    text = open(os.path.join(ROOT, "include", "r2f.h")).read()
    body = text[text.index("typedef struct r2f_xtrans_params {"):text.index("} r2f_xtrans_params;")]
    order = [body.index(w) for w in ("uint8_t cfa[36];", "uint8_t gap[36][4];", "uint16_t taps[36][2];", "uint8_t wsum[36][2];",
                                     "uint8_t cell_count[4][3];", "uint32_t recip[36][2];", "int32_t black[36];", "float mul[3];",
                                     "float M[9];", "int32_t reduced, out_h, out_w;")]
    assert order == sorted(order)
    body = text[text.index("typedef struct r2f_xtrans_profile {"):text.index("} r2f_xtrans_profile;")]
    order = [body.index(w) for w in ("int32_t pattern[36];", "int32_t reduced;", "double black[36];", "double mul[3];", "double matrix[9];")]
    assert order == sorted(order)
    assert f"R2F_XTRANS_TILE_W = {xm.TILE_W}, R2F_XTRANS_TILE_H = {xm.TILE_H}" in text
    assert (_lib.XTRANS_TILE_W, _lib.XTRANS_TILE_H) == (xm.TILE_W, xm.TILE_H)
    definition = text[text.index("Demosaic of a mosaic with a 6 x 6"):text.index("typedef struct r2f_xtrans_profile")]
    assert "UNPINNED" in definition and "NOT" in definition and "A THIRD" in definition


# ---- XTransProfile
def test_profile_is_frozen_and_hashable():
    a = XTransProfile(list(XTRANS), black=[64] * 36, multipliers=[2.0, 1.0, 1.5], matrix=np.array(xm.CAMERA))
    b = XTransProfile("".join(XTRANS), black=64, multipliers=(2.0, 1.0, 1.5), matrix=xm.CAMERA)
    assert a == b and hash(a) == hash(b) and {a: 1}[b] == 1
    assert a != XTransProfile(XTRANS, black=65, multipliers=(2.0, 1.0, 1.5), matrix=xm.CAMERA)
    assert a != XTransProfile(xm.shifted(0, 1), black=64, multipliers=(2.0, 1.0, 1.5), matrix=xm.CAMERA)
    assert a != RawProfile("RGGB") and XTransProfile() == XTransProfile(XTRANS)
    with pytest.raises(Exception):
        a.pattern = XTRANS
    assert a.pattern == XTRANS and len(a.black) == 36 and (a.reduction, RawProfile.reduction) == (3, 2)
    assert RawProfile("RGGB") == RawProfile("RGGB", black=0) and "reduction" not in repr(RawProfile("RGGB"))


@pytest.mark.parametrize("kw", [
    dict(pattern="RGGB"), dict(pattern=0), dict(pattern=XTRANS[:5]), dict(pattern=XTRANS + ("GRGGBG",)), dict(pattern="".join(XTRANS).lower()),
    dict(pattern=("GBGGRG", "RGRBGB", "GBGGRG", "GRGGBG", "BGBRGR", "GRGGB")), dict(pattern=("GBGGRG", "RGRBGB", "GBGGRG", "GRGGBG", "BGBRGR", "GRGGBX")),
    dict(pattern=tuple(r.replace("B", "R") for r in XTRANS)), dict(pattern=(1, 2, 3, 4, 5, 6)),
    dict(black=-1), dict(black=65536), dict(black=12.5), dict(black=float("nan")), dict(black=(1, 2, 3, 4)), dict(black="64"), dict(black=(0,) * 35),
    dict(multipliers=(1.0, 1.0)), dict(multipliers=(1.0, 1.0, 1.0, 1.0)), dict(multipliers=(1.0, 0.0, 1.0)), dict(multipliers=(1.0, -2.0, 1.0)),
    dict(multipliers=(1.0, 1024.5, 1.0)), dict(multipliers=(1.0, float("inf"), 1.0)), dict(multipliers=2.0),
    dict(matrix=((1, 0, 0), (0, 1, 0))), dict(matrix=((1, 0), (0, 1), (0, 0))), dict(matrix=((1, 0, 0), (0, 65, 0), (0, 0, 1))),
    dict(matrix=((1, 0, 0), (0, float("nan"), 0), (0, 0, 1))), dict(matrix=3.0),
])
def test_profile_validation_raises_before_any_work(kw):
    with pytest.raises(ValueError, match="XTransProfile"):
        XTransProfile(**kw)


def test_plan_refusals_surface_as_value_errors():
    p = XTransProfile()
    for H, W, half in ((5, 8, False), (8, 5, False), (5, 12, True)):
        with pytest.raises(ValueError, match="r2f_xtrans_plan"):
            p.plan(H, W, half)
    with pytest.raises(ValueError, match="r2f_xtrans_plan"):
        XTransProfile(multipliers=(1e-60, 1.0, 1.0)).plan(8, 8)  # (rounds to 0 as a float)
    with pytest.raises(ValueError, match="r2f_xtrans_plan"):
        XTransProfile(("GBGGRG", "RGRBGB", "GBGGRG", "GRGGBG", "BBBRGR", "GRGGBG")).plan(12, 12)  # (not admissible)
    q = p.plan(8, 10, True)
    assert (q.out_h, q.out_w, q.reduced) == (2, 3, 1)
    q = p.plan(7, 10)
    assert (q.out_h, q.out_w, q.reduced) == (7, 10, 0)


# ---- phase 1 of the processor
@pytest.fixture
def proc():
    p = HipProcessor.__new__(HipProcessor)
    p.cameras = p.lenses = None
    p.payload_alpha = True
    return p


MOSAIC, PROFILE = xm.fixture("random", xm.PATTERNS[1], 97, 146)  # (neither side a multiple of 3)
CROP_KEYS = ("final_resolution", "output_resolution", "canvas_resolution", "pipeline_resolution", "resize_to", "upscale_to", "chroma_nr",
             "u16_factor", "u16_window", "exposure_root")


@pytest.mark.parametrize("kw", [
    dict(exposure=0.5), dict(exposure=0.5, half_size=False), dict(exposure=-1.0, zoom=1.3, rotate_times=1), dict(exposure=0.0, rotation=3.5, zoom=1.2),
    dict(exposure="device", zoom=1.3), dict(exposure=None), dict(exposure=0.25, flip=True, frame_width=36, frame_height=36),
    dict(exposure=0.5, resolution=(30, 45), canvas_mode="Uniform white", canvas_scale=1.1), dict(exposure=0.5, rotate_times=3, max_scale=1.0),
])
def test_payload_is_the_mosaic_with_the_crop_numbers_of_the_demosaiced_frame(proc, kw):
    """half_size (the default) yields a third: every crop-derived number is that of the (H // 3, W // 3) frame."""
    half = kw.get("half_size", True)
    rgb = xm.demosaic(MOSAIC, PROFILE, half_size=half)
    assert rgb.shape == ((32, 48, 3) if half else (97, 146, 3))
    pay = proc.extract_image_data_cpu(MOSAIC, raw_profile=PROFILE, **kw)
    plain = proc.extract_image_data_cpu(rgb, **dict(kw, exposure="device" if kw["exposure"] is None else kw["exposure"]))
    assert set(pay) == set(plain) | {"demosaic"} and "demosaic" not in plain
    assert pay["image_array"] is MOSAIC  # 2 bytes per pixel go up, the caller's array itself
    step = pay["demosaic"]
    assert set(step) == {"params", "window", "rotate_times"} and isinstance(step["params"], _lib.XTransParams)
    assert (step["params"].out_h, step["params"].out_w, step["params"].reduced) == (rgb.shape[0], rgb.shape[1], int(half))
    for k in CROP_KEYS:
        assert pay[k] == plain[k], k
    assert (pay["warp"] is None) == (plain["warp"] is None)
    if pay["warp"] is not None:
        assert pay["warp"]["window"] == plain["warp"]["window"] and pay["warp"]["rotate_times"] == plain["warp"]["rotate_times"]
    if plain["u16_window"] is None:
        r0, c0, nr, nc = step["window"]
        assert np.array_equal(np.rot90(rgb[r0:r0 + nr, c0:c0 + nc], k=step["rotate_times"]), plain["image_array"])
    else:
        assert step["window"] is None and step["rotate_times"] == 0 and plain["image_array"].shape == rgb.shape


def test_frame_samples_follow_the_profiles_reduction():
    big = np.zeros((6000, 9000), np.uint16)
    assert mosaic_frame_samples(big, False, 1.5, False, 1.0, XTransProfile.reduction) == 6000 * 9000 * 3
    assert mosaic_frame_samples(big, True, 1.5, False, 1.0, XTransProfile.reduction) == 2000 * 3000 * 3
    assert mosaic_frame_samples(big, True, 1.5, False, 1.0, RawProfile.reduction) == 3000 * 4500 * 3
    assert mosaic_frame_samples(big, True, 1.5, False, 1.0) == 3000 * 4500 * 3  # (a Bayer mosaic's, as before)
    assert mosaic_frame_samples(MOSAIC, True, 1.5, False, 1.0, 3) == 32 * 48 * 3  # (97 x 146: the tails are dropped)


def test_wrong_sources_and_profiles_raise(proc):
    with pytest.raises(ValueError, match="mosaic"):
        proc.extract_image_data_cpu(xm.demosaic(MOSAIC, PROFILE), raw_profile=PROFILE, exposure=0.0)
    with pytest.raises(ValueError, match="raw_profile"):
        proc.extract_image_data_cpu(MOSAIC, raw_profile={"pattern": XTRANS}, exposure=0.0)
    with pytest.raises(ValueError, match="r2f_xtrans_plan"):
        proc.extract_image_data_cpu(MOSAIC[:5], raw_profile=PROFILE, exposure=0.0)  # below 6 rows
    with pytest.raises(ValueError, match="turned or rotated"):
        proc.extract_image_data_cpu(MOSAIC, raw_profile=PROFILE, rotate_times=1)


def test_both_stream_refusals_name_the_demosaic_step_and_say_not_yet(proc):
    pay = proc.extract_image_data_cpu(MOSAIC, raw_profile=PROFILE, exposure=0.5, half_size=False)
    why = stream_rejection(pay, (8192, 8192), "torch.int16", False, "gpu")
    assert why is not None and "demosaic" in why and "X-Trans mosaics do not stream yet" in why
    big = np.zeros((1 << 13, 1 << 13), np.uint16)
    # (everything a Bayer mosaic needs in order to stream is there: stops, no turn, no lens step, a large window)
    assert host_stream_gate(big, 16, 0.0, 0, "No", 0.0, False, True, stops=True, frame_samples=3 << 26) is None
    why = host_stream_gate(big, 16, 0.0, 0, "No", 0.0, False, True, stops=True, frame_samples=3 << 26, xtrans=True)
    assert why is not None and "demosaic" in why and "X-Trans mosaics do not stream yet" in why
    proc.stream_bands = 16
    settings = {k: p.default for k, p in inspect.signature(HipProcessor.process).parameters.items() if p.default is not inspect.Parameter.empty}
    why = proc._host_stream_gate(big, dict(settings, raw_profile=PROFILE, exposure=0.5, half_size=False))
    assert why is not None and "X-Trans mosaics do not stream yet" in why
    assert proc._host_stream_gate(big, dict(settings, raw_profile=RawProfile("RGGB"), exposure=0.5, half_size=False)) is None
    proc._host_stream_gate(big, dict(settings, raw_profile={"pattern": XTRANS}, exposure=0.5))  # (a wrong type is check_profiles' to refuse)


def test_a_changed_profile_invalidates_the_image_cache_and_an_equal_one_does_not(proc):
    uploads = []

    def prepare(payload):
        uploads.append(payload.get("demosaic"))
        proc._texture = ("frame", None, {})
        proc.image_param_dict = None

    proc.prepare_gpu_textures = prepare
    a = XTransProfile(xm.PATTERNS[1], black=64, multipliers=(2.0, 1.0, 1.5))
    proc.load_image_texture(MOSAIC, raw_profile=a, exposure=0.0)
    proc.load_image_texture(MOSAIC, raw_profile=XTransProfile("".join(xm.PATTERNS[1]), black=[64] * 36, multipliers=[2.0, 1.0, 1.5]), exposure=0.0)
    assert len(uploads) == 1 and uploads[0] is not None
    proc.load_image_texture(MOSAIC, raw_profile=XTransProfile(xm.PATTERNS[1], black=65, multipliers=(2.0, 1.0, 1.5)), exposure=0.0)
    assert len(uploads) == 2
    proc.load_image_texture(MOSAIC, raw_profile=a, exposure=0.0, half_size=False)
    assert len(uploads) == 3 and uploads[2]["params"].reduced == 0
    proc.load_image_texture(MOSAIC, raw_profile=a, exposure=0.0, half_size=False)
    assert len(uploads) == 3
