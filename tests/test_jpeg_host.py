"""The JPEG export's host side, without a GPU: the NumPy model of the encoder (tests/jpeg_model.py) writes Pillow's bytes, the
library's header and bound agree with it, and raw2film_amd/csrc/r2f_jpeg_plan.cpp runs clean under AddressSanitizer / UBSan."""

import ctypes
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_extremes as jx
import jpeg_model as jm

Image = pytest.importorskip("PIL.Image")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUALITIES = (0, 1, 50, 75, 95, 100)
SIZES = ((1, 1), (7, 5), (16, 16), (17, 33), (31, 64), (256, 383))


def pillow_jpeg(a, quality):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", quality=quality)
    return buf.getvalue()


def contents(H, W, seed=0):
    """noise, a constant frame (long zero runs: ZRL and EOB), pure white, gradients"""
    rng = np.random.default_rng(seed + H * 1000 + W)
    yy, xx = np.mgrid[0:H, 0:W]
    grad = np.stack([xx * 255 // max(W - 1, 1), yy * 255 // max(H - 1, 1), (xx * 5 + yy * 3) % 256], -1).astype(np.uint8)
    return {
        "noise": rng.integers(0, 256, (H, W, 3), dtype=np.uint8),
        "constant": np.full((H, W, 3), (90, 140, 200), dtype=np.uint8),
        "white": np.full((H, W, 3), 255, dtype=np.uint8),
        "gradient": grad,
    }


@pytest.mark.parametrize("H,W", SIZES)
def test_model_writes_pillows_bytes(H, W):
    for name, a in contents(H, W).items():
        for q in QUALITIES:
            assert jm.encode(a, q) == pillow_jpeg(a, q), (name, q)


def test_model_header_is_pillows_up_to_sos():
    a = np.zeros((40, 70, 3), dtype=np.uint8)
    for q in QUALITIES:
        h = jm.header(q, 40, 70)
        assert pillow_jpeg(a, q)[: len(h)] == h and h.endswith(bytes([0xFF, 0xDA, 0, 12, 3, 1, 0, 2, 0x11, 3, 0x11, 0, 63, 0]))


def test_quality_zero_writes_what_one_writes():
    a = contents(31, 64)["noise"]
    assert jm.encode(a, 0) == jm.encode(a, 1) == pillow_jpeg(a, 0)


def test_bound_holds_for_the_worst_case():
    # noise at q100 is as dense as scans get; the bound covers the whole file with every scan byte stuffed
    for H, W in ((16, 16), (17, 33), (64, 64)):
        out = jm.encode(contents(H, W)["noise"], 100)
        assert len(out) <= jm.bound_bytes(H, W)
        scan_bits = 8 * (len(out) - len(jm.header(100, H, W)) - 2 - out.count(b"\xff\x00"))
        assert scan_bits <= jm.mcus(H, W) * 6 * jm.block_bound_bits()
    assert jm.block_bound_bits() == 1660


# ---- coefficients at the ends of their ranges (tests/jpeg_extremes.py)
@pytest.mark.parametrize("H,W", jx.SIZES)
def test_model_writes_pillows_bytes_for_extreme_coefficients(H, W):
    for name, a in jx.frames(H, W).items():
        for q in jx.QUALITIES:
            assert jm.encode(a, q) == pillow_jpeg(a, q), (name, q)


def test_extreme_frames_are_not_vacuous():
    """What the frames are for, counted on the coefficients the 4:2:0 baseline scan codes at quality 100: the widest DC difference
    (category 11) in every component and the longest AC symbol (category 10); contents() stops at AC category 9 and, in luma and
    Cb, at DC category 10."""
    cat = {name: jx.categories(a) for name, a in jx.frames(64, 96).items()}
    assert cat["block_checker"]["y_dc"] == 11 and cat["blue_yellow"]["y_dc"] == 11
    assert cat["blue_yellow"]["cb_dc"] == 11
    assert cat["red_cyan16"]["cr_dc"] == 11
    assert cat["pixel_checker"]["ac"] == 10 and cat["lines"]["ac"] == 10
    usual = [jx.categories(a, q) for a in contents(64, 96).values() for q in (100, 75)]
    assert max(c["ac"] for c in usual) <= 9 and max(max(c["y_dc"], c["cb_dc"]) for c in usual) <= 10


# ---- the library's plan-only exports (no GPU, no context)
def _lib():
    from raw2film_amd import _lib

    return _lib.load()


@pytest.mark.parametrize("q", QUALITIES)
def test_library_header_equals_pillows(q):
    lib = _lib()
    for H, W in SIZES + ((4000, 6000), (12288, 8192), (65535, 65535)):
        buf = (ctypes.c_uint8 * 1024)()
        n = ctypes.c_size_t()
        assert lib.r2f_jpeg_header(q, H, W, buf, len(buf), ctypes.byref(n)) == 0
        got = bytes(buf[: n.value])
        assert got == jm.header(q, H, W)
        if H * W <= 256 * 383:
            assert pillow_jpeg(np.zeros((H, W, 3), dtype=np.uint8), q)[: n.value] == got


def test_library_bound_and_refusals():
    lib = _lib()
    for H, W in SIZES + ((12288, 8192),):
        assert lib.r2f_jpeg_bound_bytes(H, W) == jm.bound_bytes(H, W)
    assert 8 * lib.r2f_jpeg_bound_bytes(12288, 8192) > 1 << 32  # a 100 MP frame's worst-case file exceeds 2^32 bits
    assert lib.r2f_jpeg_bound_bytes(0, 5) == 0 and lib.r2f_jpeg_bound_bytes(5, 65536) == 0
    buf = (ctypes.c_uint8 * 1024)()
    n = ctypes.c_size_t()
    assert lib.r2f_jpeg_header(101, 8, 8, buf, len(buf), ctypes.byref(n)) == -1
    assert lib.r2f_jpeg_header(-1, 8, 8, buf, len(buf), ctypes.byref(n)) == -1
    assert lib.r2f_jpeg_header(50, 8, 8, buf, 100, ctypes.byref(n)) == -1


# ---- r2f_jpeg_plan.cpp under the sanitizers
@pytest.fixture(scope="module")
def check_binary(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("jpeg_plan") / "jpeg_plan_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "jpeg_plan_check.cpp"), os.path.join(ROOT, "raw2film_amd", "csrc", "r2f_jpeg_plan.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


def _run(binary, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([binary, *map(str, args)], capture_output=True, text=True, env=env, timeout=600)


@pytest.mark.parametrize("seed", [1, 2, 20261015])
def test_jpeg_plan_is_clean_under_asan_and_ubsan(check_binary, seed):
    res = _run(check_binary, "fuzz", seed, 2000)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    assert "cases ok" in res.stdout


def test_sanitized_header_equals_the_model(check_binary):
    for q, H, W in ((0, 1, 1), (75, 17, 33), (100, 8192, 12288)):
        res = _run(check_binary, "header", q, H, W)
        assert res.returncode == 0, res.stderr
        assert bytes.fromhex(res.stdout.strip()) == jm.header(q, H, W)
