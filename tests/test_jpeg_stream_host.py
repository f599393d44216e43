"""The streamed JPEG export's host side, without a GPU: the JPEG sink's row bookkeeping (which rows the encoder takes after each
band), the early gates of a streamed export, the output helpers, the row-wise entry points in the C ABI, and rows_grid of
raw2film_amd/csrc/r2f_jpeg_plan.cpp under AddressSanitizer / UBSan."""

import io
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from raw2film_amd import _lib
from raw2film_amd.hip_processor import plan_bands
from raw2film_amd.payload import host_stream_gate
from raw2film_amd.jpeg_stream import deliver, jpeg_row_steps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_steps(bounds, H):
    steps = jpeg_row_steps(bounds, H)
    assert len(steps) == len(bounds) - 1
    done = 0
    for b, step in enumerate(steps):
        if step is None:
            continue
        y0, y1 = step
        assert y0 == done and y1 > y0, (bounds, steps)
        assert y1 <= bounds[b + 1], "rows past the band's last finished row"
        assert y1 % 16 == 0 or y1 == H, "an MCU row cut"
        done = y1
    assert done == H and steps[-1] is not None and steps[-1][1] == H
    return steps


def test_row_steps_partition_plan_bands_bounds():
    rng = random.Random(20261015)
    for _ in range(3000):
        H = rng.randint(1024, 65535)
        bands = rng.choice((2, 3, 5, 16, 40, 100))
        taper = rng.randint(0, 3)
        ha = (rng.randint(0, 60), rng.randint(0, 60))
        bounds, why = plan_bands(H, 0, ha, (0, 0), bands, taper)
        if bounds is None:
            assert why
            continue
        check_steps(bounds, H)


def test_row_steps_of_random_bounds():
    rng = random.Random(7)
    for _ in range(3000):
        H = rng.randint(1, 3000)
        cuts = sorted(set(rng.sample(range(1, H), min(H - 1, rng.randint(0, 12))))) if H > 1 else []
        check_steps([0] + cuts + [H], H)


def test_row_steps_at_mcu_boundaries():
    # bounds on, just before and just after a multiple of 16
    assert jpeg_row_steps([0, 32, 64, 100], 100) == [(0, 32), (32, 64), (64, 100)]
    assert jpeg_row_steps([0, 31, 47, 100], 100) == [(0, 16), (16, 32), (32, 100)]
    assert jpeg_row_steps([0, 33, 47, 100], 100) == [(0, 32), None, (32, 100)]
    assert jpeg_row_steps([0, 5, 10, 15, 17], 17) == [None, None, None, (0, 17)]


def test_host_stream_gate_names_each_reason():
    big = np.zeros((1, 1 << 22, 4), np.float32)  # 16.7 M samples, no memory touched
    assert host_stream_gate(big, 16) is None
    assert "stream_bands" in host_stream_gate(big, 0)
    assert "stream_bands" in host_stream_gate(big, 1)
    assert "not a host array" in host_stream_gate("frame.npy", 16)
    assert "below" in host_stream_gate(np.zeros((64, 64, 3), np.float32), 16)
    for kw in (dict(rotation=3.0), dict(chroma_nr=2), dict(canvas_mode="Even"), dict(highlight_burn=0.5)):
        why = host_stream_gate(big, 16, **kw)
        assert why and list(kw)[0] in why, kw


def test_deliver_returns_bytes_or_writes(tmp_path):
    data = bytes(range(256)) * 7
    assert deliver(data, None) is data
    buf = io.BytesIO()
    assert deliver(data, buf) == len(data) and buf.getvalue() == data
    path = tmp_path / "x.jpg"
    assert deliver(data, str(path)) == len(data) and path.read_bytes() == data
    assert deliver(data, path) == len(data) and path.read_bytes() == data
    with pytest.raises(TypeError):
        deliver(data, 42)


def test_row_wise_entry_points_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "r2f.h")).read()
    for name in ("r2f_jpeg_rows_begin", "r2f_jpeg_rows"):
        assert f"{name}(" in text
        assert name in _lib.EXPORTED_SYMBOLS


# ---- rows_grid of r2f_jpeg_plan.cpp under the sanitizers
@pytest.fixture(scope="module")
def rows_check_binary(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("jpeg_rows_plan") / "jpeg_rows_plan_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "jpeg_rows_plan_check.cpp"), os.path.join(ROOT, "raw2film_amd", "csrc", "r2f_jpeg_plan.cpp"),
           "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


@pytest.mark.parametrize("seed", [1, 2, 20261015])
def test_rows_grid_is_clean_under_asan_and_ubsan(rows_check_binary, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([rows_check_binary, "fuzz", str(seed), "2000"], capture_output=True, text=True, env=env, timeout=600)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    assert "cases ok" in res.stdout
