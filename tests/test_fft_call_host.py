"""plan::fft_call (raw2film_amd/csrc/r2f_plan.cpp) -- every host decision of one call of the FFT stencil form -- without a GPU:
tests/fft_call_check.cpp walks it over the product of the facts and switches its scratch element and real spectrum hang on, and over
a list of tap boxes, frames, row ranges and batch options; the expected lines are tests/fft_call_model.py's, the rules restated from
the launch function as it stood before the planner existed."""

import os
import shutil
import subprocess

import pytest

import fft_call_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fft_call_decides_every_case_as_the_model_does(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "fft_call_check")
    res = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                          os.path.join(ROOT, "tests", "fft_call_check.cpp"), os.path.join(ROOT, "raw2film_amd", "csrc", "r2f_plan.cpp"),
                          "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    got, want = res.stdout.splitlines(), model.lines()
    assert len(want) == 2 * 2 ** 13 + 5 * 2 * 3 * 2 * 3 * 2 * 2 and len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    # the walk reaches every element, both window heights, a real and a complex spectrum, one lane and several
    seen = {(w.split(" e ")[1].split()[0], w.split(" : ")[1].split()[0]) for w in want}
    assert seen == {(e, ny) for e in "012" for ny in ("256", "512")} | {("3", "256")}
    assert any(" k 1 " in w for w in want) and any(" k 0 " in w for w in want)
    assert {w.split(" s ")[1].split()[0] for w in want} == {"1", "2", "4"}
