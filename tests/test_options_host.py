"""r2f_set_option's table (raw2film_amd/csrc/r2f_plan.cpp: find_option / store_option) without a GPU: tests/options_plan_check.cpp
walks every option name x value through it and prints what r2f_set_option would answer; the expected answers are the walk recorded
from the library as it was before the table existed (tests/golden/option_walk.json, see tests/option_walk.py)."""

import json
import os
import shutil
import subprocess

import pytest

from option_walk import NAMES, UNKNOWN, VALUES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_option_table_answers_every_name_and_value_as_recorded(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "options_plan_check")
    res = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                          os.path.join(ROOT, "tests", "options_plan_check.cpp"), os.path.join(ROOT, "raw2film_amd", "csrc", "r2f_plan.cpp"),
                          "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "option_walk.json")))["rows"]
    assert len(NAMES) == 28 and len(want) == (len(NAMES) + 1) * len(VALUES)
    res = subprocess.run([exe] + NAMES + [UNKNOWN, "--"] + [str(v) for v in VALUES], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    got = [line.split("\t") for line in res.stdout.splitlines()]
    assert len(got) == len(want)
    for g, (name, value, rc, err, _step) in zip(got, want):
        # the recorded r2f_last_error text is the last failure's: what the check prints the same way
        assert g == [name, str(value), str(rc), err], (g, name, value, rc, err)
    # what is stored: switches 0 / 1, kernel_timing & 7, the two raw options as given
    assert "stored\tkernel_timing\t300\t4" in res.stderr and "stored\tstencil_ablate\t-2\t-2" in res.stderr
    assert "stored\trender_graph\t64\t1" in res.stderr and "stored\tstencil_fft_min_taps\t2147483647\t2147483647" in res.stderr
