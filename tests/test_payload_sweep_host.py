"""Phase 1's payload against the record of the commit before raw2film_amd/payload.py existed (tests/golden/payload_sweep.json,
written by tools/make_golden_payload_sweep.py from a checkout of that commit): every key in its order, every tuple, int, float and
None, every refusal's type and text, and for `image_array` its shape, dtype, whether it is the caller's array and whether it shares
the source's memory.  What the file leaves out is compared here: a step's `params` with the profile's own plan, byte for byte, and
a float `u16_factor` with decode.py's (inside the tool's record())."""

import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_payload_sweep as sweep  # noqa: E402

from raw2film_amd import decode  # noqa: E402
from raw2film_amd.hip_processor import HipProcessor  # noqa: E402
from raw2film_amd.lens import LensProfile  # noqa: E402
from raw2film_amd.raw import RawProfile  # noqa: E402

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "payload_sweep.json")))


def test_the_record_is_of_this_case_list():
    assert GOLDEN["stride"] == sweep.STRIDE and len(GOLDEN["cases"]) == len(sweep.CASES)
    assert "recorded by running that tool against a checkout of commit" in GOLDEN["header"]
    # every combination of source kind, exposure mode, rotation, lens step and quarter turns keeps a case
    assert len({sweep._class(c) for c in sweep.CASES}) == 5 * 3 * 2 * 2 * 2
    # and a good share of the cases returns a payload
    assert sum(isinstance(row, list) for row in GOLDEN["cases"]) >= len(sweep.CASES) // 2


@pytest.mark.parametrize("part", range(8))
def test_payloads_are_the_recorded_ones(part):
    texts = GOLDEN["texts"]
    for case, row in list(zip(sweep.CASES, GOLDEN["cases"]))[part::8]:
        try:
            src, payload, profiles = sweep.call(HipProcessor, LensProfile, RawProfile, case)
        except Exception as e:
            assert isinstance(row, dict) and f"{type(e).__name__}: {e}" == texts[row["raises"]], (case, e)
            continue
        assert isinstance(row, list), (case, texts[row["raises"]])
        assert sweep.record(src, payload, case[2], decode) == [texts[i] for i in row], case
        rows, cols = src.shape[:2]
        if "demosaic" in payload:
            plan = profiles["raw_profile"].plan(rows, cols, profiles["half_size"])
            assert bytes(payload["demosaic"]["params"]) == bytes(plan), case
            rows, cols = plan.out_h, plan.out_w
        if "lens" in payload:
            assert bytes(payload["lens"]["params"]) == bytes(profiles["lens_profile"].plan(rows, cols)), case
