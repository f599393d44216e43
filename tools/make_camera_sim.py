#!/usr/bin/env python3
"""tests/golden/camera_sim.json: what the simulated camera and lens of tests/camera_sim.py measure on the project's NumPy models.

    python tools/make_camera_sim.py [-o tests/golden/camera_sim.json]

No GPU.  The models are the reference here: the device's bytes equal theirs by the bit-for-bit tests.  For every check of
camera_sim.CHECKS the file records the RMS error against the scene under the correct reading and under every named misreading,
the smallest gap between the two in dB, and the check's threshold: the geometric mean of the correct error and the smallest
misreading's.  Nothing in the file is chosen by hand or measured on the device.  A misreading below 20 dB (10 x in RMS) needs a
sentence in NOTES, or the tool refuses to write; one below 10 dB is refused outright.

The file holds numbers and names only."""

from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import camera_sim as cs  # noqa: E402
import denoise_model as dnm  # noqa: E402
import highlight_model as hm  # noqa: E402
import lens_model as lm  # noqa: E402
import lens_projection_model as lpm  # noqa: E402
import lens_tca_model as tm  # noqa: E402
import levels_model as lvm  # noqa: E402
import median_model as mm  # noqa: E402
import repair_model as rm  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "camera_sim.json")
MIN_GAP_DB, FLOOR_GAP_DB = 20.0, 10.0
DIGITS = 6  # significant digits of a recorded error

# why a misreading stays below MIN_GAP_DB: "check/misreading" -> a sentence
_COMPOSED_FLOOR = ("a composed frame's error under the correct reading is the sum of its steps' floors -- the noise the denoise leaves, the "
                   "repaired samples, the demosaic's and the lens step's interpolation -- at about 0.0025 of the white level")
NOTES = {
    "composed_bayer/black": f"{_COMPOSED_FLOOR}; black levels turned by one site move a sample by some 70 of 13300 units, 0.011 behind the multipliers",
    "composed_xtrans/black": f"{_COMPOSED_FLOOR}; black levels turned by one site move a sample by some 70 of 13300 units, 0.011 behind the multipliers",
    "composed_bayer/lens_distortion": f"{_COMPOSED_FLOOR}; a stronger distortion than this one's 11 % would sample beyond the 150 x 98 frame's border",
    "composed_xtrans/lens_distortion": f"{_COMPOSED_FLOOR}; a stronger distortion than this one's 11 % would sample beyond the 149 x 97 frame's border",
    "composed_xtrans/repair": f"{_COMPOSED_FLOOR}; 0.3 % of stuck samples weigh 0.026, and without a denoise the X-Trans floor lies a little above the Bayer one",
}


class ModelBackend:
    """camera_sim's backend over the NumPy models of tests/*_model.py (the route of tests/prepath_cases.raw_model, with the repair)."""

    def develop(self, mosaic, profile, half_size=False, denoise=None, repair=None, keep_units=False):
        from raw2film_amd.raw import XTransProfile

        xtrans = isinstance(profile, XTransProfile)
        period = 6 if xtrans else 2
        black = [int(b) for b in profile.black]
        if repair is not None:
            cfa = np.array([["RGB".index(c) for c in row] for row in profile.pattern]) if xtrans else None
            mosaic, _ = rm.repair(mosaic, period, black, repair.threshold, repair.q, repair.min_neighbours, cfa)
        numeric, clip, used = profile, profile.blend_clip, None
        if profile.deferred:
            levels = profile.multipliers
            mode = {"clip": hm.CLIP, "unclip": hm.UNCLIP, "blend": hm.BLEND}[profile.highlight]
            d = lvm.data_maximum(mosaic, black, period)
            mul, used, _, clip = hm.scale(levels.white_balance, levels.white_level, levels.adjust_maximum_thr, black, d, mode)
            clip = clip if profile.highlight == "blend" else None
            numeric = profile._replace(multipliers=mul, highlight="clip")
        if denoise is not None:
            maximum = denoise.maximum if denoise.maximum is not None else used
            shift = 0 if keep_units else dnm.shift_of(maximum)
            mosaic = dnm.denoise(mosaic, black, maximum, denoise.threshold)
            numeric = numeric._replace(black=(0.0,) * 4, multipliers=tuple(m * 2.0 ** -shift for m in numeric.multipliers))
        D = mm.demosaic(mosaic, numeric, profile.median_passes, clip, half_size=half_size, xtrans=xtrans)
        return hm.orient(D, profile.orientation)

    def lens(self, picture, profile, window=None):
        H, W = picture.shape[:2]
        c = lm.rounded(lm.constants(profile, H, W))
        tca = None if profile.tca is None else tm.record(profile, lm.F)
        if profile.projection is not None:
            return lpm.correct(picture, c, lpm.record(profile), tca, window)
        if tca is not None:
            return tm.correct_tca(picture, c, tca, window)
        return lm.correct(picture, c, window)

    def composed(self, mosaic, profile, denoise, repair, lens_profile, keywords):
        from raw2film_amd.hip_processor import HipProcessor

        bare = HipProcessor.__new__(HipProcessor)  # (phase 1 touches no instance state)
        payload = HipProcessor.extract_image_data_cpu(bare, mosaic, raw_profile=profile, raw_denoise=denoise, raw_repair=repair,
                                                      lens_profile=lens_profile, **keywords)
        assert payload["demosaic"]["window"] is None and not payload["demosaic"]["rotate_times"] and not payload["lens"]["rotate_times"]
        F = self.develop(mosaic, profile, keywords["half_size"], denoise, repair)
        frame = F.astype(np.float32) / np.float32(65535.0)  # (the exposure factor divided out)
        window = payload["lens"]["window"]
        return np.asarray(self.lens(frame, lens_profile, window), np.float64), window[:2]


def rounded(x):
    return float(f"{x:.{DIGITS}g}")


def threshold_of(correct, wrong) -> float:
    """The geometric mean of the correct reading's figure and the smallest misreading's."""
    return math.sqrt(abs(correct) * min(abs(w) for w in wrong))


def record(name, backend=None) -> dict:
    """One check's entry of the file: camera_sim.measure's figures, rounded, with the threshold and the smallest gap."""
    m = cs.measure(name, backend or ModelBackend())
    if "figures" in m:
        return {"figures": {k: rounded(v) for k, v in m["figures"].items()}}
    entry = {"correct": rounded(m["correct"]), "misreadings": {k: rounded(v) for k, v in m["misreadings"].items()}}
    smallest = min(m["misreadings"].values())
    entry["threshold"] = rounded(threshold_of(m["correct"], m["misreadings"].values()))
    entry["gap_db"] = round(cs.decibels(smallest / m["correct"]), 2)
    if "noisy" in m:  # the bias bound follows the thresholds' rule: between the mean's move under the correct reading and the misreading
        entry.update(noisy=rounded(m["noisy"]), bias=rounded(m["bias"]), bias_bound=rounded(threshold_of(max(abs(m["bias"]), 1e-9), [m["misread_bias"]])))
    residual = cs.case(name).extras.get("residual_px")
    if residual is not None:
        entry["lens_inverse_residual_px"] = rounded(residual)
    return entry


def build(names=None) -> dict:
    checks = {name: record(name) for name in (names or cs.CHECKS)}
    return {"comment": "written by tools/make_camera_sim.py from the NumPy models; RMS errors in scene units (1.0 is the white level)",
            "notes": dict(NOTES), "checks": checks}


def violations(data) -> list:
    """What the 20 dB condition refuses: a misreading below the floor, or below 20 dB without its note."""
    out = []
    for name, entry in data["checks"].items():
        for wrong, err in entry.get("misreadings", {}).items():
            gap = cs.decibels(err / entry["correct"])
            if gap < FLOOR_GAP_DB:
                out.append(f"{name}/{wrong}: {gap:.1f} dB, below the floor of {FLOOR_GAP_DB:g} dB")
            elif gap < MIN_GAP_DB and f"{name}/{wrong}" not in data["notes"]:
                out.append(f"{name}/{wrong}: {gap:.1f} dB, below {MIN_GAP_DB:g} dB without a note")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("-o", "--output", default=GOLDEN)
    ap.add_argument("--only", nargs="*", help="print these checks' entries and write nothing")
    args = ap.parse_args()
    if args.only:
        print(json.dumps(build(args.only)["checks"], indent=1))
        return
    data = build()
    bad = violations(data)
    for line in bad:
        print("REFUSED", line, file=sys.stderr)
    if bad:
        raise SystemExit(1)
    with open(args.output, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, entry in data["checks"].items():
        print(f"{name:24s} " + (f"correct {entry['correct']:.3g}  threshold {entry['threshold']:.3g}  gap {entry['gap_db']:.1f} dB"
                                if "correct" in entry else str(entry["figures"])))


if __name__ == "__main__":
    main()
