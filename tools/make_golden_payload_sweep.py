#!/usr/bin/env python3
"""tests/golden/payload_sweep.json: what HipProcessor.extract_image_data_cpu returns over a fixed list of cases, recorded from a
checkout of the commit BEFORE phase 1 moved into raw2film_amd/payload.py (tests/test_payload_sweep_host.py holds every later
commit to it).

    python tools/make_golden_payload_sweep.py --root CHECKOUT --commit NAME [-o tests/golden/payload_sweep.json]

CHECKOUT is the tree whose raw2film_amd is recorded (with its library built: the lens and demosaic planners are native); the run is
a process of its own, and the case list and the recording are this file's whichever tree is recorded.

The cases are a thinned cross product (CASES: every STRIDE-th one, and the first of every combination of source kind, exposure
mode, rotation, lens step and quarter turns that the stride would miss) of: two frame sizes (even ones for a mosaic); float32
frames of 3 and 4 channels, a uint16 frame, a uint16 Bayer mosaic with a RawProfile at half and at full size; exposure None, 0.5
stops, "device"; rotation 0 and 3.5; zoom 1 and 1.3; rotate_times 0, 1, 2, 3, 5; flip; no LensProfile, one with lens_correction,
one without; `_internal`; `payload_alpha`; and two film formats of tools/make_golden_payload.py, one whose preview resolution
shrinks the frame and one that runs at `max_scale` and goes back up.

A case's record is the list of its payload's `key=repr(value)` texts in the payload's order, or the exception's type and
message.  repr keeps tuples, ints, floats and None apart.  Left out of the file is whatever depends on the host's libm or is
large: `image_array` is recorded as its shape, dtype, whether it is the caller's array object and whether it shares memory with
the source; a float `u16_factor` as the stops it must be the float32 factor of (checked here against decode.py, computed again
by the test); `m_dst_to_src` as float.hex texts; a step's `params` as a mark (the test compares the bytes with the profile's own
plan)."""

from __future__ import annotations

import argparse
import itertools
import json
import os
import sys

import numpy as np

FRAMES = ((61, 97), (97, 61))
MOSAICS = ((62, 98), (98, 62))  # (a half-size demosaic needs even sides)
SOURCES = ("f32x3", "f32x4", "u16", "mosaic_half", "mosaic_full")
EXPOSURES = (None, 0.5, "device")
ROTATIONS = (0.0, 3.5)
ZOOMS = (1.0, 1.3)
TURNS = (0, 1, 2, 3, 5)
FLIPS = (False, True)
LENSES = ("none", "corrected", "ignored")  # no profile; a profile with lens_correction=True; the same with lens_correction=False
INTERNAL = (False, True)
ALPHA = (True, False)
# (frame_width, frame_height, resolution, max_scale, canvas_mode, canvas_scale, canvas_ratio): super 8 with a preview resolution
# that max_scale shrinks below the frame (and a canvas); super 8 rendered at max_scale and scaled back up to the frame's own size
FILMS = ((5.79, 4.01, (200, 300), 15.0, "Proportional white", 1.2, 1.5), (5.79, 4.01, None, 15.0, "No", 1.0, 1.0))
AXES = (FRAMES, SOURCES, EXPOSURES, ROTATIONS, ZOOMS, TURNS, FLIPS, LENSES, INTERNAL, ALPHA, FILMS)
STRIDE = 149  # (prime to every axis length: consecutive kept cases differ along all of them)

LENS_SPEC = dict(distortion="ptlens", coefficients=(0.02, -0.06, 0.01), vignetting=(-0.3, 0.1, -0.02), center=(0.01, -0.006))
RAW_SPEC = dict(pattern="GRBG", black=(64, 60, 66, 64), multipliers=(2.1, 1.0, 1.6),
                matrix=((1.62, -0.41, -0.19), (-0.28, 1.52, -0.22), (0.04, -0.52, 1.49)))


def _class(case):
    """The combination a thinned list must still cover: source kind, exposure mode, rotated, lens step, turned."""
    _, source, exposure, rotation, _, turns, _, lens, _, _, _ = case
    return source, exposure, bool(rotation), lens == "corrected", bool(turns % 4)


def _cases():
    kept, seen = [], set()
    for i, case in enumerate(itertools.product(*AXES)):
        if i % STRIDE == 0 or _class(case) not in seen:
            kept.append(case)
        seen.add(_class(case))
    return kept


CASES = _cases()


def source(kind, frame):
    """The source array of a case: the same bytes for the same arguments."""
    H, W = MOSAICS[frame] if kind.startswith("mosaic") else FRAMES[frame]
    rng = np.random.default_rng([frame, SOURCES.index(kind)])
    if kind.startswith("mosaic"):
        return rng.integers(0, 40000, (H, W), dtype=np.uint16)
    if kind == "u16":
        return rng.integers(0, 40000, (H, W, 3), dtype=np.uint16)
    return rng.uniform(0, 2, (H, W, int(kind[-1]))).astype(np.float32)


def call(HipProcessor, LensProfile, RawProfile, case):
    """One case against HipProcessor.extract_image_data_cpu, unbound on a bare object -> (src, payload, profiles), or raises."""
    frame, kind, exposure, rotation, zoom, turns, flip, lens, internal, alpha, film = case
    fw, fh, resolution, max_scale, canvas_mode, canvas_scale, canvas_ratio = film
    proc = HipProcessor.__new__(HipProcessor)
    proc.payload_alpha = alpha
    src = source(kind, FRAMES.index(frame))
    half = kind == "mosaic_half"
    profiles = dict(lens_profile=None if lens == "none" else LensProfile(**LENS_SPEC),
                    raw_profile=RawProfile(**RAW_SPEC) if kind.startswith("mosaic") else None)
    payload = HipProcessor.extract_image_data_cpu(
        proc, src, lens_correction=lens != "ignored", frame_width=fw, frame_height=fh, rotation=rotation, zoom=zoom,
        rotate_times=turns, flip=flip, resolution=resolution, half_size=half, max_scale=max_scale, canvas_mode=canvas_mode,
        canvas_scale=canvas_scale, canvas_ratio=canvas_ratio, exposure=exposure, **profiles, **({"_internal": True} if internal else {}))
    return src, payload, dict(profiles, half_size=half)


def _plain(value):
    """repr of a value made of None, bool, int, float, str, tuples and dicts of them -- exactly those types: a NumPy scalar or a
    list in their place is named as such."""
    if type(value) is tuple:
        return "(" + ", ".join(_plain(v) for v in value) + ("," if len(value) == 1 else "") + ")"
    if type(value) is dict:
        return "{" + ", ".join(f"{_plain(k)}: {_plain(v)}" for k, v in value.items()) + "}"
    if value is None or type(value) in (bool, int, float, str):
        return repr(value)
    return f"<{type(value).__module__}.{type(value).__name__} {value!r}>"


def record(src, payload, exposure, decode):
    """The texts of one payload (see the module's text).  `decode`: raw2film_amd.decode of the tree under record."""
    out = []
    for key, value in payload.items():
        if key == "image_array":
            value = (tuple(int(n) for n in value.shape), str(value.dtype), value is src, bool(np.shares_memory(value, src)))
        elif key == "u16_factor" and type(value) is float:
            stops = decode.auto_exposure(src) if exposure in (None, "device") else float(exposure)
            assert value == float(decode.exposure_factor(stops)), (value, stops)
            value = "<the float32 factor of " + ("the host's auto exposure" if exposure in (None, "device") else f"{exposure!r} stops") + ">"
        elif key == "warp" and value is not None:
            m = value["m_dst_to_src"]
            value = dict(value, m_dst_to_src=(type(m).__name__, str(m.dtype), tuple(m.shape)) + tuple(float(v).hex() for v in m.ravel()))
        elif key in ("lens", "demosaic"):
            value = dict(value, params=f"<{type(value['params']).__name__}>")
        out.append(f"{key}={_plain(value)}")
    return out


def run(root):
    """Every case's record against the tree at `root` -> the file's `texts` and `cases`."""
    sys.path.insert(0, root)
    from raw2film_amd import decode
    from raw2film_amd.hip_processor import HipProcessor
    from raw2film_amd.lens import LensProfile
    from raw2film_amd.raw import RawProfile

    texts, index, rows = [], {}, []

    def intern(text):
        if text not in index:
            index[text] = len(texts)
            texts.append(text)
        return index[text]

    for case in CASES:
        try:
            src, payload, _ = call(HipProcessor, LensProfile, RawProfile, case)
            rows.append([intern(t) for t in record(src, payload, case[2], decode)])
        except Exception as e:  # (a refusal is part of the record)
            rows.append({"raises": intern(f"{type(e).__name__}: {e}")})
    return texts, rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--root", required=True, help="the checkout whose raw2film_amd is recorded")
    ap.add_argument("--commit", required=True, help="its commit, for the file's header")
    ap.add_argument("-o", "--output", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                           "tests", "golden", "payload_sweep.json"))
    args = ap.parse_args()
    texts, rows = run(os.path.abspath(args.root))
    header = ("HipProcessor.extract_image_data_cpu over the case list of tools/make_golden_payload_sweep.py (a thinned cross product of "
              f"frame, source, exposure, rotation, zoom, quarter turns, flip, lens, _internal, payload_alpha and film format), recorded "
              f"by running that tool against a checkout of commit {args.commit}, the one BEFORE phase 1 moved into "
              "raw2film_amd/payload.py; not written from the new code.  cases[i] belongs to CASES[i]: indices into `texts`, one per "
              "payload key in the payload's order, or {raises: the exception}")
    with open(args.output, "w") as f:
        json.dump({"header": header, "stride": STRIDE, "texts": texts, "cases": rows}, f, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {args.output}: {len(rows)} cases, {len(texts)} texts, {os.path.getsize(args.output)} bytes")


if __name__ == "__main__":
    main()
