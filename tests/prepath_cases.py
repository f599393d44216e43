"""The RAW and lens options of HipProcessor as axes: their values, the combinations the code refuses (`refusal`), the sources (a Bayer
98 x 150 and an X-Trans 97 x 149 mosaic: ragged tiles both ways, odd planes and odd half-size sides; a second Bayer shape for the
session), the calls' keywords, and the model route -- `model_frame(case)` is the uint16 frame F that the tests' own models make of a case's
mosaic (levels_model, highlight_model, denoise_model, median_model: assembled here, no arithmetic of this module's own), with
the `last_raw_scale` and `last_raw_denoise` the processor must report.  process(mosaic, raw_profile=P, ...K) must equal
process(F, ...K) byte for byte: tests/test_gpu_prepath_pairs.py over the pairwise list tests/golden/prepath_pairs.json
(tools/make_prepath_pairs.py writes it), tests/test_gpu_prepath_session.py along `session_walk`.

Host only: nothing here imports torch.  Plain module, no fixtures of pytest's."""

from __future__ import annotations

import functools
import json
import os

import numpy as np

import denoise_model as dnm
import highlight_model as hm
import levels_model as lm
import median_model as mm
import xtrans_model as xm

WB, BLACK, WHITE = (1.9, 1.0, 1.5), 512, 16383
ADJUSTED_WHITE = 20000  # 0.75 m < d < m for a mosaic that reaches WHITE: the frame is adjusted
MATRIX = ((0.52, 0.27, 0.15), (0.25, 0.68, 0.07), (0.03, 0.12, 0.81))
THRESHOLD = 300.0
FIXED_MAXIMUM = ADJUSTED_WHITE - BLACK  # 19488: shift 1, where the resolved scales' maxima (15871) give shift 2
BAYER_SHAPE, BAYER2_SHAPE, XTRANS_SHAPE = (98, 150), (66, 214), (97, 149)
TEXTURE_SHAPE = (64, 96, 4)

AXES = {
    "array": ["RGGB", "GBRG", "xtrans1", "xtrans2"],
    "half_size": [False, True],
    "orientation": [0, 1, 2, 3, 4, 5, 6, 7],
    "scale": ["numeric", "nominal", "adjusted"],  # numbers; RawLevels(thr=0); RawLevels(0.75) whose frame is adjusted
    "highlight": ["clip", "unclip", "blend"],
    "median_passes": [0, 1, 4],
    "raw_denoise": ["none", "fixed", "auto"],  # WaveletDenoise(T, maximum); WaveletDenoise(T): the resolved scale's maximum
    "exposure": ["stops", "auto"],  # 0.5 stops; None on the mosaic and "device" on the model's frame
    "format": ["36x24", "24x36", "56x56", "36x24flip"],
    "zoom": [1.0, 1.3],
    "rotate_times": [0, 1, 2, 3],
    "rotation": [0.0, 3.5],
    "lens_profile": ["none", "ptlens", "poly3tca", "fisheye"],
    "post": ["plain", "chroma_nr", "smaller", "larger", "canvas"],
    "entry": ["process8", "process16", "jpeg", "tiff16", "two_phase", "submit", "texture"],
}
RAW_AXES = ("array", "half_size", "orientation", "scale", "highlight", "median_passes", "raw_denoise")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prepath_pairs.json")
CAP = 72

# what a sibling neutralises: option -> (axis, is the option active in this case?, the neutral value)
NEUTRAL = {
    "median": ("median_passes", lambda c: c["median_passes"] == 4, 0),
    "blend": ("highlight", lambda c: c["highlight"] == "blend", "clip"),
    "denoise": ("raw_denoise", lambda c: c["raw_denoise"] != "none", "none"),
    "orientation": ("orientation", lambda c: c["orientation"] != 0, 0),
    "adjusted": ("scale", lambda c: c["scale"] == "adjusted", "numeric"),
}


def is_xtrans(case) -> bool:
    return case["array"].startswith("xtrans")


def refusal(case):
    """Why the code refuses a case -> (exception, a piece of its message, who raises it), or None for an admissible one.  Every
    rule names two values of two different axes; `entry` has no rule (output_bits=16 with dst_texture, which
    hip_processor.check_output_bits refuses, would be two values of that one axis)."""
    if is_xtrans(case) and case["raw_denoise"] != "none":
        return ValueError, "not built for X-Trans", "payload.check_denoise"
    if case["raw_denoise"] == "auto" and case["scale"] == "numeric":
        return ValueError, "raw_denoise has maximum=None", "payload.check_denoise"
    if case["highlight"] == "unclip" and case["scale"] == "numeric":
        return ValueError, "needs the sensor's levels", "raw._MosaicProfile._highlight"
    if case["exposure"] == "auto" and (case["rotation"] or case["rotate_times"] % 4):
        return ValueError, "a mosaic (raw_profile) has no RGB frame there", "payload.exposure_mode"
    return None


def admissible(case) -> bool:
    return refusal(case) is None


def pairs_of(case):
    names = list(AXES)
    return {((a, case[a]), (b, case[b])) for i, a in enumerate(names) for b in names[i + 1:]}


def all_pairs():
    names = list(AXES)
    return {((a, u), (b, v)) for i, a in enumerate(names) for b in names[i + 1:] for u in AXES[a] for v in AXES[b]}


def refused_pairs():
    """The pairs no admissible case can hold: those whose two values alone make `refusal` speak, whatever the other axes say."""
    base = {**{a: v[0] for a, v in AXES.items()}, "scale": "nominal"}  # (admissible, and no value of it takes part in a rule)
    assert admissible(base)
    return {p for p in all_pairs() if not admissible({**base, p[0][0]: p[0][1], p[1][0]: p[1][1]})}


def case_id(case) -> str:
    f = {False: "full", True: "half"}[case["half_size"]]
    return (f"{case['array']}-{f}-o{case['orientation']}-{case['scale']}-{case['highlight']}-m{case['median_passes']}-dn_{case['raw_denoise']}-"
            f"{case['exposure']}-{case['format']}-z{case['zoom']}-t{case['rotate_times']}-r{case['rotation']}-{case['lens_profile']}-"
            f"{case['post']}-{case['entry']}")


def load_list():
    """The committed list -> [(case, sibling option or None, sibling case or None)]."""
    with open(GOLDEN) as f:
        data = json.load(f)
    return [(r["case"], r["sibling"]["option"], r["sibling"]["case"]) for r in data["cases"]]


# ---- sources
def _patches(shape, tag):
    """tests/test_gpu_median_e2e.py's mosaic at another shape: black 512, white 16383, patches up to the sensor's saturation."""
    return hm.patches(*shape, f"prepath/{tag}", 15000, low=700, high=9000).astype(np.int64).clip(0, WHITE).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def _source(name):
    m = _patches({"bayer": BAYER_SHAPE, "bayer2": BAYER2_SHAPE, "xtrans": XTRANS_SHAPE}[name], name)
    m.setflags(write=False)
    return m


def mosaic_of(case):
    """The shared, read-only mosaic of a case's array."""
    return _source("xtrans" if is_xtrans(case) else "bayer")


def edit_in_place(mosaic, version):
    """A refilled decode buffer: sixteen rows in the middle of the frame, which every crop keeps, move by a step of `version`'s."""
    y = mosaic.shape[0] // 2 - 8
    band = mosaic[y:y + 16].astype(np.int64)
    mosaic[y:y + 16] = np.where(band < 9000, band + 400 + 16 * (version % 7), band).astype(np.uint16)


# ---- profiles and keywords
def _pattern(case):
    return xm.PATTERNS[int(case["array"][-1])] if is_xtrans(case) else case["array"]


def _mode(case):
    return {"clip": hm.CLIP, "unclip": hm.UNCLIP, "blend": hm.BLEND}[case["highlight"]]


def _levels(case):
    """(white level, adjust_maximum_thr) of the case's scale.  A numeric profile holds the numbers of the adjusted levels' NOMINAL
    scale (d = 0): what the adjusted frame's sibling renders with, another scale than the frame's own."""
    return {"numeric": (ADJUSTED_WHITE, 0.0), "nominal": (WHITE, 0.0), "adjusted": (ADJUSTED_WHITE, 0.75)}[case["scale"]]


def profiles(case):
    """(raw_profile, raw_denoise) of a case; raises what the constructors refuse."""
    from raw2film_amd.raw import RawLevels, RawProfile, WaveletDenoise, XTransProfile

    cls = XTransProfile if is_xtrans(case) else RawProfile
    white, thr = _levels(case)
    kw = dict(black=BLACK, matrix=MATRIX, orientation=case["orientation"], median_passes=case["median_passes"])
    if case["scale"] == "numeric":
        if case["highlight"] == "unclip":
            highlight, mul = "unclip", lm.scale(WB, white, 0.0, [BLACK], 0)[0]  # (the constructor refuses it)
        else:
            mul, _, _, clip = hm.scale(WB, white, 0.0, [BLACK], 0, _mode(case))
            highlight = ("blend", clip) if case["highlight"] == "blend" else "clip"
        profile = cls(_pattern(case), multipliers=mul, highlight=highlight, **kw)
    else:
        profile = cls(_pattern(case), multipliers=RawLevels(WB, white, thr), highlight=case["highlight"], **kw)
    denoise = {"none": None, "fixed": WaveletDenoise(THRESHOLD, FIXED_MAXIMUM), "auto": WaveletDenoise(THRESHOLD)}[case["raw_denoise"]]
    return profile, denoise


def lens_profile(name):
    from raw2film_amd.lens import LensProfile

    if name == "none":
        return None
    if name == "ptlens":  # with vignetting and an off-centre `center`
        return LensProfile("ptlens", (0.02, -0.06, 0.01), vignetting=(-0.3, 0.1, -0.02), center=(0.01, -0.006))
    if name == "poly3tca":
        return LensProfile("poly3", (-0.05,), scale=1.05, tca=("poly3", (1.002, 0.998, 0.01, -0.008, -0.02, 0.015)))
    return LensProfile("ptlens", (0.02, -0.06, 0.01), projection=("fisheye", 2.0 / np.pi), tca=("linear", (1.03, 0.97)))


def load_keywords(case):
    """The load settings of a case, the same for the mosaic and for F (`exposure` and the RAW profiles aside)."""
    fw, fh = {"36x24": (36, 24), "24x36": (24, 36), "56x56": (56, 56), "36x24flip": (36, 24)}[case["format"]]
    post = case["post"]
    return dict(frame_width=fw, frame_height=fh, flip=case["format"].endswith("flip"), zoom=case["zoom"],
                rotate_times=case["rotate_times"], rotation=case["rotation"], lens_profile=lens_profile(case["lens_profile"]),
                half_size=case["half_size"], chroma_nr=2 if post == "chroma_nr" else 0,
                # the smallest frame of the list is an X-Trans third, rotated and zoomed: 14 x 18 shrinks it, 240 x 360 enlarges the largest
                resolution={"smaller": (14, 18), "larger": (240, 360)}.get(post), max_scale=None,
                canvas_mode="Uniform white" if post == "canvas" else "No", canvas_scale=1.2 if post == "canvas" else 1.0)


def exposure_of(case, mosaic: bool):
    """The `exposure` of the call on the mosaic / on the model's frame."""
    return 0.5 if case["exposure"] == "stops" else None if mosaic else "device"


def phase1(case, src, mosaic: bool):
    """extract_image_data_cpu of the case on its mosaic or on F, on a bare object (no GPU) -> the payload."""
    from raw2film_amd.hip_processor import HipProcessor

    proc = HipProcessor.__new__(HipProcessor)
    raw = {}
    if mosaic:
        profile, denoise = profiles(case)
        raw = dict(raw_profile=profile, raw_denoise=denoise)
    return HipProcessor.extract_image_data_cpu(proc, src, exposure=exposure_of(case, mosaic), **load_keywords(case), **raw)


def demosaic_keys(case) -> set:
    """The keys a case's `demosaic` step carries (extract_image_data_cpu)."""
    keys = {"params", "window", "rotate_times"}
    keys |= {"orientation"} if case["orientation"] else set()
    keys |= {"levels"} if case["scale"] != "numeric" else set()
    keys |= {"denoise", "profile"} if case["raw_denoise"] != "none" else set()
    keys |= {"clip"} if case["scale"] == "numeric" and case["highlight"] == "blend" else set()
    keys |= {"median"} if case["median_passes"] else set()
    return keys


# ---- the model route
def raw_model(mosaic, case, stats=None):
    """(F, last_raw_scale, last_raw_denoise) of a mosaic under the case's RAW-side values.  stats: the blend's pixel classes."""
    from raw2film_amd.raw import RawProfile, XTransProfile

    xtrans = is_xtrans(case)
    period = 6 if xtrans else 2
    black = [BLACK] * period ** 2
    white, thr = _levels(case)
    numeric = case["scale"] == "numeric"
    d = 0 if numeric else lm.data_maximum(mosaic, black, period)
    mul, used, adjusted, clip = hm.scale(WB, white, thr, black, d, _mode(case))
    clip = clip if case["highlight"] == "blend" else None
    raw_scale = None if numeric else {"data_maximum": d, "maximum_used": used, "adjusted": adjusted}
    cls = XTransProfile if xtrans else RawProfile
    profile, raw_denoise = cls(_pattern(case), black=BLACK, multipliers=mul, matrix=MATRIX), None
    if case["raw_denoise"] != "none":
        maximum = FIXED_MAXIMUM if case["raw_denoise"] == "fixed" else used
        shift = dnm.shift_of(maximum)
        mosaic = dnm.denoise(mosaic, (BLACK,) * 4, maximum, THRESHOLD)
        profile = RawProfile(_pattern(case), black=0, multipliers=tuple(m * 2.0 ** -shift for m in mul), matrix=MATRIX)
        raw_denoise = {"threshold": THRESHOLD, "maximum": maximum, "shift": shift}
    if stats is not None and clip is not None:
        hm.demosaic(mosaic, profile, clip, half_size=case["half_size"], xtrans=xtrans, stats=stats)
    D = mm.demosaic(mosaic, profile, case["median_passes"], clip, half_size=case["half_size"], xtrans=xtrans)
    return hm.orient(D, case["orientation"]), raw_scale, raw_denoise


@functools.lru_cache(maxsize=None)
def _model_frame(key):
    case = dict(zip(RAW_AXES, key))
    F, scale, denoise = raw_model(mosaic_of(case), case)
    F.setflags(write=False)
    return F, scale, denoise


def model_frame(case):
    """(F, the expected last_raw_scale, the expected last_raw_denoise) of a case on its shared mosaic; computed once per set of
    RAW-side values and shared (read-only)."""
    return _model_frame(tuple(case[a] for a in RAW_AXES))


def cropped(F, payload):
    """What the crops of F's own payload keep of F (a lens step's or the device decode's window, else what the host cut)."""
    window = (payload.get("lens") or {}).get("window") or payload.get("u16_window")
    if window is None:
        return payload["image_array"][..., :3]
    r0, c0, nr, nc = window
    return F[r0:r0 + nr, c0:c0 + nc]


# ---- the session walk
SESSION_SEEDS = (3678, 7339)  # (walks whose forty steps hold what tests/test_prepath_cases_host.py asks of them)
SESSION_SOURCES = ("bayer", "bayer2", "xtrans", "frame")
SESSION_ARRAY = {"bayer": "RGGB", "bayer2": "GBRG", "xtrans": "xtrans1", "frame": "RGGB"}
STEP_KINDS = ("source", "axis", "film", "repeat", "edit")
_KIND_WEIGHTS = ("source",) * 4 + ("axis",) * 9 + ("film",) * 2 + ("repeat",) * 2 + ("edit",) * 2
FILM_SLIDERS = {"exp_comp": (0.0, 0.3, -0.2), "exp_kelvin": (6000, 5000, 6500), "sat_adjust": (1.0, 1.2)}
SESSION_START = {"half_size": True, "orientation": 5, "scale": "adjusted", "highlight": "blend", "median_passes": 1, "raw_denoise": "auto",
                 "exposure": "auto", "format": "36x24", "zoom": 1.0, "rotate_times": 0, "rotation": 0.0, "lens_profile": "none",
                 "post": "plain"}


# what comes up three times as often as the other axes: what the frame cache is keyed by since the last fuzz test was written, the
# exposure mode (a turned or rotated frame admits no "auto", so the device exposure record needs its share of the steps) and the
# post-path
_OFTEN = RAW_AXES + ("lens_profile", "exposure", "post")


class Lcg:
    """Knuth's 64-bit linear congruential generator: the walk is the same list on every Python and NumPy."""

    def __init__(self, seed):
        self.state = (int(seed) * 2654435761 + 1) & (2 ** 64 - 1)

    def below(self, n: int) -> int:
        self.state = (self.state * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        return (self.state >> 33) % n


def cache_changes(walk) -> set:
    """The axes a walk changes under the eyes of the frame cache: between two process() calls on the same mosaic (an export leaves
    the cached frame alone) -- a key of the cache that missed such an axis would hand the session a stale frame."""
    return {a for prev, step in zip(walk, walk[1:])
            if step["kind"] == "axis" and step["source"] != "frame" and step["entry"] == prev["entry"] == "process"
            for a in step["case"] if step["case"][a] != prev["case"][a]}


def auto_exposure_visits(walk) -> set:
    """Where a walk measures the exposure on the device (exposure=None on a mosaic, through process()): the sources, and "repeat" /
    "edit" where such a step repeats the call (a cache hit) or follows an in-place edit."""
    steps = [s for s in walk if s["case"]["exposure"] == "auto" and s["source"] != "frame" and s["entry"] == "process"]
    return {s["source"] for s in steps} | {s["kind"] for s in steps if s["kind"] in ("repeat", "edit")}


def same(a, b) -> bool:
    """Two results of one entry point are the same bytes: files, or arrays of one shape and dtype."""
    return a == b if isinstance(a, bytes) else a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b))


def session_source(name):
    """A writable copy of a session's source: the walk edits mosaics in place.  "frame": one F, as a plain uint16 source."""
    if name == "frame":
        return model_frame({**SESSION_START, "array": "RGGB", "half_size": False})[0].copy()
    return _source(name).copy()


def session_walk(seed, steps):
    """The steps of a session -> a list of {"kind", "source", "case" (every axis but `entry`; `array` follows the source), "film",
    "entry" ("process", or every fifth step "jpeg" / "tiff" in turn), "version" (of the source's content)}.  A step switches source,
    changes one axis value within the admissible set, moves a film slider, repeats the call, or edits the current mosaic in place
    (the caller applies `edit_in_place(mosaic, version)` of an "edit" step before its call)."""
    rng = Lcg(seed)
    source, state, film = "bayer", dict(SESSION_START), {k: v[0] for k, v in FILM_SLIDERS.items()}
    versions = dict.fromkeys(SESSION_SOURCES, 0)
    out = []
    for i in range(steps):
        kind = _KIND_WEIGHTS[rng.below(len(_KIND_WEIGHTS))] if i else "source"
        if kind == "edit" and source == "frame":
            kind = "source"  # (no mosaic to edit)
        if kind == "source":
            others = [s for s in SESSION_SOURCES if s != source] if i else [source]
            source = others[rng.below(len(others))]
            if source == "xtrans":
                state["raw_denoise"] = "none"  # (the one value an X-Trans source admits)
        elif kind == "axis":
            names = [a for a in AXES if a not in ("array", "entry") for _ in range(3 if a in _OFTEN else 1)]
            while True:
                axis = names[rng.below(len(names))]
                values = [v for v in AXES[axis] if v != state[axis]]
                new = dict(state, **{axis: values[rng.below(len(values))]})
                if admissible({**new, "array": SESSION_ARRAY[source]}):
                    state = new
                    break
        elif kind == "film":
            name = list(FILM_SLIDERS)[rng.below(len(FILM_SLIDERS))]
            values = [v for v in FILM_SLIDERS[name] if v != film[name]]
            film[name] = values[rng.below(len(values))]
        elif kind == "edit":
            versions[source] += 1
        entry = "process" if i % 5 != 4 else ("jpeg", "tiff")[(i // 5) % 2]
        out.append({"kind": kind, "source": source, "case": {**state, "array": SESSION_ARRAY[source]}, "film": dict(film), "entry": entry,
                    "version": versions[source]})
    return out
