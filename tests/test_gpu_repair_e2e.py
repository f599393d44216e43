"""raw_repair through HipProcessor, end to end, with no new oracle: process(mosaic, raw_profile=p, raw_repair=r) renders the bytes of
process(the model's repaired mosaic, raw_profile=p) (tests/repair_model.py) -- for a Bayer mosaic at full and half size, with an
orientation, for an X-Trans mosaic, with median_passes, with raw_denoise and with a ("blend", clip) profile --, `last_raw_repair`
holds the model's count, a RawLevels profile's adjust_maximum decision no longer hangs on one hot sample, and a Bayer mosaic just
above the 16.7 M-sample gate streams in row bands to the bytes and the count of the one-piece call, through process() and through
process_jpeg(stream=True)."""

import numpy as np
import pytest

import highlight_model as hm
import levels_model as lm
import repair_model as model
import xtrans_model as xm
from helpers import stocks

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KW = dict(halation=False, sharpness=False, grain=0, exp_kelvin=6000, color_masking=1.0, frame_width=36, frame_height=24, max_scale=None)
MATRIX = ((0.52, 0.27, 0.15), (0.25, 0.68, 0.07), (0.03, 0.12, 0.81))
WB, BLACK, WHITE = (1.9, 1.0, 1.5), 512, 16383
MUL = tuple(w / min(WB) * 65535.0 / (WHITE - BLACK) for w in WB)
THRESHOLD, Q, SHAPE = 3000, 128, (96, 144)


def sprinkled(shape, tag, seed, share=0.004, high=6000):
    """A smooth field with patches (image-like) that stays below half of the range, with `share` of its samples stuck near the white level."""
    base = hm.patches(shape[0], shape[1], tag, 15000, low=700, high=high).astype(np.int64).clip(0, 6000)
    rng = np.random.default_rng(seed)
    hot = rng.random(shape) < share
    return np.where(hot, rng.integers(WHITE - 400, WHITE + 1, shape), base).astype(np.uint16), hot


MOSAIC, SPRINKLED = sprinkled(SHAPE, "repair/e2e", 5)


@pytest.fixture(scope="module")
def proc():
    from raw2film_amd import HipProcessor

    p = HipProcessor(cameras={}, lenses={}, device=0)
    yield p
    p.close()


def record(mn=4):
    from raw2film_amd.raw import HotPixels

    return HotPixels(THRESHOLD, Q / 256, mn)


def profile(kind, multipliers=MUL, **kw):
    from raw2film_amd.raw import RawProfile, XTransProfile

    if kind == "bayer":
        return RawProfile("GRBG", black=BLACK, multipliers=multipliers, matrix=MATRIX, **kw)
    return XTransProfile(xm.PATTERNS[1], black=BLACK, multipliers=multipliers, matrix=MATRIX, **kw)


def repaired(mosaic, kind, mn=4):
    from raw2film_amd.raw import XTransProfile

    if kind == "bayer":
        return model.repair(mosaic, 2, (BLACK,) * 4, THRESHOLD, Q, mn)
    cfa = np.array([["RGB".index(c) for c in row] for row in XTransProfile(xm.PATTERNS[1]).pattern], np.int32)
    return model.repair(mosaic, 6, (BLACK,) * 36, THRESHOLD, Q, mn, cfa)


CASES = {
    "bayer-full": ("bayer", False, {}, {}),
    "bayer-half": ("bayer", True, {}, {}),
    "orientation-5": ("bayer", False, dict(orientation=5), {}),
    "xtrans": ("xtrans", False, {}, {}),
    "xtrans-third": ("xtrans", True, dict(orientation=6), {}),
    "median-2": ("bayer", False, dict(median_passes=2), {}),
    "denoise": ("bayer", False, {}, "denoise"),
    "blend": ("bayer", False, dict(highlight=("blend", 30000)), {}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_the_repair_renders_the_models_repaired_mosaic(proc, case):
    from raw2film_amd.raw import WaveletDenoise

    kind, half, pkw, extra = CASES[case]
    neg, prt, _ = stocks()
    prof = profile(kind, **pkw)
    extra = dict(raw_denoise=WaveletDenoise(300.0, WHITE - BLACK)) if extra == "denoise" else {}
    clean, hot = repaired(MOSAIC, kind)
    assert hot.sum() >= 0.5 * SPRINKLED.sum() > 20  # (the sprinkled samples are what the model repairs: not a vacuous equality)
    kw = dict(print_film=prt, seed=3, exposure=-0.5, raw_profile=prof, half_size=half, **extra, **KW)
    got = proc.process(MOSAIC, neg, 6, 0.4, raw_repair=record(), **kw)
    assert proc.last_raw_repair == {"threshold": THRESHOLD, "q": Q, "min_neighbours": 4, "repaired": int(hot.sum())}
    want = proc.process(clean, neg, 6, 0.4, **kw)
    assert proc.last_raw_repair is None
    assert got.shape == want.shape and got.dtype == want.dtype and got.std() > 1
    assert np.array_equal(got, want), int((got != want).sum())
    plain = proc.process(MOSAIC, neg, 6, 0.4, **kw)
    assert not np.array_equal(got, plain)  # (the defects show in the picture without the step)
    # a cached frame keeps its record; the two-phase API and one export render the same bytes
    again = proc.process(MOSAIC, neg, 6, 0.4, raw_repair=record(), **kw)
    assert np.array_equal(again, want) and proc.last_raw_repair["repaired"] == int(hot.sum())
    again = proc.process(MOSAIC, neg, 6, 0.4, raw_repair=record(), **kw)  # (the same frame: not uploaded again)
    assert np.array_equal(again, want) and proc.last_raw_repair["repaired"] == int(hot.sum())
    pay = proc.extract_image_data_cpu(MOSAIC, raw_profile=prof, raw_repair=record(), half_size=half, exposure=-0.5, frame_width=36,
                                      frame_height=24, max_scale=None, **extra)
    assert pay["demosaic"]["repair"] == record()
    rest = dict(print_film=prt, seed=3, **KW)
    assert np.array_equal(proc.process_preloaded(pay, neg, 6, 0.4, final_scaling="cpu", **rest), want)
    assert proc.last_raw_repair["repaired"] == int(hot.sum())
    assert np.array_equal(proc.submit_preloaded(pay, neg, 6, 0.4, final_scaling="cpu", **rest).result(), want)
    assert proc.last_raw_repair["repaired"] == int(hot.sum())
    a = proc.process_jpeg(MOSAIC, neg, 6, 0.4, quality=90, raw_repair=record(), **kw)
    assert proc.last_raw_repair["repaired"] == int(hot.sum())
    assert a == proc.process_jpeg(clean, neg, 6, 0.4, quality=90, **kw) and a == proc.encode_jpeg(want, 90)


def test_three_neighbours_repair_more_than_four(proc):
    neg, prt, _ = stocks()
    frame = MOSAIC.copy()
    ys, xs = np.nonzero(SPRINKLED[4:-4, 4:-6])
    frame[ys[:8] + 4, xs[:8] + 6] = WHITE  # a second stuck sample two columns on from eight of them
    kw = dict(print_film=prt, seed=3, exposure=-0.5, raw_profile=profile("bayer"), half_size=False, **KW)
    counts = {}
    for mn in (3, 4):
        clean, hot = repaired(frame, "bayer", mn)
        got = proc.process(frame, neg, 6, 0.4, raw_repair=record(mn), **kw)
        counts[mn] = proc.last_raw_repair["repaired"]
        assert counts[mn] == int(hot.sum()) and np.array_equal(got, proc.process(clean, neg, 6, 0.4, **kw))
    assert counts[3] > counts[4]


def test_one_hot_sample_no_longer_decides_adjust_maximum(proc):
    from raw2film_amd.raw import RawLevels

    neg, prt, _ = stocks()
    maximum = WHITE - BLACK
    frame = hm.patches(96, 144, "repair/levels", 15000, low=700, high=9000).astype(np.int64)
    frame = (BLACK + (frame - frame.min()) * (0.85 * maximum) / (frame.max() - frame.min())).astype(np.uint16)  # up to 85 % of the range
    y, x = np.unravel_index(np.argmin(frame[8:-8, 8:-8]), (80, 128))
    frame[y + 6:y + 11, x + 6:x + 11] = BLACK + 300  # a dark patch around ...
    frame[y + 8, x + 8] = WHITE  # ... one sample at the white level
    deferred = profile("bayer", RawLevels(WB, WHITE))
    clean, hot = repaired(frame, "bayer")
    assert hot[y + 8, x + 8] and clean[y + 8, x + 8] == BLACK + 300
    d_with, d_without = lm.data_maximum(clean, [BLACK] * 4, 2), lm.data_maximum(frame, [BLACK] * 4, 2)
    assert d_without == maximum and 0.75 * maximum < d_with < maximum
    assert lm.scale(WB, WHITE, 0.75, deferred.black, d_with)[2] and not lm.scale(WB, WHITE, 0.75, deferred.black, d_without)[2]
    kw = dict(print_film=prt, seed=3, exposure=-0.5, raw_profile=deferred, half_size=False, **KW)
    got = proc.process(frame, neg, 6, 0.4, raw_repair=record(), **kw)
    assert proc.last_raw_scale == {"data_maximum": d_with, "maximum_used": d_with, "adjusted": True}
    assert proc.last_raw_repair["repaired"] == int(hot.sum())
    want = proc.process(clean, neg, 6, 0.4, **kw)
    assert np.array_equal(got, want)
    proc.process(frame, neg, 6, 0.4, **kw)
    assert proc.last_raw_scale == {"data_maximum": maximum, "maximum_used": maximum, "adjusted": False}


# ---- the streamed band loop
# the square 36 x 36 format keeps 2368 x 2368 of a 2368 x 2400 frame: 16.8 M samples, every mosaic row travels
STREAM_KW = dict(halation=False, sharpness=False, grain=0, exp_kelvin=6000, color_masking=1.0, frame_width=36, frame_height=36, max_scale=None,
                 lens_correction=False, seed=3, exposure=0.5)


@pytest.fixture(scope="module")
def large():
    H, W = 2368, 2400
    small, _ = sprinkled((H // 8, W // 8), "repair/stream", 9, share=0.002)
    mosaic = np.tile(small, (8, 8))  # (image-like statistics with stuck samples, made cheaply)
    clean, hot = model.repair(mosaic, 2, (BLACK,) * 4, THRESHOLD, Q, 4)
    assert hot.sum() > 5000
    return mosaic, clean, int(hot.sum())


@pytest.mark.parametrize("median", [0, 2], ids=["plain", "median-2"])
def test_a_bayer_mosaic_streams_with_the_repair_to_the_one_piece_bytes_and_count(proc, large, median):
    neg, prt, _ = stocks()
    mosaic, clean, n_hot = large
    prof = profile("bayer", median_passes=median)
    kw = dict(STREAM_KW, half_size=False, cache=False, print_film=prt, raw_profile=prof)
    plans, inner = [], proc._run_bands

    def spy(frame, *a, **k):
        plans.append((list(frame.bounds), frame.source.upload_bounds(list(frame.bounds))))
        return inner(frame, *a, **k)

    proc._run_bands = spy
    try:
        assert proc.stream_bands == 16
        proc.stream_rejected = "unset"
        got = proc.process(mosaic, neg, 6, 0.4, raw_repair=record(), **kw).copy()
        assert proc.stream_rejected is None and len(plans) == 1 and len(plans[0][0]) - 1 >= 3, (proc.stream_rejected, plans)
        count = proc.last_raw_repair["repaired"]
        proc.stream_bands = 0
        want = proc.process(clean, neg, 6, 0.4, **kw).copy()
        one_piece = proc.process(mosaic, neg, 6, 0.4, raw_repair=record(), **kw).copy()
        assert proc.last_raw_repair["repaired"] == n_hot and len(plans) == 1  # (one piece: no band loop)
    finally:
        proc.stream_bands = 16
        proc._run_bands = inner
    assert plans[0][1][0] == 0 and plans[0][1][-1] == 2368  # every mosaic row travelled, so every row was repaired and counted
    assert got.std() > 1 and np.array_equal(one_piece, want)
    assert np.array_equal(got, want), int((got != want).sum())
    assert count == n_hot


def test_process_jpeg_streams_with_the_repair(proc, large):
    neg, prt, _ = stocks()
    mosaic, clean, n_hot = large
    prof = profile("bayer")
    kw = dict(STREAM_KW, half_size=False, print_film=prt, raw_profile=prof)
    a = proc.process_jpeg(mosaic, neg, 6, 0.4, quality=90, stream=True, raw_repair=record(), **kw)
    assert proc.stream_rejected is None and proc.last_raw_repair["repaired"] == n_hot
    b = proc.process_jpeg(clean, neg, 6, 0.4, quality=90, stream=False, **kw)
    assert a == b
    c = proc.process_jpeg(mosaic, neg, 6, 0.4, quality=90, stream=False, raw_repair=record(), **kw)
    assert c == b and proc.last_raw_repair["repaired"] == n_hot
