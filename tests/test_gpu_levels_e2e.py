"""A deferred profile through HipProcessor: process(mosaic, raw_profile=profile with RawLevels) measures the mosaic's data maximum on
the device, resolves the profile and renders the bytes of the same call with the resolved numeric profile -- for both arrays, both
sizes, upright and turned, with levels the frame adjusts and levels it does not (chosen on the CPU from the model's d,
tests/levels_model.py) --; `last_raw_scale` holds the model's numbers; the two-phase API, the exposure measured on the device, an
export that asked to stream, and a cached frame that is not measured twice."""

import numpy as np
import pytest

import levels_model as lm
import xtrans_model as xm
from helpers import stocks

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KW = dict(halation=False, sharpness=False, grain=0, exp_kelvin=6000, color_masking=1.0, frame_width=36, frame_height=24, max_scale=None)
MATRIX = ((0.52, 0.27, 0.15), (0.25, 0.68, 0.07), (0.03, 0.12, 0.81))
WB = (1.9, 1.0, 1.5)
BLACK = 512
ADJUSTED, NOMINAL = BLACK + 12000, 16383  # white levels: 0.75 m < d < m, and d < 0.75 m


def _mosaic():
    """A 96 x 144 mosaic with image-like statistics: a smooth ramp plus noise, black 512, a peak near 10 000."""
    rng = np.random.default_rng(17)
    y, x = np.mgrid[0:96, 0:144]
    base = 600 + 9000 * (0.5 + 0.5 * np.sin(x / 23.0) * np.cos(y / 17.0)) + rng.normal(0, 120, (96, 144))
    return np.clip(base, 0, 16383).astype(np.uint16)


MOSAIC = _mosaic()
D = {2: lm.data_maximum(MOSAIC, [BLACK] * 4, 2), 6: lm.data_maximum(MOSAIC, [BLACK] * 36, 6)}


def test_the_levels_are_what_their_names_say():
    assert D[2] == D[6] == int(MOSAIC.max()) - BLACK and 9000 < D[2] < 11000
    assert 0.75 * (ADJUSTED - BLACK) < D[2] < ADJUSTED - BLACK and D[2] < 0.75 * (NOMINAL - BLACK)
    assert lm.scale(WB, ADJUSTED, 0.75, [BLACK] * 4, D[2])[1:] == (D[2], True)
    assert lm.scale(WB, NOMINAL, 0.75, [BLACK] * 4, D[2])[1:] == (NOMINAL - BLACK, False)


@pytest.fixture(scope="module")
def proc():
    from raw2film_amd import HipProcessor

    p = HipProcessor(cameras={}, lenses={}, device=0)
    yield p
    p.close()


def profile(kind, white_level, orientation=0):
    from raw2film_amd.raw import RawLevels, RawProfile, XTransProfile

    lv = RawLevels(WB, white_level)
    if kind == "bayer":
        return RawProfile("GRBG", black=BLACK, multipliers=lv, matrix=MATRIX, orientation=orientation)
    return XTransProfile(xm.PATTERNS[1], black=BLACK, multipliers=lv, matrix=MATRIX, orientation=orientation)


@pytest.mark.parametrize("orientation", [0, 5])
@pytest.mark.parametrize("half", [True, False], ids=["reduced", "full"])
@pytest.mark.parametrize("white_level", [ADJUSTED, NOMINAL], ids=["adjusted", "nominal"])
@pytest.mark.parametrize("kind", ["bayer", "xtrans"])
def test_a_deferred_profile_renders_the_bytes_of_its_resolved_one(proc, kind, white_level, half, orientation):
    neg, prt, _ = stocks()
    deferred = profile(kind, white_level, orientation)
    d = D[6 if kind == "xtrans" else 2]
    mul, used, adjusted = lm.scale(WB, white_level, 0.75, deferred.black, d)
    kw = dict(print_film=prt, half_size=half, seed=3, exposure=0.5, **KW)
    got = proc.process(MOSAIC, neg, 6, 0.4, raw_profile=deferred, **kw)
    assert proc.last_raw_scale == {"data_maximum": d, "maximum_used": used, "adjusted": adjusted}
    assert adjusted == (white_level == ADJUSTED)
    resolved = deferred.resolve(d)
    assert tuple(resolved.multipliers) == tuple(type(deferred)(deferred.pattern, multipliers=mul).multipliers)
    want = proc.process(MOSAIC, neg, 6, 0.4, raw_profile=resolved, **kw)
    assert proc.last_raw_scale is None  # (a numeric profile)
    assert got.shape == want.shape and got.dtype == want.dtype and got.std() > 1
    assert np.array_equal(got, want), int((got != want).sum())
    nominal = proc.process(MOSAIC, neg, 6, 0.4, raw_profile=deferred.resolve(0), **kw)
    if adjusted:  # the measured scale is another render than the nominal one: the equality above cannot hold vacuously
        assert not np.array_equal(got, nominal)
    else:
        assert np.array_equal(got, nominal)


def test_the_two_phase_api_and_the_device_exposure(proc):
    neg, prt, _ = stocks()
    deferred = profile("bayer", ADJUSTED)
    resolved = deferred.resolve(D[2])
    kw = dict(print_film=prt, half_size=True, seed=3, **KW)
    want = proc.process(MOSAIC, neg, 6, 0.4, raw_profile=resolved, exposure=0.5, **kw)
    pay = proc.extract_image_data_cpu(MOSAIC, raw_profile=deferred, half_size=True, exposure=0.5, frame_width=36, frame_height=24, max_scale=None)
    assert pay["image_array"].shape == (96, 144) and pay["demosaic"]["levels"] is deferred
    assert np.array_equal(proc.process_preloaded(pay, neg, 6, 0.4, final_scaling="cpu", **kw), want)
    assert proc.last_raw_scale == {"data_maximum": D[2], "maximum_used": D[2], "adjusted": True}
    pending = proc.submit_preloaded(pay, neg, 6, 0.4, final_scaling="cpu", **kw)
    assert np.array_equal(pending.result(), want)
    # exposure=None: measured on the device, behind the resolved demosaic
    a = proc.process(MOSAIC, neg, 6, 0.4, raw_profile=deferred, exposure=None, **kw)
    stops = proc.last_auto_exposure
    b = proc.process(MOSAIC, neg, 6, 0.4, raw_profile=resolved, exposure=None, **kw)
    assert np.array_equal(a, b) and stops == proc.last_auto_exposure and proc.exposure_rejected is None
    c = proc.process(MOSAIC, neg, 6, 0.4, raw_profile=deferred.resolve(0), exposure=None, **kw)
    assert proc.last_auto_exposure != stops  # (the statistic saw the adjusted frame)
    assert c.shape == a.shape


def test_an_export_that_asks_to_stream_is_rendered_in_one_piece_and_says_why(proc, monkeypatch):
    neg, prt, _ = stocks()
    deferred = profile("bayer", ADJUSTED)
    kw = dict(print_film=prt, half_size=False, seed=3, exposure=0.5, **KW)
    whole = proc.process_jpeg(MOSAIC, neg, 6, 0.4, quality=90, raw_profile=deferred, **kw)
    assert whole == proc.process_jpeg(MOSAIC, neg, 6, 0.4, quality=90, raw_profile=deferred.resolve(D[2]), **kw)
    small = proc.process_jpeg(MOSAIC, neg, 6, 0.4, quality=90, stream=True, raw_profile=deferred, **kw)
    assert small == whole and "below 16.7 M" in proc.stream_rejected  # (the earlier reasons keep their place)
    # the same call where nothing else keeps the frame from streaming: the new reason
    monkeypatch.setattr("raw2film_amd.payload.STREAM_MIN_SAMPLES", 1)
    streamed = proc.process_jpeg(MOSAIC, neg, 6, 0.4, quality=90, stream=True, raw_profile=deferred, **kw)
    assert streamed == whole and "demosaic" in proc.stream_rejected and "RawLevels" in proc.stream_rejected
    pay = proc.extract_image_data_cpu(MOSAIC, raw_profile=deferred, half_size=False, exposure=0.5, frame_width=36, frame_height=24, max_scale=None)
    again = proc.process_preloaded_jpeg(pay, neg, 6, 0.4, quality=90, final_scaling="cpu", stream=True, print_film=prt, seed=3, **KW)
    assert again == whole and "RawLevels" in proc.stream_rejected


def test_a_cached_frame_keeps_its_scale_and_is_not_measured_again(proc, monkeypatch):
    neg, prt, _ = stocks()
    deferred = profile("xtrans", ADJUSTED, 5)
    kw = dict(print_film=prt, half_size=True, seed=3, exposure=0.5, **KW)
    calls = []
    measure = proc.ctx.mosaic_maximum
    monkeypatch.setattr(proc.ctx, "mosaic_maximum", lambda *a, **k: calls.append(1) or measure(*a, **k))
    first = proc.process(MOSAIC, neg, 6, 0.4, raw_profile=deferred, **kw)
    scale = proc.last_raw_scale
    assert len(calls) == 1 and scale == {"data_maximum": D[6], "maximum_used": D[6], "adjusted": True}
    second = proc.process(MOSAIC, neg, 6, 0.4, raw_profile=profile("xtrans", ADJUSTED, 5), **dict(kw, exp_comp=0.3))
    assert len(calls) == 1 and proc.last_raw_scale == scale and not np.array_equal(first, second)
    proc.process(MOSAIC, neg, 6, 0.4, raw_profile=profile("xtrans", NOMINAL, 5), **kw)  # other levels: another frame
    nominal = {"data_maximum": D[6], "maximum_used": NOMINAL - BLACK, "adjusted": False}
    assert len(calls) == 2 and proc.last_raw_scale == nominal
    # an export of another frame in between is that call's (a numeric profile: None) and leaves the cached frame its scale
    proc.process_jpeg(MOSAIC, neg, 6, 0.4, quality=90, raw_profile=deferred.resolve(D[6]), **kw)
    assert proc.last_raw_scale is None and len(calls) == 2
    proc.process(MOSAIC, neg, 6, 0.4, raw_profile=profile("xtrans", NOMINAL, 5), **dict(kw, exp_comp=0.1))
    assert proc.last_raw_scale == nominal and len(calls) == 2
    # a numeric profile behind a deferred one is None whichever path the call takes: here the row-band gates are asked first
    monkeypatch.setattr("raw2film_amd.payload.STREAM_MIN_SAMPLES", 1)
    numeric = profile("bayer", ADJUSTED).resolve(D[2])
    proc.process(MOSAIC, neg, 6, 0.4, raw_profile=numeric, **dict(kw, cache=False, half_size=False))
    assert proc.last_raw_scale is None and len(calls) == 2
