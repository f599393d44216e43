"""raw_denoise through HipProcessor on a 96 x 144 mosaic: process(mosaic, raw_profile=P, raw_denoise=Dn) renders the bytes of
process(the model's denoised mosaic, raw_profile=P') with P' numeric, black 0 and P's multipliers times 2^-shift (built here by hand,
the mosaic by tests/denoise_model.py) -- at both sizes, turned, and with a deferred "blend" profile whose resolved maximum the denoise
takes --; `last_raw_denoise` and `last_raw_scale`; an export that asked to stream; the frame cache; the two-phase API."""

import numpy as np
import pytest

import denoise_model as model
import levels_model as lm
from helpers import stocks

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KW = dict(halation=False, sharpness=False, grain=0, exp_kelvin=6000, color_masking=1.0, frame_width=36, frame_height=24, max_scale=None)
MATRIX = ((0.52, 0.27, 0.15), (0.25, 0.68, 0.07), (0.03, 0.12, 0.81))
WB = (1.9, 1.0, 1.5)
BLACK = (512, 515, 509, 512)
WHITE = 16383
MAXIMUM = WHITE - min(BLACK)  # 15874: shift 2
T = 300.0


def _mosaic():
    """A 96 x 144 mosaic with image-like statistics: a smooth ramp plus sensor-like noise, black about 512, a peak near 10 000."""
    rng = np.random.default_rng(29)
    y, x = np.mgrid[0:96, 0:144]
    base = 600 + 9000 * (0.5 + 0.5 * np.sin(x / 23.0) * np.cos(y / 17.0)) + rng.normal(0, 160, (96, 144))
    return np.clip(base, 0, 16383).astype(np.uint16)


MOSAIC = _mosaic()


@pytest.fixture(scope="module")
def proc():
    from raw2film_amd import HipProcessor

    p = HipProcessor(cameras={}, lenses={}, device=0)
    yield p
    p.close()


def numeric(orientation=0):
    from raw2film_amd.raw import RawProfile

    mul = tuple(w / min(WB) * 65535.0 / MAXIMUM for w in WB)
    return RawProfile("GRBG", black=BLACK, multipliers=mul, matrix=MATRIX, orientation=orientation)


def behind(profile, shift):
    """P' of include/r2f.h: the numeric profile the demosaic behind the denoise runs with, spelled out."""
    from raw2film_amd.raw import RawProfile

    return RawProfile(profile.pattern, black=0, multipliers=tuple(m * 2.0 ** -shift for m in profile.multipliers), matrix=profile.matrix,
                      highlight=profile.highlight, orientation=profile.orientation)


def test_the_model_changes_the_mosaic():
    clean = model.denoise(MOSAIC, BLACK, MAXIMUM, T)
    barely = model.denoise(MOSAIC, BLACK, MAXIMUM, 0.001)
    assert model.shift_of(MAXIMUM) == 2 and not np.array_equal(clean, barely)
    # (neighbours of one plane lie closer together behind the larger threshold)
    assert np.abs(np.diff(clean[::2, ::2].astype(np.int64), axis=1)).mean() < np.abs(np.diff(barely[::2, ::2].astype(np.int64), axis=1)).mean()


@pytest.mark.parametrize("orientation", [0, 5])
@pytest.mark.parametrize("half", [True, False], ids=["half", "full"])
def test_a_denoised_call_renders_the_bytes_of_the_models_mosaic(proc, half, orientation):
    from raw2film_amd.raw import WaveletDenoise

    neg, prt, _ = stocks()
    P = numeric(orientation)
    kw = dict(print_film=prt, half_size=half, seed=3, exposure=0.5, **KW)
    got = proc.process(MOSAIC, neg, 6, 0.4, raw_profile=P, raw_denoise=WaveletDenoise(T, MAXIMUM), **kw)
    assert proc.last_raw_denoise == {"threshold": T, "maximum": MAXIMUM, "shift": 2} and proc.last_raw_scale is None
    want = proc.process(model.denoise(MOSAIC, BLACK, MAXIMUM, T), neg, 6, 0.4, raw_profile=behind(P, 2), **kw)
    assert proc.last_raw_denoise is None
    assert got.shape == want.shape and got.dtype == want.dtype and got.std() > 1
    assert np.array_equal(got, want), int((got != want).sum())
    plain = proc.process(MOSAIC, neg, 6, 0.4, raw_profile=P, **kw)
    assert plain.shape == got.shape and not np.array_equal(got, plain)  # (the equality above cannot hold vacuously)


def test_a_deferred_blend_profile_hands_its_resolved_maximum_to_the_denoise(proc):
    from raw2film_amd.raw import RawLevels, RawProfile, WaveletDenoise

    neg, prt, _ = stocks()
    white = min(BLACK) + 12000  # 0.75 m < d < m: the frame is adjusted, and the maximum is the measured one
    deferred = RawProfile("GRBG", black=BLACK, multipliers=RawLevels(WB, white), matrix=MATRIX, highlight="blend")
    d = lm.data_maximum(MOSAIC, list(BLACK), 2)
    resolved, scale = deferred.resolve_scale(d)
    used = int(scale.maximum_used)
    assert used == d and bool(scale.adjusted) and resolved.blend_clip is not None
    shift = model.shift_of(used)
    for half in (True, False):
        kw = dict(print_film=prt, half_size=half, seed=3, exposure=0.5, **KW)
        got = proc.process(MOSAIC, neg, 6, 0.4, raw_profile=deferred, raw_denoise=WaveletDenoise(T), **kw)
        assert proc.last_raw_scale == {"data_maximum": d, "maximum_used": used, "adjusted": True}
        assert proc.last_raw_denoise == {"threshold": T, "maximum": used, "shift": shift}
        want = proc.process(model.denoise(MOSAIC, BLACK, used, T), neg, 6, 0.4, raw_profile=behind(resolved, shift), **kw)
        assert np.array_equal(got, want), (half, int((got != want).sum()))
        assert not np.array_equal(got, proc.process(MOSAIC, neg, 6, 0.4, raw_profile=deferred, **kw))
    # a maximum of the record's own wins over the resolved one
    proc.process(MOSAIC, neg, 6, 0.4, raw_profile=deferred, raw_denoise=WaveletDenoise(T, 4000), **kw)
    assert proc.last_raw_denoise == {"threshold": T, "maximum": 4000, "shift": 4} and proc.last_raw_scale["maximum_used"] == used


def test_an_export_that_asks_to_stream_is_rendered_in_one_piece_and_names_the_denoise(proc, monkeypatch):
    from raw2film_amd.raw import WaveletDenoise

    neg, prt, _ = stocks()
    P, dn = numeric(), WaveletDenoise(T, MAXIMUM)
    kw = dict(print_film=prt, half_size=False, seed=3, exposure=0.5, **KW)
    whole = proc.process_jpeg(MOSAIC, neg, 6, 0.4, quality=90, raw_profile=P, raw_denoise=dn, **kw)
    assert whole == proc.process_jpeg(model.denoise(MOSAIC, BLACK, MAXIMUM, T), neg, 6, 0.4, quality=90, raw_profile=behind(P, 2), **kw)
    small = proc.process_jpeg(MOSAIC, neg, 6, 0.4, quality=90, stream=True, raw_profile=P, raw_denoise=dn, **kw)
    assert small == whole and "below 16.7 M" in proc.stream_rejected  # (the earlier reasons keep their place)
    monkeypatch.setattr("raw2film_amd.payload.STREAM_MIN_SAMPLES", 1)  # where nothing else keeps the frame from streaming
    streamed = proc.process_jpeg(MOSAIC, neg, 6, 0.4, quality=90, stream=True, raw_profile=P, raw_denoise=dn, **kw)
    assert streamed == whole and proc.stream_rejected.startswith("the demosaic step (raw_profile): ") and "raw_denoise" in proc.stream_rejected
    assert proc.last_raw_denoise == {"threshold": T, "maximum": MAXIMUM, "shift": 2}
    pay = proc.extract_image_data_cpu(MOSAIC, raw_profile=P, raw_denoise=dn, half_size=False, exposure=0.5, frame_width=36, frame_height=24,
                                      max_scale=None)
    again = proc.process_preloaded_jpeg(pay, neg, 6, 0.4, quality=90, final_scaling="cpu", stream=True, print_film=prt, seed=3, **KW)
    assert again == whole and "raw_denoise" in proc.stream_rejected
    # process(cache=False) asks the same gates and renders the one-piece bytes
    a = proc.process(MOSAIC, neg, 6, 0.4, raw_profile=P, raw_denoise=dn, **dict(kw, cache=False))
    assert np.array_equal(a, proc.process(MOSAIC, neg, 6, 0.4, raw_profile=P, raw_denoise=dn, **kw))


def test_a_cached_frame_is_not_denoised_again_and_a_changed_threshold_is(proc, monkeypatch):
    from raw2film_amd.raw import WaveletDenoise

    neg, prt, _ = stocks()
    P = numeric()
    kw = dict(print_film=prt, half_size=True, seed=3, exposure=0.5, **KW)
    calls = []
    run = proc.ctx.mosaic_denoise
    monkeypatch.setattr(proc.ctx, "mosaic_denoise", lambda *a, **k: calls.append(1) or run(*a, **k))
    first = proc.process(MOSAIC, neg, 6, 0.4, raw_profile=P, raw_denoise=WaveletDenoise(T, MAXIMUM), **kw)
    record = proc.last_raw_denoise
    assert len(calls) == 1 and record == {"threshold": T, "maximum": MAXIMUM, "shift": 2}
    second = proc.process(MOSAIC, neg, 6, 0.4, raw_profile=numeric(), raw_denoise=WaveletDenoise(T, MAXIMUM), **dict(kw, exp_comp=0.3))
    assert len(calls) == 1 and proc.last_raw_denoise == record and not np.array_equal(first, second)
    third = proc.process(MOSAIC, neg, 6, 0.4, raw_profile=P, raw_denoise=WaveletDenoise(T / 2, MAXIMUM), **kw)
    assert len(calls) == 2 and proc.last_raw_denoise == {"threshold": T / 2, "maximum": MAXIMUM, "shift": 2}
    assert not np.array_equal(first, third)
    proc.process(MOSAIC, neg, 6, 0.4, raw_profile=P, **kw)  # no record: another frame, and nothing to report
    assert len(calls) == 2 and proc.last_raw_denoise is None


def test_the_two_phase_api_yields_the_same_frame(proc):
    from raw2film_amd.raw import WaveletDenoise

    neg, prt, _ = stocks()
    P, dn = numeric(), WaveletDenoise(T, MAXIMUM)
    kw = dict(print_film=prt, half_size=True, seed=3, **KW)
    want = proc.process(MOSAIC, neg, 6, 0.4, raw_profile=P, raw_denoise=dn, exposure=0.5, **kw)
    pay = proc.extract_image_data_cpu(MOSAIC, raw_profile=P, raw_denoise=dn, half_size=True, exposure=0.5, frame_width=36, frame_height=24,
                                      max_scale=None)
    assert pay["image_array"].shape == (96, 144) and pay["demosaic"]["denoise"] is dn
    assert np.array_equal(proc.process_preloaded(pay, neg, 6, 0.4, final_scaling="cpu", **kw), want)
    assert proc.last_raw_denoise == {"threshold": T, "maximum": MAXIMUM, "shift": 2}
    pending = proc.submit_preloaded(pay, neg, 6, 0.4, final_scaling="cpu", **kw)
    assert np.array_equal(pending.result(), want)
