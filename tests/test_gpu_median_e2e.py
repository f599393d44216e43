"""median_passes through HipProcessor, end to end: process(mosaic, raw_profile=a profile with median_passes=2) renders what
process() of the model's demosaiced frame renders (tests/median_model.py: the demosaic, step M, Blend, step C) -- for both arrays,
both sizes, upright and with orientation=6 --, and so do process_jpeg and the two-phase API; combined with raw_denoise, and with
RawLevels and highlight="blend"; and a Bayer mosaic just above the 16.7 M-sample gate streams in row bands
(r2f_demosaic_median_f32) to the bytes of the one-piece call."""

import numpy as np
import pytest

import denoise_model
import highlight_model as hm
import levels_model as lm
import median_model as mm
import xtrans_model as xm
from helpers import stocks

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KW = dict(halation=False, sharpness=False, grain=0, exp_kelvin=6000, color_masking=1.0, frame_width=36, frame_height=24, max_scale=None)
MATRIX = ((0.52, 0.27, 0.15), (0.25, 0.68, 0.07), (0.03, 0.12, 0.81))
WB, BLACK, WHITE = (1.9, 1.0, 1.5), 512, 16383
MUL = tuple(w / min(WB) * 65535.0 / (WHITE - BLACK) for w in WB)
N = 2


def _mosaic():
    """96 x 144, black 512, white 16383: a smooth field plus patches up to the sensor's saturation."""
    return hm.patches(96, 144, "median/e2e", 15000, low=700, high=9000).astype(np.int64).clip(0, WHITE).astype(np.uint16)


MOSAIC = _mosaic()


@pytest.fixture(scope="module")
def proc():
    from raw2film_amd import HipProcessor

    p = HipProcessor(cameras={}, lenses={}, device=0)
    yield p
    p.close()


def profile(kind, multipliers=MUL, **kw):
    from raw2film_amd.raw import RawProfile, XTransProfile

    if kind == "bayer":
        return RawProfile("GRBG", black=BLACK, multipliers=multipliers, matrix=MATRIX, **kw)
    return XTransProfile(xm.PATTERNS[1], black=BLACK, multipliers=multipliers, matrix=MATRIX, **kw)


@pytest.mark.parametrize("orientation", [0, 6])
@pytest.mark.parametrize("half", [True, False], ids=["reduced", "full"])
@pytest.mark.parametrize("kind", ["bayer", "xtrans"])
def test_median_passes_render_the_models_demosaiced_frame(proc, kind, half, orientation):
    neg, prt, _ = stocks()
    xtrans = kind == "xtrans"
    prof = profile(kind, orientation=orientation, median_passes=N)
    frame = hm.orient(mm.demosaic(MOSAIC, profile(kind), N, half_size=half, xtrans=xtrans), orientation)
    kw = dict(print_film=prt, seed=3, exposure=-0.5, **KW)
    got = proc.process(MOSAIC, neg, 6, 0.4, raw_profile=prof, half_size=half, **kw)
    want = proc.process(frame, neg, 6, 0.4, **kw)
    assert got.shape == want.shape and got.dtype == want.dtype and got.std() > 1
    assert np.array_equal(got, want), int((got != want).sum())
    plain = proc.process(MOSAIC, neg, 6, 0.4, raw_profile=profile(kind, orientation=orientation), half_size=half, **kw)
    assert not np.array_equal(got, plain)  # (step M changed the picture: the equality above does not hold vacuously)
    # median_passes=0 is the call of before
    assert np.array_equal(plain, proc.process(MOSAIC, neg, 6, 0.4, raw_profile=profile(kind, orientation=orientation, median_passes=0),
                                              half_size=half, **kw))
    # one export, and the two-phase API
    a = proc.process_jpeg(MOSAIC, neg, 6, 0.4, quality=90, raw_profile=prof, half_size=half, **kw)
    assert a == proc.process_jpeg(frame, neg, 6, 0.4, quality=90, **kw) and a == proc.encode_jpeg(want, 90)
    pay = proc.extract_image_data_cpu(MOSAIC, raw_profile=prof, half_size=half, exposure=-0.5, frame_width=36, frame_height=24, max_scale=None)
    assert pay["image_array"].shape == (96, 144) and pay["demosaic"]["median"] == N
    rest = dict(print_film=prt, seed=3, **KW)
    assert np.array_equal(proc.process_preloaded(pay, neg, 6, 0.4, final_scaling="cpu", **rest), want)
    assert np.array_equal(proc.submit_preloaded(pay, neg, 6, 0.4, final_scaling="cpu", **rest).result(), want)


@pytest.mark.parametrize("half", [True, False], ids=["half", "full"])
def test_with_raw_denoise_the_median_runs_on_the_denoised_mosaics_frame(proc, half):
    from raw2film_amd.raw import RawProfile, WaveletDenoise

    neg, prt, _ = stocks()
    maximum, T = WHITE - BLACK, 300.0
    shift = denoise_model.shift_of(maximum)
    prof = profile("bayer", orientation=6, median_passes=N)
    behind = RawProfile("GRBG", black=0, multipliers=tuple(m * 2.0 ** -shift for m in prof.multipliers), matrix=MATRIX)
    clean = denoise_model.denoise(MOSAIC, (BLACK,) * 4, maximum, T)
    frame = hm.orient(mm.demosaic(clean, behind, N, half_size=half), 6)
    kw = dict(print_film=prt, seed=3, exposure=0.5, **KW)
    got = proc.process(MOSAIC, neg, 6, 0.4, raw_profile=prof, raw_denoise=WaveletDenoise(T, maximum), half_size=half, **kw)
    assert proc.last_raw_denoise == {"threshold": T, "maximum": maximum, "shift": shift}
    want = proc.process(frame, neg, 6, 0.4, **kw)
    assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())
    undenoised = proc.process(MOSAIC, neg, 6, 0.4, raw_profile=prof, half_size=half, **kw)
    unfiltered = proc.process(MOSAIC, neg, 6, 0.4, raw_profile=profile("bayer", orientation=6), raw_denoise=WaveletDenoise(T, maximum),
                              half_size=half, **kw)
    assert not np.array_equal(got, undenoised) and not np.array_equal(got, unfiltered)


@pytest.mark.parametrize("half", [True, False], ids=["reduced", "full"])
@pytest.mark.parametrize("kind, orientation", [("bayer", 0), ("xtrans", 6)])
def test_with_levels_and_blend_the_median_runs_ahead_of_the_blend(proc, kind, orientation, half):
    from raw2film_amd.raw import RawLevels

    neg, prt, _ = stocks()
    xtrans = kind == "xtrans"
    deferred = profile(kind, RawLevels(WB, WHITE), highlight="blend", orientation=orientation, median_passes=N)
    period = 6 if xtrans else 2
    d = lm.data_maximum(MOSAIC, [BLACK] * period ** 2, period)
    mul, used, adjusted, clip = hm.scale(WB, WHITE, 0.75, deferred.black, d, hm.BLEND)
    assert deferred.resolve(d) == profile(kind, mul, highlight=("blend", clip), orientation=orientation, median_passes=N)
    stats = {}
    hm.demosaic(MOSAIC, profile(kind, mul), clip, half_size=half, xtrans=xtrans, stats=stats)
    assert stats["blended"] >= hm.MIN_BLENDED * stats["pixels"], stats
    frame = hm.orient(mm.demosaic(MOSAIC, profile(kind, mul), N, clip, half_size=half, xtrans=xtrans), orientation)
    kw = dict(print_film=prt, seed=3, exposure=-0.5, **KW)
    got = proc.process(MOSAIC, neg, 6, 0.4, raw_profile=deferred, half_size=half, **kw)
    assert proc.last_raw_scale == {"data_maximum": d, "maximum_used": used, "adjusted": adjusted}
    want = proc.process(frame, neg, 6, 0.4, **kw)
    assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())
    # neither step alone, nor the two the other way round, gives these bytes
    blend_only = hm.demosaic(MOSAIC, profile(kind, mul), clip, half_size=half, xtrans=xtrans)
    median_only = mm.demosaic(MOSAIC, profile(kind, mul), N, None, half_size=half, xtrans=xtrans)
    unoriented = mm.demosaic(MOSAIC, profile(kind, mul), N, clip, half_size=half, xtrans=xtrans)
    assert not np.array_equal(unoriented, blend_only) and not np.array_equal(unoriented, median_only)


# ---- the streamed band loop
# the square 36 x 36 format keeps 2368 x 2368 of a 2400 x 2368 frame: 16.8 M samples, row0 = 16
STREAM_KW = dict(halation=False, sharpness=False, grain=0, exp_kelvin=6000, color_masking=1.0, frame_width=36, frame_height=36, max_scale=None,
                 lens_correction=False, seed=3, exposure=0.5, half_size=False)


def test_a_bayer_mosaic_with_median_passes_streams_to_the_one_piece_bytes(proc):
    from raw2film_amd.raw import RawProfile

    neg, prt, _ = stocks()
    H, W = 2400, 2368
    small = hm.patches(H // 8, W // 8, "median/stream", 15000, low=700, high=9000).astype(np.int64).clip(0, WHITE).astype(np.uint16)
    mosaic = np.tile(small, (8, 8))  # (image-like statistics with saturated patches, made cheaply)
    mul, _, _, clip = hm.scale(WB, WHITE, 0.0, [BLACK] * 4, 0, hm.BLEND)
    prof = RawProfile("RGGB", black=BLACK, multipliers=mul, matrix=MATRIX, highlight=("blend", clip), median_passes=4)
    plans, inner = [], proc._run_bands

    def spy(frame, *a, **k):
        plans.append(list(frame.bounds))
        return inner(frame, *a, **k)

    proc._run_bands = spy
    try:
        assert proc.stream_bands == 16
        proc.stream_rejected = "unset"
        got = proc.process(mosaic, neg, 6, 0.4, cache=False, print_film=prt, raw_profile=prof, **STREAM_KW).copy()
        assert proc.stream_rejected is None and len(plans) == 1 and len(plans[0]) - 1 >= 3, (proc.stream_rejected, plans)
        proc.stream_bands = 0
        want = proc.process(mosaic, neg, 6, 0.4, cache=False, print_film=prt, raw_profile=prof, **STREAM_KW).copy()
        assert len(plans) == 1  # (one piece: no band loop)
        plain = proc.process(mosaic, neg, 6, 0.4, cache=False, print_film=prt,
                             raw_profile=RawProfile("RGGB", black=BLACK, multipliers=mul, matrix=MATRIX, highlight=("blend", clip)), **STREAM_KW)
    finally:
        proc.stream_bands = 16
        proc._run_bands = inner
    assert got.shape == want.shape == (2368, 2368, 3) and got.std() > 1
    assert np.array_equal(got, want), int((got != want).sum())
    assert not np.array_equal(got, plain)  # (the median entry point ran)
