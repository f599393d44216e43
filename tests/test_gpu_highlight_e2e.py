"""highlight="blend" through HipProcessor, end to end: process(mosaic, raw_profile=a profile with RawLevels and highlight="blend")
renders what process() of the model's demosaiced frame renders (tests/highlight_model.py: Scale with mode 2 from the model's data
maximum, the demosaic, Blend, step C), for both arrays, both sizes, upright and turned; and a numeric ("blend", clip) Bayer profile
just above the 16.7 M-sample gate streams in row bands (r2f_demosaic_blend_f32) to the bytes of the one-piece call."""

import numpy as np
import pytest

import highlight_model as hm
import levels_model as lm
import xtrans_model as xm
from helpers import stocks

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KW = dict(halation=False, sharpness=False, grain=0, exp_kelvin=6000, color_masking=1.0, frame_width=36, frame_height=24, max_scale=None)
MATRIX = ((0.52, 0.27, 0.15), (0.25, 0.68, 0.07), (0.03, 0.12, 0.81))
WB, BLACK, WHITE = (1.9, 1.0, 1.5), 512, 16383


def _mosaic():
    """96 x 144, black 512, white 16383: a smooth field plus patches up to the sensor's saturation."""
    return hm.patches(96, 144, "e2e", 15000, low=700, high=9000).astype(np.int64).clip(0, WHITE).astype(np.uint16)


MOSAIC = _mosaic()


@pytest.fixture(scope="module")
def proc():
    from raw2film_amd import HipProcessor

    p = HipProcessor(cameras={}, lenses={}, device=0)
    yield p
    p.close()


def profile(kind, orientation=0):
    from raw2film_amd.raw import RawLevels, RawProfile, XTransProfile

    lv = RawLevels(WB, WHITE)
    if kind == "bayer":
        return RawProfile("GRBG", black=BLACK, multipliers=lv, matrix=MATRIX, orientation=orientation, highlight="blend")
    return XTransProfile(xm.PATTERNS[1], black=BLACK, multipliers=lv, matrix=MATRIX, orientation=orientation, highlight="blend")


@pytest.mark.parametrize("orientation", [0, 5])
@pytest.mark.parametrize("half", [True, False], ids=["reduced", "full"])
@pytest.mark.parametrize("kind", ["bayer", "xtrans"])
def test_blend_renders_the_models_demosaiced_frame(proc, kind, half, orientation):
    neg, prt, _ = stocks()
    deferred = profile(kind, orientation)
    period = 6 if kind == "xtrans" else 2
    d = lm.data_maximum(MOSAIC, [BLACK] * period ** 2, period)
    mul, used, adjusted, clip = hm.scale(WB, WHITE, 0.75, deferred.black, d, hm.BLEND)
    numeric = type(deferred)(deferred.pattern, black=BLACK, multipliers=mul, matrix=MATRIX)
    stats = {}
    frame = hm.orient(hm.demosaic(MOSAIC, numeric, clip, half_size=half, xtrans=kind == "xtrans", stats=stats), orientation)
    assert stats["blended"] >= hm.MIN_BLENDED * stats["pixels"], stats
    kw = dict(print_film=prt, seed=3, exposure=-0.5, **KW)
    got = proc.process(MOSAIC, neg, 6, 0.4, raw_profile=deferred, half_size=half, **kw)
    assert proc.last_raw_scale == {"data_maximum": d, "maximum_used": used, "adjusted": adjusted}
    assert deferred.resolve(d).blend_clip == clip  # (the clip level is the resolved profile's to tell)
    want = proc.process(frame, neg, 6, 0.4, **kw)
    assert got.shape == want.shape and got.dtype == want.dtype and got.std() > 1
    assert np.array_equal(got, want), int((got != want).sum())
    plain = proc.process(hm.orient(hm.demosaic(MOSAIC, numeric, None, half_size=half, xtrans=kind == "xtrans"), orientation), neg, 6, 0.4, **kw)
    assert not np.array_equal(got, plain)  # (Blend changed the picture: the equality above does not hold vacuously)


# ---- the streamed band loop
# the square 36 x 36 format keeps 2368 x 2368 of a 2400 x 2368 frame: 16.8 M samples, row0 = 16
STREAM_KW = dict(halation=False, sharpness=False, grain=0, exp_kelvin=6000, color_masking=1.0, frame_width=36, frame_height=36, max_scale=None,
                 lens_correction=False, seed=3, exposure=0.5, half_size=False)


def test_a_numeric_blend_profile_streams_to_the_one_piece_bytes(proc):
    from raw2film_amd.raw import RawProfile

    neg, prt, _ = stocks()
    H, W = 2400, 2368
    small = hm.patches(H // 8, W // 8, "stream", 15000, low=700, high=9000).astype(np.int64).clip(0, WHITE).astype(np.uint16)
    mosaic = np.tile(small, (8, 8))  # (image-like statistics with saturated patches, made cheaply)
    mul, _, _, clip = hm.scale(WB, WHITE, 0.0, [BLACK] * 4, 0, hm.BLEND)
    prof = RawProfile("RGGB", black=BLACK, multipliers=mul, matrix=MATRIX, highlight=("blend", clip))
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
    finally:
        proc.stream_bands = 16
        proc._run_bands = inner
    assert got.shape == want.shape == (2368, 2368, 3) and got.std() > 1
    assert np.array_equal(got, want), int((got != want).sum())
    proc.stream_bands = 0
    try:
        plain = proc.process(mosaic, neg, 6, 0.4, cache=False, print_film=prt,
                             raw_profile=RawProfile("RGGB", black=BLACK, multipliers=mul, matrix=MATRIX), **STREAM_KW)
    finally:
        proc.stream_bands = 16
    assert not np.array_equal(got, plain)  # (the blend entry point ran)
