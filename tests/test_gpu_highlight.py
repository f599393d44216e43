"""Blend (LibRaw's highlight mode 2) in the device demosaics, bit for bit against the NumPy model (tests/highlight_model.py) through
each of the three entry points: r2f_demosaic_blend_u16 and r2f_demosaic_xtrans_blend_u16 at full and reduced size, every pattern,
orientations 0, 3, 5 and 6, one ragged tile and 2 x 3 ragged tiles; r2f_demosaic_blend_f32 in windows with an odd origin and row
cuts off the tile grid.  The mosaics are a smooth field plus compact saturated patches (highlight_model.patches); their conditions
-- at least 10 % of the pixels blended, every class of pixel present -- are asserted on the model's output here and were checked on
the CPU where the fixtures were chosen (tests/test_highlight_host.py).  clip = 65535 gives the plain entry point's bytes; through the
processor, highlight="clip" is the render of before, "unclip" that of the max-normalised numeric profile and "blend" that of the
resolved ("blend", clip) one."""

import ctypes as C

import numpy as np
import pytest

import demosaic_model as dm
import highlight_model as hm
import levels_model as lm
import xtrans_model as xm
from helpers import stocks

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ORIENTATIONS = (0, 3, 5, 6)


@pytest.fixture(scope="module")
def ctx():
    from raw2film_amd.context import HipContext

    c = HipContext(0)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint16)


def check_conditions(stats, kind, what):
    assert stats["blended"] >= hm.MIN_BLENDED * stats["pixels"], (what, stats)
    if kind == "equal":
        assert all(stats[k] > 0 for k in hm.CLASSES), (what, stats)


@pytest.mark.parametrize("half", [False, True], ids=["full", "half"])
@pytest.mark.parametrize("kind", ["equal", "wb"])
@pytest.mark.parametrize("pattern", dm.PATTERNS)
def test_bayer_blend_equals_the_model(ctx, pattern, kind, half):
    for shape in (hm.ONE_TILE, hm.BAYER_FRAME):
        mosaic, prof, clip = hm.bayer_case(kind, pattern, shape)
        stats = {}
        want = hm.demosaic(mosaic, prof, clip, half_size=half, stats=stats)
        check_conditions(stats, kind, (pattern, shape, half))
        plain = dm.demosaic(mosaic, prof, half_size=half)
        assert np.count_nonzero((want != plain).any(axis=-1)) >= 0.05 * stats["pixels"]  # (Blend is not a no-op here)
        params, m = prof.plan(*shape, half), dev(mosaic)
        for o in ORIENTATIONS:
            got = host(ctx.demosaic_blend_u16(m, params, clip, orientation=o))
            ref = hm.orient(want, o)
            assert got.shape == ref.shape and np.array_equal(got, ref), (pattern, kind, shape, half, o, int((got != ref).sum()))
        # a row cut off the tile grid composes to the whole frame
        out = torch.zeros(want.shape, dtype=torch.int16, device="cuda")
        for y0, y1 in ((0, 5), (5, 5), (5, want.shape[0] - 3), (want.shape[0] - 3, want.shape[0])):
            ctx.demosaic_blend_u16(m, params, clip, out=out, rows=(y0, y1))
        assert np.array_equal(host(out), want)
        assert np.array_equal(host(ctx.demosaic_blend_u16(m, params, 65535)), host(ctx.demosaic_u16(m, params)))
        assert np.array_equal(host(ctx.demosaic_blend_u16(m, params, 65535, orientation=5)), host(ctx.demosaic_u16(m, params, orientation=5)))


@pytest.mark.parametrize("half", [False, True], ids=["full", "third"])
@pytest.mark.parametrize("kind", ["equal", "wb"])
@pytest.mark.parametrize("pattern", xm.PATTERNS[:2], ids=["canonical", "shifted"])
def test_xtrans_blend_equals_the_model(ctx, pattern, kind, half):
    for shape in (hm.ONE_TILE, hm.XTRANS_FRAME):
        mosaic, prof, clip = hm.xtrans_case(kind, pattern, shape)
        stats = {}
        want = hm.demosaic(mosaic, prof, clip, half_size=half, xtrans=True, stats=stats)
        check_conditions(stats, kind, (shape, half))
        plain = xm.demosaic(mosaic, prof, half_size=half)
        assert np.count_nonzero((want != plain).any(axis=-1)) >= 0.05 * stats["pixels"]
        params, m = prof.plan(*shape, half), dev(mosaic)
        for o in ORIENTATIONS:
            got = host(ctx.demosaic_xtrans_blend(m, params, clip, orientation=o))
            ref = hm.orient(want, o)
            assert got.shape == ref.shape and np.array_equal(got, ref), (kind, shape, half, o, int((got != ref).sum()))
        out = torch.zeros(want.shape, dtype=torch.int16, device="cuda")
        for y0, y1 in ((0, 5), (5, want.shape[0] - 3), (want.shape[0] - 3, want.shape[0])):
            ctx.demosaic_xtrans_blend(m, params, clip, out=out, rows=(y0, y1))
        assert np.array_equal(host(out), want)
        assert np.array_equal(host(ctx.demosaic_xtrans_blend(m, params, 65535)), host(ctx.demosaic_xtrans(m, params)))
        assert np.array_equal(host(ctx.demosaic_xtrans_blend(m, params, 65535, orientation=6)), host(ctx.demosaic_xtrans(m, params, orientation=6)))


def decode(u16, factor, divisor=65535.0):
    """r2f_decode_u16's expression: two correctly rounded fp32 operations and the clamp."""
    return np.minimum(u16.astype(np.float32) / np.float32(divisor) * np.float32(factor), np.float32(65504.0))


@pytest.mark.parametrize("half", [False, True], ids=["full", "half"])
@pytest.mark.parametrize("pattern", dm.PATTERNS)
def test_the_float_epilogue_equals_the_models_decoded_window(ctx, pattern, half):
    factor = float(np.float32(2.0 ** 0.5))
    for kind, shape in (("equal", hm.BAYER_FRAME), ("wb", hm.ONE_TILE)):
        mosaic, prof, clip = hm.bayer_case(kind, pattern, shape)
        frame = hm.demosaic(mosaic, prof, clip, half_size=half)
        params, m = prof.plan(*shape, half), dev(mosaic)
        oh, ow = frame.shape[:2]
        for window in ((0, 0, oh, ow), (3, 5, oh - 7, ow - 9), (1, 1, oh - 1, ow - 2)):  # odd col0: lanes are masked, tiles stay
            r0, c0, nr, nc = window
            want = decode(frame[r0:r0 + nr, c0:c0 + nc], factor)
            out = torch.full((nr, nc, 3), -1.0, dtype=torch.float32, device="cuda")
            for y0, y1 in ((0, nr // 3), (nr // 3, nr - nr // 4), (nr - nr // 4, nr)):  # cuts that are no multiples of the tile's 32 rows
                ctx.demosaic_blend_f32(m, params, clip, factor, window=window, out=out, rows=(y0, y1))
            got = out.cpu().numpy()
            assert np.array_equal(got, want), (pattern, kind, half, window, int((got != want).sum()))
        plain = ctx.demosaic_f32(m, params, factor, window=(3, 5, oh - 7, ow - 9)).cpu().numpy()
        same = ctx.demosaic_blend_f32(m, params, 65535, factor, window=(3, 5, oh - 7, ow - 9)).cpu().numpy()
        assert np.array_equal(same, plain)


def test_a_clip_outside_its_range_is_refused_before_any_launch(ctx):
    mosaic, prof, _ = hm.bayer_case("equal", "RGGB", hm.ONE_TILE)
    xmosaic, xprof, _ = hm.xtrans_case("equal", xm.PATTERNS[0], hm.ONE_TILE)
    H, W = hm.ONE_TILE
    p, xp, m, xmo = prof.plan(H, W), xprof.plan(H, W), dev(mosaic), dev(xmosaic)
    out = torch.full((H, W, 3), 7, dtype=torch.int16, device="cuda")
    fout = torch.full((H, W, 3), 7.0, dtype=torch.float32, device="cuda")
    lib, h, s = ctx._lib, ctx._h, ctx._stream()
    for clip in (0, -1, 65536, 2 ** 31 - 1):
        assert lib.r2f_demosaic_blend_u16(h, m.data_ptr(), 0, H, W, H, W, C.byref(p), 0, clip, out.data_ptr(), 0, H, s) == -1
        assert b"clip" in lib.r2f_last_error(h)
        assert lib.r2f_demosaic_xtrans_blend_u16(h, xmo.data_ptr(), 0, H, W, H, W, C.byref(xp), 0, clip, out.data_ptr(), 0, H, s) == -1
        assert lib.r2f_demosaic_blend_f32(h, m.data_ptr(), 0, H, W, H, W, C.byref(p), clip, 0, 0, H, W, 65535.0, 1.0, fout.data_ptr(), 0, H, s) == -1
    assert lib.r2f_demosaic_blend_u16(h, m.data_ptr(), 0, H, W, H, W, C.byref(p), 8, 100, out.data_ptr(), 0, H, s) == -1  # the orientation's
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((fout == 7.0).all())
    for bad in (0, 65536, 1.5, True, None):
        with pytest.raises(ValueError, match="clip"):
            ctx.demosaic_blend_u16(m, p, bad)


# ---- through the processor
KW = dict(halation=False, sharpness=False, grain=0, exp_kelvin=6000, color_masking=1.0, frame_width=36, frame_height=24, max_scale=None)
MATRIX = ((0.52, 0.27, 0.15), (0.25, 0.68, 0.07), (0.03, 0.12, 0.81))
WB, BLACK, WHITE = (1.9, 1.0, 1.5), 512, 16383


@pytest.fixture(scope="module")
def proc():
    from raw2film_amd import HipProcessor

    p = HipProcessor(cameras={}, lenses={}, device=0)
    yield p
    p.close()


def profile(kind, highlight, multipliers=None, orientation=0):
    from raw2film_amd.raw import RawLevels, RawProfile, XTransProfile

    mul = RawLevels(WB, WHITE) if multipliers is None else multipliers
    if kind == "bayer":
        return RawProfile("GRBG", black=BLACK, multipliers=mul, matrix=MATRIX, orientation=orientation, highlight=highlight)
    return XTransProfile(xm.PATTERNS[1], black=BLACK, multipliers=mul, matrix=MATRIX, orientation=orientation, highlight=highlight)


def sensor_mosaic():
    """96 x 144, black 512, white 16383: a smooth field plus patches at the sensor's saturation."""
    return (hm.patches(96, 144, "sensor", 15000, low=700, high=9000).astype(np.int64).clip(0, WHITE)).astype(np.uint16)


@pytest.mark.parametrize("half", [True, False], ids=["reduced", "full"])
@pytest.mark.parametrize("kind, orientation", [("bayer", 0), ("bayer", 5), ("xtrans", 0), ("xtrans", 6)])
def test_the_three_modes_through_the_processor(proc, kind, orientation, half):
    neg, prt, _ = stocks()
    mosaic = sensor_mosaic()
    period = 6 if kind == "xtrans" else 2
    d = lm.data_maximum(mosaic, [BLACK] * period ** 2, period)
    kw = dict(print_film=prt, half_size=half, seed=3, exposure=-0.5, **KW)
    black = [BLACK] * period ** 2
    renders = {}
    for name, mode in (("clip", 0), ("unclip", 1), ("blend", 2)):
        mul, used, adjusted, clip = hm.scale(WB, WHITE, 0.75, black, d, mode)
        got = proc.process(mosaic, neg, 6, 0.4, raw_profile=profile(kind, name, orientation=orientation), **kw)
        assert proc.last_raw_scale == {"data_maximum": d, "maximum_used": used, "adjusted": adjusted}
        numeric = profile(kind, ("blend", clip) if mode == 2 else "clip", mul, orientation)
        assert profile(kind, name, orientation=orientation).resolve(d) == numeric
        want = proc.process(mosaic, neg, 6, 0.4, raw_profile=numeric, **kw)
        assert got.shape == want.shape and got.std() > 1 and np.array_equal(got, want), (name, int((got != want).sum()))
        renders[name] = got
    # "clip" is the render of before this field: the profile without it, and the numbers of levels_model
    today = type(profile(kind, "clip"))(profile(kind, "clip").pattern, black=BLACK, multipliers=lm.scale(WB, WHITE, 0.75, black, d)[0],
                                        matrix=MATRIX, orientation=orientation)
    assert np.array_equal(renders["clip"], proc.process(mosaic, neg, 6, 0.4, raw_profile=today, **kw))
    assert not np.array_equal(renders["clip"], renders["unclip"]) and not np.array_equal(renders["unclip"], renders["blend"])
