"""The X-Trans demosaic on the device: r2f_demosaic_xtrans_u16 against the NumPy model of its definition (tests/xtrans_model.py), byte
for byte and without a tolerance -- a frame that is all border, one with a single interior pixel, sides that are no multiple of 6,
aprons across a tile edge, and three tiles each way with the four layouts that put every phase at a tile origin; pitched and
misaligned sources (the 16-bit load path); row bands cut at rows that are no multiple of 6 or 3 from row windows that hold exactly
what the contract names; and a mosaic through HipProcessor against the same call on the model's frame."""

import ctypes as C

import numpy as np
import pytest

import xtrans_model as xm
from helpers import stocks

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TH, TW = xm.TILE_H, xm.TILE_W
SHAPES = [(6, 6), (7, 7), (9, 11), (TH + 7, TW + 7)]
BIG = (3 * TH + 5, 3 * TW + 5)
# admissible arrays that are not Fujifilm's (tests/test_xtrans_host.py): other gaps, weight sums 1 .. 7
OTHER_PATTERNS = [("GBGGRG", "RGRBGB", "GBGGRG", "GRGGBB", "GGBRGR", "GRGRBG"), ("GBBGRG", "RGRBGB", "GBGGRG", "BRGGBG", "BGBRGR", "GRGGBB")]
CANARY = 0xA5A5


@pytest.fixture(scope="module")
def proc():
    from raw2film_amd import HipProcessor

    p = HipProcessor(cameras={}, lenses={}, device=0)
    yield p
    p.close()


_MODEL = {}


def model(kind, pattern, shape, half=False):
    """(mosaic, profile, the model's frame), computed once per case and shared by the tests."""
    key = (kind, pattern, shape, half)
    if key not in _MODEL:
        mosaic, prof = xm.fixture(kind, pattern, *shape)
        _MODEL[key] = (mosaic, prof, xm.demosaic(mosaic, prof, half_size=half))
    return _MODEL[key]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint16)


def call(ctx, src, gy0, nrows, pitch, H, W, params, out, y0, y1):
    return ctx._lib.r2f_demosaic_xtrans_u16(ctx._h, src.data_ptr(), gy0, nrows, pitch, H, W, C.byref(params), out.data_ptr(), y0, y1,
                                            ctx._stream())


def _compare(proc, kind, pattern, shape, half):
    mosaic, prof, want = model(kind, pattern, shape, half)
    got = host(proc.ctx.demosaic_xtrans(dev(mosaic), prof.plan(*shape, half)))
    assert got.shape == want.shape == ((shape[0] // 3, shape[1] // 3, 3) if half else shape + (3,))
    assert np.array_equal(got, want), (kind, pattern[0], shape, half, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("half", [False, True], ids=["full", "third"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_frames_are_byte_identical_to_the_model(proc, shape, half):
    for pattern in (xm.PATTERNS[0], xm.PATTERNS[3]):
        for kind in xm.KINDS:
            _compare(proc, kind, pattern, shape, half)


@pytest.mark.parametrize("half", [False, True], ids=["full", "third"])
@pytest.mark.parametrize("pattern", xm.PATTERNS, ids=lambda p: p[0])
def test_three_tiles_each_way_are_byte_identical_to_the_model(proc, pattern, half):
    for kind in xm.KINDS:
        _compare(proc, kind, pattern, BIG, half)


@pytest.mark.parametrize("pattern", OTHER_PATTERNS, ids=lambda p: p[3])
def test_an_admissible_pattern_that_is_not_fujifilms(proc, pattern):
    from raw2film_amd.raw import XTransProfile

    prof = XTransProfile(pattern, black=64, multipliers=(1.9, 1.0, 1.4), matrix=xm.CAMERA)
    rng = np.random.default_rng(11)
    shape = (TH + 7, TW + 7)
    for mosaic in (rng.integers(0, 65536, shape, dtype=np.uint16), (rng.integers(0, 2, shape) * 65535).astype(np.uint16)):
        for half in (False, True):
            got = host(proc.ctx.demosaic_xtrans(dev(mosaic), prof.plan(*shape, half)))
            assert np.array_equal(got, xm.demosaic(mosaic, prof, half_size=half)), (pattern, half)


@pytest.mark.parametrize("half", [False, True], ids=["full", "third"])
def test_pitch_and_alignment_select_the_load_path_not_the_bytes(proc, half):
    shape = (TH + 7, TW + 7)
    H, W = shape
    mosaic, prof, want = model("random", xm.PATTERNS[2], shape, half)
    params = prof.plan(H, W, half)
    m = dev(mosaic)
    # (extra samples per row, samples the first one lies past a 4-byte boundary): an odd pitch and an odd origin each defeat the
    # 32-bit loads; an even pitch from an aligned origin keeps them
    for extra, off in ((5, 0), (0, 1), (6, 0), (6, 1), (5, 1)):
        flat = torch.full((H * (W + extra) + 2,), 0x1234, dtype=torch.int16, device="cuda")
        view = torch.as_strided(flat, (H, W), (W + extra, 1), off)
        view.copy_(m)
        assert view.data_ptr() % 4 == 2 * off and flat.data_ptr() % 4 == 0
        got = host(proc.ctx.demosaic_xtrans(view, params))
        assert np.array_equal(got, want), (extra, off, int((got != want).sum()))


@pytest.mark.parametrize("half", [False, True], ids=["full", "third"])
@pytest.mark.parametrize("pattern", [xm.PATTERNS[1], xm.PATTERNS[3]], ids=lambda p: p[0])
def test_bands_from_exact_row_windows_concatenate_to_the_whole_frame(proc, pattern, half):
    ctx = proc.ctx
    shape = BIG if half else (2 * TH - 1, TW + 7)
    H, W = shape
    mosaic, prof, want = model("random", pattern, shape, half)
    params = prof.plan(H, W, half)
    Ho = params.out_h
    cuts = [0, 1, 4, 5, 11, Ho // 2 + 1, Ho - 2, Ho]  # (no multiples of 6 or 3 among the inner ones)
    assert all(c % 3 for c in cuts[1:-1]) and cuts == sorted(set(cuts))
    out = torch.full((Ho, params.out_w, 3), CANARY - 65536, dtype=torch.int16, device="cuda")
    bands = list(zip(cuts[:-1], cuts[1:]))
    windows = []
    for k in np.random.default_rng(5).permutation(len(bands)):  # (in any order)
        y0, y1 = bands[k]
        lo, hi = xm.source_rows(y0, y1, H, half)
        win = dev(mosaic[lo:hi])  # exactly the rows the contract names, in an allocation of their own
        windows.append(win)
        assert call(ctx, win, lo, hi - lo, W, H, W, params, out, y0, y1) == 0, ctx._lib.r2f_last_error(ctx._h)
    torch.cuda.synchronize()
    assert np.array_equal(host(out), want)


@pytest.mark.parametrize("half", [False, True], ids=["full", "third"])
def test_a_window_one_row_short_is_refused_and_nothing_is_written(proc, half):
    ctx = proc.ctx
    H, W = BIG
    mosaic, prof, _ = model("random", xm.PATTERNS[0], (H, W), half)
    params = prof.plan(H, W, half)
    out = torch.full((params.out_h, params.out_w, 3), CANARY - 65536, dtype=torch.int16, device="cuda")
    y0, y1 = 8, 20
    lo, hi = xm.source_rows(y0, y1, H, half)
    win = dev(mosaic[lo:hi])
    for gy0, nrows in ((lo, hi - lo - 1), (lo + 1, hi - lo - 1), (lo + 1, hi - lo)):  # short at the end, at the start, shifted
        assert call(ctx, win, gy0, nrows, W, H, W, params, out, y0, y1) == -1
    assert b"read mosaic rows" in ctx._lib.r2f_last_error(ctx._h)
    assert call(ctx, win, lo, hi - lo, W - 1, H, W, params, out, y0, y1) == -1  # a pitch below W
    assert call(ctx, win, lo, hi - lo, W, H, W, params, out, y0, params.out_h + 1) == -1
    assert call(ctx, win, lo, hi - lo, W, H, W, params, out, -1, y1) == -1 and call(ctx, win, lo, hi - lo, W, H, W, params, out, y1, y0) == -1
    assert call(ctx, win, lo, hi - lo, W, H, W, prof.plan(H + 3, W, half), out, y0, y1) == -1  # the params of another frame size
    assert call(ctx, win, lo, hi - lo, W, H, W, prof.plan(H, W, not half), out, y0, y1) == -1  # ... of the other form
    assert call(ctx, win, lo, hi - lo, W, 5, W, params, out, y0, y1) == -1  # a frame below 6 rows
    for field, ph in (("gap", 1), ("taps", 0), ("wsum", 0), ("recip", 0), ("cell_count", 0), ("cfa", 7)):  # tables that are not the planner's
        bad = prof.plan(H, W, half)
        if field == "cfa":
            bad.cfa[ph] = 3
        else:
            getattr(bad, field)[ph][1] += 1
        assert call(ctx, win, lo, hi - lo, W, H, W, bad, out, y0, y1) == -1, field
        assert b"tables" in ctx._lib.r2f_last_error(ctx._h)
    torch.cuda.synchronize()
    assert bool((out == CANARY - 65536).all())
    assert call(ctx, win, lo, hi - lo, W, H, W, params, out, y0, y1) == 0
    assert call(ctx, win, lo, hi - lo, W, H, W, params, out, y0, y0) == 0  # (no rows: nothing to do, nothing read)
    torch.cuda.synchronize()
    written = (out != CANARY - 65536).any(dim=2).any(dim=1).cpu().numpy()
    assert not written[:y0].any() and not written[y1:].any() and written[y0:y1].all()


def test_context_method_arguments(proc):
    shape = (TH + 7, TW + 7)
    mosaic, prof, want = model("random", xm.PATTERNS[0], shape)
    m = dev(mosaic)
    out = torch.zeros(shape + (3,), dtype=torch.int16, device="cuda")
    assert proc.ctx.demosaic_xtrans(m, prof, out=out, rows=(5, 9)) is out  # (a profile: planned full size for this mosaic)
    got = host(out)
    assert np.array_equal(got[5:9], want[5:9]) and not got[:5].any() and not got[9:].any()
    with pytest.raises(ValueError):
        proc.ctx.demosaic_xtrans(m.cpu(), prof)
    with pytest.raises(ValueError):
        proc.ctx.demosaic_xtrans(m[:, ::2], prof)
    with pytest.raises(ValueError):
        proc.ctx.demosaic_xtrans(m[:5], prof)
    with pytest.raises(ValueError):
        proc.ctx.demosaic_xtrans(m, prof, out=out[:32])


# ---------------------------------------------------------------------------------------------- through the processor
KW = dict(halation=False, sharpness=False, grain=0, exp_kelvin=6000, color_masking=1.0, frame_width=36, frame_height=24, max_scale=None)


def _e2e_mosaic(pattern):
    """A 96 x 144 mosaic with image-like statistics (a smooth ramp plus noise, well inside 14 bits) and a camera-like profile."""
    from raw2film_amd.raw import XTransProfile

    rng = np.random.default_rng(17)
    y, x = np.mgrid[0:96, 0:144]
    base = 600 + 9000 * (0.5 + 0.5 * np.sin(x / 23.0) * np.cos(y / 17.0)) + rng.normal(0, 120, (96, 144))
    mosaic = np.clip(base, 0, 16383).astype(np.uint16)
    prof = XTransProfile(pattern, black=512, multipliers=(7.9, 4.1, 6.2), matrix=((0.52, 0.27, 0.15), (0.25, 0.68, 0.07), (0.03, 0.12, 0.81)))
    return mosaic, prof


@pytest.mark.parametrize("half", [True, False], ids=["third", "full"])
def test_a_mosaic_through_the_processor_equals_the_models_frame_through_it(proc, half):
    neg, prt, _ = stocks()
    mosaic, prof = _e2e_mosaic(xm.PATTERNS[1] if half else xm.PATTERNS[0])
    rgb = xm.demosaic(mosaic, prof, half_size=half)
    assert rgb.shape == ((32, 48, 3) if half else (96, 144, 3)) and 1000 < rgb.mean() < 60000
    kw = dict(print_film=prt, half_size=half, seed=3, **KW)

    def both(mosaic_kw, rgb_kw, **extra):
        a = proc.process(mosaic, neg, 6, 0.4, raw_profile=prof, **mosaic_kw, **extra, **kw)
        b = proc.process(rgb, neg, 6, 0.4, **rgb_kw, **extra, **kw)
        assert a.shape == b.shape and a.dtype == b.dtype
        assert np.array_equal(a, b), (mosaic_kw, extra, int((a != b).sum()))
        return a

    plain = both(dict(exposure=0.5), dict(exposure=0.5))
    assert plain.std() > 1  # (a picture, not a flat field)
    both(dict(exposure=None), dict(exposure="device"))  # no RGB frame on the host: measured on the device
    assert proc.exposure_rejected is None
    both(dict(exposure=0.5), dict(exposure=0.5), zoom=1.3, rotate_times=1)
    # one export: the same file bytes, and stream=True yields the one-piece bytes with the named rejection
    a = proc.process_jpeg(mosaic, neg, 6, 0.4, quality=90, raw_profile=prof, exposure=0.5, **kw)
    b = proc.process_jpeg(rgb, neg, 6, 0.4, quality=90, exposure=0.5, **kw)
    assert a == b and a == proc.encode_jpeg(plain, 90)
    c = proc.process_jpeg(mosaic, neg, 6, 0.4, quality=90, stream=True, raw_profile=prof, exposure=0.5, **kw)
    assert c == a and "demosaic" in proc.stream_rejected and "X-Trans mosaics do not stream yet" in proc.stream_rejected
    # the two-phase API
    pay = proc.extract_image_data_cpu(mosaic, raw_profile=prof, half_size=half, exposure=0.5, frame_width=36, frame_height=24, max_scale=None)
    assert pay["image_array"].shape == (96, 144)
    assert np.array_equal(proc.process_preloaded(pay, neg, 6, 0.4, final_scaling="cpu", **kw), plain)
