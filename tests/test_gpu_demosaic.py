"""The Bayer demosaic on the device: r2f_demosaic_u16 against the NumPy model of its definition (tests/demosaic_model.py), byte for
byte and without a tolerance -- every pattern, the smallest frames with no interior, with one interior pixel, with a tile seam
through the apron and with an odd tail; pitched and misaligned sources (the 16-bit load path); row bands from row windows that hold
exactly what the contract names; and a mosaic through HipProcessor against the same call on the model's frame."""

import ctypes as C

import numpy as np
import pytest

import demosaic_model as dm
from helpers import stocks

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TH, TW = dm.TILE_H, dm.TILE_W
FULL_SHAPES = [(2, 2), (3, 3), (6, 7), (7, 7), (8, 8), (TH + 1, TW + 1), (2 * TH - 1, 2 * TW + 3), (33, 130)]
HALF_SHAPES = [(2, 2), (4, 6), (66, 130)]
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
        mosaic, prof = dm.fixture(kind, pattern, *shape)
        _MODEL[key] = (mosaic, prof, dm.demosaic(mosaic, prof, half_size=half))
    return _MODEL[key]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint16)


def call(ctx, src, gy0, nrows, pitch, H, W, params, out, y0, y1):
    return ctx._lib.r2f_demosaic_u16(ctx._h, src.data_ptr(), gy0, nrows, pitch, H, W, C.byref(params), out.data_ptr(), y0, y1, ctx._stream())


@pytest.mark.parametrize("pattern", dm.PATTERNS)
@pytest.mark.parametrize("shape", FULL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_full_size_is_byte_identical_to_the_model(proc, shape, pattern):
    for kind in dm.KINDS:
        mosaic, prof, want = model(kind, pattern, shape)
        got = host(proc.ctx.demosaic_u16(dev(mosaic), prof))
        assert got.shape == want.shape
        assert np.array_equal(got, want), (kind, pattern, shape, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("pattern", dm.PATTERNS)
@pytest.mark.parametrize("shape", HALF_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_half_size_is_byte_identical_to_the_model(proc, shape, pattern):
    for kind in dm.KINDS:
        mosaic, prof, want = model(kind, pattern, shape, True)
        got = host(proc.ctx.demosaic_u16(dev(mosaic), prof.plan(*shape, True)))
        assert got.shape == want.shape == (shape[0] // 2, shape[1] // 2, 3)
        assert np.array_equal(got, want), (kind, pattern, shape, int((got != want).sum()))


@pytest.mark.parametrize("half", [False, True], ids=["full", "half"])
@pytest.mark.parametrize("pattern", ["RGGB", "GBRG"])
def test_pitch_and_alignment_select_the_load_path_not_the_bytes(proc, pattern, half):
    shape = (66, 130) if half else (2 * TH - 1, 2 * TW + 3)
    H, W = shape
    mosaic, prof, want = model("random", pattern, shape, half)
    params = prof.plan(H, W, half)
    m = dev(mosaic)
    # (extra samples per row, samples the first one lies past a 4-byte boundary): an odd pitch and an odd origin each defeat the
    # 32-bit loads; an even pitch from an aligned origin keeps them
    for extra, off in ((5, 0), (0, 1), (6, 0), (6, 1), (5, 1)):
        flat = torch.full((H * (W + extra) + 2,), 0x1234, dtype=torch.int16, device="cuda")
        view = torch.as_strided(flat, (H, W), (W + extra, 1), off)
        view.copy_(m)
        assert view.data_ptr() % 4 == 2 * off and flat.data_ptr() % 4 == 0
        got = host(proc.ctx.demosaic_u16(view, params))
        assert np.array_equal(got, want), (extra, off, int((got != want).sum()))


@pytest.mark.parametrize("half", [False, True], ids=["full", "half"])
@pytest.mark.parametrize("pattern", ["BGGR", "GRBG"])
def test_bands_from_exact_row_windows_concatenate_to_the_whole_frame(proc, pattern, half):
    ctx = proc.ctx
    shape = (2 * (2 * TH - 1), 2 * TW + 4) if half else (2 * TH - 1, 2 * TW + 3)
    H, W = shape
    mosaic, prof, want = model("random", pattern, shape, half)
    params = prof.plan(H, W, half)
    Ho = params.out_h
    cuts = [0, 1, 3, 4, 5, TH - 1, Ho - 2, Ho]
    whole = host(ctx.demosaic_u16(dev(mosaic), params))
    assert np.array_equal(whole, want)
    out = torch.full((Ho, params.out_w, 3), CANARY - 65536, dtype=torch.int16, device="cuda")
    bands = list(zip(cuts[:-1], cuts[1:]))
    windows = []
    for k in np.random.default_rng(5).permutation(len(bands)):  # (in any order)
        y0, y1 = bands[k]
        lo, hi = (2 * y0, 2 * y1) if half else (max(y0 - 4, 0), min(y1 + 4, H))
        win = dev(mosaic[lo:hi])  # exactly the rows the contract names, in an allocation of their own
        windows.append(win)
        assert call(ctx, win, lo, hi - lo, W, H, W, params, out, y0, y1) == 0, ctx._lib.r2f_last_error(ctx._h)
    torch.cuda.synchronize()
    assert np.array_equal(host(out), want)


@pytest.mark.parametrize("half", [False, True], ids=["full", "half"])
def test_a_window_one_row_short_is_refused_and_nothing_is_written(proc, half):
    ctx = proc.ctx
    H, W = 66, 130
    mosaic, prof, _ = model("random", "RGGB", (H, W), half)
    params = prof.plan(H, W, half)
    out = torch.full((params.out_h, params.out_w, 3), CANARY - 65536, dtype=torch.int16, device="cuda")
    y0, y1 = 8, 20
    lo, hi = (2 * y0, 2 * y1) if half else (y0 - 4, y1 + 4)
    win = dev(mosaic[lo:hi])
    for gy0, nrows in ((lo, hi - lo - 1), (lo + 1, hi - lo - 1), (lo + 1, hi - lo)):  # short at the end, at the start, shifted
        assert call(ctx, win, gy0, nrows, W, H, W, params, out, y0, y1) == -1
    assert call(ctx, win, lo, hi - lo, W - 1, H, W, params, out, y0, y1) == -1  # a pitch below W
    assert call(ctx, win, lo, hi - lo, W, H, W, params, out, y0, params.out_h + 1) == -1
    other = prof.plan(H + 2, W, half)
    assert call(ctx, win, lo, hi - lo, W, H, W, other, out, y0, y1) == -1  # the params of another frame size
    torch.cuda.synchronize()
    assert bool((out == CANARY - 65536).all())
    assert call(ctx, win, lo, hi - lo, W, H, W, params, out, y0, y1) == 0
    assert call(ctx, win, lo, hi - lo, W, H, W, params, out, y0, y0) == 0  # (no rows: nothing to do, nothing read)
    torch.cuda.synchronize()
    written = (out != CANARY - 65536).any(dim=2).any(dim=1).cpu().numpy()
    assert not written[:y0].any() and not written[y1:].any() and written[y0:y1].all()


def test_context_method_arguments(proc):
    mosaic, prof, want = model("random", "RGGB", (33, 130))
    m = dev(mosaic)
    out = torch.zeros((33, 130, 3), dtype=torch.int16, device="cuda")
    assert proc.ctx.demosaic_u16(m, prof, out=out, rows=(5, 9)) is out
    got = host(out)
    assert np.array_equal(got[5:9], want[5:9]) and not got[:5].any() and not got[9:].any()
    with pytest.raises(ValueError):
        proc.ctx.demosaic_u16(m.cpu(), prof)
    with pytest.raises(ValueError):
        proc.ctx.demosaic_u16(m[:, ::2], prof)
    with pytest.raises(ValueError):
        proc.ctx.demosaic_u16(m, prof, out=out[:32])
    bad = prof.plan(33, 130)
    bad.cfa[0] = 7
    with pytest.raises(Exception, match="colour id"):
        proc.ctx.demosaic_u16(m, bad)


# ---------------------------------------------------------------------------------------------- through the processor
KW = dict(halation=False, sharpness=False, grain=0, exp_kelvin=6000, color_masking=1.0, frame_width=36, frame_height=24, max_scale=None)


def _e2e_mosaic(pattern):
    """A 96 x 144 mosaic with image-like statistics (a smooth ramp plus noise, well inside 14 bits) and a camera-like profile."""
    from raw2film_amd.raw import RawProfile

    rng = np.random.default_rng(17)
    y, x = np.mgrid[0:96, 0:144]
    base = 600 + 9000 * (0.5 + 0.5 * np.sin(x / 23.0) * np.cos(y / 17.0)) + rng.normal(0, 120, (96, 144))
    mosaic = np.clip(base, 0, 16383).astype(np.uint16)
    prof = RawProfile(pattern, black=512, multipliers=(7.9, 4.1, 6.2), matrix=((0.52, 0.27, 0.15), (0.25, 0.68, 0.07), (0.03, 0.12, 0.81)))
    return mosaic, prof


@pytest.mark.parametrize("half", [True, False], ids=["half", "full"])
def test_a_mosaic_through_the_processor_equals_the_models_frame_through_it(proc, half, tmp_path):
    from raw2film_amd.lens import LensProfile

    neg, prt, _ = stocks()
    mosaic, prof = _e2e_mosaic("GRBG" if half else "RGGB")
    rgb = dm.demosaic(mosaic, prof, half_size=half)
    assert rgb.shape == ((48, 72, 3) if half else (96, 144, 3)) and 1000 < rgb.mean() < 60000
    kw = dict(print_film=prt, half_size=half, seed=3, **KW)

    def both(mosaic_kw, rgb_kw, **extra):
        a = proc.process(mosaic, neg, 6, 0.4, raw_profile=prof, **mosaic_kw, **extra, **kw)
        b = proc.process(rgb, neg, 6, 0.4, **rgb_kw, **extra, **kw)
        assert a.shape == b.shape and a.dtype == b.dtype
        assert np.array_equal(a, b), (mosaic_kw, extra, int((a != b).sum()))
        return a

    plain = both(dict(exposure=0.5), dict(exposure=0.5))
    assert plain.std() > 1  # (a picture, not a flat field)
    both(dict(exposure="device"), dict(exposure="device"))
    stops = proc.last_auto_exposure
    both(dict(exposure=None), dict(exposure="device"))
    assert proc.exposure_rejected is None and proc.last_auto_exposure == stops
    both(dict(exposure=0.5), dict(exposure=0.5), lens_profile=LensProfile("ptlens", (0.02, -0.06, 0.01), scale=1.02))
    both(dict(exposure=None), dict(exposure="device"), lens_profile=LensProfile("poly3", (0.03,), scale=1.05), zoom=1.2)
    both(dict(exposure=0.5), dict(exposure=0.5), zoom=1.3, rotate_times=1)
    both(dict(exposure=0.5), dict(exposure=0.5), rotation=3.5)
    assert both(dict(exposure=0.5), dict(exposure=0.5), output_bits=16).dtype == np.uint16
    # the exports: the same file bytes
    a = proc.process_jpeg(mosaic, neg, 6, 0.4, quality=90, raw_profile=prof, exposure=0.5, **kw)
    b = proc.process_jpeg(rgb, neg, 6, 0.4, quality=90, exposure=0.5, **kw)
    assert a == b and a == proc.encode_jpeg(plain, 90)
    c = proc.process_jpeg(mosaic, neg, 6, 0.4, quality=90, stream=True, raw_profile=prof, exposure=0.5, **kw)
    assert c == a and "demosaic" in proc.stream_rejected
    # the two-phase API
    pay = proc.extract_image_data_cpu(mosaic, raw_profile=prof, half_size=half, exposure=0.5, frame_width=36, frame_height=24, max_scale=None)
    assert pay["image_array"].shape == (96, 144)
    assert np.array_equal(proc.process_preloaded(pay, neg, 6, 0.4, final_scaling="cpu", **kw), plain)
    assert np.array_equal(proc.submit_preloaded(pay, neg, 6, 0.4, final_scaling="cpu", **kw).result(), plain)
    # a mosaic without a profile, and a turned one without stops
    with pytest.raises(ValueError):
        proc.process(mosaic, neg, 6, 0.4, **kw)
    with pytest.raises(ValueError, match="turned or rotated"):
        proc.process(mosaic, neg, 6, 0.4, raw_profile=prof, rotate_times=1, **kw)
