"""r2f_demosaic_f32, the demosaic fused with the uint16 hand-off's decode, against the NumPy model of the demosaic
(tests/demosaic_model.py) followed by the NumPy expression of r2f_decode_u16: np.minimum(u.astype(f32) / f32(divisor) * f32(factor),
f32(65504)).  Equality is on the bits, without a tolerance -- every pattern, shapes below, at and around the tile, windows with odd
origins and 1 x 1 windows on the border ring's boundaries, factors that leave the clamp alone and that reach it, every cut of a
window's rows into two calls (in either order, from source windows that hold exactly the rows read, pitched and misaligned), and the
refusals, which leave the destination as it was."""

import ctypes as C

import numpy as np
import pytest

import demosaic_model as dm
from raw2film_amd.raw import RawProfile

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TH, TW = dm.TILE_H, dm.TILE_W
f32 = np.float32
# below the tile; at the tile and one around it; a second tile column with a narrow remainder; two tile rows
SHAPES = [(2, 2), (3, 5), (7, 7), (TH - 1, TW - 1), (TH - 1, TW + 1), (TH, TW), (TH + 1, TW - 1), (TH + 1, TW + 1), (TH, 2 * TW + 1),
          (TH + 1, 2 * TW + 5), (2 * TH + 6, 2 * TW + 2)]
assert (70, 130) in SHAPES and (33, 133) in SHAPES and (32, 129) in SHAPES
HALF_SHAPES = [s for s in SHAPES if s[0] % 2 == 0 and s[1] % 2 == 0]
FACTORS = [f32(1.0), f32(2 ** 0.37), f32(3e-3), f32(7e4)]
KINDS = dm.KINDS + ("clamps",)
CANARY_BITS = 0x7FC5CA1E  # a quiet NaN with a payload no kernel computes (tests/arena.py)


@pytest.fixture(scope="module")
def ctx():
    from raw2film_amd.context import HipContext

    c = HipContext(0)
    yield c
    c.close()


_MODEL = {}


def model(kind, pattern, shape, half=False):
    """(mosaic, profile, the model's uint16 frame), computed once per case and shared by the tests.  "clamps": full-range random
    samples under a matrix with negative off-diagonal entries, so that step C clamps at 0 and at 65535."""
    key = (kind, pattern, shape, half)
    if key not in _MODEL:
        if kind == "clamps":
            rng = np.random.default_rng(1000 * shape[0] + shape[1])
            mosaic = rng.integers(0, 65536, shape, dtype=np.uint16)
            prof = RawProfile(pattern, black=0, multipliers=(1.0, 1.0, 1.0), matrix=((1.8, -0.6, -0.2), (-0.5, 1.9, -0.4), (-0.1, -0.7, 1.8)))
        else:
            mosaic, prof = dm.fixture(kind, pattern, *shape)
        stats = {}
        _MODEL[key] = (mosaic, prof, dm.demosaic(mosaic, prof, half_size=half, stats=stats), stats)
    return _MODEL[key][:3]


def decode(u, factor, divisor=65535.0):
    return np.minimum(u.astype(f32) / f32(divisor) * f32(factor), f32(65504))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def canary(shape):
    return torch.full(shape, CANARY_BITS, dtype=torch.int32, device="cuda").view(torch.float32)


def bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)).view(np.uint32)


def same(got, want):
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def windows(h, w):
    """Windows of an h x w demosaiced frame: the whole, one pixel in, an odd origin past the first tile column, one that ends at
    the last row and column, and 1 x 1 windows on the boundaries of the border ring."""
    out = [None]
    if h > 2 and w > 2:
        out.append((1, 1, h - 2, w - 2))
    if w >= 2 * TW + 1 and h > 3:
        out.append((3, TW + 1, h - 3, w - TW - 1))
        out.append((2, TW - 1, h - 3, 3))  # across the tile seam, ending mid-tile
    out.append((h // 2, w // 3, h - h // 2, w - w // 3))
    for y, x in ((0, 0), (2, 2), (3, 3), (h - 1, w - 1)):
        if y < h and x < w:
            out.append((y, x, 1, 1))
    return out


def check_frame(ctx, kind, pattern, shape, half):
    mosaic, prof, want_u16 = model(kind, pattern, shape, half)
    params = prof.plan(*shape, half)
    m = dev(mosaic)
    h, w = want_u16.shape[:2]
    top = f32(0)
    for factor in FACTORS:
        want = decode(want_u16, factor)
        top = max(top, want.max())
        got = ctx.demosaic_f32(m, params, factor)
        assert same(got, want), (kind, pattern, shape, half, float(factor), int((bits(got) != bits(want)).sum()))
    factor = FACTORS[1]
    want = decode(want_u16, factor)
    for win in windows(h, w)[1:]:
        r0, c0, nr, nc = win
        got = ctx.demosaic_f32(m, params, factor, window=win)
        assert same(got, want[r0:r0 + nr, c0:c0 + nc]), (kind, pattern, shape, half, win)
    return want_u16, top


@pytest.mark.parametrize("pattern", dm.PATTERNS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_full_size_is_bit_identical_to_the_model_and_the_decode(ctx, shape, pattern):
    for kind in KINDS:
        want_u16, top = check_frame(ctx, kind, pattern, shape, False)
        if kind == "clamps" and shape[0] * shape[1] >= (TH - 1) * (TW - 1):
            stats = _MODEL[(kind, pattern, shape, False)][3]
            assert stats["c_clip_0"] > 0 and stats["c_clip_65535"] > 0  # step C clamps at both ends ...
            assert want_u16.min() == 0 and want_u16.max() == 65535
            assert top == f32(65504)                                     # ... and 7e4 takes 65535 to the float clamp


@pytest.mark.parametrize("pattern", dm.PATTERNS)
@pytest.mark.parametrize("shape", HALF_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_half_size_is_bit_identical_to_the_model_and_the_decode(ctx, shape, pattern):
    for kind in KINDS:
        want_u16, top = check_frame(ctx, kind, pattern, shape, True)
        assert want_u16.shape == (shape[0] // 2, shape[1] // 2, 3)
        if kind == "clamps" and shape[0] >= TH:
            assert want_u16.min() == 0 and want_u16.max() == 65535 and top == f32(65504)


def test_other_divisors_and_the_one_piece_path_of_the_context(ctx):
    """decode_u16(demosaic_u16(whole)[window]) -- the two kernels the fused one replaces -- gives the same bits."""
    mosaic, prof, want_u16 = model("random", "GRBG", (TH + 1, 2 * TW + 5))
    m = dev(mosaic)
    win = (3, TW + 1, 20, 50)
    for divisor, factor in ((65535.0, FACTORS[1]), (16383.0, f32(0.77)), (1.0, f32(1.0))):
        got = ctx.demosaic_f32(m, prof, factor, divisor=divisor, window=win)
        assert same(got, decode(want_u16, factor, divisor)[3:23, TW + 1:TW + 51])
        two = ctx.decode_u16(ctx.demosaic_u16(m, prof)[3:23, TW + 1:TW + 51].contiguous(), factor, divisor=divisor)
        assert same(got, two)


def raw_call(ctx, src, gy0, nrows, pitch, H, W, params, window, factor, out, y0, y1, divisor=65535.0):
    return ctx._lib.r2f_demosaic_f32(ctx._h, src.data_ptr(), gy0, nrows, pitch, H, W, C.byref(params), *window, float(f32(divisor)),
                                     float(factor), out.data_ptr(), y0, y1, ctx._stream())


@pytest.mark.parametrize("half", [False, True], ids=["full", "half"])
@pytest.mark.parametrize("mode", ["plain", "reversed", "minimal-pitched", "offset"])
def test_every_cut_of_the_rows_gives_the_whole(ctx, mode, half):
    """A 41 x 70 demosaiced frame, a window with an odd origin, its rows split at every y into two calls into a canary buffer."""
    H, W = (82, 140) if half else (41, 70)
    mosaic, prof, want_u16 = model("random", "BGGR", (H, W), half)
    params = prof.plan(H, W, half)
    factor = FACTORS[1]
    win = (1, 3, 38, 65)
    r0, c0, nr, nc = win
    want = decode(want_u16, factor)[r0:r0 + nr, c0:c0 + nc]
    m = dev(mosaic)
    whole = ctx.demosaic_f32(m, params, factor, window=win)
    assert same(whole, want)
    if mode == "offset":  # one sample past a 4-byte boundary: the 16-bit load path
        flat = torch.zeros(H * W + 2, dtype=torch.int16, device="cuda")
        m = torch.as_strided(flat, (H, W), (W, 1), 1)
        m.copy_(dev(mosaic))
        assert m.data_ptr() % 4 == 2
    keep = []
    for cut in range(nr + 1):
        out = canary((nr, nc, 3))
        parts = [(0, cut), (cut, nr)]
        for y0, y1 in (reversed(parts) if mode == "reversed" else parts):
            if mode != "minimal-pitched":
                assert ctx.demosaic_f32(m, params, factor, window=win, out=out, rows=(y0, y1)) is out
                continue
            if y0 == y1:  # (no rows: no source rows to hold)
                continue
            # exactly the rows the contract names, in an allocation of their own with a pitch of W + 1
            lo, hi = (2 * (r0 + y0), 2 * (r0 + y1)) if half else (max(r0 + y0 - 4, 0), min(r0 + y1 + 4, H))
            flat = torch.zeros((hi - lo) * (W + 1), dtype=torch.int16, device="cuda")
            src = torch.as_strided(flat, (hi - lo, W), (W + 1, 1), 0)
            src.copy_(dev(mosaic[lo:hi]))
            keep.append(flat)
            assert raw_call(ctx, src, lo, hi - lo, W + 1, H, W, params, win, factor, out, y0, y1) == 0, ctx._lib.r2f_last_error(ctx._h)
        assert same(out, want), (mode, half, cut, int((bits(out) != bits(want)).sum()))
    torch.cuda.synchronize()


@pytest.mark.parametrize("half", [False, True], ids=["full", "half"])
def test_refusals_leave_the_destination_untouched(ctx, half):
    H, W = 66, 130
    mosaic, prof, _ = model("random", "RGGB", (H, W), half)
    params = prof.plan(H, W, half)
    h, w = params.out_h, params.out_w
    m = dev(mosaic)
    factor = FACTORS[1]
    win = (2, 3, 20, 40)
    out = canary((20, 40, 3))
    whole_out = canary((h, w, 3))

    def raw(window=win, y0=0, y1=20, gy0=0, nrows=H, pitch=W, p=params, divisor=65535.0, src=m, dst=out):
        return raw_call(ctx, src, gy0, nrows, pitch, H, W, p, window, factor, dst, y0, y1, divisor)

    # a window outside the demosaiced frame, or an empty one
    for window in ((0, 0, h + 1, w), (0, 0, h, w + 1), (1, 0, h, w), (0, 1, h, w), (-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0)):
        assert raw(window=window, dst=whole_out, y0=0, y1=1) == -1, window
        with pytest.raises(ValueError):
            ctx.demosaic_f32(m, params, factor, window=window)
    # rows outside the window
    for y0, y1 in ((-1, 4), (3, 2), (0, 21), (21, 21)):
        assert raw(y0=y0, y1=y1) == -1, (y0, y1)
        with pytest.raises(Exception):
            ctx.demosaic_f32(m, params, factor, window=win, out=out, rows=(y0, y1))
    # a source window one row short at either end
    y0, y1 = 4, 12
    lo, hi = (2 * (2 + y0), 2 * (2 + y1)) if half else (2 + y0 - 4, 2 + y1 + 4)
    for gy0, nrows in ((lo, hi - lo - 1), (lo + 1, hi - lo - 1), (lo + 1, hi - lo)):
        assert raw(y0=y0, y1=y1, gy0=gy0, nrows=nrows, src=m[lo:hi]) == -1
    assert raw(pitch=W - 1) == -1
    # the params of another frame size, no Bayer pattern, a divisor that is not positive, null pointers
    assert raw(p=prof.plan(H + 2, W, half)) == -1
    bad = prof.plan(H, W, half)
    bad.cfa[1] = bad.cfa[0]
    assert raw(p=bad) == -1
    for divisor in (0.0, -1.0, float("nan")):
        assert raw(divisor=divisor) == -1
        with pytest.raises(Exception):
            ctx.demosaic_f32(m, params, factor, divisor=divisor, window=win, out=out)
    assert ctx._lib.r2f_demosaic_f32(ctx._h, None, 0, H, W, H, W, C.byref(params), *win, 65535.0, 1.0, out.data_ptr(), 0, 20, ctx._stream()) == -1
    assert ctx._lib.r2f_demosaic_f32(ctx._h, m.data_ptr(), 0, H, W, H, W, C.byref(params), *win, 65535.0, 1.0, None, 0, 20, ctx._stream()) == -1
    with pytest.raises(ValueError):
        ctx.demosaic_f32(m.cpu(), params, factor)
    with pytest.raises(ValueError):
        ctx.demosaic_f32(m, params, factor, window=win, out=out[:19])
    torch.cuda.synchronize()
    for t in (out, whole_out):
        assert bool((t.view(torch.int32) == CANARY_BITS).all())
    # ... and the call they all refused goes through: its rows, nothing else
    assert raw(y0=y0, y1=y1, gy0=lo, nrows=hi - lo, src=m[lo:hi]) == 0 and raw(y0=y0, y1=y0) == 0
    torch.cuda.synchronize()
    written = (out.view(torch.int32) != CANARY_BITS).all(dim=2).all(dim=1).cpu().numpy()
    untouched = (out.view(torch.int32) == CANARY_BITS).all(dim=2).all(dim=1).cpu().numpy()
    assert written[y0:y1].all() and untouched[:y0].all() and untouched[y1:].all()
