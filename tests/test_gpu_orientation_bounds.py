"""r2f_demosaic_oriented_u16 and r2f_demosaic_xtrans_oriented_u16 write exactly their rows of the oriented frame O: the uint16
(rows, cols, 3) destination in a canary arena (tests/arena.py) -- contiguous behind its guard, and one element off a 4-byte boundary,
which turns the kernels' 32-bit stores into 16-bit ones --, the mosaic in a source arena that holds exactly the mosaic rows the
contract names, contiguous or pitched; rows [y0, y1) of O are written, all of them, and nothing else, the source (guards included) is
untouched, and a refused call (a source window one row short; with bit 4 any window short of [0, H); an orientation outside 0 .. 7)
returns R2F_EINVAL and leaves the arena as it was."""

import ctypes as C

import numpy as np
import pytest

import demosaic_model as dm
import xtrans_model as xm
from arena import Arena

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# (the model, the oriented entry point, the pattern, the reach of the full size, what the reduced size divides by, the mosaic)
BAYER = ("bayer", dm, "r2f_demosaic_oriented_u16", "GRBG", 4, 2, (70, 134))
XTRANS = ("xtrans", xm, "r2f_demosaic_xtrans_oriented_u16", xm.PATTERNS[3], 3, 3, (71, 137))


@pytest.fixture(scope="module")
def ctx():
    from raw2film_amd.context import HipContext

    c = HipContext(0)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def orient(D, o):
    """The NumPy statement of include/r2f.h."""
    E = D
    if o & 2:
        E = E[::-1]
    if o & 1:
        E = E[:, ::-1]
    if o & 4:
        E = E.transpose(1, 0, 2)
    return np.ascontiguousarray(E)


def source_rows(kind, o, y0, y1, out_h, H, half):
    """The mosaic rows the contract of include/r2f.h names for rows [y0, y1) of O."""
    if o & 4:
        return 0, H
    a, b = (out_h - y1, out_h - y0) if o & 2 else (y0, y1)  # the rows of D
    return (kind[5] * a, kind[5] * b) if half else (max(a - kind[4], 0), min(b + kind[4], H))


_MODEL = {}


def model(kind, half):
    key = (kind[0], half)
    if key not in _MODEL:
        mosaic, prof = kind[1].fixture("random", kind[3], *kind[6])
        _MODEL[key] = (mosaic, prof, kind[1].demosaic(mosaic, prof, half_size=half))
    return _MODEL[key]


def bands_of(rows):
    """The whole frame, its first row, a middle band across the seams, its last rows."""
    return [(0, rows), (0, 1), (rows // 3 + 1, 2 * rows // 3 + 2), (rows - 3, rows)]


@pytest.mark.parametrize("o", range(8), ids=lambda o: f"orientation{o}")
@pytest.mark.parametrize("half", [False, True], ids=["full", "reduced"])
@pytest.mark.parametrize("kind", [BAYER, XTRANS], ids=lambda k: k[0])
def test_a_call_writes_its_rows_of_the_oriented_frame_and_nothing_else(ctx, kind, half, o):
    H, W = kind[6]
    mosaic, prof, D = model(kind, half)
    params = prof.plan(H, W, half)
    want = orient(D, o)
    rows, cols = want.shape[:2]
    for n, (y0, y1) in enumerate(bands_of(rows)):
        dst_mis, src_mis, pad = n & 1, (n >> 1) & 1, (0, 3, 0, 4)[n]
        lo, hi = source_rows(kind, o, y0, y1, D.shape[0], H, half)
        src = Arena.holding(dev(mosaic[lo:hi]), misalign=src_mis, pad=pad)  # exactly the rows the contract names
        dst = Arena.hwc(rows, cols, torch.int16, misalign=dst_mis, device="cuda")
        what = f"{kind[2]} orientation {o} rows [{y0}, {y1}) of {rows} x {cols}, mosaic rows [{lo}, {hi})"
        rc = getattr(ctx._lib, kind[2])(ctx._h, src.view.data_ptr(), lo, hi - lo, W + pad, H, W, C.byref(params), o, dst.view.data_ptr(), y0,
                                        y1, ctx._stream())
        assert rc == 0, (what, ctx._lib.r2f_last_error(ctx._h))
        torch.cuda.synchronize()
        dst.check(dst.rows_mask(y0, y1), expected=want.view(np.int16), what=what)
        got = dst.view[y0:y1].cpu().numpy().view(np.uint16)
        assert np.array_equal(got, want[y0:y1]), what
        src.unchanged(what)


@pytest.mark.parametrize("half", [False, True], ids=["full", "reduced"])
@pytest.mark.parametrize("kind", [BAYER, XTRANS], ids=lambda k: k[0])
def test_refused_calls_return_einval_and_leave_the_arena_untouched(ctx, kind, half):
    H, W = kind[6]
    mosaic, prof, D = model(kind, half)
    params = prof.plan(H, W, half)
    src = Arena.holding(dev(mosaic))
    dst = Arena.hwc(max(D.shape[:2]), max(D.shape[:2]), torch.int16, device="cuda")  # (room for O either way round)

    def call(o, gy0, nrows, y0, y1, pitch=W, p=params, s=src.view.data_ptr(), d=dst.view.data_ptr()):
        first = src.view.data_ptr() if s is None else s + 2 * gy0 * W
        return getattr(ctx._lib, kind[2])(ctx._h, None if s is None else first, gy0, nrows, pitch, H, W, C.byref(p), o, d, y0, y1, ctx._stream())

    for o in range(8):
        rows = D.shape[1] if o & 4 else D.shape[0]
        for y0, y1 in ((0, rows), (rows // 3 + 1, 2 * rows // 3 + 2)):
            lo, hi = source_rows(kind, o, y0, y1, D.shape[0], H, half)
            assert call(o, lo, hi - lo - 1, y0, y1) == -1, (o, y0, y1)        # the window ends a row early
            assert b"read mosaic rows" in ctx._lib.r2f_last_error(ctx._h)
            if lo + 1 < hi:
                assert call(o, lo + 1, hi - lo - 1, y0, y1) == -1, (o, y0, y1)    # ... begins a row late
            if o & 4:  # any window short of [0, H), whichever rows of O are asked for
                assert (lo, hi) == (0, H)
                assert call(o, 0, H - 1, 0, 1) == -1 and call(o, 1, H - 1, rows - 1, rows) == -1 and call(o, H // 2, H - H // 2, 0, 1) == -1
        assert call(o, 0, H, -1, 4) == -1 and call(o, 0, H, 3, 2) == -1 and call(o, 0, H, 0, rows + 1) == -1
        assert call(o, 0, H, 0, 4, pitch=W - 1) == -1                          # what the upright entry point refuses
        assert call(o, 0, H, 0, 4, p=prof.plan(H + 6, W, half)) == -1
        assert call(o, 0, H, 0, 4, s=None) == -1 and call(o, 0, H, 0, 4, d=None) == -1
    for o in (-1, 8, 16, -8):
        assert call(o, 0, H, 0, 4) == -1, o
        assert b"orientation" in ctx._lib.r2f_last_error(ctx._h)
    torch.cuda.synchronize()
    dst.check(None, what=f"refused {kind[2]}")
    src.unchanged(f"refused {kind[2]}")
    assert call(5, 0, H, 0, 0) == 0 and call(3, 0, 0, 2, 2) == 0  # (no rows: nothing to do, nothing read)
    torch.cuda.synchronize()
    dst.check(None, what=f"{kind[2]} with no rows")
