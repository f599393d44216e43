"""r2f_demosaic_f32 writes exactly its rows and bytes: the float32 (rows, cols, 3) destination in a canary arena (tests/arena.py) --
contiguous behind its guard, and one to three floats off a 16-byte boundary, which moves the head of every row segment's 16-byte
stores --, the mosaic in a source arena, contiguous or pitched; rows [y0, y1) of the window are written, all of them, and nothing
else, the source (guards included) is untouched, and a refused call leaves the arena as it was."""

import ctypes as C

import numpy as np
import pytest

import demosaic_model as dm
from arena import Arena

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TH, TW = dm.TILE_H, dm.TILE_W
FACTOR = np.float32(2 ** 0.37)


@pytest.fixture(scope="module")
def ctx():
    from raw2film_amd.context import HipContext

    c = HipContext(0)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def decode(u, factor):
    return np.minimum(u.astype(np.float32) / np.float32(65535.0) * np.float32(factor), np.float32(65504))


# (mosaic shape, half size, window of the demosaiced frame or None, window rows [y0, y1) or None, destination misalignment in floats,
#  source misalignment in samples, source row pad)
GEOMETRIES = [
    ((2, 2), False, None, None, 0, 0, 0),
    ((7, 7), False, None, None, 1, 1, 0),
    ((TH + 1, TW + 1), False, None, None, 0, 0, 0),                       # a second tile row and column of one pixel each
    ((TH + 1, TW + 1), False, None, None, 3, 0, 3),
    ((2 * TH - 1, 2 * TW + 3), False, None, (5, TH + 2), 2, 0, 0),        # a band across the tile seam
    ((2 * TH - 1, 2 * TW + 3), False, None, (TH - 1, TH), 1, 1, 4),       # one row
    ((33, 130), False, None, (30, 33), 0, 1, 1),                          # the last rows
    ((2 * TH - 1, 2 * TW + 3), False, (3, TW + 1, TH + 5, TW - 1), None, 0, 0, 0),   # a window with an odd origin in the second tile column
    ((2 * TH - 1, 2 * TW + 3), False, (3, TW + 1, TH + 5, TW - 1), (4, TH + 3), 1, 1, 1),
    ((2 * TH - 1, 2 * TW + 3), False, (1, 5, TH + 9, TW + 22), None, 3, 0, 0),       # a window that ends mid-tile in x and in y
    ((2 * TH - 1, 2 * TW + 3), False, (1, 5, TH + 9, TW + 22), (TH - 3, TH + 9), 2, 0, 2),
    ((2 * TH - 1, 2 * TW + 3), False, (TH, TW - 1, 1, 2), None, 1, 0, 0),            # two pixels across the seam
    ((2, 2), True, None, None, 0, 0, 0),
    ((4, 6), True, None, None, 1, 0, 1),
    ((66, 130), True, None, None, 0, 0, 0),
    ((66, 130), True, None, (7, 30), 3, 1, 2),
    ((66, 130), True, (2, 1, 29, 63), None, 2, 0, 0),                     # a window; its 63 columns end inside the first block of lanes
    ((66, 260), True, (5, 3, 20, 70), (3, 17), 1, 1, 0),                  # ... and one that ends inside the second
]


def _id(g):
    return f"{g[0][0]}x{g[0][1]}-{'half' if g[1] else 'full'}-win{g[2]}-rows{g[3]}-mis{g[4]}{g[5]}-pad{g[6]}".replace(" ", "")


@pytest.mark.parametrize("geo", GEOMETRIES, ids=_id)
def test_demosaic_f32_writes_its_rows_and_nothing_else(ctx, geo):
    (H, W), half, window, rows, dst_mis, src_mis, pad = geo
    mosaic, prof = dm.fixture("random", "GBRG", H, W)
    params = prof.plan(H, W, half)
    r0, c0, nr, nc = window or (0, 0, params.out_h, params.out_w)
    want = decode(dm.demosaic(mosaic, prof, half_size=half), FACTOR)[r0:r0 + nr, c0:c0 + nc]
    y0, y1 = rows or (0, nr)
    src = Arena.holding(dev(mosaic), misalign=src_mis, pad=pad)
    dst = Arena.hwc(nr, nc, torch.float32, misalign=dst_mis, device="cuda")
    assert dst.view.data_ptr() % 16 == 4 * dst_mis
    what = f"r2f_demosaic_f32 {geo}"
    rc = ctx._lib.r2f_demosaic_f32(ctx._h, src.view.data_ptr(), 0, H, W + pad, H, W, C.byref(params), r0, c0, nr, nc, 65535.0, float(FACTOR),
                                   dst.view.data_ptr(), y0, y1, ctx._stream())
    assert rc == 0, (what, ctx._lib.r2f_last_error(ctx._h))
    torch.cuda.synchronize()
    dst.check(dst.rows_mask(y0, y1), expected=want, what=what)
    got = dst.view[y0:y1].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want[y0:y1]).view(np.uint32)), what
    src.unchanged(what)


@pytest.mark.parametrize("half", [False, True], ids=["full", "half"])
def test_refused_calls_leave_the_arena_untouched(ctx, half):
    H, W = 66, 130
    mosaic, prof = dm.fixture("random", "RGGB", H, W)
    params = prof.plan(H, W, half)
    win = (2, 3, 20, 40)
    src = Arena.holding(dev(mosaic))
    dst = Arena.hwc(20, 40, torch.float32, device="cuda")

    def call(gy0, nrows, pitch, p, y0, y1, window=win, divisor=65535.0, s=src.view.data_ptr(), d=dst.view.data_ptr()):
        return ctx._lib.r2f_demosaic_f32(ctx._h, s, gy0, nrows, pitch, H, W, C.byref(p), *window, divisor, float(FACTOR), d, y0, y1,
                                         ctx._stream())

    lo, hi = (4, 44) if half else (0, 26)  # what rows [0, 20) of the window read
    assert call(lo, hi - lo, W, params, 0, 20, s=src.view[lo:].data_ptr()) == 0
    torch.cuda.synchronize()
    dst.buf.view(torch.int32).fill_(dst.canary)
    assert call(lo, hi - lo - 1, W, params, 0, 20, s=src.view[lo:].data_ptr()) == -1   # the source window ends a row early
    assert call(lo + 1, hi - lo - 1, W, params, 0, 20, s=src.view[lo + 1:].data_ptr()) == -1  # ... begins a row late
    assert call(0, H, W - 1, params, 0, 20) == -1                                      # a pitch below W
    assert call(0, H, W, params, -1, 4) == -1 and call(0, H, W, params, 3, 2) == -1 and call(0, H, W, params, 0, 21) == -1
    assert call(0, H, W, params, 0, 4, window=(params.out_h - 19, 3, 20, 40)) == -1    # a window past the last row
    assert call(0, H, W, params, 0, 4, window=(2, params.out_w - 39, 20, 40)) == -1    # ... past the last column
    assert call(0, H, W, params, 0, 0, window=(2, 3, 0, 40)) == -1                     # an empty one
    assert call(0, H, W, prof.plan(H + 2, W, half), 0, 4) == -1                        # the params of another frame size
    bad = prof.plan(H, W, half)
    bad.cfa[1] = bad.cfa[0]                                                            # not a Bayer pattern
    assert call(0, H, W, bad, 0, 4) == -1
    assert call(0, H, W, params, 0, 4, divisor=0.0) == -1 and call(0, H, W, params, 0, 4, divisor=-65535.0) == -1
    assert call(0, H, W, params, 0, 4, s=None) == -1 and call(0, H, W, params, 0, 4, d=None) == -1
    assert call(0, H, W, params, 0, 4, d=dst.view.data_ptr() + 2) == -1                # a destination no float can start at
    torch.cuda.synchronize()
    dst.check(None, what="refused r2f_demosaic_f32")
    src.unchanged("refused r2f_demosaic_f32")
