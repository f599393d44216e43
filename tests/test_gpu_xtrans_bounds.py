"""r2f_demosaic_xtrans_u16 writes exactly its rows and bytes: the uint16 (rows, W, 3) destination in a canary arena (tests/arena.py)
-- contiguous behind its guard, and one element off a 4-byte boundary, which turns the kernel's 32-bit row stores into 16-bit ones --,
the mosaic in a source arena, contiguous or pitched; for a whole frame and a middle band, full size and reduced, rows [y0, y1) are
written, all of them, and nothing else, the source (guards included) is untouched, and a refused call leaves the arena as it was."""

import ctypes as C

import numpy as np
import pytest

import xtrans_model as xm
from arena import Arena

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TH, TW = xm.TILE_H, xm.TILE_W


@pytest.fixture(scope="module")
def ctx():
    from raw2film_amd.context import HipContext

    c = HipContext(0)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


# (mosaic shape, reduced size, output rows [y0, y1), destination misalignment in elements, source misalignment, source row pad)
GEOMETRIES = [
    ((6, 6), False, None, 0, 0, 0),
    ((7, 7), False, None, 1, 1, 0),
    ((TH + 7, TW + 7), False, None, 0, 0, 0),               # a second tile row and column of seven pixels, an odd row length
    ((TH + 7, TW + 7), False, None, 1, 0, 3),
    ((2 * TH + 5, 2 * TW + 5), False, (5, TH + 2), 0, 0, 0),  # a middle band across the tile seam
    ((2 * TH + 5, 2 * TW + 5), False, (TH - 1, TH), 1, 1, 4),  # one row
    ((TH + 7, TW + 7), False, (TH + 4, TH + 7), 0, 1, 1),   # the last rows
    ((6, 6), True, None, 0, 0, 0),
    ((8, 10), True, None, 1, 0, 1),                          # tails that fill no cell
    ((3 * TH + 5, 3 * TW + 5), True, None, 0, 0, 0),
    ((3 * TH + 5, 3 * TW + 5), True, (7, 30), 1, 1, 2),      # a middle band
]


@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: f"{g[0][0]}x{g[0][1]}-{'third' if g[1] else 'full'}-rows{g[2]}-mis{g[3]}{g[4]}-pad{g[5]}")
def test_demosaic_writes_its_rows_and_nothing_else(ctx, geo):
    (H, W), half, rows, dst_mis, src_mis, pad = geo
    mosaic, prof = xm.fixture("random", xm.PATTERNS[3], H, W)
    params = prof.plan(H, W, half)
    want = xm.demosaic(mosaic, prof, half_size=half)
    y0, y1 = rows or (0, params.out_h)
    src = Arena.holding(dev(mosaic), misalign=src_mis, pad=pad)
    dst = Arena.hwc(params.out_h, params.out_w, torch.int16, misalign=dst_mis, device="cuda")
    what = f"r2f_demosaic_xtrans_u16 {geo}"
    rc = ctx._lib.r2f_demosaic_xtrans_u16(ctx._h, src.view.data_ptr(), 0, H, W + pad, H, W, C.byref(params), dst.view.data_ptr(), y0, y1,
                                          ctx._stream())
    assert rc == 0, (what, ctx._lib.r2f_last_error(ctx._h))
    torch.cuda.synchronize()
    dst.check(dst.rows_mask(y0, y1), expected=want.view(np.int16), what=what)
    got = dst.view[y0:y1].cpu().numpy().view(np.uint16)
    assert np.array_equal(got, want[y0:y1]), what
    src.unchanged(what)


@pytest.mark.parametrize("half", [False, True], ids=["full", "third"])
def test_refused_calls_leave_the_arena_untouched(ctx, half):
    H, W = TH + 7, TW + 7
    mosaic, prof = xm.fixture("random", xm.PATTERNS[0], H, W)
    params = prof.plan(H, W, half)
    src = Arena.holding(dev(mosaic))
    dst = Arena.hwc(params.out_h, params.out_w, torch.int16, device="cuda")

    def call(gy0, nrows, pitch, p, y0, y1, s=src.view.data_ptr(), d=dst.view.data_ptr()):
        return ctx._lib.r2f_demosaic_xtrans_u16(ctx._h, s, gy0, nrows, pitch, H, W, C.byref(p), d, y0, y1, ctx._stream())

    last = 3 * params.out_h if half else H  # the mosaic rows the whole output reads end here
    assert call(0, last - 1, W, params, 0, params.out_h) == -1    # the window ends a row early
    assert call(1, H - 1, W, params, 0, params.out_h) == -1       # ... begins a row late
    assert call(0, H, W - 1, params, 0, params.out_h) == -1       # a pitch below W
    assert call(0, H, W, params, -1, 4) == -1 and call(0, H, W, params, 3, 2) == -1 and call(0, H, W, params, 0, params.out_h + 1) == -1
    assert call(0, H, W, prof.plan(H + 3, W, half), 0, 4) == -1   # the params of another frame size
    bad = prof.plan(H, W, half)
    bad.gap[1][0] = 3                                             # a table that would index outside the staged tile
    assert call(0, H, W, bad, 0, 4) == -1
    bad = prof.plan(H, W, half)
    bad.cfa[0], bad.cfa[1] = bad.cfa[1], bad.cfa[0]               # another pattern under the same tables
    assert call(0, H, W, bad, 0, 4) == -1
    assert call(0, H, W, params, 0, 4, s=None) == -1 and call(0, H, W, params, 0, 4, d=None) == -1
    torch.cuda.synchronize()
    dst.check(None, what="refused r2f_demosaic_xtrans_u16")
    src.unchanged("refused r2f_demosaic_xtrans_u16")
