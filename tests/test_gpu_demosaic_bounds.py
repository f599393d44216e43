"""r2f_demosaic_u16 writes exactly its rows and bytes: the uint16 (rows, W, 3) destination in a canary arena (tests/arena.py) --
contiguous behind its guard, and one element off a 4-byte boundary, which turns the kernel's 32-bit row stores into 16-bit ones --,
the mosaic in a source arena, contiguous or pitched; rows [y0, y1) are written, all of them, and nothing else, the source (guards
included) is untouched, and a refused call leaves the arena as it was."""

import ctypes as C

import numpy as np
import pytest

import demosaic_model as dm
from arena import Arena

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TH, TW = dm.TILE_H, dm.TILE_W


@pytest.fixture(scope="module")
def ctx():
    from raw2film_amd.context import HipContext

    c = HipContext(0)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


# (mosaic shape, half size, output rows [y0, y1), destination misalignment in elements, source misalignment, source row pad)
GEOMETRIES = [
    ((2, 2), False, None, 0, 0, 0),
    ((7, 7), False, None, 1, 1, 0),
    ((TH + 1, TW + 1), False, None, 0, 0, 0),              # a second tile row and column of one pixel each, an odd row length
    ((TH + 1, TW + 1), False, None, 1, 0, 3),
    ((2 * TH - 1, 2 * TW + 3), False, (5, TH + 2), 0, 0, 0),  # a band across the tile seam
    ((2 * TH - 1, 2 * TW + 3), False, (TH - 1, TH), 1, 1, 4),  # one row
    ((33, 130), False, (30, 33), 0, 1, 1),                 # the last rows
    ((2, 2), True, None, 0, 0, 0),
    ((4, 6), True, None, 1, 0, 1),
    ((66, 130), True, None, 0, 0, 0),
    ((66, 130), True, (7, 30), 1, 1, 2),
]


@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: f"{g[0][0]}x{g[0][1]}-{'half' if g[1] else 'full'}-rows{g[2]}-mis{g[3]}{g[4]}-pad{g[5]}")
def test_demosaic_writes_its_rows_and_nothing_else(ctx, geo):
    (H, W), half, rows, dst_mis, src_mis, pad = geo
    mosaic, prof = dm.fixture("random", "GBRG", H, W)
    params = prof.plan(H, W, half)
    want = dm.demosaic(mosaic, prof, half_size=half)
    y0, y1 = rows or (0, params.out_h)
    src = Arena.holding(dev(mosaic), misalign=src_mis, pad=pad)
    dst = Arena.hwc(params.out_h, params.out_w, torch.int16, misalign=dst_mis, device="cuda")
    what = f"r2f_demosaic_u16 {geo}"
    rc = ctx._lib.r2f_demosaic_u16(ctx._h, src.view.data_ptr(), 0, H, W + pad, H, W, C.byref(params), dst.view.data_ptr(), y0, y1,
                                   ctx._stream())
    assert rc == 0, (what, ctx._lib.r2f_last_error(ctx._h))
    torch.cuda.synchronize()
    dst.check(dst.rows_mask(y0, y1), expected=want.view(np.int16), what=what)
    got = dst.view[y0:y1].cpu().numpy().view(np.uint16)
    assert np.array_equal(got, want[y0:y1]), what
    src.unchanged(what)


@pytest.mark.parametrize("half", [False, True], ids=["full", "half"])
def test_refused_calls_leave_the_arena_untouched(ctx, half):
    H, W = 66, 130
    mosaic, prof = dm.fixture("random", "RGGB", H, W)
    params = prof.plan(H, W, half)
    src = Arena.holding(dev(mosaic))
    dst = Arena.hwc(params.out_h, params.out_w, torch.int16, device="cuda")

    def call(gy0, nrows, pitch, p, y0, y1, s=src.view.data_ptr(), d=dst.view.data_ptr()):
        return ctx._lib.r2f_demosaic_u16(ctx._h, s, gy0, nrows, pitch, H, W, C.byref(p), d, y0, y1, ctx._stream())

    assert call(0, H - 1, W, params, 0, params.out_h) == -1       # the window ends a row early
    assert call(1, H - 1, W, params, 0, params.out_h) == -1       # ... begins a row late
    assert call(0, H, W - 1, params, 0, params.out_h) == -1       # a pitch below W
    assert call(0, H, W, params, -1, 4) == -1 and call(0, H, W, params, 3, 2) == -1 and call(0, H, W, params, 0, params.out_h + 1) == -1
    assert call(0, H, W, prof.plan(H + 2, W, half), 0, 4) == -1   # the params of another frame size
    bad = prof.plan(H, W, half)
    bad.cfa[1] = bad.cfa[0]                                       # not a Bayer pattern
    assert call(0, H, W, bad, 0, 4) == -1
    assert call(0, H, W, params, 0, 4, s=None) == -1 and call(0, H, W, params, 0, 4, d=None) == -1
    torch.cuda.synchronize()
    dst.check(None, what="refused r2f_demosaic_u16")
    src.unchanged("refused r2f_demosaic_u16")
