"""r2f_mosaic_maximum writes the 4 bytes of its word and reads the rows it was given: the destination word in a canary arena
(tests/arena.py) between its guards, the mosaic in a source arena -- contiguous or pitched, aligned or one sample off, its pad
holding the canary (0xA5A5, above every d of these frames) and the rows outside the source window poisoned with 0xFFFF.  After the
call only the word changed, the mosaic (guards included) is bit-identical, and the value is the model's over [y0, y1): a read
outside the rows or the columns would have raised it."""

import ctypes as C

import numpy as np
import pytest

import levels_model as lm
from arena import Arena
from raw2film_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

V, R = _lib.MOSAIC_MAX_VEC, _lib.MOSAIC_MAX_ROWS


@pytest.fixture(scope="module")
def ctx():
    from raw2film_amd.context import HipContext

    c = HipContext(0)
    yield c
    c.close()


def levels(P):
    return [900 + 41 * ((7 * i + 3) % (P * P)) for i in range(P * P)]


# (period, frame (H, W), source window (gy0, nrows), rows [y0, y1), source misalignment in samples, source row pad)
GEOMETRIES = [
    (2, (2, 2), (0, 2), (0, 2), 0, 0),
    (6, (6, 6), (0, 6), (0, 6), 1, 0),
    (2, (R + 1, V + 1), (0, R + 1), (0, R + 1), 0, 0),
    (6, (37, 2 * V + 3), (0, 37), (0, 37), 1, 3),
    (2, (37, 64 * V + 1), (5, 20), (5, 25), 0, 1),          # the whole window, which begins below the frame's top
    (6, (37, 64 * V + 1), (5, 20), (6, 24), 1, 7),          # a row in from both of its ends
    (6, (37, 64 * V - 1), (1, 30), (1 + R, 2 + R), 0, 0),   # one row
    (2, (37, 2 * V + 3), (1, 36), (36, 37), 1, 1),          # the last row alone
    (6, (37, V - 1), (0, 37), (3, 3 + R - 1), 0, 7),
]


@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: f"p{g[0]}-{g[1][0]}x{g[1][1]}-win{g[2]}-rows{g[3]}-mis{g[4]}-pad{g[5]}")
def test_the_call_writes_its_word_and_reads_its_rows(ctx, geo):
    P, (H, W), (gy0, nrows), (y0, y1), mis, pad = geo
    black = levels(P)
    rng = np.random.default_rng(H * 1000 + W)
    frame = (lm.black_plane(black, P, H, W) + rng.integers(-30, 31, (H, W))).astype(np.uint16)
    want = lm.data_maximum(frame, black, P, (y0, y1))
    assert 0 < want <= 30
    poisoned = frame.copy()
    poisoned[:gy0], poisoned[gy0 + nrows:] = 0xFFFF, 0xFFFF  # the rows outside the source window
    src = Arena.holding(torch.from_numpy(poisoned.view(np.int16)).cuda(), misalign=mis, pad=pad)
    dst = Arena.flat_of(torch.int32, 1, device="cuda")
    dst.view.zero_()  # the caller zeroes the word
    what = f"r2f_mosaic_maximum {geo}"
    rc = ctx._lib.r2f_mosaic_maximum(ctx._h, src.view[gy0:].data_ptr(), gy0, nrows, W + pad, H, W, P, (C.c_int32 * len(black))(*black), y0, y1,
                                     dst.view.data_ptr(), ctx._stream())
    assert rc == 0, (what, ctx._lib.r2f_last_error(ctx._h))
    torch.cuda.synchronize()
    dst.check(torch.ones(1, dtype=torch.bool), what=what)
    assert int(dst.view.item()) == want, what
    src.unchanged(what)


def test_refused_calls_leave_both_arenas_untouched(ctx):
    P, H, W = 6, 37, 2 * V + 3
    black = levels(P)
    frame = np.random.default_rng(3).integers(0, 65536, (H, W)).astype(np.uint16)
    src = Arena.holding(torch.from_numpy(frame.view(np.int16)).cuda())
    dst = Arena.flat_of(torch.int32, 1, device="cuda")
    table = (C.c_int32 * 36)(*black)

    def call(gy0=0, nrows=H, pitch=W, H=H, W=W, period=P, y0=0, y1=H, s=src.view.data_ptr(), d=dst.view.data_ptr(), b=table):
        return ctx._lib.r2f_mosaic_maximum(ctx._h, s, gy0, nrows, pitch, H, W, period, b, y0, y1, d, ctx._stream())

    for kw in (dict(nrows=H - 1), dict(gy0=1), dict(pitch=W - 1), dict(period=4), dict(H=5, y1=5), dict(W=5, pitch=5), dict(y0=-1), dict(y1=H + 1),
               dict(y0=4, y1=3), dict(s=None), dict(d=None), dict(b=None), dict(b=(C.c_int32 * 36)(*([0] * 35 + [65536])))):
        assert call(**kw) == _lib.EINVAL, kw
    assert call(y0=7, y1=7) == _lib.OK  # no rows: no launch, the word keeps whatever it held
    torch.cuda.synchronize()
    dst.check(None, what="refused r2f_mosaic_maximum")
    src.unchanged("refused r2f_mosaic_maximum")
