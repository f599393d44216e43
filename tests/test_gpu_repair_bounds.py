"""r2f_mosaic_repair writes the rows it was given and reads the rows it may: the destination mosaic in a canary arena
(tests/arena.py) between its guards, contiguous or pitched, aligned like the source or not; the source in an arena of its own, its
pad holding the canary and the rows outside the source window poisoned with 0xFFFF (a read of one would make a neighbour of a hot
sample stand above it, and the bytes would differ from the model's).  After the call rows [y0, y1) of the destination hold the
model's bytes, all of them, nothing else changed, the count word alone moved, and the source (guards included) is bit-identical.
The refusals leave both alone."""

import ctypes as C

import numpy as np
import pytest

import repair_model as model
from arena import Arena, guard_elems
from raw2film_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

V, R = _lib.MOSAIC_REPAIR_VEC, _lib.MOSAIC_REPAIR_ROWS
BLACK = (512, 520, 500, 512)
BLACK36 = tuple(400 + 7 * ((5 * i + 3) % 36) for i in range(36))


@pytest.fixture(scope="module")
def ctx():
    from raw2film_amd.context import HipContext

    c = HipContext(0)
    yield c
    c.close()


def plan(P, shape, mn=3):
    out = _lib.RepairParams()
    black = BLACK if P == 2 else BLACK36
    ids = None if P == 2 else (C.c_int32 * 36)(*[int(v) for v in model.cfa_ids(model.CANONICAL, 2, 1).ravel()])
    assert _lib.load().r2f_mosaic_repair_plan(P, ids, (C.c_double * len(black))(*black), 1000, 32, mn, shape[0], shape[1], C.byref(out)) == _lib.OK
    return out, black, None if P == 2 else model.cfa_ids(model.CANONICAL, 2, 1)


# (period, frame (H, W), source window (gy0, nrows), rows [y0, y1), source misalignment and pad, destination misalignment and pad)
GEOMETRIES = [
    (2, (6, 6), (0, 6), (0, 6), 0, 0, 0, 0),
    (6, (6, 6), (0, 6), (0, 6), 1, 0, 0, 3),
    (2, (37, 70), (0, 37), (0, 37), 0, 0, 0, 0),
    (6, (37, 2 * V + 3), (0, 37), (0, 37), 1, 3, 1, 3),
    (2, (37, 64 * V + 1), (3, 24), (5, 25), 0, 1, 3, 0),          # rows [3, 27) are read: the whole window
    (6, (37, 64 * V + 1), (5, 20), (7, 23), 1, 7, 0, 7),
    (6, (37, 64 * V - 1), (1, 30), (1 + R, 2 + R), 0, 0, 5, 1),   # one row
    (2, (37, 2 * V + 3), (33, 4), (35, 37), 1, 1, 0, 0),          # the last two rows: the frame ends the reach
    (2, (37, V - 1), (0, 5), (0, 3), 3, 7, 2, 0),                 # the first three: the same at the top
    (6, (70, 200), (0, 70), (R, 70 - R + 1), 0, 0, 4, 8),
]


@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: f"p{g[0]}-{g[1][0]}x{g[1][1]}-win{g[2]}-rows{g[3]}-src{g[4]}+{g[5]}-dst{g[6]}+{g[7]}")
def test_the_call_writes_its_rows_and_reads_its_window(ctx, geo):
    P, (H, W), (gy0, nrows), (y0, y1), smis, spad, dmis, dpad = geo
    params, black, cfa = plan(P, (H, W))
    frame = model.field((H, W), H * 1000 + W)
    want, hot = model.repair(frame, P, black, 1000, 32, 3, cfa)
    poisoned = frame.copy()
    poisoned[:gy0], poisoned[gy0 + nrows:] = 0xFFFF, 0xFFFF  # the rows outside the source window
    src = Arena.holding(torch.from_numpy(poisoned.view(np.int16)).cuda(), misalign=smis, pad=spad)
    dst = Arena(torch.int16, (H, W), (W + dpad, 1), guard=guard_elems(W + dpad, 1), misalign=dmis, device="cuda", names=("row", "column"))
    count = Arena.flat_of(torch.int32, 1, device="cuda")
    count.view.zero_()
    what = f"r2f_mosaic_repair {geo}"
    rc = ctx._lib.r2f_mosaic_repair(ctx._h, src.view[gy0:].data_ptr(), gy0, nrows, W + spad, H, W, C.byref(params), dst.view.data_ptr(), W + dpad,
                                    y0, y1, count.view.data_ptr(), ctx._stream())
    assert rc == 0, (what, ctx._lib.r2f_last_error(ctx._h))
    torch.cuda.synchronize()
    written = torch.zeros((H, W), dtype=torch.bool)
    written[y0:y1] = True
    expected = torch.from_numpy(want.view(np.int16).copy())
    dst.check(written, what=what, expected=expected)
    got = dst.view.cpu().numpy().view(np.uint16)
    assert np.array_equal(got[y0:y1], want[y0:y1]), (what, int((got[y0:y1] != want[y0:y1]).sum()))
    count.check(torch.ones(1, dtype=torch.bool), what=what)
    assert int(count.view.item()) == int(hot[y0:y1].sum()), what
    src.unchanged(what)


def test_refused_calls_leave_both_arenas_untouched(ctx):
    P, H, W = 6, 37, 2 * V + 3
    params, _, _ = plan(P, (H, W))
    frame = model.field((H, W), 3)
    src = Arena.holding(torch.from_numpy(frame.view(np.int16)).cuda())
    dst = Arena(torch.int16, (H, W), (W, 1), guard=guard_elems(W, 1), device="cuda", names=("row", "column"))
    count = Arena.flat_of(torch.int32, 1, device="cuda")

    def bad(**fields):
        p = _lib.RepairParams.from_buffer_copy(params)
        for k, v in fields.items():
            if k == "offset":
                p.offset[7][2][0], p.offset[7][2][1] = v
            elif k == "black":
                p.black[35] = v
            else:
                setattr(p, k, v)
        return p

    def call(gy0=0, nrows=H, pitch=W, H=H, W=W, p=params, dpitch=W, y0=0, y1=H, s=src.view.data_ptr(), d=dst.view.data_ptr()):
        return ctx._lib.r2f_mosaic_repair(ctx._h, s, gy0, nrows, pitch, H, W, None if p is None else C.byref(p), d, dpitch, y0, y1,
                                          count.view.data_ptr(), ctx._stream())

    for kw in (dict(nrows=H - 1), dict(gy0=1), dict(y0=4, y1=20, gy0=3, nrows=18), dict(y0=4, y1=20, gy0=2, nrows=19), dict(pitch=W - 1),
               dict(dpitch=W - 1), dict(H=5, y1=5), dict(W=5, pitch=5, dpitch=5), dict(y0=-1), dict(y1=H + 1), dict(y0=4, y1=3), dict(s=None),
               dict(d=None), dict(p=None), dict(p=bad(period=4)), dict(p=bad(threshold=65536)), dict(p=bad(q=0)), dict(p=bad(q=256)),
               dict(p=bad(min_neighbours=2)), dict(p=bad(black=65536)), dict(p=bad(black=-1)), dict(p=bad(offset=(3, 0))),
               dict(p=bad(offset=(0, 0))), dict(p=bad(period=2)),  # (a period-2 table holds the Bayer offsets and nothing else)
               dict(d=src.view.data_ptr()), dict(d=src.view[1:].data_ptr(), y1=H - 1), dict(y0=10, y1=12, d=src.view[2:].data_ptr())):
        assert call(**kw) == _lib.EINVAL, kw
    assert call(y0=7, y1=7) == _lib.OK  # no rows: no launch
    torch.cuda.synchronize()
    dst.check(None, what="refused r2f_mosaic_repair")
    count.check(None, what="refused r2f_mosaic_repair")
    src.unchanged("refused r2f_mosaic_repair")
