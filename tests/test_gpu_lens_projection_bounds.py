"""r2f_lens_correct_projected writes exactly its window's rows and bytes of all three planes: destination planes in canary arenas
(tests/arena.py) -- contiguous, with a pad between the planes, off a 16-byte boundary, taller than the window -- for every input
layout, without a TCA record and with one; everything around the window's samples keeps the canary, every sample of the window is
written, and the source (guards included) is untouched.  The records are the equisolid one at scale 0.5 (tiles that work in two
halves, each with a box of its own) with the TCA spec `edge` (red and blue reach further out of the frame than green does), and
the fisheye at scale 0.25 (tiles that gather)."""

import ctypes as C

import numpy as np
import pytest

import lens_model as lm
import lens_projection_model as pm
import lens_tca_model as tm
from arena import Arena

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ctx():
    from raw2film_amd.context import HipContext

    c = HipContext(0)
    yield c
    c.close()


LAYOUTS = {"hwc3": 0, "hwc4": 1, "chw": 2}
# (frame, window (row0, col0, rows, cols), rows of the destination, its first global row, pad, misalign): test_gpu_lens_bounds.py's
GEOMETRIES = [
    ((33, 47), (0, 0, 33, 47), 33, 0, 0, 0),
    ((33, 47), (3, 5, 21, 30), 21, 0, 1, 1),      # an odd window, padded planes one float off a 16-byte boundary
    ((96, 128), (0, 0, 96, 128), 96, 0, 4, 0),    # whole tiles: 2 x 6 blocks
    ((96, 128), (10, 64, 67, 64), 80, -6, 0, 1),  # a destination taller than the window: rows 6 .. 72 of it are written
    ((150, 210), (-7, -9, 160, 230), 160, 0, 0, 0),  # a window that reaches past every edge of the frame
    ((7, 9), (0, 0, 7, 9), 7, 0, 4, 1),
    ((1, 64), (0, 0, 1, 64), 1, 0, 0, 0),
    ((64, 1), (0, 0, 64, 1), 64, 0, 1, 0),
]
RECORDS = {"halves-tca": ("vignetting", "equisolid", "edge", dict(scale=0.5)), "gather": ("none", "fisheye", None, dict(scale=0.25))}


@pytest.mark.parametrize("record", list(RECORDS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: f"{g[0][0]}x{g[0][1]}-win{g[1][2]}x{g[1][3]}-pad{g[4]}-mis{g[5]}")
def test_lens_correct_projected_writes_its_window_and_nothing_else(ctx, geo, layout, record):
    (H, W), (r0, c0, nr, nc), rows_alloc, gy0, pad, misalign = geo
    img = lm.frame(H, W)
    a = img if layout == "hwc3" else np.concatenate([img, np.ones((H, W, 1), np.float32)], -1) if layout == "hwc4" \
        else np.ascontiguousarray(img.transpose(2, 0, 1))
    src = Arena.holding(torch.from_numpy(a).cuda(), misalign=misalign)
    dst = Arena.planes(rows_alloc, nc, pad=pad, misalign=misalign, device="cuda")
    pd = ctx.planes(dst.view, gy0)
    name, projection, tca_spec, changes = RECORDS[record]
    params, proj, tca = pm.profile(name, projection, tca_spec, **changes).plan_projected(H, W)
    what = f"r2f_lens_correct_projected {record} {geo} {layout}"
    rc = ctx._lib.r2f_lens_correct_projected(ctx._h, src.view.data_ptr(), LAYOUTS[layout], H, W, C.byref(params), C.byref(proj),
                                             None if tca is None else C.byref(tca), C.byref(pd), nr, nc, r0, c0, ctx._stream())
    assert rc == 0, (what, ctx._lib.r2f_last_error(ctx._h))
    torch.cuda.synchronize()
    dst.check(dst.rows_mask(-gy0, -gy0 + nr), what=what)
    want = pm.correct(img, lm.from_params(params), pm.from_params(proj), None if tca is None else tm.from_params(tca), (r0, c0, nr, nc))
    got = dst.view[:, -gy0:-gy0 + nr].cpu().numpy().transpose(1, 2, 0)
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), what
    src.unchanged(what)


@pytest.mark.parametrize("with_tca", [False, True], ids=["plain", "tca"])
def test_rows_outside_the_destination_are_refused_and_nothing_is_written(ctx, with_tca):
    img = torch.from_numpy(lm.frame(33, 47)).cuda()
    dst = Arena.planes(20, 47, device="cuda")
    pd = ctx.planes(dst.view, 0)
    params, proj, tca = pm.profile("ptlens", "fisheye", "linear" if with_tca else None).plan_projected(33, 47)
    rc = ctx._lib.r2f_lens_correct_projected(ctx._h, img.data_ptr(), 0, 33, 47, C.byref(params), C.byref(proj),
                                             C.byref(tca) if with_tca else None, C.byref(pd), 21, 47, 0, 0, ctx._stream())
    assert rc == -1
    torch.cuda.synchronize()
    dst.check(None, what="refused r2f_lens_correct_projected")
