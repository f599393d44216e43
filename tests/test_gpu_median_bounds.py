"""The three median entry points write exactly their rows and bytes: the destination in a canary arena (tests/arena.py) -- behind
its guard, aligned or one element off --, the mosaic in a source arena, contiguous or pitched and misaligned; rows [y0, y1) are
written, all of them, and nothing else -- for a middle band, the first and the last band and y0 == y1, upright and turned, with one
pass and with four --, the source (guards included) is untouched, and a refused call leaves the arena as it was."""

import ctypes as C

import numpy as np
import pytest

import highlight_model as hm
import median_model as mm
import xtrans_model as xm
from arena import Arena

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FACTOR = np.float32(2.0 ** 0.5)


@pytest.fixture(scope="module")
def ctx():
    from raw2film_amd.context import HipContext

    c = HipContext(0)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def bands(n):
    """The first, a middle and the last band of n rows, none on the tile grid, and an empty one."""
    a, b = n // 3, n - n // 4
    return ((0, a), (a, b), (b, n), (a, a))


# (reduced size, orientation, passes, clip or not, destination misalignment in elements, source misalignment, source row pad)
U16 = [(False, 0, 1, False, 0, 0, 0), (False, 0, 4, True, 1, 1, 3), (False, 3, 2, False, 0, 0, 1), (False, 5, 4, True, 1, 1, 0),
       (False, 6, 1, False, 0, 0, 2), (True, 0, 4, False, 1, 0, 1), (True, 5, 1, True, 0, 1, 0), (True, 3, 2, True, 0, 0, 0)]


def geo_id(g):
    return f"{'reduced' if g[0] else 'full'}-o{g[1]}-n{g[2]}-{'blend' if g[3] else 'plain'}-mis{g[4]}{g[5]}-pad{g[6]}"


def _u16(ctx, fn, case, geo, xtrans):
    reduced, o, n, blend, dst_mis, src_mis, pad = geo
    mosaic, prof, clip = case
    clip = clip if blend else None
    H, W = mosaic.shape
    params = prof.plan(H, W, reduced)
    want = hm.orient(mm.demosaic(mosaic, prof, n, clip, half_size=reduced, xtrans=xtrans), o)
    src = Arena.holding(dev(mosaic), misalign=src_mis, pad=pad)
    for y0, y1 in bands(want.shape[0]):
        dst = Arena.hwc(want.shape[0], want.shape[1], torch.int16, misalign=dst_mis, device="cuda")
        what = f"{fn} {geo} rows [{y0}, {y1})"
        rc = getattr(ctx._lib, fn)(ctx._h, src.view.data_ptr(), 0, H, W + pad, H, W, C.byref(params), o, clip or 0, n, dst.view.data_ptr(), y0, y1,
                                   ctx._stream())
        assert rc == 0, (what, ctx._lib.r2f_last_error(ctx._h))
        torch.cuda.synchronize()
        dst.check(dst.rows_mask(y0, y1), expected=want.view(np.int16), what=what)
        assert np.array_equal(dst.view[y0:y1].cpu().numpy().view(np.uint16), want[y0:y1]), what
    src.unchanged(fn)


@pytest.mark.parametrize("geo", U16, ids=geo_id)
def test_bayer_median_writes_its_rows_and_nothing_else(ctx, geo):
    shape = (2 * hm.BAYER_FRAME[0], 2 * hm.BAYER_FRAME[1]) if geo[0] else hm.BAYER_FRAME
    _u16(ctx, "r2f_demosaic_median_u16", hm.bayer_case("equal", "GBRG", shape), geo, False)


@pytest.mark.parametrize("geo", U16, ids=geo_id)
def test_xtrans_median_writes_its_rows_and_nothing_else(ctx, geo):
    shape = (3 * hm.XTRANS_FRAME[0], 3 * hm.XTRANS_FRAME[1]) if geo[0] else hm.XTRANS_FRAME
    _u16(ctx, "r2f_demosaic_xtrans_median_u16", hm.xtrans_case("equal", xm.PATTERNS[1], shape), geo, True)


# (half size, window of the demosaiced frame or None, passes, clip or not, destination misalignment in floats, source misalignment, pad)
F32 = [(False, None, 1, False, 0, 0, 0), (False, (3, 65, 37, 63), 4, True, 1, 1, 1), (False, (1, 5, 41, 86), 2, False, 3, 0, 2),
       (True, None, 4, True, 2, 1, 0), (True, (2, 1, 21, 63), 1, False, 1, 0, 3), (True, (33, 65, 20, 100), 4, False, 0, 0, 0)]


@pytest.mark.parametrize("geo", F32, ids=lambda g: f"{'half' if g[0] else 'full'}-win{g[1]}-n{g[2]}-{'blend' if g[3] else 'plain'}"
                                                     f"-mis{g[4]}{g[5]}-pad{g[6]}".replace(" ", ""))
def test_the_float_epilogue_writes_its_rows_and_nothing_else(ctx, geo):
    half, window, n, blend, dst_mis, src_mis, pad = geo
    shape = (2 * hm.BAYER_FRAME[0], 2 * hm.BAYER_FRAME[1]) if half else hm.BAYER_FRAME
    mosaic, prof, clip = hm.bayer_case("wb", "RGGB", shape)
    clip = clip if blend else None
    H, W = mosaic.shape
    params = prof.plan(H, W, half)
    r0, c0, nr, nc = window or (0, 0, params.out_h, params.out_w)
    frame = mm.demosaic(mosaic, prof, n, clip, half_size=half)[r0:r0 + nr, c0:c0 + nc]
    want = np.minimum(frame.astype(np.float32) / np.float32(65535.0) * FACTOR, np.float32(65504))
    src = Arena.holding(dev(mosaic), misalign=src_mis, pad=pad)
    for y0, y1 in bands(nr):
        dst = Arena.hwc(nr, nc, torch.float32, misalign=dst_mis, device="cuda")
        what = f"r2f_demosaic_median_f32 {geo} rows [{y0}, {y1})"
        rc = ctx._lib.r2f_demosaic_median_f32(ctx._h, src.view.data_ptr(), 0, H, W + pad, H, W, C.byref(params), clip or 0, n, r0, c0, nr, nc,
                                              65535.0, float(FACTOR), dst.view.data_ptr(), y0, y1, ctx._stream())
        assert rc == 0, (what, ctx._lib.r2f_last_error(ctx._h))
        torch.cuda.synchronize()
        dst.check(dst.rows_mask(y0, y1), expected=want, what=what)
        assert np.array_equal(dst.view[y0:y1].cpu().numpy().view(np.uint32), np.ascontiguousarray(want[y0:y1]).view(np.uint32)), what
    src.unchanged("r2f_demosaic_median_f32")


def test_refused_calls_leave_the_arenas_untouched(ctx):
    mosaic, prof, clip = hm.bayer_case("equal", "RGGB", hm.BAYER_FRAME)
    xmosaic, xprof, _ = hm.xtrans_case("equal", xm.PATTERNS[0], hm.XTRANS_FRAME)
    (H, W), (XH, XW) = mosaic.shape, xmosaic.shape
    p, xp = prof.plan(H, W), xprof.plan(XH, XW)
    src, xsrc = Arena.holding(dev(mosaic)), Arena.holding(dev(xmosaic))
    dst, xdst = Arena.hwc(H, W, torch.int16, device="cuda"), Arena.hwc(XH, XW, torch.int16, device="cuda")
    fdst = Arena.hwc(20, 40, torch.float32, device="cuda")
    lib, h, s = ctx._lib, ctx._h, ctx._stream()

    def bayer(gy0=0, nrows=H, pitch=W, params=p, o=0, c=clip, n=2, y0=0, y1=H, sp=src.view.data_ptr(), dp=dst.view.data_ptr()):
        return lib.r2f_demosaic_median_u16(h, sp, gy0, nrows, pitch, H, W, C.byref(params), o, c, n, dp, y0, y1, s)

    def xtrans(gy0=0, nrows=XH, pitch=XW, o=0, c=clip, n=2, y0=0, y1=XH):
        return lib.r2f_demosaic_xtrans_median_u16(h, xsrc.view.data_ptr(), gy0, nrows, pitch, XH, XW, C.byref(xp), o, c, n, xdst.view.data_ptr(), y0,
                                                  y1, s)

    def f32(nrows=H, c=clip, n=2, win=(2, 3, 20, 40), divisor=65535.0, y0=0, y1=20, off=0):
        return lib.r2f_demosaic_median_f32(h, src.view.data_ptr(), 0, nrows, W, H, W, C.byref(p), c, n, *win, divisor, 1.0,
                                           fdst.view.data_ptr() + off, y0, y1, s)

    for call in (bayer, xtrans, f32):
        assert call(n=0) == -1 and call(n=5) == -1 and call(n=-3) == -1        # passes outside [1, 4]
        assert call(c=65536) == -1 and call(c=-1) == -1                        # clip neither 0 nor inside [1, 65535]
        assert call(nrows=20) == -1                                            # the source window ends early
        assert call(y0=3, y1=2) == -1 and call(y0=-1) == -1
    # the reach of step M: a band that the plain entry point's window would serve is refused
    assert bayer(gy0=6, nrows=30, y0=10, y1=20, n=1) == -1 and bayer(gy0=5, nrows=19, y0=10, y1=20, n=1) == -1
    assert b"read mosaic rows [5, 25)" in lib.r2f_last_error(h)
    assert xtrans(gy0=6, nrows=30, y0=10, y1=20, n=2) == -1
    assert b"read mosaic rows [5, 25)" in lib.r2f_last_error(h)
    assert f32(nrows=27, n=4, y0=0, y1=18) == -1                               # window rows [2, 20) read mosaic rows [0, 28)
    assert b"read mosaic rows [0, 28)" in lib.r2f_last_error(h)
    assert bayer(gy0=1, nrows=H - 1) == -1 and bayer(pitch=W - 1) == -1 and bayer(y1=H + 1) == -1 and bayer(o=8) == -1 and bayer(o=-1) == -1
    assert bayer(params=prof.plan(H + 2, W)) == -1 and bayer(sp=None) == -1 and bayer(dp=None) == -1
    assert bayer(o=5, nrows=H - 1, y0=0, y1=4) == -1                           # a turned band reads every mosaic row
    assert xtrans(pitch=XW - 1) == -1 and xtrans(y1=XH + 1) == -1 and xtrans(o=9) == -1
    assert f32(win=(2, 3, 20, W)) == -1 and f32(win=(2, 3, 0, 40)) == -1 and f32(divisor=0.0) == -1 and f32(y1=21) == -1 and f32(off=2) == -1
    torch.cuda.synchronize()
    for a in (dst, xdst, fdst):
        a.check(None, what="refused median calls")
    src.unchanged("refused median calls")
    xsrc.unchanged("refused median calls")
