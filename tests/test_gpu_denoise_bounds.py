"""r2f_mosaic_denoise writes the H x W samples of dst, all of them, and bytes inside the workspace it was given, and nothing else: dst
(contiguous or pitched, aligned or one sample off) and the workspace sit in canary arenas (tests/arena.py) between their guards, the
source in a third whose every byte stays what it was.  A call the entry point refuses -- params the planner does not produce among
them -- writes nothing at all."""

import ctypes as C

import numpy as np
import pytest

import denoise_cases as cases
from arena import Arena, guard_elems
from raw2film_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ctx():
    from raw2film_amd.context import HipContext

    c = HipContext(0)
    yield c
    c.close()


def params(shape, threshold=100.0, maximum=16383 - 512):
    from raw2film_amd.raw import WaveletDenoise

    return WaveletDenoise(threshold, maximum).plan(cases.BLACK, *shape)


def dst_arena(shape, pad, misalign):
    H, W = shape
    return Arena(torch.int16, (H, W), (W + pad, 1), guard=guard_elems(W + pad, 1), misalign=misalign, device="cuda", names=("row", "column"))


# (shape, source pad, source misalignment, destination pad, destination misalignment), in samples
GEOMETRIES = [(cases.SHAPES[0], 0, 0, 0, 0), (cases.SHAPES[1], 3, 1, 0, 1), (cases.SHAPES[2], 0, 0, 5, 0), (cases.SHAPES[3], 1, 1, 7, 1),
              (cases.SHAPES[3], 2, 0, 2, 0)]


@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: f"{g[0][0]}x{g[0][1]}-src{g[1]}+{g[2]}-dst{g[3]}+{g[4]}")
def test_the_call_writes_its_samples_and_its_workspace(ctx, geo):
    shape, spad, smis, dpad, dmis = geo
    H, W = shape
    T, M = 100.0, 16383 - 512
    want = cases.expected(shape, "edge", T, M)
    src = Arena.holding(torch.from_numpy(cases.mosaic(shape, "edge").view(np.int16).copy()).cuda(), misalign=smis, pad=spad)
    dst = dst_arena(shape, dpad, dmis)
    need = int(ctx._lib.r2f_mosaic_denoise_workspace_bytes(H, W))
    assert need == 12 * H * W
    ws = Arena.flat(need, device="cuda")
    assert ws.view.data_ptr() % 16 == 0
    what = f"r2f_mosaic_denoise {geo}"
    rc = ctx._lib.r2f_mosaic_denoise(ctx._h, src.view.data_ptr(), W + spad, H, W, C.byref(params(shape, T, M)), dst.view.data_ptr(), W + dpad,
                                     ws.view.data_ptr(), need, ctx._stream())
    assert rc == 0, (what, ctx._lib.r2f_last_error(ctx._h))
    torch.cuda.synchronize()
    expected = torch.from_numpy(want.view(np.int16).copy())
    dst.check(torch.ones(shape, dtype=torch.bool), expected=expected, what=what)
    assert np.array_equal(dst.view.cpu().numpy().view(np.uint16), want), what
    ws.check(torch.ones(need, dtype=torch.bool), require_written=False, what=what + " (workspace)")
    src.unchanged(what)


def test_refused_calls_write_nothing(ctx):
    shape = cases.SHAPES[1]
    H, W = shape
    src = Arena.holding(torch.from_numpy(cases.mosaic(shape, "edge").view(np.int16).copy()).cuda())
    dst = dst_arena(shape, 0, 0)
    need = 12 * H * W
    ws = Arena.flat(need, device="cuda")
    good = params(shape)

    def call(p=good, s=src.view.data_ptr(), d=dst.view.data_ptr(), w=ws.view.data_ptr(), H=H, W=W, sp=W, dp=W, n=need):
        return ctx._lib.r2f_mosaic_denoise(ctx._h, s, sp, H, W, None if p is None else C.byref(p), d, dp, w, n, ctx._stream())

    def tampered(**kw):
        p = _lib.DenoiseParams.from_buffer_copy(good)
        for k, v in kw.items():
            if k == "black":
                p.black[v[0]] = v[1]
            else:
                setattr(p, k, v)
        return p

    for p in (tampered(shift=16), tampered(shift=-1), tampered(shift=1 << 20), tampered(black=(0, -1)), tampered(black=(3, 65536)),
              tampered(threshold=0.0), tampered(threshold=-5.0), tampered(threshold=float("nan")), tampered(threshold=2e6), None):
        assert call(p=p) == _lib.EINVAL, p and (tuple(p.black), p.shift, p.threshold)
    for kw in (dict(s=None), dict(d=None), dict(w=None), dict(n=need - 1), dict(w=ws.view.data_ptr() + 4), dict(sp=W - 1), dict(dp=W - 2),
               dict(H=H - 1), dict(W=W - 1), dict(H=62), dict(W=62, sp=62, dp=62), dict(w=dst.view.data_ptr()), dict(w=src.view.data_ptr())):
        assert call(**kw) == _lib.EINVAL, kw
    torch.cuda.synchronize()
    dst.check(None, what="refused r2f_mosaic_denoise")
    ws.check(None, what="refused r2f_mosaic_denoise (workspace)")
    src.unchanged("refused r2f_mosaic_denoise")
    assert call() == _lib.OK  # (and the same buffers with the planner's own params run)
    torch.cuda.synchronize()
    assert np.array_equal(dst.view.cpu().numpy().view(np.uint16), cases.expected(shape, "edge", 100.0, 16383 - 512))
