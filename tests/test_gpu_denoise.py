"""r2f_mosaic_denoise against the NumPy model of include/r2f.h (tests/denoise_model.py): the device's bytes equal the model's, no
tolerance.  The shapes, inputs, thresholds, maxima and black levels are tests/denoise_cases.py's (derived from the kernel's tile);
every shape sees every threshold with every maximum on every input, and the source and destination layouts that select between
32-bit and 16-bit accesses: a pitch above W, a base one sample off a 4-byte boundary, both, and dst == src."""

import numpy as np
import pytest

import denoise_cases as cases

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

IDS = [f"{h}x{w}" for h, w in cases.SHAPES]


@pytest.fixture(scope="module")
def ctx():
    from raw2film_amd.context import HipContext

    c = HipContext(0)
    yield c
    c.close()


def plan(shape, threshold, maximum):
    from raw2film_amd.raw import WaveletDenoise

    p = WaveletDenoise(threshold, maximum).plan(cases.BLACK, *shape)
    assert p.shift == cases.SHIFTS[cases.MAXIMA.index(maximum)]
    return p


def device_view(frame, pad=0, offset=0, fill=0x5A5A):
    """`frame` on the device as a view of a flat int16 buffer: rows W + pad samples apart, the first sample `offset` samples behind
    the (256-byte aligned) base; the pad holds `fill`."""
    H, W = frame.shape
    flat = torch.full((offset + H * (W + pad),), fill, dtype=torch.int16, device="cuda")
    view = torch.as_strided(flat, (H, W), (W + pad, 1), offset)
    view.copy_(torch.from_numpy(frame.view(np.int16).copy()))
    assert view.data_ptr() % 4 == (2 * offset) % 4
    return view


def host(t):
    return t.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("shape", cases.SHAPES, ids=IDS)
def test_the_devices_bytes_equal_the_models(ctx, shape):
    for name in cases.INPUTS:
        src = torch.from_numpy(cases.mosaic(shape, name).view(np.int16).copy()).cuda()
        for T in cases.THRESHOLDS:
            for M in cases.MAXIMA:
                got = host(ctx.mosaic_denoise(src, plan(shape, T, M)))
                want = cases.expected(shape, name, T, M)
                assert np.array_equal(got, want), (name, T, M, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
        assert np.array_equal(host(src), cases.mosaic(shape, name))  # (the source is only read)


@pytest.mark.parametrize("shape", cases.SHAPES, ids=IDS)
def test_pitch_and_alignment_only_select_the_access_width(ctx, shape):
    for name, T, M in (("edge", 100.0, 16383 - 512), ("impulses", 400.0, 255)):
        frame, want, p = cases.mosaic(shape, name), cases.expected(shape, name, T, M), plan(shape, T, M)
        for src_pad, src_off, dst_pad, dst_off in ((3, 0, 0, 0), (0, 1, 0, 0), (4, 1, 0, 0), (0, 0, 5, 0), (0, 0, 0, 1), (2, 0, 6, 1), (1, 1, 1, 1)):
            src = device_view(frame, src_pad, src_off)
            out = device_view(np.zeros_like(frame), dst_pad, dst_off)
            res = ctx.mosaic_denoise(src, p, out=out)
            assert res is out
            what = (name, src_pad, src_off, dst_pad, dst_off)
            assert np.array_equal(host(out), want), what
            assert np.array_equal(host(src), frame), what


@pytest.mark.parametrize("shape", cases.SHAPES, ids=IDS)
def test_the_destination_may_be_the_source(ctx, shape):
    for name, T, M in (("edge", 400.0, 32767), ("impulses", 1.0, 1), ("edge", 1e5, 32768)):
        want, p = cases.expected(shape, name, T, M), plan(shape, T, M)
        for pad, off in ((0, 0), (3, 1)):
            buf = device_view(cases.mosaic(shape, name), pad, off)
            assert ctx.mosaic_denoise(buf, p, out=buf) is buf
            assert np.array_equal(host(buf), want), (name, T, M, pad, off)


def test_the_workspace_is_kept_and_reused(ctx):
    big, small = cases.SHAPES[-1], cases.SHAPES[0]
    src = torch.from_numpy(cases.mosaic(big, "edge").view(np.int16).copy()).cuda()
    ctx.mosaic_denoise(src, plan(big, 100.0, 255))
    ws = ctx._denoise_workspace
    assert ws is not None and ws.numel() >= 12 * big[0] * big[1]
    got = host(ctx.mosaic_denoise(torch.from_numpy(cases.mosaic(small, "edge").view(np.int16).copy()).cuda(), plan(small, 100.0, 255)))
    assert ctx._denoise_workspace is ws  # (a smaller frame behind a larger one: the same buffer, stale bytes behind its share)
    assert np.array_equal(got, cases.expected(small, "edge", 100.0, 255))


def test_the_context_refuses_what_is_no_mosaic_of_the_step(ctx):
    p = plan((64, 64), 100.0, 255)
    ok = torch.zeros((64, 64), dtype=torch.int16, device="cuda")
    for bad in (torch.zeros((62, 64), dtype=torch.int16, device="cuda"), torch.zeros((64, 64), dtype=torch.float32, device="cuda"),
                torch.zeros((64, 64), dtype=torch.int16), ok[:, ::2]):
        with pytest.raises(ValueError):
            ctx.mosaic_denoise(bad, p)
    with pytest.raises(ValueError):
        ctx.mosaic_denoise(torch.zeros((66, 65), dtype=torch.int16, device="cuda"), p)  # (an odd side: the entry point's refusal)
    with pytest.raises(ValueError):
        ctx.mosaic_denoise(ok, p, out=torch.zeros((64, 66), dtype=torch.int16, device="cuda"))
    with pytest.raises(ValueError):
        ctx.mosaic_denoise(ok, (512, 512, 512, 512))
