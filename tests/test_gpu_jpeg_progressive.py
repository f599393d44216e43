"""The JPEG export's progressive option on a real GPU: encode_jpeg, process_jpeg and process_preloaded_jpeg with
progressive=True write the bytes Pillow's `save(f, "JPEG", quality=q, subsampling=s, progressive=True, exif=e)` writes."""

import numpy as np
import pytest

import jpeg_extremes as jx
from helpers import SEED, stocks, synthetic_frame
from test_gpu_jpeg import smooth
from test_gpu_jpeg_stream import MARK, render_kw
from test_jpeg_host import contents
from test_jpeg_options_host import EXIF, pillow_jpeg
from test_jpeg_progressive_host import SIZES, correction_frame, pillow_progressive, smooth_field

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def proc():
    from raw2film_amd import HipProcessor

    p = HipProcessor(cameras={}, lenses={}, device=0)
    yield p
    p.close()


@pytest.mark.parametrize("H,W", SIZES + ((256, 383), (1000, 1501)))
def test_encode_jpeg_progressive_writes_pillows_bytes(proc, H, W):
    for name, a in list(contents(H, W).items()) + [("black", np.zeros((H, W, 3), np.uint8))]:
        for q in (1, 75, 100):
            for s in (0, 1, 2):
                e = EXIF if (q + s) % 2 else b""
                got = proc.encode_jpeg(a, q, subsampling=s, progressive=True, exif=e)
                assert got == pillow_progressive(a, q, s, e), (name, q, s)


@pytest.mark.parametrize("H,W", jx.SIZES)
def test_encode_jpeg_progressive_extreme_coefficients(proc, H, W):
    """tests/jpeg_extremes.py: the DC scans with category-11 differences, the AC scans with 10-bit magnitudes to refine."""
    for name, a in jx.frames(H, W).items():
        for q in jx.QUALITIES:
            for s in (0, 1, 2):
                assert proc.encode_jpeg(a, q, subsampling=s, progressive=True) == pillow_progressive(a, q, s), (name, q, s)


def test_run_flushes_on_both_caps(proc):
    a = correction_frame(60, 90)  # refinement runs flushed at 937 buffered bits
    b = smooth_field(1456, 1456)  # first-scan runs flushed at 0x7FFF blocks
    for s in (0, 1, 2):
        assert proc.encode_jpeg(a, 100, subsampling=s, progressive=True) == pillow_progressive(a, 100, s), s
        assert proc.encode_jpeg(b, 75, subsampling=s, progressive=1, optimize=True) == pillow_progressive(b, 75, s), s


def test_row_strided_view_and_device_input(proc):
    a = contents(257, 390)["noise"]
    dev = torch.from_numpy(a).cuda()
    wide = torch.zeros((300, 512, 3), dtype=torch.uint8, device="cuda")
    wide[10:267, 40:430] = dev
    for s in (0, 1, 2):
        want = pillow_progressive(a, 90, s)
        assert proc.encode_jpeg(dev, 90, subsampling=s, progressive=True) == want
        assert proc.encode_jpeg(wide[10:267, 40:430], 90, subsampling=s, progressive=np.bool_(True)) == want


def test_full_size_frame_100mp(proc):
    H, W = 12288, 8192
    a = smooth(H, W)
    a[::7, ::5] ^= 0x55  # (texture: every scan has work)
    assert proc.encode_jpeg(a, 95, subsampling=2, progressive=True) == pillow_progressive(a, 95, 2)


def test_process_jpeg_progressive_is_pillow_of_process(proc):
    neg, prt, _ = stocks()
    H, W, fw = 210, 333, 1.0
    img = synthetic_frame(H, W, seed=5)
    kw = dict(print_film=prt, frame_width=fw, frame_height=fw * H / W, halation_green_factor=0.3, exp_kelvin=6000,
              color_masking=1.0, seed=SEED)
    px = proc.process(img, neg, 6, 0.4, **kw)
    for s in (0, 1, 2):
        got = proc.process_jpeg(img, neg, 6, 0.4, quality=97, subsampling=s, progressive=True, exif=EXIF, **kw)
        assert got == pillow_progressive(px, 97, s, EXIF), s
    pay = proc.extract_image_data_cpu(img, lens_correction=False, frame_width=fw, frame_height=fw * H / W)
    pre = dict(print_film=prt, halation_green_factor=0.3, exp_kelvin=6000, color_masking=1.0, seed=SEED)
    px = proc.process_preloaded(pay, neg, 6, 0.4, final_scaling="cpu", **pre)
    got = proc.process_preloaded_jpeg(pay, neg, 6, 0.4, quality=100, final_scaling="cpu", subsampling=1, progressive=True, **pre)
    assert got == pillow_progressive(px, 100, 1)


def test_progressive_with_stream_falls_back(proc):
    neg, prt, _ = stocks()
    H, W = 2416, 2400
    img = synthetic_frame(H, W, seed=9)
    kw = render_kw(prt, False, H, W)
    px = proc.process(img, neg, 6, 0.4, cache=False, **kw)
    proc.stream_rejected = MARK
    got = proc.process_jpeg(img, neg, 6, 0.4, quality=95, stream=True, subsampling=0, progressive=True, **kw)
    assert "progressive" in proc.stream_rejected
    assert got == pillow_progressive(px, 95, 0)
    pay = proc.extract_image_data_cpu(img, lens_correction=False, frame_width=kw["frame_width"], frame_height=kw["frame_height"])
    pre = {k: v for k, v in kw.items() if k not in ("lens_correction", "frame_width", "frame_height")}
    proc.stream_rejected = MARK
    got = proc.process_preloaded_jpeg(pay, neg, 6, 0.4, quality=95, stream=True, progressive=True, **pre)
    assert "progressive" in proc.stream_rejected
    assert got == pillow_progressive(proc.process_preloaded(pay, neg, 6, 0.4, **pre), 95, -1)


def test_invalid_values_and_the_c_abi(proc):
    a = contents(31, 64)["noise"]
    neg, prt, _ = stocks()
    img = synthetic_frame(32, 48, seed=1)
    for bad in (2, "yes", None, 1.5):
        with pytest.raises(ValueError):
            proc.encode_jpeg(a, 90, progressive=bad)
        with pytest.raises(ValueError):
            proc.process_jpeg(img, neg, 6, 0.4, print_film=prt, progressive=bad)
    from raw2film_amd import _lib

    ctx = proc.ctx
    H, W = 16, 24
    frame = torch.from_numpy(contents(H, W)["noise"]).cuda()
    bound = ctx.jpeg_bound_bytes_opts(H, W, 90, 0, False, True)
    out = torch.empty(bound, dtype=torch.uint8, device="cuda")
    length = torch.zeros(1, dtype=torch.int64, device="cuda")

    def encode(opts, cap):
        return ctx._lib.r2f_jpeg_encode_ex(ctx._h, frame.data_ptr(), H, W, 3 * W, opts, out.data_ptr(), cap, length.data_ptr(),
                                           ctx._stream())

    assert encode(_lib.JpegOpts(90, 0, 0, 2), bound) == -1  # R2F_EINVAL
    assert encode(_lib.JpegOpts(90, 0, 0, 1), bound - 1) == -1  # below the progressive bound
    assert encode(_lib.JpegOpts(90, 0, 0, 1), bound) == 0
    torch.cuda.synchronize()
    n = int(length.item())
    assert bytes(out[:n].cpu().numpy()) == pillow_progressive(contents(H, W)["noise"], 90, 0)
    rc = ctx._lib.r2f_jpeg_rows_begin_ex(ctx._h, H, W, _lib.JpegOpts(90, 0, 0, 1), out.data_ptr(), out.numel(), length.data_ptr(),
                                         ctx._stream())
    assert rc == -1
    assert proc.encode_jpeg(a, 90, progressive=True) == pillow_progressive(a, 90)
    assert proc.encode_jpeg(a, 90) == proc.encode_jpeg(a, 90, progressive=False) == pillow_jpeg(a, 90)
