"""The JPEG export's subsampling / optimize / exif options on a real GPU: encode_jpeg, process_jpeg and process_preloaded_jpeg
write the bytes Pillow's `save(f, "JPEG", quality=q, subsampling=s, optimize=o, exif=e)` writes, with no tolerance."""

import gc

import numpy as np
import pytest

import jpeg_extremes as jx
from helpers import SEED, stocks, synthetic_frame
from test_gpu_jpeg import smooth
from test_gpu_jpeg_stream import MARK, render_kw, streamed
from test_jpeg_host import SIZES, contents
from test_jpeg_options_host import EXIF, pillow_jpeg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

OPTIONS = [(s, o) for s in (0, 1, 2) for o in (False, True)]


@pytest.fixture(scope="module")
def proc():
    from raw2film_amd import HipProcessor

    p = HipProcessor(cameras={}, lenses={}, device=0)
    yield p
    p.close()


@pytest.mark.parametrize("H,W", SIZES + ((1000, 1501),))
def test_encode_jpeg_options_write_pillows_bytes(proc, H, W):
    for name, a in contents(H, W).items():
        for q in (1, 50, 100):
            for s, o in OPTIONS:
                e = EXIF if (q + s) % 2 else b""
                got = proc.encode_jpeg(a, q, subsampling=s, optimize=o, exif=e)
                assert got == pillow_jpeg(a, q, s, o, e), (name, q, s, o)


@pytest.mark.parametrize("H,W", jx.SIZES)
def test_encode_jpeg_options_extreme_coefficients(proc, H, W):
    """tests/jpeg_extremes.py through every sampling, with the standard and the optimized tables: in 4:4:4 and 4:2:2 the 8 x 8
    colour checker keeps its chroma swing, and optimize has to build codes for the categories no other frame uses."""
    for name, a in jx.frames(H, W).items():
        for q in jx.QUALITIES:
            for s, o in OPTIONS:
                assert proc.encode_jpeg(a, q, subsampling=s, optimize=o) == pillow_jpeg(a, q, s, o), (name, q, s, o)


@pytest.mark.parametrize("H,W", ((4000, 6000), (12288, 8192)))
def test_encode_jpeg_options_full_size_frames(proc, H, W):
    rng = np.random.default_rng(H + 1)
    for a in (rng.integers(0, 256, (H, W, 3), dtype=np.uint8), smooth(H, W)):
        for s, o in ((0, False), (1, True), (0, True), (2, True)):
            assert proc.encode_jpeg(a, 100, subsampling=s, optimize=o) == pillow_jpeg(a, 100, s, o), (s, o)


def test_string_values_device_inputs_and_row_strided_views(proc):
    a = contents(257, 390)["noise"]
    dev = torch.from_numpy(a).cuda()
    wide = torch.zeros((300, 512, 3), dtype=torch.uint8, device="cuda")
    wide[10:267, 40:430] = dev
    view = wide[10:267, 40:430]
    for s, name in ((0, "4:4:4"), (1, "4:2:2"), (2, "4:2:0")):
        for o in (False, True):
            want = pillow_jpeg(a, 90, s, o)
            assert proc.encode_jpeg(dev, 90, subsampling=name, optimize=o) == want
            assert proc.encode_jpeg(view, 90, subsampling=s, optimize=int(o)) == want
    assert proc.encode_jpeg(a, 90, subsampling=-1) == pillow_jpeg(a, 90)


def test_pil_exif_object(proc):
    Image = pytest.importorskip("PIL.Image")
    exif = Image.Exif()
    exif[0x010F] = "raw2film"
    exif[0x0131] = "raw2film_amd"
    a = smooth(123, 457)
    assert proc.encode_jpeg(a, 95, subsampling=0, optimize=True, exif=exif) == pillow_jpeg(a, 95, 0, True, exif.tobytes())


def test_process_jpeg_options_are_pillow_of_process(proc):
    neg, prt, _ = stocks()
    H, W, fw = 210, 333, 1.0
    img = synthetic_frame(H, W, seed=5)
    kw = dict(print_film=prt, frame_width=fw, frame_height=fw * H / W, halation_green_factor=0.3, exp_kelvin=6000,
              color_masking=1.0, seed=SEED)
    px = proc.process(img, neg, 6, 0.4, **kw)
    for s, o in OPTIONS:
        got = proc.process_jpeg(img, neg, 6, 0.4, quality=97, subsampling=s, optimize=o, exif=EXIF, **kw)
        assert got == pillow_jpeg(px, 97, s, o, EXIF), (s, o)
    pay = proc.extract_image_data_cpu(img, lens_correction=False, frame_width=fw, frame_height=fw * H / W)
    pre = dict(print_film=prt, halation_green_factor=0.3, exp_kelvin=6000, color_masking=1.0, seed=SEED)
    px = proc.process_preloaded(pay, neg, 6, 0.4, final_scaling="cpu", **pre)
    for s, o in ((0, True), (1, False)):
        got = proc.process_preloaded_jpeg(pay, neg, 6, 0.4, quality=100, final_scaling="cpu", subsampling=s, optimize=o, **pre)
        assert got == pillow_jpeg(px, 100, s, o), (s, o)


# (H, W): H mod 8 in {0, 1, 7}; several stream_bands; 4:4:4 and 4:2:2, with and without exif
STREAM_CASES = [
    ((2416, 2400), 3, 0, b""),
    ((2417, 2401), 5, 1, EXIF),
    ((8207, 720), 16, 0, EXIF),
    ((8199, 721), 40, 1, b""),
]


@pytest.mark.parametrize("shape,bands,s,e", STREAM_CASES)
def test_streamed_export_options_are_pillow_of_the_streamed_render(proc, shape, bands, s, e, tmp_path):
    neg, prt, _ = stocks()
    H, W = shape
    img = synthetic_frame(H, W, seed=H + W)
    kw = render_kw(prt, bands % 2 == 1, H, W)
    proc.stream_bands = bands
    try:
        proc.stream_rejected = MARK
        px = proc.process(img, neg, 6, 0.4, cache=False, **kw)
        assert proc.stream_rejected is None
        want = pillow_jpeg(px, 95, s, False, e)
        assert streamed(proc, proc.process_jpeg, img, neg, 6, 0.4, quality=95, subsampling=s, exif=e, **kw) == want
        path = tmp_path / "out.jpg"
        n = streamed(proc, proc.process_jpeg, img, neg, 6, 0.4, quality=95, file=str(path), subsampling=s, exif=e, **kw)
        assert n == len(want) and path.read_bytes() == want
    finally:
        proc.stream_bands = 16


def test_streamed_payload_export_options(proc):
    neg, prt, _ = stocks()
    H, W = 2417, 2408
    kw = render_kw(prt, True, H, W)
    pre = {k: v for k, v in kw.items() if k not in ("lens_correction", "frame_width", "frame_height")}
    img = synthetic_frame(H, W, seed=4)
    pay = proc.extract_image_data_cpu(img, lens_correction=False, frame_width=kw["frame_width"], frame_height=kw["frame_height"])
    px = proc.process_preloaded(pay, neg, 6, 0.4, **pre)
    got = streamed(proc, proc.process_preloaded_jpeg, pay, neg, 6, 0.4, quality=90, subsampling="4:2:2", exif=EXIF, **pre)
    assert got == pillow_jpeg(px, 90, 1, False, EXIF)


def test_optimize_with_stream_falls_back(proc):
    neg, prt, _ = stocks()
    H, W = 2416, 2400
    img = synthetic_frame(H, W, seed=9)
    kw = render_kw(prt, False, H, W)
    px = proc.process(img, neg, 6, 0.4, cache=False, **kw)
    proc.stream_rejected = MARK
    got = proc.process_jpeg(img, neg, 6, 0.4, quality=95, stream=True, subsampling=0, optimize=True, **kw)
    assert "optimize" in proc.stream_rejected
    assert got == pillow_jpeg(px, 95, 0, True)
    pay = proc.extract_image_data_cpu(img, lens_correction=False, frame_width=kw["frame_width"], frame_height=kw["frame_height"])
    pre = {k: v for k, v in kw.items() if k not in ("lens_correction", "frame_width", "frame_height")}
    proc.stream_rejected = MARK
    got = proc.process_preloaded_jpeg(pay, neg, 6, 0.4, quality=95, stream=True, optimize=True, **pre)
    assert "optimize" in proc.stream_rejected
    assert got == pillow_jpeg(proc.process_preloaded(pay, neg, 6, 0.4, **pre), 95, -1, True)


def test_invalid_options_raise_and_leave_the_processor_usable(proc):
    a = contents(31, 64)["noise"]
    neg, prt, _ = stocks()
    img = synthetic_frame(32, 48, seed=1)
    for bad in (dict(subsampling="keep"), dict(subsampling="4:1:1"), dict(subsampling=3), dict(subsampling=True),
                dict(exif=b"x" * 65534), dict(exif="text")):
        with pytest.raises(ValueError):
            proc.encode_jpeg(a, 90, **bad)
        with pytest.raises(ValueError):
            proc.process_jpeg(img, neg, 6, 0.4, print_film=prt, **bad)
    from raw2film_amd import _lib

    ctx = proc.ctx
    out = torch.empty(ctx.jpeg_bound_bytes(8, 8, 0), dtype=torch.uint8, device="cuda")
    length = torch.empty(1, dtype=torch.int64, device="cuda")
    frame = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    for opts in (_lib.JpegOpts(90, 3, 0, 0), _lib.JpegOpts(90, 0, 2, 0), _lib.JpegOpts(90, 0, 0, 1)):
        rc = ctx._lib.r2f_jpeg_encode_ex(ctx._h, frame.data_ptr(), 8, 8, 24, opts, out.data_ptr(), out.numel(), length.data_ptr(),
                                         ctx._stream())
        assert rc == -1  # R2F_EINVAL
    with pytest.raises(Exception):  # (the row-wise encoder refuses optimize)
        rc = ctx._lib.r2f_jpeg_rows_begin_ex(ctx._h, 8, 8, _lib.JpegOpts(90, 0, 1, 0), out.data_ptr(), out.numel(),
                                             length.data_ptr(), ctx._stream())
        ctx._check(rc)
    with pytest.raises(Exception):  # 4:4:4 rows must end on multiples of 8
        enc = ctx.jpeg_rows(24, 8, 90, 0)
        enc.rows(torch.zeros((24, 8, 3), dtype=torch.uint8, device="cuda"), 0, 12)
    assert proc.encode_jpeg(a, 90, subsampling=0, optimize=True) == pillow_jpeg(a, 90, 0, True)
    assert proc.encode_jpeg(a, 90) == pillow_jpeg(a, 90)


def test_context_rows_in_8_row_mcus_match_the_one_shot_encoder(proc):
    ctx = proc.ctx
    a = contents(257, 390)["gradient"]
    dev = torch.from_numpy(a).cuda()
    for s in (0, 1):
        want = pillow_jpeg(a, 85, s)
        enc = ctx.jpeg_rows(257, 390, 85, s)
        for y0, y1 in ((0, 8), (8, 136), (136, 256), (256, 257)):
            enc.rows(dev, y0, y1)
        n = int(enc.length.item())
        assert enc.done and enc.out[:n].cpu().numpy().tobytes() == want


def test_a_444_scan_longer_than_2_to_the_32_bits(proc):
    # uniform noise at q100 in 4:4:4 takes ~4.1 bytes per pixel: 151 MP is a 0.62 GB file, whose scan bit offsets pass 2^32
    H, W = 12288, 12288
    a = np.random.default_rng(44).integers(0, 256, (H, W, 3), dtype=np.uint8)
    want = pillow_jpeg(a, 100, 0)
    assert 8 * len(want) > 1 << 32
    got = proc.encode_jpeg(a, 100, subsampling=0)
    assert len(got) == len(want) and got == want
    del a, got, want
    gc.collect()


def test_closing_a_processor_frees_the_444_scratch():
    from raw2film_amd import HipProcessor

    frame = torch.zeros((8192, 12288, 3), dtype=torch.uint8, device="cuda")  # 100 MP in 4:4:4: ~1.6 GB of scratch

    def cycle():
        p = HipProcessor(device=0)
        p.encode_jpeg(frame, 90, subsampling=0, optimize=True)
        p.close()
        del p
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        return torch.cuda.mem_get_info()[0]

    free0 = cycle()
    free1 = cycle()
    free2 = cycle()
    assert free2 >= free0 - (256 << 20) and free2 >= free1 - (256 << 20), (free0, free1, free2)
