"""The JPEG export on a real GPU: HipProcessor.encode_jpeg / process_jpeg / process_preloaded_jpeg write the bytes Pillow's
`Image.fromarray(a).save(f, "JPEG", quality=q)` writes (gui.py:2338-2341), with no tolerance."""

import io

import numpy as np
import pytest

import jpeg_extremes as jx
from helpers import SEED, stocks, synthetic_frame
from test_jpeg_host import QUALITIES, SIZES, contents, pillow_jpeg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def proc():
    from raw2film_amd import HipProcessor

    p = HipProcessor(cameras={}, lenses={}, device=0)
    yield p
    p.close()


def smooth(H, W):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    r = 127.5 + 127.5 * np.sin(xx / (W / 7.0)) * np.cos(yy / (H / 5.0))
    g = 255.0 * xx / max(W - 1, 1)
    b = 255.0 * (0.5 + 0.5 * np.cos((xx + yy) / (W / 3.0)))
    return np.stack([r, g, b], -1).astype(np.uint8)


@pytest.mark.parametrize("H,W", SIZES + ((1000, 1501),))
def test_encode_jpeg_writes_pillows_bytes(proc, H, W):
    for name, a in contents(H, W).items():
        for q in QUALITIES:
            assert proc.encode_jpeg(a, q) == pillow_jpeg(a, q), (name, q)


@pytest.mark.parametrize("H,W", jx.SIZES)
def test_encode_jpeg_extreme_coefficients(proc, H, W):
    """Category-11 DC differences in all three components and category-10 AC coefficients (tests/jpeg_extremes.py)."""
    for name, a in jx.frames(H, W).items():
        for q in jx.QUALITIES:
            assert proc.encode_jpeg(a, q) == pillow_jpeg(a, q), (name, q)


@pytest.mark.parametrize("H,W", ((4000, 6000), (12288, 8192)))
def test_encode_jpeg_full_size_frames(proc, H, W):
    rng = np.random.default_rng(H)
    for a in (rng.integers(0, 256, (H, W, 3), dtype=np.uint8), smooth(H, W)):
        for q in (100, 75):
            assert proc.encode_jpeg(a, q) == pillow_jpeg(a, q), q


def test_device_inputs_and_row_strided_views(proc):
    a = contents(257, 390)["noise"]
    dev = torch.from_numpy(a).cuda()
    want = pillow_jpeg(a, 90)
    assert proc.encode_jpeg(dev, 90) == want
    assert proc.encode_jpeg(torch.from_numpy(a), 90) == want  # a host tensor is uploaded
    # a crop of a wider frame: rows strided, pixels packed -- encoded in place
    wide = torch.zeros((300, 512, 3), dtype=torch.uint8, device="cuda")
    wide[10:267, 40:430] = dev
    view = wide[10:267, 40:430]
    assert not view.is_contiguous() and view.stride(1) == 3
    assert proc.encode_jpeg(view, 90) == want
    # every other column: not packed, made contiguous first
    assert proc.encode_jpeg(dev[:, ::2], 90) == pillow_jpeg(np.ascontiguousarray(a[:, ::2]), 90)


def test_alternating_sizes_stay_byte_exact(proc):
    frames = [contents(H, W, seed=3)["noise"] for H, W in ((1000, 1501), (17, 33), (1000, 1501), (256, 383), (31, 64))]
    for q in (100, 50):
        for a in frames:
            assert proc.encode_jpeg(a, q) == pillow_jpeg(a, q)


def test_process_jpeg_is_pillow_of_process(proc):
    neg, prt, _ = stocks()
    H, W, fw = 210, 333, 1.0
    img = synthetic_frame(H, W, seed=5)
    kw = dict(print_film=prt, frame_width=fw, frame_height=fw * H / W, halation_green_factor=0.3, exp_kelvin=6000,
              color_masking=1.0, profile="Default")  # (GUI extras are swallowed like process() swallows them)
    for s, q in ((SEED, 100), (SEED + 1, 85), (7, 0)):
        want = pillow_jpeg(proc.process(img, neg, 6, 0.4, seed=s, **kw), q)
        assert proc.process_jpeg(img, neg, 6, 0.4, quality=q, seed=s, **kw) == want, (s, q)
    # canvas and output resolution on the way (the uint8 post-path runs before the encoder)
    kw2 = dict(kw, canvas_mode="Proportional", canvas_scale=1.1, resolution=(180, 180))
    assert proc.process_jpeg(img, neg, 6, 0.4, seed=SEED, **kw2) == pillow_jpeg(proc.process(img, neg, 6, 0.4, seed=SEED, **kw2), 100)


def test_process_preloaded_jpeg_uint16_payload_with_canvas_and_resolution(proc):
    neg, prt, _ = stocks()
    rng = np.random.default_rng(11)
    raw = rng.integers(0, 65536, (240, 360, 3), dtype=np.uint16)
    kw = dict(print_film=prt, lens_correction=False, frame_width=36, frame_height=24, exposure=0.5, canvas_mode="Proportional",
              canvas_scale=1.1, resolution=(200, 200))
    pay = proc.extract_image_data_cpu(raw, **kw)
    assert pay["image_array"].dtype == np.uint16
    for q in (100, 60):
        want = pillow_jpeg(proc.process_preloaded(pay, neg, 6, 0.4, seed=SEED, final_scaling="cpu", **kw), q)
        assert proc.process_preloaded_jpeg(pay, neg, 6, 0.4, quality=q, seed=SEED, final_scaling="cpu", **kw) == want
    want = pillow_jpeg(proc.process_preloaded(pay, neg, 6, 0.4, seed=SEED, **kw), 100)
    assert proc.process_preloaded_jpeg(pay, neg, 6, 0.4, seed=SEED, **kw) == want


def test_a_preview_rerender_after_process_jpeg_uploads_nothing(proc):
    neg, prt, _ = stocks()
    img = synthetic_frame(200, 300, seed=9)
    base = dict(print_film=prt, frame_width=1.0, frame_height=200 / 300, halation_green_factor=0.3, exp_kelvin=6000, color_masking=1.0,
                seed=SEED)
    want = pillow_jpeg(proc.process(img, neg, 6, 0.4, cache=False, **base), 95)
    loads = []
    inner = proc.prepare_gpu_textures
    proc.prepare_gpu_textures = lambda p: (loads.append(1), inner(p))[1]
    try:
        pv = dict(base, resolution=(150, 150))
        p1 = proc.process(img, neg, 6, 0.4, **pv)
        assert loads == [1]
        assert proc.process_jpeg(img, neg, 6, 0.4, quality=95, **base) == want  # the export
        p2 = proc.process(img, neg, 6, 0.4, **pv)
        np.testing.assert_array_equal(p1, p2)
        assert loads == [1], "the preview's frame had to be uploaded again"
    finally:
        proc.prepare_gpu_textures = inner


def test_the_file_decodes(proc):
    Image = pytest.importorskip("PIL.Image")
    a = smooth(123, 457)
    back = np.asarray(Image.open(io.BytesIO(proc.encode_jpeg(a, 95))))
    assert back.shape == a.shape and np.abs(back.astype(int) - a.astype(int)).mean() < 3


def test_invalid_inputs_raise(proc):
    a = np.zeros((16, 16, 3), dtype=np.uint8)
    for bad in (101, -1, 50.0, True, "75", None):
        with pytest.raises(ValueError):
            proc.encode_jpeg(a, bad)
    for img in (np.zeros((16, 16, 3), np.float32), np.zeros((16, 16, 4), np.uint8), np.zeros((16, 16), np.uint8),
                np.zeros((0, 16, 3), np.uint8), np.zeros((16, 16, 1), np.uint8), torch.zeros((16, 16, 3), dtype=torch.int16).cuda(),
                [[[0, 0, 0]]]):
        with pytest.raises(ValueError):
            proc.encode_jpeg(img, 90)
    neg, prt, _ = stocks()
    img = synthetic_frame(32, 48, seed=1)
    tex = torch.zeros((32, 48, 4), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        proc.process_jpeg(img, neg, 6, 0.4, dst_texture=tex, print_film=prt)
    with pytest.raises(ValueError):
        proc.process_jpeg(img, neg, 6, 0.4, histogram_texture=tex, print_film=prt)
    with pytest.raises(ValueError):
        proc.process_jpeg(img, neg, 6, 0.4, quality=101, print_film=prt)
    pay = proc.extract_image_data_cpu(img, lens_correction=False)
    with pytest.raises(ValueError):
        proc.process_preloaded_jpeg(pay, neg, 6, 0.4, dst_texture=tex, print_film=prt)
    with pytest.raises(ValueError):
        proc.ctx.jpeg_encode(torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda"), 101)  # the library refuses it too


def test_a_scan_longer_than_2_to_the_32_bits(proc):
    # uniform noise at q100 takes ~15.8 bits per pixel: 335 MP is a 0.66 GB file, whose scan bit offsets pass 2^32 (64-bit offsets)
    H, W = 16384, 20480
    a = np.random.default_rng(32).integers(0, 256, (H, W, 3), dtype=np.uint8)
    want = pillow_jpeg(a, 100)
    assert 8 * len(want) > 1 << 32
    got = proc.encode_jpeg(a, 100)
    assert len(got) == len(want) and got == want


def test_closing_a_processor_frees_the_encoders_scratch():
    from raw2film_amd import HipProcessor

    frame = torch.zeros((8192, 12288, 3), dtype=torch.uint8, device="cuda")  # 100 MP: ~0.8 GB of scratch

    def cycle():
        p = HipProcessor(device=0)
        p.encode_jpeg(frame, 90)
        p.close()
        del p
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        return torch.cuda.mem_get_info()[0]

    free0 = cycle()  # (first use: code objects, torch's own pools)
    free1 = cycle()
    free2 = cycle()
    assert free2 >= free0 - (256 << 20) and free2 >= free1 - (256 << 20), (free0, free1, free2)
