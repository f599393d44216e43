"""The streamed JPEG export on a real GPU: process_jpeg / process_preloaded_jpeg with stream=True write, byte for byte, the file
Pillow writes for the pixels process(cache=False) / process_preloaded return -- band by band when the frame streams, in one piece
(with `stream_rejected` saying why) when it does not -- and the row-wise encoder of the context writes the one-shot encoder's file
for any 16-aligned split of a frame."""

import gc
import io

import numpy as np
import pytest

from helpers import stocks, synthetic_frame
from test_jpeg_host import pillow_jpeg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MARK = "not asked"  # stream_rejected before a call: a streamed call must leave None behind


@pytest.fixture(scope="module")
def proc():
    from raw2film_amd import HipProcessor

    p = HipProcessor(cameras={}, lenses={}, device=0)
    yield p
    p.close()


@pytest.fixture(scope="module")
def films():
    neg, prt, _ = stocks()
    return neg, prt


def frame_for(H, W):
    """frame_width / frame_height whose aspect crop keeps an H x W frame whole (geometry.crop_box: the longer side is matched), at
    most 341 px/mm like a 100 MP frame on 135 film (below `max_scale`, which would scale the render)."""
    from raw2film_amd.geometry import crop_box

    long_mm = max(36.0, max(H, W) / 341.0)
    for k in (0, 1, -1, 2, -2):
        a = max(H, W) / min(H, W) * (1 + k * 2.0 ** -52)
        fw, fh = long_mm, long_mm / a
        if crop_box(H, W, 1, fw / fh) == (0, 0, H, W):
            return dict(frame_width=fw, frame_height=fh)
    raise AssertionError((H, W))


def render_kw(prt, full, H, W):
    kw = dict(print_film=prt, lens_correction=False, seed=11, **frame_for(H, W))
    if full:  # halation, MTF and grain: the stencil stages' band calls
        return dict(kw, halation_green_factor=0.3, sharpening_strength=0.5, grain=2)
    return dict(kw, halation=False, sharpness=False, grain=0)  # LUTs only: the fused pointwise band path


def streamed(proc, fn, *a, **kw):
    proc.stream_rejected = MARK
    out = fn(*a, stream=True, **kw)
    assert proc.stream_rejected is None, proc.stream_rejected
    return out


# (H, W): H mod 16 in {0, 1, 15}, W mod 16 in {0, 1, 8}; stream_bands with the default taper; the LUT-only and the full render
CASES = [
    ((2416, 2400), 3, False, 100),
    ((2417, 2401), 5, True, 75),
    ((8207, 720), 16, True, 95),
    ((20497, 280), 40, False, 1),
    ((20480, 289), 40, True, 100),
]


@pytest.mark.parametrize("shape,bands,full,q", CASES)
def test_streamed_export_is_pillow_of_the_streamed_render(proc, films, shape, bands, full, q):
    neg, prt = films
    H, W = shape
    img = synthetic_frame(H, W, seed=H + W)
    kw = render_kw(prt, full, H, W)
    proc.stream_bands = bands
    try:
        proc.stream_rejected = MARK
        px = proc.process(img, neg, 6, 0.4, cache=False, **kw)
        assert proc.stream_rejected is None  # (the pixels themselves come through the bands)
        want = pillow_jpeg(px, q)
        assert streamed(proc, proc.process_jpeg, img, neg, 6, 0.4, quality=q, **kw) == want
    finally:
        proc.stream_bands = 16


def test_streamed_export_at_100_mp(proc, films):
    from raw2film_amd.synthetic import synthetic_frame_device

    neg, prt = films
    img = synthetic_frame_device(8192, 12288, seed=3, kind="smooth").cpu().numpy()
    kw = render_kw(prt, True, 8192, 12288)
    want = pillow_jpeg(proc.process(img, neg, 6, 0.4, cache=False, **kw), 100)
    assert streamed(proc, proc.process_jpeg, img, neg, 6, 0.4, quality=100, **kw) == want


def test_streamed_payload_exports(proc, films):
    neg, prt = films
    H, W = 2417, 2408
    kw = render_kw(prt, True, H, W)
    pre = {k: v for k, v in kw.items() if k not in ("lens_correction", "frame_width", "frame_height")}
    img = synthetic_frame(H, W, seed=4)
    raw = np.random.default_rng(5).integers(0, 65536, (H, W, 3), dtype=np.uint16)
    pay_f = proc.extract_image_data_cpu(img, lens_correction=False, **frame_for(H, W))  # with the alpha plane
    pay_u = proc.extract_image_data_cpu(raw, lens_correction=False, exposure=0.5, **frame_for(H, W))
    assert pay_f["image_array"].shape[2] == 4 and pay_u["image_array"].dtype == np.uint16
    pinned = dict(pay_f, image_array=torch.from_numpy(np.ascontiguousarray(pay_f["image_array"])).pin_memory())
    for name, pay, q in (("float32 + alpha, pageable", pay_f, 95), ("uint16", pay_u, 100), ("float32, pinned", pinned, 75)):
        proc.stream_rejected = MARK
        px = proc.process_preloaded(pay, neg, 6, 0.4, **pre)
        assert proc.stream_rejected is None, name
        got = streamed(proc, proc.process_preloaded_jpeg, pay, neg, 6, 0.4, quality=q, **pre)
        assert got == pillow_jpeg(px, q), name


def test_frames_that_do_not_stream_fall_back(proc, films, tmp_path):
    neg, prt = films
    kw = render_kw(prt, True, 2400, 2400)
    big = synthetic_frame(2400, 2400, seed=6)
    small = synthetic_frame(300, 451, seed=7)
    path = str(tmp_path / "frame.npy")
    np.save(path, small)
    cases = [
        ("small frame", small, {}),
        ("a .npy path", path, {}),
        ("rotation", big, dict(rotation=2.5)),
        ("canvas", big, dict(canvas_mode="Proportional", canvas_scale=1.1)),
        ("highlight burn", big, dict(highlight_burn=0.5)),
    ]
    for name, src, extra in cases:
        want = pillow_jpeg(proc.process(src, neg, 6, 0.4, cache=False, **kw, **extra), 90)
        proc.stream_rejected = MARK
        got = proc.process_jpeg(src, neg, 6, 0.4, quality=90, stream=True, **kw, **extra)
        assert got == want, name
        assert isinstance(proc.stream_rejected, str) and proc.stream_rejected and proc.stream_rejected != MARK, name
    proc.stream_bands = 0
    try:
        want = pillow_jpeg(proc.process(big, neg, 6, 0.4, cache=False, **kw), 90)
        proc.stream_rejected = MARK
        assert proc.process_jpeg(big, neg, 6, 0.4, quality=90, stream=True, **kw) == want
        assert "stream_bands" in proc.stream_rejected
        pay = proc.extract_image_data_cpu(big, lens_correction=False, **frame_for(2400, 2400))
        pre = {k: v for k, v in kw.items() if k not in ("lens_correction", "frame_width", "frame_height")}
        want = pillow_jpeg(proc.process_preloaded(pay, neg, 6, 0.4, **pre), 90)
        proc.stream_rejected = MARK
        assert proc.process_preloaded_jpeg(pay, neg, 6, 0.4, quality=90, stream=True, **pre) == want
        assert "stream_bands" in proc.stream_rejected
    finally:
        proc.stream_bands = 16


class FailingWriter(io.RawIOBase):
    def __init__(self, after):
        self.after, self.calls = after, 0

    def writable(self):
        return True

    def write(self, b):
        self.calls += 1
        if self.calls > self.after:
            raise OSError("disk full")
        return len(b)


def test_file_outputs_and_a_failing_writer(proc, films, tmp_path):
    neg, prt = films
    kw = render_kw(prt, True, 4000, 3000)
    img = synthetic_frame(4000, 3000, seed=8)  # (at q 100 a file of ~17 MB, in several writes)
    want = pillow_jpeg(proc.process(img, neg, 6, 0.4, cache=False, **kw), 100)
    assert streamed(proc, proc.process_jpeg, img, neg, 6, 0.4, quality=100, **kw) == want
    path = tmp_path / "out.jpg"
    assert streamed(proc, proc.process_jpeg, img, neg, 6, 0.4, quality=100, file=str(path), **kw) == len(want)
    assert path.read_bytes() == want
    buf = io.BytesIO()
    assert streamed(proc, proc.process_jpeg, img, neg, 6, 0.4, quality=100, file=buf, **kw) == len(want)
    assert buf.getvalue() == want
    # the one-piece path writes a file too
    assert proc.process_jpeg(img, neg, 6, 0.4, quality=100, file=tmp_path / "one.jpg", **kw) == len(proc.process_jpeg(
        img, neg, 6, 0.4, quality=100, **kw))
    bad = FailingWriter(after=2)
    with pytest.raises(OSError, match="disk full"):
        proc.process_jpeg(img, neg, 6, 0.4, quality=100, stream=True, file=bad, **kw)
    assert bad.calls == 3  # (nothing is written after the failure)
    assert streamed(proc, proc.process_jpeg, img, neg, 6, 0.4, quality=100, **kw) == want  # the next export is still exact


def test_interleaved_exports_encodes_and_previews(proc, films):
    neg, prt = films
    kw = render_kw(prt, True, 2400, 2416)
    kw2 = render_kw(prt, True, 2416, 2401)
    img = synthetic_frame(2400, 2416, seed=10)
    img2 = synthetic_frame(2416, 2401, seed=12)
    other = np.random.default_rng(3).integers(0, 256, (517, 333, 3), dtype=np.uint8)
    want1 = pillow_jpeg(proc.process(img, neg, 6, 0.4, cache=False, **kw), 95)
    want2 = pillow_jpeg(proc.process(img2, neg, 6, 0.4, cache=False, **kw2), 85)
    loads = []
    inner = proc.prepare_gpu_textures
    proc.prepare_gpu_textures = lambda p: (loads.append(1), inner(p))[1]
    try:
        pv = dict(kw, resolution=(300, 300))
        p1 = proc.process(img, neg, 6, 0.4, **pv)
        assert loads == [1]
        assert streamed(proc, proc.process_jpeg, img, neg, 6, 0.4, quality=95, **kw) == want1
        assert proc.encode_jpeg(other, 60) == pillow_jpeg(other, 60)
        p2 = proc.process(img, neg, 6, 0.4, **pv)
        np.testing.assert_array_equal(p1, p2)
        assert streamed(proc, proc.process_jpeg, img2, neg, 6, 0.4, quality=85, **kw2) == want2
        p3 = proc.process(img, neg, 6, 0.4, **pv)
        np.testing.assert_array_equal(p1, p3)
        assert loads == [1], "the preview's frame had to be uploaded again"
    finally:
        proc.prepare_gpu_textures = inner


def rows_encode(ctx, dev, q, ends):
    enc = ctx.jpeg_rows(dev.shape[0], dev.shape[1], q)
    y0, finals = 0, []
    for y1 in ends:
        enc.rows(dev, y0, y1)
        finals.append(int(enc.length.item()))
        y0 = y1
    assert enc.done
    return bytes(enc.out[:finals[-1]].cpu().numpy()), finals


def oneshot(ctx, dev, q):
    out, n = ctx.jpeg_encode(dev, q)
    return bytes(out[:int(n.item())].cpu().numpy())


def random_ends(rng, H):
    ends, y = [], 0
    while y < H:
        y = min(y + 16 * int(rng.choice([1, 1, 2, 3, 17, 64])), H)
        ends.append(y)
    return ends


def test_context_rows_match_the_one_shot_encoder(proc):
    ctx = proc.ctx
    rng = np.random.default_rng(21)
    for H, W in ((16, 16), (1, 1), (17, 33), (255, 383), (1000, 1501), (1040, 1024)):
        a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        a[: H // 2] //= 64  # (some long zero runs too)
        dev = torch.from_numpy(a).cuda()
        for q in (1, 75, 100):
            want = oneshot(ctx, dev, q)
            assert want == pillow_jpeg(a, q)
            for ends in ([H], list(range(16, H, 16)) + [H], random_ends(rng, H)):
                got, finals = rows_encode(ctx, dev, q, ends)
                assert got == want, (H, W, q, ends[:5])
                assert finals == sorted(finals) and finals[-1] == len(want)
                # every final byte reported after a call is the file's
                assert all(f <= len(want) for f in finals)
    # a row-strided view, rows split
    wide = torch.zeros((300, 512, 3), dtype=torch.uint8, device="cuda")
    wide[10:267, 40:430] = torch.from_numpy(rng.integers(0, 256, (257, 390, 3), dtype=np.uint8)).cuda()
    view = wide[10:267, 40:430]
    assert rows_encode(ctx, view, 90, [16, 48, 257])[0] == oneshot(ctx, view.contiguous(), 90)


def test_context_rows_refusals_leave_the_context_usable(proc):
    ctx = proc.ctx
    a = np.random.default_rng(1).integers(0, 256, (100, 70, 3), dtype=np.uint8)
    dev = torch.from_numpy(a).cuda()
    want = oneshot(ctx, dev, 80)
    enc = ctx.jpeg_rows(100, 70, 80)
    for y0, y1 in ((16, 32), (0, 17), (0, 0), (0, 101), (-16, 16)):
        with pytest.raises(ValueError):
            enc.rows(dev, y0, y1)
    enc.rows(dev, 0, 32)  # (the refusals left the encode where it was)
    with pytest.raises(ValueError):
        enc.rows(dev, 0, 48)  # out of order
    with pytest.raises(ValueError):
        enc.rows(torch.zeros((100, 71, 3), dtype=torch.uint8, device="cuda"), 32, 48)  # another frame
    assert oneshot(ctx, dev, 80) == want  # a one-shot encode in the middle ends the open one ...
    with pytest.raises(ValueError):
        enc.rows(dev, 32, 48)
    got, _ = rows_encode(ctx, dev, 80, [32, 96, 100])  # ... and the context goes on
    assert got == want
    enc = ctx.jpeg_rows(100, 70, 80)
    enc.rows(dev, 0, 48)
    got, _ = rows_encode(ctx, dev, 80, [64, 100])  # a new begin ends an open encode too
    assert got == want
    with pytest.raises(ValueError):
        enc.rows(dev, 48, 100)
    with pytest.raises(ValueError):
        ctx.jpeg_rows(100, 70, 101)
    with pytest.raises(ValueError):
        ctx.jpeg_rows(0, 70, 80)


def test_context_rows_past_2_to_the_32_bits(proc):
    # uniform noise at q100: ~15.8 bits per pixel, so a 335 MP scan passes bit 2^32 -- split at every MCU row, one split falls
    # right after it
    ctx = proc.ctx
    H, W = 16384, 20480
    g = torch.Generator(device="cuda")
    g.manual_seed(32)
    dev = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    want = oneshot(ctx, dev, 100)
    assert 8 * len(want) > 1 << 32
    got, finals = rows_encode(ctx, dev, 100, list(range(16, H + 1, 16)))
    assert len(got) == len(want) and got == want
    assert any(8 * f < 1 << 32 for f in finals) and any(8 * f > 1 << 32 for f in finals)
    del dev
    gc.collect()
    torch.cuda.empty_cache()


def test_closing_a_processor_frees_the_export_staging(films):
    from raw2film_amd import HipProcessor

    neg, prt = films
    p = HipProcessor(device=0)
    img = synthetic_frame(2400, 2400, seed=13)
    kw = render_kw(prt, False, 2400, 2400)
    want = pillow_jpeg(p.process(img, neg, 6, 0.4, cache=False, **kw), 90)
    assert streamed(p, p.process_jpeg, img, neg, 6, 0.4, quality=90, **kw) == want
    staging = p._jpeg_staging
    assert staging is not None and staging.ring is not None
    p.close()
    assert p._jpeg_staging is None and staging.ring is None and staging.lens is None
    assert staging.fetcher._shutdown and staging.writer._shutdown
