"""The JPEG export's restart markers, ICC profile, XMP, comment and dpi on a real GPU: encode_jpeg, the row-wise encoder, the
streamed export, process_jpeg and process_preloaded_jpeg write the bytes Pillow's save() writes for the same options, with no
tolerance."""

import ctypes as C

import numpy as np
import pytest

import jpeg_extremes as jx
from arena import Arena
from helpers import SEED, stocks, synthetic_frame
from test_gpu_jpeg_options import STREAM_CASES
from test_gpu_jpeg_stream import MARK, render_kw, streamed
from test_jpeg_options_host import EXIF
from test_jpeg_restart_host import COMMENT, DPI, ICC, METADATA, XMP, noise, pillow_save, scene

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def proc():
    from raw2film_amd import HipProcessor

    p = HipProcessor(cameras={}, lenses={}, device=0)
    yield p
    p.close()


def interval_of(W, s, blocks=0, rows=0):
    return min(rows * -(-W // (8 if s == 0 else 16)), 65535) if rows > 0 else blocks


def marker_positions(f):
    """(RSTn markers of a file's scan, those directly behind a stuffed 0xFF): a marker byte pair can only be FF D0 .. D7 in the
    stuffed scan, where every data 0xFF is followed by 0x00."""
    scan = np.frombuffer(f, np.uint8)[f.index(b"\xff\xda") + 14:]
    at = np.flatnonzero((scan[:-1] == 0xFF) & (scan[1:] >= 0xD0) & (scan[1:] <= 0xD7))
    behind = at[(at >= 2) & (scan[at - 2] == 0xFF) & (scan[at - 1] == 0x00)]
    return scan[at + 1], behind


@pytest.mark.parametrize("H,W", ((40, 56), (50, 70)))
def test_encode_jpeg_restart_intervals_write_pillows_bytes(proc, H, W):
    for a, q in ((noise(H, W), 90), (scene(H, W), 75)):
        dev = torch.from_numpy(a).cuda()
        for s in (0, 1, 2):
            for o in (False, True):
                for blocks in (1, 3, 5, 11, 12):
                    for rows in (0, 1, 2):
                        got = proc.encode_jpeg(dev, q, subsampling=s, optimize=o, restart_marker_blocks=blocks, restart_marker_rows=rows)
                        want = pillow_save(a, q, s, o, restart_marker_blocks=blocks, restart_marker_rows=rows)
                        assert got == want, (s, o, blocks, rows)


@pytest.mark.parametrize("H,W", jx.SIZES)
def test_encode_jpeg_restart_extreme_coefficients(proc, H, W):
    """tests/jpeg_extremes.py with an interval of three MCUs: category-11 DC differences inside an interval, and the predictor
    reset right behind a DC at the end of its range."""
    for name, a in jx.frames(H, W).items():
        for q in jx.QUALITIES:
            for s in (0, 1, 2):
                for o in (False, True):
                    got = proc.encode_jpeg(a, q, subsampling=s, optimize=o, restart_marker_blocks=3)
                    assert got == pillow_save(a, q, s, o, restart_marker_blocks=3), (name, q, s, o)


def test_one_mcu_gets_a_dri_and_no_marker(proc):
    a = scene(8, 8)
    for o in (False, True):
        got = proc.encode_jpeg(a, 90, subsampling=0, optimize=o, restart_marker_blocks=1)
        assert got == pillow_save(a, 90, 0, o, restart_marker_blocks=1)
        assert b"\xff\xdd\x00\x04\x00\x01" in got and len(marker_positions(got)[0]) == 0


@pytest.mark.parametrize("q", (90, 100))
def test_an_interval_per_mcu_of_noise(proc, q):
    """(264, 264): 1089 intervals in 4:4:4 -- more than one scan block holds, RSTn wraps 136 times, the scan spans many stuffing
    chunks -- and uniform noise puts stuffed 0xFF bytes directly in front of markers."""
    a = noise(264, 264, seed=q)
    for s, n_mcus in ((0, 1089), (1, 561), (2, 289)):
        want = pillow_save(a, q, s, restart_marker_blocks=1)
        marks, behind = marker_positions(want)
        assert len(behind) >= 1, "precondition: Pillow's file holds FF 00 FF Dn"
        assert len(marks) == n_mcus - 1 and (marks == 0xD0 + np.arange(n_mcus - 1) % 8).all()
        for o in (False, True):
            got = proc.encode_jpeg(a, q, subsampling=s, optimize=o, restart_marker_blocks=1)
            assert got == (pillow_save(a, q, s, True, restart_marker_blocks=1) if o else want), (s, o)


def test_rows_in_bands_of_one_mcu_row_straddle_every_interval(proc):
    ctx = proc.ctx
    H, W, q, interval = 40, 56, 90, 5
    a = noise(H, W)
    dev = torch.from_numpy(a).cuda()
    for s, per_row, mh in ((2, 4, 16), (0, 7, 8), (1, 4, 8)):
        assert -(-W // (8 if s == 0 else 16)) == per_row and per_row % interval
        want = pillow_save(a, q, s, restart_marker_blocks=interval, dpi=DPI)
        out, n = ctx.jpeg_encode(dev, q, s, restart=interval, density=(300, 73))
        assert out[:int(n.item())].cpu().numpy().tobytes() == want
        enc = ctx.jpeg_rows(H, W, q, s, interval, (300, 73))
        lengths = [int(enc.length.item())]
        assert lengths[0] == 629 and enc.out[:629].cpu().numpy().tobytes() == want[:629]
        for y0 in range(0, H, mh):
            enc.rows(dev, y0, min(y0 + mh, H))
            lengths.append(int(enc.length.item()))
            assert enc.out[:lengths[-1]].cpu().numpy().tobytes() == want[:lengths[-1]], (s, y0)
        assert enc.done and lengths == sorted(lengths) and lengths[-1] == len(want)


def test_streamed_export_with_restart_rows_and_metadata(proc, tmp_path):
    shape, bands, s, _ = min(STREAM_CASES, key=lambda c: (c[0][0] * c[0][1], c[1]))
    neg, prt, _ = stocks()
    H, W = shape
    img = synthetic_frame(H, W, seed=H + W)
    kw = render_kw(prt, bands % 2 == 1, H, W)
    options = dict(restart_marker_rows=1, exif=EXIF, **METADATA)
    proc.stream_bands = bands
    try:
        proc.stream_rejected = MARK
        px = proc.process(img, neg, 6, 0.4, cache=False, **kw)
        assert proc.stream_rejected is None
        want = pillow_save(px, 95, s, **options)
        assert streamed(proc, proc.process_jpeg, img, neg, 6, 0.4, quality=95, subsampling=s, **options, **kw) == want
        path = tmp_path / "out.jpg"
        n = streamed(proc, proc.process_jpeg, img, neg, 6, 0.4, quality=95, file=str(path), subsampling=s, **options, **kw)
        assert n == len(want) and path.read_bytes() == want
    finally:
        proc.stream_bands = 16


def test_process_jpeg_with_all_six_options_is_pillow_of_process(proc):
    neg, prt, _ = stocks()
    H, W, fw = 210, 333, 1.0
    img = synthetic_frame(H, W, seed=5)
    kw = dict(print_film=prt, frame_width=fw, frame_height=fw * H / W, halation_green_factor=0.3, exp_kelvin=6000,
              color_masking=1.0, seed=SEED)
    options = dict(restart_marker_blocks=7, restart_marker_rows=2, **METADATA)
    px = proc.process(img, neg, 6, 0.4, **kw)
    for s, o in ((0, False), (1, True), (2, False)):
        got = proc.process_jpeg(img, neg, 6, 0.4, quality=97, subsampling=s, optimize=o, exif=EXIF, **options, **kw)
        assert got == pillow_save(px, 97, s, o, exif=EXIF, **options), (s, o)
    pay = proc.extract_image_data_cpu(img, lens_correction=False, frame_width=fw, frame_height=fw * H / W)
    pre = dict(print_film=prt, halation_green_factor=0.3, exp_kelvin=6000, color_masking=1.0, seed=SEED)
    px = proc.process_preloaded(pay, neg, 6, 0.4, final_scaling="cpu", **pre)
    for s, o in ((0, True), (2, False)):
        got = proc.process_preloaded_jpeg(pay, neg, 6, 0.4, quality=100, final_scaling="cpu", subsampling=s, optimize=o, **options, **pre)
        assert got == pillow_save(px, 100, s, o, **options), (s, o)


def test_progressive_takes_the_metadata_and_refuses_restart_intervals(proc):
    from raw2film_amd import _lib

    a = scene(50, 70)
    for s in (0, 2):
        got = proc.encode_jpeg(a, 85, subsampling=s, progressive=True, exif=EXIF, **METADATA)
        assert got == pillow_save(a, 85, s, progressive=True, exif=EXIF, **METADATA)
    neg, prt, _ = stocks()
    img = synthetic_frame(64, 96, seed=2)
    kw = dict(print_film=prt, seed=SEED)
    before = proc.process(img, neg, 6, 0.4, **kw)
    for bad in (dict(restart_marker_blocks=3), dict(restart_marker_rows=1)):
        with pytest.raises(ValueError, match="progressive.*restart_marker"):
            proc.encode_jpeg(a, 85, progressive=True, **bad)
        with pytest.raises(ValueError, match="progressive.*restart_marker"):
            proc.process_jpeg(img, neg, 6, 0.4, progressive=True, print_film=prt, **bad)
    ctx = proc.ctx
    bound = ctx.jpeg_bound_bytes_opts(8, 8, 90, 0, False, True)
    out = torch.empty(bound, dtype=torch.uint8, device="cuda")
    length = torch.empty(1, dtype=torch.int64, device="cuda")
    frame = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    for opts in (_lib.JpegOpts(90, 0, 0, 1, 3), _lib.JpegOpts(90, 0, 0, 0, 65536), _lib.JpegOpts(90, 0, 0, 0, -1),
                 _lib.JpegOpts(90, 0, 0, 0, 0, 65536, 1)):
        rc = ctx._lib.r2f_jpeg_encode_ex(ctx._h, frame.data_ptr(), 8, 8, 24, C.byref(opts), out.data_ptr(), bound, length.data_ptr(),
                                         ctx._stream())
        assert rc == -1  # R2F_EINVAL
    assert np.array_equal(proc.process(img, neg, 6, 0.4, **kw), before)  # the next frame renders as before
    assert proc.encode_jpeg(a, 85, restart_marker_rows=1) == pillow_save(a, 85, restart_marker_rows=1)


def test_a_24_mp_frame_with_an_interval_per_mcu_row(proc):
    H, W = 4000, 6000
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    a = np.stack([127.5 + 127.5 * np.sin(xx / 37.0) * np.cos(yy / 29.0), 255.0 * xx / (W - 1), 128 + 127 * np.cos((xx + yy) / 53.0)], -1)
    a = np.clip(a + np.random.default_rng(24).integers(-20, 21, (H, W, 3)), 0, 255).astype(np.uint8)
    got = proc.encode_jpeg(a, 90, subsampling=2, restart_marker_rows=1)
    assert got == pillow_save(a, 90, 2, restart_marker_rows=1)


@pytest.mark.parametrize("s,rows", ((0, False), (1, False), (2, False), (2, True), (0, True)))
def test_an_encode_into_exactly_the_bound_writes_nothing_outside(proc, s, rows):
    from raw2film_amd import _lib

    ctx = proc.ctx
    H, W, q = 50, 70, 100
    a = noise(H, W, seed=3)
    src = torch.from_numpy(a).cuda()
    opts = _lib.JpegOpts(q, s, 0, 0, 1)
    cap = int(ctx._lib.r2f_jpeg_bound_bytes_opts(C.byref(opts), H, W))
    assert cap == ctx.jpeg_bound_bytes(H, W, s) + 6 + 4 * (-(-H // (16 if s == 2 else 8)) * -(-W // (8 if s == 0 else 16)))
    out = Arena.flat(cap, misalign=1, device="cuda")
    length = Arena.flat_of(torch.int64, 1, device="cuda")
    args = (out.view.data_ptr(), cap, length.view.data_ptr(), ctx._stream())
    if rows:
        mh = 16 if s == 2 else 8
        rc = ctx._lib.r2f_jpeg_rows_begin_ex(ctx._h, H, W, C.byref(opts), *args)
        for y in range(0, H, mh):
            rc = rc or ctx._lib.r2f_jpeg_rows(ctx._h, src.data_ptr(), 3 * W, y, min(y + mh, H), ctx._stream())
    else:
        rc = ctx._lib.r2f_jpeg_encode_ex(ctx._h, src.data_ptr(), H, W, 3 * W, C.byref(opts), *args)
    assert rc == 0, ctx._lib.r2f_last_error(ctx._h)
    torch.cuda.synchronize()
    what = f"jpeg restart 1 sampling {s} rows {rows}"
    n = int(length.view.cpu()[0])
    want = pillow_save(a, q, s, restart_marker_blocks=1)
    assert n == len(want) <= cap and out.view[:n].cpu().numpy().tobytes() == want
    written = torch.zeros(cap, dtype=torch.bool)
    written[:n] = True
    out.check(written, expected=torch.from_numpy(np.frombuffer(want + bytes(cap - n), np.uint8).copy()), what=what + " file")
    length.check(torch.ones(1, dtype=torch.bool), what=what + " length word")
    rc = ctx._lib.r2f_jpeg_encode_ex(ctx._h, src.data_ptr(), H, W, 3 * W, C.byref(opts), out.view.data_ptr(), cap - 1,
                                     length.view.data_ptr(), ctx._stream())
    assert rc == -1  # a capacity below the bound is refused
