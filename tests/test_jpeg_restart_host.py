"""The JPEG export's restart markers, ICC profile, XMP, comment and dpi on the host, without a GPU: the restart-aware NumPy model
(tests/jpeg_restart_model.py) writes Pillow's bytes, the library's plan-only entry points write Pillow's header (density, DRI) and
bound its files, the option parsers take and refuse what the export documents, and the planner's new host code runs clean under
AddressSanitizer / UBSan in a stand-alone program."""

import ctypes
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_options_model as om
import jpeg_restart_model as rm
from test_jpeg_options_host import EXIF

Image = pytest.importorskip("PIL.Image")
ImageFile = pytest.importorskip("PIL.ImageFile")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1), (8, 8), (40, 56), (50, 70))
BLOCKS = (1, 3, 5, 11, 12, 65535)
ROWS = (1, 2, 5)
ICC = bytes((i * 7 + i // 251) % 256 for i in range(70000))  # (two APP2 chunks)
XMP = b"<x:xmpmeta xmlns:x='adobe:ns:meta/'><rdf:RDF/></x:xmpmeta>"
COMMENT = b"scanned on a drum"
DPI = (300, 72.6)
METADATA = dict(icc_profile=ICC, xmp=XMP, comment=COMMENT, dpi=DPI)


def pillow_save(a, quality, subsampling=-1, optimize=False, **options):
    """Pillow's file for any of its save options.  (Pillow sizes its output buffer from the pixel count and some of the
    segments; a larger one gives libjpeg's bytes where that would fall short.)"""
    old = ImageFile.MAXBLOCK
    extra = sum(len(v) for v in options.values() if isinstance(v, (bytes, str)))
    ImageFile.MAXBLOCK = max(old, 32 * a.shape[0] * a.shape[1] + 2 * extra + (1 << 17))
    try:
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, "JPEG", quality=quality, subsampling=subsampling, optimize=optimize, **options)
        return buf.getvalue()
    finally:
        ImageFile.MAXBLOCK = old


def noise(H, W, seed=0):
    return np.random.default_rng(1000 * H + W + seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def scene(H, W):
    """Smooth ramps with some noise on top: long zero runs, DC differences of both signs, non-trivial optimized tables."""
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([(x * 5 + y) % 256, (y * 7) % 256, (x + y) * 3 % 256], axis=-1)
    return np.clip(base + np.random.default_rng(H + W).integers(-6, 7, (H, W, 3)), 0, 255).astype(np.uint8)


def _lib():
    from raw2film_amd import _lib as L

    return L.load()


# ---- the model against Pillow
@pytest.mark.parametrize("H,W", SHAPES)
def test_model_writes_pillows_bytes_for_restart_blocks_and_rows(H, W):
    for a, q in ((noise(H, W), 90), (scene(H, W), 75)):
        for s in (0, 1, 2):
            for o in (False, True):
                for blocks in BLOCKS:
                    got = rm.encode(a, q, s, o, restart_marker_blocks=blocks)
                    assert got == pillow_save(a, q, s, o, restart_marker_blocks=blocks), (s, o, blocks)
                for rows in ROWS:
                    got = rm.encode(a, q, s, o, restart_marker_rows=rows)
                    assert got == pillow_save(a, q, s, o, restart_marker_rows=rows), (s, o, rows)
                # rows win over blocks
                got = rm.encode(a, q, s, o, restart_marker_blocks=3, restart_marker_rows=2)
                assert got == pillow_save(a, q, s, o, restart_marker_blocks=3, restart_marker_rows=2)
                assert got == rm.encode(a, q, s, o, restart_marker_rows=2)


def test_restart_facts():
    """What the model (and the device encoder) rests on, from Pillow's files alone."""
    a = scene(24, 32)  # 12 MCUs in 4:4:4
    plain = pillow_save(a, 90, 0)
    for blocks, markers in ((12, 0), (11, 1), (13, 0)):
        f = pillow_save(a, 90, 0, restart_marker_blocks=blocks)
        sos = f.index(b"\xff\xda")
        assert f[sos - 6:sos] == b"\xff\xdd\x00\x04" + blocks.to_bytes(2, "big") and f[sos - 189:sos - 185] == b"\xff\xc4\x00\xb5"  # behind the last DHT
        assert sum(f.count(bytes([0xFF, 0xD0 + i]), sos) for i in range(8)) == markers
        assert f[:sos - 6] == plain[:sos - 6]
    f = pillow_save(a, 90, 0, restart_marker_blocks=1)
    scan = f[f.index(b"\xff\xda") + 14:]
    marks = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
    assert marks == [0xD0 + i % 8 for i in range(11)]
    # optimize counts the restarted DC differences: other tables than without an interval
    b = scene(40, 56)
    with_dri, without = pillow_save(b, 90, 0, True, restart_marker_blocks=1), pillow_save(b, 90, 0, True)
    assert with_dri[:with_dri.index(b"\xff\xdd")] != without[:without.index(b"\xff\xda")]
    assert rm.restart_interval(2400, 0, rows=219) == 65535 and rm.restart_interval(2400, 0, rows=218) == 65400


def test_the_interval_is_clamped_to_65535_mcus():
    a = np.zeros((219 * 8 + 8, 2400, 3), np.uint8)  # 300 MCUs per row in 4:4:4, 220 rows
    a[::3, ::5] = 200
    for rows, dri in ((219, 65535), (218, 65400)):
        want = pillow_save(a, 50, 0, restart_marker_rows=rows)
        sos = want.index(b"\xff\xda")
        assert want[sos - 6:sos] == b"\xff\xdd\x00\x04" + dri.to_bytes(2, "big")
        assert rm.encode(a, 50, 0, restart_marker_rows=rows) == want


def test_model_writes_pillows_segments():
    a = scene(17, 33)
    cases = [dict(icc_profile=ICC), dict(xmp=XMP), dict(comment=COMMENT), dict(comment="héllo"), dict(dpi=DPI), dict(dpi=(0.5, 300)),
             dict(dpi=(2.5, 3.5)), dict(exif=EXIF, **METADATA), dict(exif=EXIF, restart_marker_blocks=2, **METADATA)]
    for options in cases:
        for s, o in ((0, False), (2, True)):
            want = pillow_save(a, 92, s, o, **options)
            assert rm.encode(a, 92, s, o, **options) == want, list(options)
    want = pillow_save(a, 92, 0, exif=EXIF, **METADATA)
    kinds, i = [], 2
    while want[i + 1] != 0xDB:
        kinds.append((want[i + 1], int.from_bytes(want[i + 2:i + 4], "big")))
        i += 2 + kinds[-1][1]
    assert kinds == [(0xE0, 16), (0xE1, len(EXIF) + 2), (0xE1, len(XMP) + 31), (0xE2, 65535), (0xE2, 4497), (0xFE, len(COMMENT) + 2)]
    assert want[13:18] == bytes([1, 1, 0x2C, 0, 0x49]) and pillow_save(a, 92, 0)[13:18] == bytes([0, 0, 1, 0, 1])


def test_the_package_builds_the_models_segments():
    from raw2film_amd.jpeg_stream import app1_segment, metadata_segments

    assert metadata_segments() == b"" and metadata_segments(EXIF) == app1_segment(EXIF)
    assert metadata_segments(EXIF, XMP, ICC, COMMENT) == rm.segments(EXIF, XMP, ICC, COMMENT)
    assert metadata_segments(icc_profile=ICC[:65519]) == rm.segments(icc_profile=ICC[:65519])  # (one full chunk, no empty second)
    for kw in (dict(xmp=XMP), dict(icc_profile=ICC), dict(comment=COMMENT)):
        assert metadata_segments(**kw) == rm.segments(**kw)


# ---- the library's plan-only entry points
def _opts(q, s, restart=0, density=(0, 0), optimize=0, progressive=0):
    from raw2film_amd import _lib as L

    return L.JpegOpts(q, s, optimize, progressive, restart, *density)


def _header_ex(lib, opts, H, W, cap=1024):
    buf, n = (ctypes.c_uint8 * 1024)(), ctypes.c_size_t()
    rc = lib.r2f_jpeg_header_ex(ctypes.byref(opts), H, W, buf, cap, ctypes.byref(n))
    return rc, bytes(buf[: n.value])


def test_library_header_and_bound_are_pillows_with_density_and_dri():
    from raw2film_amd import _lib as L

    lib = _lib()
    for H, W in SHAPES:
        a = noise(H, W)
        for s in (0, 1, 2):
            for blocks, rows in [(b, 0) for b in BLOCKS] + [(0, r) for r in ROWS] + [(3, 2)]:
                for dpi in ((0, 0), DPI):
                    interval = rm.restart_interval(W, s, blocks, rows)
                    density = tuple(round(v) for v in dpi)
                    want = pillow_save(a, 100, s, restart_marker_blocks=blocks, restart_marker_rows=rows, dpi=dpi)
                    rc, h = _header_ex(lib, _opts(100, s, interval, density), H, W)
                    assert rc == 0 and h == want[: len(h)] == rm.header(100, H, W, s, None, interval, dpi), (H, W, s, blocks, rows, dpi)
                    assert h[-20:-14] == b"\xff\xdd\x00\x04" + interval.to_bytes(2, "big")
                    bound = lib.r2f_jpeg_bound_bytes_opts(ctypes.byref(_opts(100, s, interval)), H, W)
                    assert bound == rm.bound_bytes(H, W, s, interval)
                    for o in (False, True):
                        f = pillow_save(a, 100, s, o, restart_marker_blocks=blocks, restart_marker_rows=rows)
                        assert len(f) <= bound, (H, W, s, blocks, rows, o)
    # the four-field calls: what they returned before there were more fields
    for s in (0, 1, 2):
        four = L.JpegOpts(75, s, 0, 0)
        rc, h = _header_ex(lib, four, 40, 56)
        assert rc == 0 and h == om.header(75, 40, 56, s) and len(h) == 623
        assert lib.r2f_jpeg_bound_bytes_opts(ctypes.byref(four), 40, 56) == lib.r2f_jpeg_bound_bytes_ex(40, 56, s) == om.bound_bytes(40, 56, s)
    assert _header_ex(lib, _opts(75, 0, 5), 8, 8, cap=628)[0] == -1 and _header_ex(lib, _opts(75, 0, 5), 8, 8, cap=629)[0] == 0
    for bad in (-1, 65536, 70000):
        assert _header_ex(lib, _opts(75, 0, bad), 8, 8)[0] == -1
        assert lib.r2f_jpeg_bound_bytes_opts(ctypes.byref(_opts(75, 0, bad)), 8, 8) == 0
    for bad in ((-1, 72), (72, 65536)):
        assert _header_ex(lib, _opts(75, 0, 0, bad), 8, 8)[0] == -1
    assert lib.r2f_jpeg_bound_bytes_opts(ctypes.byref(_opts(75, 0, 5, progressive=1)), 8, 8) == 0
    assert b"abi7" in lib.r2f_version()


# ---- the option parsers
def test_restart_and_metadata_parsers():
    from raw2film_amd.jpeg_options import _jpeg_extras

    def parse(**kw):
        args = dict(icc_profile=b"", xmp=b"", comment=b"", dpi=(0, 0), restart_marker_blocks=0, restart_marker_rows=0)
        args.update(kw)
        return _jpeg_extras(**args)

    none = parse()
    assert none == (b"", b"", b"", (0, 0), 0, 0) and none.restart(56, 0) == 0 and none.segments(b"") == b""
    x = parse(icc_profile=bytearray(ICC), xmp=memoryview(XMP), comment="héllo", dpi=DPI, restart_marker_blocks=np.int64(5))
    assert x == (ICC, XMP, "héllo".encode(), (300, 73), 5, 0) and x.segments(EXIF) == rm.segments(EXIF, XMP, ICC, "héllo")
    assert parse(dpi=(0.4, 300)).density == (0, 0) and parse(dpi=[2.5, np.float32(3.5)]).density == (2, 4)
    assert parse(restart_marker_blocks=65535).restart(56, 0) == 65535 and parse(restart_marker_blocks=True).blocks == 1
    for W, s, per_row in ((56, 0, 7), (56, 1, 4), (56, 2, 4), (70, 2, 5), (2400, 0, 300)):
        assert parse(restart_marker_rows=2, restart_marker_blocks=3).restart(W, s) == 2 * per_row == rm.restart_interval(W, s, 3, 2)
    assert parse(restart_marker_rows=219).restart(2400, 0) == 65535 and parse(restart_marker_rows=10**9).restart(8, 0) == 65535
    assert parse(xmp=b"x" * (65533 - 29)).xmp and parse(comment=b"c" * 65533).comment
    bad = [("restart_marker_blocks", v) for v in (-1, 65536, 70000, 1.0, "1", None)]
    bad += [("restart_marker_rows", v) for v in (-1, 2.0, "2", None)]
    bad += [("dpi", v) for v in ((-5, 300), (70000, 300), (300,), 300, ("a", "b"), (1, 2, 3), (float("nan"), 1), None)]
    bad += [("xmp", v) for v in ("str", b"x" * (65533 - 28), 5)]
    bad += [("comment", v) for v in (b"c" * 65534, 5, bytearray(b"ab"), None)]
    bad += [("icc_profile", v) for v in ("str", None, bytes(255 * 65519 + 1))]
    for name, value in bad:
        with pytest.raises(ValueError, match=name):
            parse(**{name: value})
    for kw in (dict(restart_marker_blocks=1), dict(restart_marker_rows=1)):
        with pytest.raises(ValueError, match="progressive.*restart_marker"):
            parse(progressive=True, **kw)
    assert parse(progressive=True, **METADATA).density == (300, 73)


def test_bad_options_raise_before_any_work():
    """The export calls check every option ahead of the frame: a processor that was never given a device is enough to see it."""
    from raw2film_amd.hip_processor import HipProcessor

    proc = object.__new__(HipProcessor)  # (no context, no device: any work would fail with AttributeError)
    a = np.zeros((8, 8, 3), np.uint8)
    for kw in (dict(restart_marker_blocks=-1), dict(restart_marker_blocks=65536), dict(restart_marker_rows=-1), dict(dpi=(1,)),
               dict(xmp="text"), dict(comment=b"c" * 65534), dict(icc_profile="text"),
               dict(progressive=True, restart_marker_rows=1)):
        name = [k for k in kw if k != "progressive"][0]
        with pytest.raises(ValueError, match=name):
            proc.encode_jpeg(a, 90, **kw)
        with pytest.raises(ValueError, match=name):
            proc.process_jpeg(a, None, 0.0, 0.0, 90, **kw)
        with pytest.raises(ValueError, match=name):
            proc.process_preloaded_jpeg(a, None, 0.0, 0.0, 90, **kw)
    assert not vars(proc)  # nothing half-done: no state was made or touched


# ---- the planner's new host code under the sanitizers, in a program of its own
@pytest.fixture(scope="module")
def restart_check_binary(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("jpeg_restart_plan") / "jpeg_restart_plan_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "jpeg_restart_plan_check.cpp"), os.path.join(ROOT, "raw2film_amd", "csrc", "r2f_jpeg_plan.cpp"),
           "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


def _run(binary, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([binary, *map(str, args)], capture_output=True, text=True, env=env, timeout=600)


@pytest.mark.parametrize("seed", [1, 2, 20261018])
def test_restart_plan_is_clean_under_asan_and_ubsan(restart_check_binary, seed):
    res = _run(restart_check_binary, "fuzz", seed, 1500)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    assert "cases ok" in res.stdout


def test_sanitized_header_and_bound_equal_pillows(restart_check_binary):
    a = noise(40, 56)
    for s in (0, 1, 2):
        for interval, density in ((5, (300, 73)), (65535, (0, 0)), (1, (1, 65535)), (0, (72, 72))):
            res = _run(restart_check_binary, "header", 85, s, 40, 56, interval, *density)
            assert res.returncode == 0, res.stderr
            hexed, bound = res.stdout.split()
            h = bytes.fromhex(hexed)
            dpi = {"dpi": density} if all(density) else {}
            want = pillow_save(a, 85, s, restart_marker_blocks=interval, **dpi)
            assert h == want[: len(h)] and len(want) <= int(bound) == rm.bound_bytes(40, 56, s, interval)
    assert _run(restart_check_binary, "header", 85, 0, 40, 56, 65536, 0, 0).returncode == 3
