"""The JPEG export's progressive option on the host, without a GPU: the progressive NumPy model (tests/jpeg_progressive_model.py)
writes Pillow's progressive=True bytes -- on frames whose EOB runs are flushed by the 0x7FFF cap and by the 937 buffered
correction bits -- the library's progressive headers and bound agree with it, and the planner runs clean under the sanitizers."""

import ctypes
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_model as jm
import jpeg_options_model as om
import jpeg_progressive_model as pm
from test_jpeg_host import contents
from test_jpeg_options_host import EXIF

Image = pytest.importorskip("PIL.Image")
ImageFile = pytest.importorskip("PIL.ImageFile")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((1, 1), (1, 17), (17, 1), (7, 5), (17, 33), (31, 64), (40, 70))


def pillow_progressive(a, quality, subsampling=-1, exif=b"", optimize=False):
    """Pillow's progressive file (its output buffer enlarged: a noisy progressive file outgrows the default one and Pillow then
    fails with "Suspension not allowed here")."""
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(old, 32 * a.shape[0] * a.shape[1] + len(exif) + (1 << 16))
    try:
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, "JPEG", quality=quality, subsampling=subsampling, progressive=True, optimize=optimize,
                                exif=exif)
        return buf.getvalue()
    finally:
        ImageFile.MAXBLOCK = old


def correction_frame(bh, bw, seed=0):
    """A grey frame of 8 x 8 blocks whose 63 AC coefficients at q100 all have magnitude 2 .. 4 (signs random): the last luma
    refinement scan codes nothing new in them and buffers 63 correction bits per block, so its EOB runs are flushed by the
    937-bit limit every 15 blocks."""
    rng = np.random.default_rng(seed)
    x = np.arange(8)
    c = np.where(x == 0, np.sqrt(0.125), 0.5)
    basis = c[:, None] * np.cos((2 * x[None, :] + 1) * x[:, None] * np.pi / 16)  # [u][x], orthonormal
    F = 3.0 * rng.choice([-1.0, 1.0], (bh, bw, 8, 8))
    F[..., 0, 0] = 0
    px = np.einsum("ux,vy,abvu->abyx", basis, basis, F)
    grey = np.clip(np.rint(128 + px), 0, 255).astype(np.uint8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)
    return np.repeat(grey[..., None], 3, axis=2)


def smooth_field(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([xx * 255 // max(W - 1, 1), yy * 255 // max(H - 1, 1), (xx + yy) * 255 // max(H + W - 2, 1)], -1).astype(np.uint8)


@pytest.mark.parametrize("H,W", SIZES)
def test_model_writes_pillows_progressive_bytes(H, W):
    for name, a in list(contents(H, W).items()) + [("black", np.zeros((H, W, 3), np.uint8))]:
        for q in (1, 75, 100):
            for s in (0, 1, 2):
                e = EXIF if (q + s) % 2 else b""
                assert pm.encode(a, q, s, e) == pillow_progressive(a, q, s, e), (name, q, s, bool(e))


def test_optimize_makes_no_difference_and_default_sampling_is_420():
    a = contents(31, 64)["noise"]
    want = pillow_progressive(a, 90, -1)
    assert pillow_progressive(a, 90, -1, optimize=True) == want == pm.encode(a, 90, -1) == pm.encode(a, 90, 2)


def test_refinement_runs_flushed_at_937_correction_bits():
    a = correction_frame(24, 40)
    for s in (0, 1, 2):
        st = {}
        assert pm.encode(a, 100, s, stats=st) == pillow_progressive(a, 100, s), s
        assert st.get("be_cap", 0) >= 20, (s, st)


def test_first_scan_runs_flushed_at_0x7fff_blocks():
    a = smooth_field(1456, 1456)  # 182 x 182 = 33124 blocks per component at 4:4:4
    st = {}
    assert pm.encode(a, 75, 0, stats=st) == pillow_progressive(a, 75, 0)
    assert st.get("eobrun_cap", 0) >= 3, st
    st = {}
    b = np.zeros((1456, 1456, 3), np.uint8)
    assert pm.encode(b, 50, 0, stats=st) == pillow_progressive(b, 50, 0)
    assert st.get("eobrun_cap", 0) == 8, st  # (every AC scan: one full run of 0x7FFF blocks, then the rest at the end)


# ---- the library's plan-only exports
def _lib():
    from raw2film_amd import _lib

    return _lib.load()


def _opts(q, s, progressive, optimize=0):
    from raw2film_amd import _lib as L

    return L.JpegOpts(q, s, optimize, progressive)


def test_library_bound_holds_for_the_worst_case():
    lib = _lib()
    for s in (0, 1, 2):
        for H, W in ((16, 16), (17, 33), (64, 64)):
            bound = lib.r2f_jpeg_bound_bytes_opts(ctypes.byref(_opts(100, s, 1)), H, W)
            assert bound > lib.r2f_jpeg_bound_bytes_ex(H, W, s)
            for a in (contents(H, W)["noise"], correction_frame(-(-H // 8), -(-W // 8))[:H, :W]):
                assert len(pm.encode(a, 100, s)) <= bound
        assert lib.r2f_jpeg_bound_bytes_opts(ctypes.byref(_opts(90, s, 0)), 100, 200) == lib.r2f_jpeg_bound_bytes_ex(100, 200, s)
    # per pixel at size: 12.05 / 16.06 / 24.09 bytes
    for s, per_px in ((2, 12.05), (1, 16.06), (0, 24.09)):
        assert abs(lib.r2f_jpeg_bound_bytes_opts(ctypes.byref(_opts(90, s, 1)), 8192, 12288) / (8192 * 12288) - per_px) < 0.01
    assert lib.r2f_jpeg_bound_bytes_opts(ctypes.byref(_opts(90, 0, 2)), 8, 8) == 0
    assert lib.r2f_jpeg_bound_bytes_opts(ctypes.byref(_opts(90, 3, 1)), 8, 8) == 0
    assert lib.r2f_jpeg_bound_bytes_opts(ctypes.byref(_opts(90, 0, 1)), 0, 8) == 0


def test_constructed_worst_case_per_block():
    """Per block, every AC coefficient at the most expensive value each scan can see (odd magnitudes that need all their bits,
    alternating signs) against the planner's per-block bit bounds."""
    rng = np.random.default_rng(3)
    blocks = np.zeros((1, 6, 64), np.int64)
    blocks[0, :, 1:] = rng.choice([-1, 1], (6, 63)) * 1023
    blocks[0, :, 0] = 1023 * np.array([1, -1, 1, -1, 1, -1])
    for scan in pm.SCRIPT:
        ev = pm.scan_events(blocks, 16, 16, 2, scan)
        # every symbol at the longest code (16 bits) plus its raw bits
        bits = sum(16 if k == 0 else b for k, _, b in ev.ev)
        n = 6 if scan[1] == 0 else (4 if scan[0] == (0,) else 1)
        assert bits <= n * (63 * 27 + 3 * 16 + 30), scan
    assert pm.encode(np.zeros((16, 16, 3), np.uint8), 100, 2)  # (sanity)


def test_header_ex_refuses_progressive():
    lib = _lib()
    buf, n = (ctypes.c_uint8 * 1024)(), ctypes.c_size_t()
    assert lib.r2f_jpeg_header_ex(ctypes.byref(_opts(50, 0, 1)), 8, 8, buf, len(buf), ctypes.byref(n)) == -1
    assert lib.r2f_jpeg_header_ex(ctypes.byref(_opts(50, 0, 0)), 8, 8, buf, len(buf), ctypes.byref(n)) == 0


def test_progressive_parser():
    from raw2film_amd.jpeg_options import _jpeg_progressive

    for v, want in ((True, True), (False, False), (0, False), (1, True), (np.bool_(True), True), (np.int64(1), True)):
        assert _jpeg_progressive(v) is want
    for bad in (2, -1, "yes", None, 1.0, b"1", [1]):
        with pytest.raises(ValueError):
            _jpeg_progressive(bad)


# ---- the progressive plan under the sanitizers
@pytest.fixture(scope="module")
def plan_check_binary(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("jpeg_progressive_plan") / "jpeg_progressive_plan_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "jpeg_progressive_plan_check.cpp"),
           os.path.join(ROOT, "raw2film_amd", "csrc", "r2f_jpeg_plan.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


def _run(binary, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([binary, *map(str, args)], capture_output=True, text=True, env=env, timeout=600)


@pytest.mark.parametrize("seed", [1, 20261016])
def test_progressive_plan_is_clean_under_asan_and_ubsan(plan_check_binary, seed):
    res = _run(plan_check_binary, "fuzz", seed, 400)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    assert "cases ok" in res.stdout


@pytest.mark.parametrize("s", [0, 1, 2])
def test_library_headers_equal_the_models(plan_check_binary, s):
    """The planner's SOF2 frame header and every scan's DHT + SOS from the scans' counts, and its exact scan bits, equal the
    model's on a real frame."""
    a = contents(40, 70)["gradient"]
    H, W = a.shape[:2]
    q = 85
    coefs = om.coefficients(a, q, s)
    res = _run(plan_check_binary, "frame", q, s, H, W)
    assert res.returncode == 0, res.stderr
    assert bytes.fromhex(res.stdout.strip()) == pm.frame_header(q, H, W, s)
    for i, scan in enumerate(pm.SCRIPT):
        ev = pm.scan_events(coefs, H, W, s, scan)
        slots = 2 if scan[1] == 0 else 1
        freq = ev.counts(slots)[:, :256] if not (scan[1] == 0 and scan[3]) else np.zeros((2, 256), np.int64)
        raw = sum(b for k, _, b in ev.ev if k == 1)
        sym_raw = 0
        for k, slot, sym in ev.ev:
            if k == 0:
                sym_raw += sym if scan[1] == 0 else ((sym & 15) or (0 if sym == 0xF0 else sym >> 4))
        extra = raw - sym_raw  # (the correction bits, or one per block of the DC refinement)
        f = np.zeros((2, 256), np.int64)
        f[: freq.shape[0]] = freq
        res = _run(plan_check_binary, "scan", i, extra, *f.reshape(-1).tolist())
        assert res.returncode == 0, res.stderr
        hdr_hex, bits = res.stdout.split()
        tables = [] if (scan[1] == 0 and scan[3]) else [(b[1:17], hv) for b, hv in (om.optimal_table(f[k]) for k in range(slots))]
        assert bytes.fromhex(hdr_hex) == pm.scan_header(scan, tables), i
        codes = [jm.huff_codes(t) for t in tables]
        want_bits = sum(codes[slot][sym][1] if k == 0 else 0 for k, slot, sym in ev.ev) + raw
        assert int(bits) == want_bits, i
