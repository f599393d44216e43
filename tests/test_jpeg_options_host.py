"""The JPEG export's subsampling / optimize / exif options on the host, without a GPU: the extended NumPy model
(tests/jpeg_options_model.py) writes Pillow's bytes, the library's plan-only entry points agree with it, the option parser takes
Pillow's values, and the sampling-aware host code runs clean under AddressSanitizer / UBSan."""

import ctypes
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_model as jm
import jpeg_options_model as om
from test_jpeg_host import SIZES, contents

Image = pytest.importorskip("PIL.Image")
ImageFile = pytest.importorskip("PIL.ImageFile")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXIF = b"Exif\x00\x00MM\x00*\x00\x00\x00\x08\x00\x00"  # (an empty big-endian TIFF directory)


def pillow_jpeg(a, quality, subsampling=-1, optimize=False, exif=b""):
    """Pillow's file.  (With optimize, Pillow sizes its output buffer from the pixel count; a noise frame at q100 can outgrow it
    and Pillow then fails -- a larger buffer gives libjpeg's bytes.)"""
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(old, 24 * a.shape[0] * a.shape[1] + len(exif) + (1 << 16))
    try:
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, "JPEG", quality=quality, subsampling=subsampling, optimize=optimize, exif=exif)
        return buf.getvalue()
    finally:
        ImageFile.MAXBLOCK = old


@pytest.mark.parametrize("H,W", SIZES)
def test_model_writes_pillows_bytes_for_every_option(H, W):
    for name, a in contents(H, W).items():
        for q in (1, 75, 100):
            for s in (0, 1, 2):
                for o in (False, True):
                    e = EXIF if (q + s) % 2 else b""
                    assert om.encode(a, q, s, o, e) == pillow_jpeg(a, q, s, o, e), (name, q, s, o, bool(e))


def test_model_default_options_are_jpeg_models():
    a = contents(31, 64)["noise"]
    assert om.encode(a, 90) == om.encode(a, 90, -1) == jm.encode(a, 90) == pillow_jpeg(a, 90)


def test_exif_splice_is_pillows():
    a = contents(17, 33)["gradient"]
    exif = Image.Exif()
    exif[0x010F] = "maker"
    exif[0x0110] = "model"
    for e in (exif.tobytes(), bytes(range(256)) * 10, b"x"):
        want = pillow_jpeg(a, 95, 0, False, e)
        plain = pillow_jpeg(a, 95, 0)
        assert want == om.splice_exif(plain, e) and want[20:24] == b"\xff\xe1" + (len(e) + 2).to_bytes(2, "big")


# ---- Annex K.3: code lengths over 16
def fibonacci_counts(n):
    """2, 2, 4, 6, 10, ...: with the reserved symbol's count of 1, every merge takes the tree built so far, so the code lengths
    run to n (plain Fibonacci counts next to that 1 build two chains of half the depth)."""
    f = [2, 2]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def test_k3_adjustment_on_a_fibonacci_histogram():
    lib = _lib()
    for n in (18, 20, 24, 30):
        freq = np.zeros(256, dtype=np.uint64)
        syms = np.random.default_rng(n).permutation(256)[:n]
        freq[syms] = fibonacci_counts(n)
        st = {}
        want = om.optimal_table(freq, st)
        assert st["adjusted"], n
        assert _optimal_table(lib, freq) == want
        assert sum(want[0]) == n and max(i for i in range(17) if want[0][i]) <= 16


def _block_for(pos, value, ql):
    """A grey 8 x 8 pixel block whose only non-zero quantised coefficient is `value` at zigzag position `pos` (DC 0), or None."""
    nat = int(jm.ZIGZAG[pos])
    u, v = nat % 8, nat // 8
    F = value * int(ql[nat])
    x = np.arange(8)
    cu, cv = (np.sqrt(0.5) if u == 0 else 1.0), (np.sqrt(0.5) if v == 0 else 1.0)
    f = 0.25 * cu * cv * F * np.outer(np.cos((2 * x + 1) * v * np.pi / 16), np.cos((2 * x + 1) * u * np.pi / 16))
    px = np.clip(np.rint(128 + f), 0, 255).astype(np.int64)
    q = jm.quantize(jm.fdct_islow(px[None] - 128), ql)[0].reshape(64)[jm.ZIGZAG]
    want = np.zeros(64, dtype=np.int64)
    want[pos] = value
    return px.astype(np.uint8) if np.array_equal(q, want) else None


def test_k3_adjustment_end_to_end():
    """A grey frame of blocks that each carry one chosen AC coefficient, at q50 (pixel rounding stays below every quantisation
    step), whose luma AC symbols have Fibonacci-like counts: the optimized table needs the K.3 folding, and the bytes are Pillow's."""
    q = 50
    ql, _ = jm.quant_tables(q)
    blocks = []
    for pos, value in [(p, 1) for p in range(1, 15)] + [(p, 3) for p in range(1, 5)]:
        b = _block_for(pos, value, ql)
        assert b is not None, (pos, value)
        blocks.append(b)
    counts = fibonacci_counts(len(blocks))
    seq = np.concatenate([np.full(c, i) for i, c in enumerate(counts)])
    seq = seq[np.random.default_rng(1).permutation(len(seq))]
    bw = 128
    bh = -(-len(seq) // bw)
    bh += bh % 2  # (4:2:0: whole MCU rows of real blocks)
    tiles = np.full((bh * bw, 8, 8), 128, dtype=np.uint8)
    tiles[: len(seq)] = np.stack(blocks)[seq]
    grey = tiles.reshape(bh, bw, 8, 8).swapaxes(1, 2).reshape(bh * 8, bw * 8)
    a = np.repeat(grey[..., None], 3, axis=2)
    st = {}
    got = om.encode(a, q, 2, True, b"", stats=st)
    assert st["adjusted"]
    assert got == pillow_jpeg(a, q, 2, True)


# ---- the library's plan-only exports
def _lib():
    from raw2film_amd import _lib

    return _lib.load()


def _optimal_table(lib, freq):
    freq = np.ascontiguousarray(freq, dtype=np.uint64)
    bits, hv, n = (ctypes.c_uint8 * 17)(), (ctypes.c_uint8 * 256)(), ctypes.c_int()
    rc = lib.r2f_jpeg_optimal_table(freq.ctypes.data, bits, hv, ctypes.byref(n))
    assert rc in (0, -1)
    return (list(bits), list(hv[: n.value])) if rc == 0 else None


def test_library_optimal_table_equals_the_model():
    lib = _lib()
    rng = np.random.default_rng(7)
    cases = []
    for _ in range(60):
        f = np.zeros(256, dtype=np.uint64)
        k = int(rng.integers(1, 257))
        idx = rng.choice(256, k, replace=False)
        f[idx] = rng.integers(1, int(rng.choice([3, 100, 10**6, 10**9])), k)
        cases.append(f)
    single = np.zeros(256, dtype=np.uint64)
    single[0x37] = 5
    cases += [single, np.ones(256, dtype=np.uint64), np.full(256, 10**9, dtype=np.uint64),
              (2.0 ** (np.arange(256) % 40)).astype(np.uint64), np.array([2 ** 40] + [1] * 255, dtype=np.uint64)]
    refused = 0
    for f in cases:
        want = om.optimal_table(f)
        assert _optimal_table(lib, f) == want
        refused += want is None
    assert 1 <= refused <= 20  # (the sentinel cases: libjpeg refuses what its merge leaves)
    bits, hv, n = (ctypes.c_uint8 * 17)(), (ctypes.c_uint8 * 256)(), ctypes.c_int()
    assert lib.r2f_jpeg_optimal_table(np.zeros(256, np.uint64).ctypes.data, bits, hv, ctypes.byref(n)) == -1


def _header_ex(lib, q, s, H, W, optimize=0):
    from raw2film_amd import _lib as L

    buf, n = (ctypes.c_uint8 * 1024)(), ctypes.c_size_t()
    rc = lib.r2f_jpeg_header_ex(ctypes.byref(L.JpegOpts(q, s, optimize, 0)), H, W, buf, len(buf), ctypes.byref(n))
    return rc, bytes(buf[: n.value])


def test_library_header_ex_equals_pillows_up_to_sos():
    lib = _lib()
    for s in (0, 1, 2):
        for q in (0, 50, 100):
            for H, W in ((1, 1), (17, 33), (256, 383), (12288, 8192)):
                rc, h = _header_ex(lib, q, s, H, W)
                assert rc == 0 and h == om.header(q, H, W, s)
                if H * W < 1e5:
                    assert pillow_jpeg(np.zeros((H, W, 3), np.uint8), q, s)[: len(h)] == h
    assert _header_ex(lib, 50, 0, 8, 8, optimize=1)[0] == -1
    assert _header_ex(lib, 50, 3, 8, 8)[0] == -1 and _header_ex(lib, 50, -1, 8, 8)[0] == -1


def test_old_entry_points_equal_ex_with_sampling_2():
    lib = _lib()
    for H, W in SIZES + ((12288, 8192), (65535, 65535)):
        assert lib.r2f_jpeg_bound_bytes(H, W) == lib.r2f_jpeg_bound_bytes_ex(H, W, 2)
        buf, n = (ctypes.c_uint8 * 1024)(), ctypes.c_size_t()
        assert lib.r2f_jpeg_header(75, H, W, buf, len(buf), ctypes.byref(n)) == 0
        assert _header_ex(lib, 75, 2, H, W) == (0, bytes(buf[: n.value]))


def test_library_bound_ex_holds_for_the_worst_case():
    lib = _lib()
    for s in (0, 1, 2):
        for H, W in ((16, 16), (17, 33), (64, 64)):
            assert lib.r2f_jpeg_bound_bytes_ex(H, W, s) == om.bound_bytes(H, W, s)
            for o in (False, True):
                out = om.encode(contents(H, W)["noise"], 100, s, o)
                assert len(out) <= lib.r2f_jpeg_bound_bytes_ex(H, W, s)
    # per pixel at size: 9.7 / 13.0 / 19.5 bytes
    for s, per_px in ((2, 9.73), (1, 12.97), (0, 19.46)):
        assert abs(lib.r2f_jpeg_bound_bytes_ex(8192, 12288, s) / (8192 * 12288) - per_px) < 0.01
    assert lib.r2f_jpeg_bound_bytes_ex(8, 8, 3) == 0 and lib.r2f_jpeg_bound_bytes_ex(0, 8, 0) == 0


# ---- the option parser and the streamed export's row steps
def test_subsampling_parser():
    from raw2film_amd.jpeg_options import _jpeg_exif, _jpeg_options, _jpeg_subsampling

    for v, want in ((-1, 2), (0, 0), (1, 1), (2, 2), ("4:4:4", 0), ("4:2:2", 1), ("4:2:0", 2), (np.int64(1), 1)):
        assert _jpeg_subsampling(v) == want
    for bad in ("keep", "4:1:1", "web_high", 3, -2, 1.0, True, None, b"4:4:4", "444"):
        with pytest.raises(ValueError, match=repr(bad).replace("(", r"\(").replace(")", r"\)")[:6]):
            _jpeg_subsampling(bad)
    exif = Image.Exif()
    exif[0x0131] = "raw2film"
    assert _jpeg_exif(exif) == exif.tobytes() and _jpeg_exif(bytearray(b"ab")) == b"ab" and _jpeg_exif(b"") == b""
    assert _jpeg_exif(b"x" * 65533) == b"x" * 65533
    for bad in (b"x" * 65534, "text", 5):
        with pytest.raises(ValueError):
            _jpeg_exif(bad)
    assert _jpeg_options(-1, 0, b"") == (2, False, b"") and _jpeg_options("4:4:4", [1], EXIF) == (0, True, EXIF)


def test_row_steps_with_8_row_mcus():
    from raw2film_amd.jpeg_stream import jpeg_row_steps

    assert jpeg_row_steps([0, 20, 40, 57], 57, 8) == [(0, 16), (16, 40), (40, 57)]
    assert jpeg_row_steps([0, 20, 40, 57], 57) == [(0, 16), (16, 32), (32, 57)]
    assert jpeg_row_steps([0, 5, 12, 17], 17, 8) == [None, (0, 8), (8, 17)]
    rng = np.random.default_rng(3)
    for _ in range(200):
        H = int(rng.integers(1, 3000))
        cuts = sorted(set(rng.integers(1, H, int(rng.integers(0, 12))).tolist())) if H > 1 else []
        bounds = [0] + cuts + [H]
        steps = jpeg_row_steps(bounds, H, 8)
        done = [s for s in steps if s is not None]
        assert done[0][0] == 0 and done[-1][1] == H
        assert all(a[1] == b[0] for a, b in zip(done, done[1:]))
        assert all(y1 % 8 == 0 or y1 == H for _, y1 in done)


# ---- the sampling-aware plan under the sanitizers
@pytest.fixture(scope="module")
def options_check_binary(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("jpeg_options_plan") / "jpeg_options_plan_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "jpeg_options_plan_check.cpp"), os.path.join(ROOT, "raw2film_amd", "csrc", "r2f_jpeg_plan.cpp"),
           "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


def _run(binary, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([binary, *map(str, args)], capture_output=True, text=True, env=env, timeout=600)


@pytest.mark.parametrize("seed", [1, 2, 20261015])
def test_options_plan_is_clean_under_asan_and_ubsan(options_check_binary, seed):
    res = _run(options_check_binary, "fuzz", seed, 1500)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    assert "cases ok" in res.stdout


def test_sanitized_optimal_table_and_header_equal_the_model(options_check_binary):
    rng = np.random.default_rng(11)
    freq = np.zeros((4, 256), dtype=np.uint64)
    freq[0, :12] = rng.integers(0, 50, 12)
    freq[0, 0] += 1
    freq[2, :12] = rng.integers(1, 5000, 12)
    for t in (1, 3):
        syms = [0, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]
        freq[t, syms] = rng.integers(0, 10**6, len(syms))
    freq[1, 0] += 1
    freq[3, 0] += 1
    for s in (0, 1, 2):
        res = _run(options_check_binary, "header", 85, s, 123, 457, *freq.reshape(-1).tolist())
        assert res.returncode == 0, res.stderr
        tables = tuple((b[1:17], hv) for b, hv in (om.optimal_table(freq[t]) for t in range(4)))
        assert bytes.fromhex(res.stdout.strip()) == om.header(85, 123, 457, s, tables)
