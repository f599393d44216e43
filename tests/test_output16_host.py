"""The host side of the 16-bit output (no GPU): the TIFF header planner r2f_tiff_header against an independent reader and against
Pillow, its refusal of files past 4 GiB, the planner source under AddressSanitizer / UBSan, and the validation of `output_bits`
on every call that takes it."""

import ctypes
import inspect
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

from output16_model import read_tiff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# W = 1, odd widths, one strip and several with a short last one (strips aim at 256 KiB: 515 px x 6 B -> 84 rows per strip)
SHAPES = [(1, 1), (3, 7), (70, 257), (200, 515), (85, 515), (300, 1)]
ICCS = [b"", b"not a real profile, but an odd number of bytes.."[:37]]


def _frame(H, W, bits, seed=0):
    rng = np.random.default_rng(seed + H * 1000 + W)
    return rng.integers(0, 1 << bits, size=(H, W, 3), dtype=np.uint16 if bits == 16 else np.uint8)


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("icc", ICCS)
def test_header_reads_back_with_an_independent_reader_and_with_pillow(shape, bits, icc):
    from PIL import Image

    from raw2film_amd import tiff

    H, W = shape
    arr = _frame(H, W, bits)
    head, plan = tiff.header(H, W, bits, icc)
    data = tiff.encode(arr, icc)
    assert data[:len(head)] == head and len(head) == plan.header_bytes and len(data) == plan.file_bytes
    assert plan.row_bytes == W * 3 * bits // 8 and plan.strips == -(-H // plan.rows_per_strip)
    got, tags, where = read_tiff(data)
    assert got.dtype.itemsize * 8 == bits and np.array_equal(got, arr)
    assert tags[278] == plan.rows_per_strip and tags[258] == (bits,) * 3
    offs = tags[273] if isinstance(tags[273], tuple) else (tags[273],)
    cnts = tags[279] if isinstance(tags[279], tuple) else (tags[279],)
    assert len(offs) == len(cnts) == plan.strips
    assert offs[0] == plan.header_bytes and sum(cnts) == H * plan.row_bytes
    assert all(o1 == o0 + c0 for o0, c0, o1 in zip(offs, cnts, offs[1:]))  # one behind the other: row y at header + y * row_bytes
    if plan.strips > 1:
        assert cnts[-1] == (H - (plan.strips - 1) * plan.rows_per_strip) * plan.row_bytes
    # TIFF 6.0: every offset in the file lies on a word boundary
    assert all(o % 2 == 0 for o in list(offs) + list(where.values()) + [8])
    assert (tags.get(34675) == icc) if icc else (34675 not in tags)
    img = Image.open(io.BytesIO(data))
    assert img.size == (W, H)
    assert np.array_equal(np.asarray(img), arr if bits == 8 else (arr >> 8).astype(np.uint8))
    if icc:
        assert img.info.get("icc_profile") == icc


def test_strip_counts_cover_one_and_several_with_a_short_last_strip():
    from raw2film_amd import tiff

    assert tiff.header(3, 7, 16)[1].strips == 1
    plan = tiff.header(200, 515, 16)[1]
    assert plan.strips == 3 and 200 % plan.rows_per_strip != 0
    assert tiff.header(85, 515, 16)[1].strips == 2  # 84 + 1 rows


def test_a_file_past_four_gib_is_refused_from_the_geometry_alone():
    from raw2film_amd import _lib, tiff

    with pytest.raises(ValueError, match=r"96\d{8} bytes"):  # 9.6e9 bytes of pixels plus the header: the message names the size
        tiff.header(40000, 40000, 16)
    tiff.header(26000, 26000, 16)  # 4.06e9 bytes: still a classic TIFF
    lib, plan, n = _lib.load(), _lib.TiffPlan(), ctypes.c_size_t()
    assert lib.r2f_tiff_header(40000, 40000, 16, None, 0, None, 0, ctypes.byref(n), ctypes.byref(plan)) == _lib.ETOOLARGE
    assert plan.file_bytes > 1 << 32 and n.value == 0
    # H * row_bytes passes 2^64 here: refused with a saturated size, not wrapped into a small one
    assert lib.r2f_tiff_header(2**31 - 1, 2**31 - 1, 16, None, 0, None, 0, ctypes.byref(n), ctypes.byref(plan)) == _lib.ETOOLARGE
    assert plan.file_bytes == 2**64 - 1 and n.value == 0
    for bad in ((0, 5, 16), (5, 0, 8), (5, 5, 12), (-1, 5, 8)):
        assert lib.r2f_tiff_header(*bad, None, 0, None, 0, ctypes.byref(n), ctypes.byref(plan)) == _lib.EINVAL
    buf = (ctypes.c_uint8 * 16)()
    assert lib.r2f_tiff_header(4, 4, 8, None, 0, buf, 16, ctypes.byref(n), ctypes.byref(plan)) == _lib.EINVAL  # too small a buffer


def test_output_bits_is_validated_before_any_work():
    from raw2film_amd import hip_processor as hp

    for bad in (0, 12, 32, "16", 16.0, None, True):
        with pytest.raises(ValueError, match="output_bits"):
            hp.check_output_bits(bad)
    assert hp.check_output_bits(8) == 8 and hp.check_output_bits(np.int64(16)) == 16
    with pytest.raises(ValueError, match="RGBA8"):
        hp.check_output_bits(16, dst_texture=object())
    assert hp.check_output_bits(8, dst_texture=object()) == 8


@pytest.mark.parametrize("method,args", [("process", (None, None, 6, 0.4)), ("process_preloaded", ({}, None, 6, 0.4)),
                                         ("submit_preloaded", ({}, None, 6, 0.4)), ("process_array", (None, None)),
                                         ("process_tiff", (None, None, 6, 0.4)), ("process_preloaded_tiff", ({}, None, 6, 0.4))])
def test_every_call_that_takes_output_bits_refuses_a_bad_value_first(method, args):
    """On an object that has no context, no device and no attributes at all: the refusal comes before anything is touched."""
    from raw2film_amd.hip_processor import HipProcessor

    proc = object.__new__(HipProcessor)
    fn = getattr(proc, method)
    assert "output_bits" in inspect.signature(fn).parameters or method in ("process_preloaded", "submit_preloaded")
    for bad in (12, "8"):
        with pytest.raises(ValueError, match="output_bits must be 8 or 16"):
            fn(*args, output_bits=bad)
    if method in ("process", "process_preloaded"):
        with pytest.raises(ValueError, match="RGBA8"):
            fn(*args, dst_texture=object(), output_bits=16)


def test_defaults_are_eight_bits_for_renders_and_sixteen_for_tiff():
    from raw2film_amd.hip_processor import HipProcessor

    sig = lambda name: inspect.signature(getattr(HipProcessor, name)).parameters  # noqa: E731
    assert sig("process")["output_bits"].default == 8 and sig("process_array")["output_bits"].default == 8
    assert sig("process_tiff")["output_bits"].default == 16 and sig("process_preloaded_tiff")["output_bits"].default == 16
    assert sig("process_tiff")["output_bits"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(sig("process_tiff"))[:6] == ["self", "src", "negative_film", "grain_size", "grain_sigma", "file"]


def test_result_pools_are_kept_apart_by_dtype():
    from raw2film_amd.results import ResultBuffers

    made = []
    pool8 = ResultBuffers(lambda shape: made.append(("u8", shape)) or np.zeros(shape, np.uint8))
    pool16 = ResultBuffers(lambda shape: made.append(("i16", shape)) or np.zeros(shape, np.int16), np.uint16)
    a, b = pool8.lease((4, 5, 3)), pool16.lease((4, 5, 3))
    assert a.dtype == np.uint8 and b.dtype == np.int16 and made == [("u8", (4, 5, 3)), ("i16", (4, 5, 3))]
    pool8._free.append(a)
    assert pool16.lease((4, 5, 3)) is not a and pool8.lease((4, 5, 3)) is a


def test_tiff_planner_is_clean_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    out = str(tmp_path / "tiff_plan_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "tiff_plan_check.cpp"), os.path.join(ROOT, "raw2film_amd", "csrc", "r2f_tiff_plan.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([out], capture_output=True, text=True, env=env, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    assert "cases ok" in res.stdout
