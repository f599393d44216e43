"""tests/arena.py bites: on CPU tensors, a correct fake kernel passes `check`, and four broken ones -- one element past the row end,
one row past y1, one element in front of the base, one remainder column left unwritten -- each fail it at the right plane / row /
column.  (The GPU battery, tests/test_gpu_write_bounds.py, never writes out of bounds on purpose; this is where the helper is
shown to notice.)"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from arena import CANARY_F32_BITS, TALLEST_TILE_ROWS, Arena, canary_value, guard_elems  # noqa: E402

W, ROWS, R0, R1 = 37, 12, 3, 9  # the view holds 12 rows; the "call" is entitled to rows [3, 9) of it


def fake_kernel(arena, *, past_row_end=False, row_past_y1=False, before_base=False, skip_remainder=False):
    """What a 4-pixels-per-lane kernel does, in NumPy, on the arena's flat memory: rows [R0, R1) of each plane, quads of columns with
    a remainder.  The flags each break it in one way."""
    flat = arena.buf.numpy()  # CPU tensor: shares memory
    stride = arena.strides[0]
    for p in range(3):
        base = arena.start + p * stride
        for y in range(R0, R1 + (1 if row_past_y1 else 0)):
            for x in range(0, W, 4):
                nv = min(4, W - x)
                if skip_remainder and nv < 4:
                    nv -= 1
                flat[base + y * W + x: base + y * W + x + nv] = 0.25 * p + 0.001 * (y * W + x)
    if past_row_end:  # a partial quad stored one element too wide, on the last entitled row of plane 1
        flat[arena.start + stride + (R1 - 1) * W + W] = 7.0
    if before_base:
        flat[arena.start - 1] = 7.0


def make(pad=1, misalign=1):
    return Arena.planes(ROWS, W, pad=pad, misalign=misalign)


def entitled():
    return [(p, (R0, R1)) for p in range(3)]


def test_canary_is_a_quiet_nan_compared_as_bits():
    a = make()
    assert np.isnan(a.buf.numpy()).all()
    assert (a.buf.numpy().view(np.uint32) == CANARY_F32_BITS).all()
    assert canary_value(torch.uint8) == 0xA5 and canary_value(torch.int32) == np.array([0xA5A5A5A5], np.uint32).view(np.int32)[0]
    assert a.start - 1 == guard_elems(W) >= 2 * TALLEST_TILE_ROWS * W * 3 + 4096  # the guard in front of the view (misalign = 1)
    assert a.total - (a.start + 2 * a.strides[0] + ROWS * W) >= 2 * TALLEST_TILE_ROWS * W * 3 + 4096  # the guard behind the view


@pytest.mark.parametrize("pad,misalign", [(0, 0), (1, 0), (4, 1), (0, 1)])
def test_correct_kernel_passes(pad, misalign):
    a = make(pad, misalign)
    assert a.view.data_ptr() % 16 == 4 * misalign
    fake_kernel(a)
    a.check(entitled(), what="correct")
    a.check(a.rows_mask(R0, R1), what="correct, boolean mask")


def test_one_element_past_the_row_end_is_caught():
    a = make()
    fake_kernel(a, past_row_end=True)
    with pytest.raises(AssertionError, match=rf"wrote outside its rows: 1 element\(s\), first at plane 1 / row {R1} / column 0 "):
        a.check(entitled(), what="past row end")


def test_one_row_past_y1_is_caught():
    a = make()
    fake_kernel(a, row_past_y1=True)
    with pytest.raises(AssertionError, match=rf"wrote outside its rows: {3 * W} element\(s\), first at plane 0 / row {R1} / column 0 "):
        a.check(entitled(), what="row past y1")


def test_one_element_in_front_of_the_base_is_caught():
    a = make()
    fake_kernel(a, before_base=True)
    with pytest.raises(AssertionError, match=rf"first at plane 0 / row -1 / column {W - 1} \(element -1 from the view's base\)"):
        a.check(entitled(), what="before base")


def test_an_unwritten_remainder_column_is_caught():
    a = make()
    fake_kernel(a, skip_remainder=True)
    with pytest.raises(AssertionError, match=rf"left {3 * (R1 - R0)} element\(s\) of its rows unwritten, first at plane 0 / row {R0} / column {W - 1} "):
        a.check(entitled(), what="remainder")


def test_a_write_into_the_pad_between_planes_is_caught():
    a = make(pad=4, misalign=0)
    fake_kernel(a)
    a.buf[a.start + ROWS * W + 2] = 1.0  # plane 0's pad
    with pytest.raises(AssertionError, match=rf"first at plane 0 / row {ROWS} / column 2 "):
        a.check(entitled(), what="pad")


def test_uint8_pixels_that_are_the_canary_need_the_expected_values():
    a = Arena.hwc(6, 5, torch.uint8, misalign=1)
    assert a.view.data_ptr() % 4 == 1
    exp = torch.full((6, 5, 3), 7, dtype=torch.uint8)
    exp[2, 1, 0] = 0xA5  # a pixel that really is 165
    a.view[1:4] = exp[1:4]
    a.check([(None, (1, 4))], expected=exp, what="u8")
    with pytest.raises(AssertionError, match=r"left 1 element\(s\) of its rows unwritten, first at row 2 / column 1 / channel 0 "):
        a.check([(None, (1, 4))], what="u8 without expected values")
    a.view[4, 4, 2] = 9
    with pytest.raises(AssertionError, match=r"first at row 4 / column 4 / channel 2 "):
        a.check([(None, (1, 4))], expected=exp, what="u8 overrun")


def test_source_arena_notices_a_scribble():
    src = Arena.holding(torch.arange(3 * 4 * 5, dtype=torch.float32).reshape(3, 4, 5), misalign=1, pad=1)
    src.unchanged("untouched")
    src.view[1, 2, 3] = -1.0
    with pytest.raises(AssertionError, match="changed its source"):
        src.unchanged("scribbled")
    flat = Arena.flat(100, misalign=1)
    flat.check(None, what="nothing entitled, nothing written")
    flat.view[100 - 1] = 3
    flat.check(torch.ones(100, dtype=torch.bool), require_written=False, what="bytes a call may write")
    flat.buf[flat.start + 100] = 3
    with pytest.raises(AssertionError, match="first at offset 100,"):
        flat.check(torch.ones(100, dtype=torch.bool), require_written=False, what="past the capacity")
