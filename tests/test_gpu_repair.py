"""r2f_mosaic_repair on the device against the NumPy model of include/r2f.h (tests/repair_model.py), bit for bit and count for count:
frames from 6 x 6 to several row groups and past three rounds of a lane's vectors; all four Bayer tables and four shifts of the
X-Trans pattern with different levels at every site; pitched, 2-byte aligned and differently pitched buffers; every single-row band
against the whole call; the constructed cases of the hot test; random fields that the model repairs a stated share of."""

import ctypes as C

import numpy as np
import pytest

import repair_model as model
from raw2film_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

V, R = _lib.MOSAIC_REPAIR_VEC, _lib.MOSAIC_REPAIR_ROWS
BLACK = (512, 520, 500, 512)
BLACK36 = tuple(400 + 7 * ((5 * i + 3) % 36) for i in range(36))
ONE_TILE, GROUPS, ROUNDS = (37, 70), (70, 200), (9, 3 * 64 * V + 67)  # (the last: a lane's levels go once round their three registers)
SHORT = (9, 11)  # with a source 3 samples past a 16-byte boundary: a head of 5 and fewer than 8 samples behind it


@pytest.fixture(scope="module")
def ctx():
    from raw2film_amd.context import HipContext

    c = HipContext(0)
    yield c
    c.close()


def plan(P, black, threshold, q, mn, shape, cfa=None):
    out = _lib.RepairParams()
    ids = None if cfa is None else (C.c_int32 * 36)(*[int(v) for v in np.asarray(cfa).ravel()])
    rc = _lib.load().r2f_mosaic_repair_plan(P, ids, (C.c_double * len(black))(*black), threshold, q, mn, shape[0], shape[1], C.byref(out))
    assert rc == _lib.OK
    return out


def placed(frame, pitch, mis, fill=None):
    """`frame` (or a buffer of its shape holding `fill`) as an int16 CUDA view with rows `pitch` samples apart that begins `mis` samples
    past a 256-byte boundary."""
    H, W = frame.shape
    buf = torch.full((mis + H * pitch + 64,), -1 if fill is None else fill, dtype=torch.int16, device="cuda")
    view = torch.as_strided(buf, (H, W), (pitch, 1), mis)
    if fill is None:
        view.copy_(torch.from_numpy(frame.view(np.int16)))
    return view


def run(ctx, frame, params, rows=None, pitch=None, mis=0, dst_pitch=None, dst_mis=0, dst=None):
    """-> (dst as uint16 NumPy, the count the call added)"""
    H, W = frame.shape
    src = placed(frame, pitch or W, mis)
    if dst is None:
        dst = placed(frame, dst_pitch or W, dst_mis, fill=0x5A5A)
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    y0, y1 = rows or (0, H)
    rc = ctx._lib.r2f_mosaic_repair(ctx._h, src.data_ptr(), 0, H, int(src.stride(0)), H, W, C.byref(params), dst.data_ptr(),
                                    int(dst.stride(0)), y0, y1, count.data_ptr(), ctx._stream())
    assert rc == _lib.OK, ctx._lib.r2f_last_error(ctx._h)
    torch.cuda.synchronize()
    assert torch.equal(src.cpu(), torch.from_numpy(frame.view(np.int16)))  # the source is unchanged
    return dst.cpu().numpy().view(np.uint16), int(count.item())


def check(ctx, frame, P, black, threshold, q, mn, cfa=None, min_share=0.0, **kw):
    want, hot = model.repair(frame, P, black, threshold, q, mn, cfa)
    assert hot.mean() >= min_share, hot.mean()
    got, n = run(ctx, frame, plan(P, black, threshold, q, mn, frame.shape, cfa), **kw)
    assert np.array_equal(got, want), (int((got != want).sum()), np.argwhere(got != want)[:5])
    assert n == int(hot.sum())
    return want, hot


# ---- frames, tables and profiles: random fields that do not pass vacuously
@pytest.mark.parametrize("mn", [4, 3])
@pytest.mark.parametrize("shape", [(6, 6), (33, 65), ONE_TILE, GROUPS, ROUNDS], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_random_bayer_field_is_the_models(ctx, shape, mn):
    frame = model.field(shape, 100 * shape[0] + shape[1])
    check(ctx, frame, 2, BLACK, 1000, 32, mn, min_share=0.02 if shape[0] >= 33 else 0.0)


@pytest.mark.parametrize("shape", [(33, 65), GROUPS], ids=lambda s: f"{s[0]}x{s[1]}")
def test_three_and_four_neighbours_differ(ctx, shape):
    frame = model.field(shape, 7)
    a, hot4 = check(ctx, frame, 2, BLACK, 1000, 32, 4, min_share=0.02)
    b, hot3 = check(ctx, frame, 2, BLACK, 1000, 32, 3, min_share=0.02)
    assert not np.array_equal(a, b) and hot3.sum() > hot4.sum()


@pytest.mark.parametrize("pattern, black", [("RGGB", (512, 520, 500, 531)), ("BGGR", (531, 500, 520, 512)), ("GRBG", (520, 512, 531, 500)),
                                            ("GBRG", (500, 531, 512, 520))])
def test_all_four_bayer_tables_with_four_different_levels(ctx, pattern, black):
    from raw2film_amd.raw import HotPixels, RawProfile

    frame = model.field(ONE_TILE, 31)
    want, hot = model.repair(frame, 2, black, 1000, 32, 4)
    params = HotPixels(1000).plan(RawProfile(pattern, black=black), *ONE_TILE)
    got, n = run(ctx, frame, params)
    assert hot.mean() >= 0.02 and np.array_equal(got, want) and n == int(hot.sum())


@pytest.mark.parametrize("shape", [(6, 6), ONE_TILE, GROUPS, ROUNDS], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("shift", [(0, 0), (1, 2), (4, 5), (3, 1)], ids=lambda s: f"shift{s[0]}{s[1]}")
def test_xtrans_canonical_and_three_shifts_with_36_different_levels(ctx, shift, shape):
    from raw2film_amd.raw import HotPixels, XTransProfile

    cfa = model.cfa_ids(model.CANONICAL, *shift)
    frame = model.field(shape, 17 + shift[0])
    want, hot = check(ctx, frame, 6, BLACK36, 1000, 32, 3, cfa, min_share=0.02 if shape[0] >= 33 else 0.0)
    params = HotPixels(1000, min_neighbours=3).plan(XTransProfile(model.shifted_pattern(*shift), black=BLACK36), *shape)
    got, n = run(ctx, frame, params)  # the record's plan is the same table
    assert np.array_equal(got, want) and n == int(hot.sum())


# ---- sources and bands
@pytest.mark.parametrize("P", [2, 6])
@pytest.mark.parametrize("kw", [dict(pitch=77), dict(mis=1), dict(mis=3, pitch=73), dict(dst_pitch=91), dict(pitch=72, dst_pitch=80, dst_mis=1),
                                dict(mis=5, dst_mis=5)], ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_pitch_and_alignment_select_accesses_not_samples(ctx, P, kw):
    black, cfa = (BLACK, None) if P == 2 else (BLACK36, model.cfa_ids(model.CANONICAL, 2, 3))
    check(ctx, model.field(ONE_TILE, 5), P, black, 1000, 32, 4, cfa, min_share=0.02, **kw)


@pytest.mark.parametrize("P", [2, 6])
def test_a_row_of_fewer_than_8_samples_past_its_head(ctx, P):
    black, cfa = (BLACK, None) if P == 2 else (BLACK36, model.cfa_ids(model.CANONICAL, 0, 0))
    check(ctx, model.field(SHORT, 9), P, black, 1000, 32, 3, cfa, mis=3)
    check(ctx, model.field((8, 7), 9), P, black, 1000, 32, 3, cfa, mis=1)  # the head is the whole row


@pytest.mark.parametrize("P", [2, 6])
def test_every_single_row_band_is_the_whole_calls_rows_and_count(ctx, P):
    black, cfa = (BLACK, None) if P == 2 else (BLACK36, model.cfa_ids(model.CANONICAL, 1, 1))
    frame = model.field(ONE_TILE, 3)
    H, W = frame.shape
    params = plan(P, black, 1000, 32, 4, frame.shape, cfa)
    whole, n_whole = run(ctx, frame, params)
    want, hot = model.repair(frame, P, black, 1000, 32, 4, cfa)
    assert np.array_equal(whole, want) and n_whole == int(hot.sum()) > 0
    dst = placed(frame, W + 3, 1, fill=0x5A5A)
    total = 0
    for y in range(H):
        got, n = run(ctx, frame, params, rows=(y, y + 1), pitch=W + 5, mis=y % 8, dst=dst)
        assert n == int(hot[y].sum()), y
        assert np.array_equal(got[y], whole[y]) and (got[y + 1:] == 0x5A5A).all(), y  # (and the rows below are not yet written)
        total += n
    assert np.array_equal(got, whole) and total == n_whole


# ---- constructed cases
def flat(shape=(16, 24), level=1000):
    return np.full(shape, level, np.uint16)


def test_one_hot_sample_on_each_site_of_the_period(ctx):
    for P, black, cfa in ((2, BLACK, None), (6, BLACK36, model.cfa_ids(model.CANONICAL, 0, 0))):
        for py in range(P):
            for px in range(P):
                frame = flat()
                frame[6 + py, 6 + px] = 30000
                want, hot = check(ctx, frame, P, black, 5000, 32, 4, cfa)
                assert hot.sum() == 1 and hot[6 + py, 6 + px]
                # every neighbour's t is 1000 less its own level: the largest of them, on the centre's level
                levels = model.black_plane(black, P, 16, 24)
                offs = model.neighbour_table(P, cfa)[((6 + py) % P) * P + (6 + px) % P]
                assert want[6 + py, 6 + px] == max(1000 - levels[6 + py + dy, 6 + px + dx] for dy, dx in offs) + levels[6 + py, 6 + px]


def test_two_hot_samples_at_distance_2_are_repaired_with_3_neighbours_and_left_with_4(ctx):
    frame = flat()
    frame[8, 8] = frame[8, 10] = 30000
    _, hot3 = check(ctx, frame, 2, BLACK, 5000, 32, 3)
    _, hot4 = check(ctx, frame, 2, BLACK, 5000, 32, 4)
    assert hot3.sum() == 2 and hot3[8, 8] and hot3[8, 10] and not hot4.any()


def test_a_hot_sample_in_the_2_sample_ring_is_unchanged(ctx):
    for y, x in ((0, 7), (1, 7), (7, 0), (7, 1), (15, 7), (14, 7), (7, 23), (7, 22), (1, 1), (14, 22)):
        frame = flat()
        frame[y, x] = 30000
        want, hot = check(ctx, frame, 2, BLACK, 5000, 32, 3)
        assert not hot.any() and np.array_equal(want, frame)
    frame = flat()
    frame[2, 2] = frame[13, 21] = 30000  # the first sites inside the ring
    assert check(ctx, frame, 2, BLACK, 5000, 32, 4)[1].sum() == 2
    cfa = model.cfa_ids(model.CANONICAL, 0, 0)
    for y, x in ((0, 7), (7, 0), (15, 8), (8, 23)):  # X-Trans: a neighbour of these lies outside the frame
        frame = flat()
        frame[y, x] = 30000
        assert not check(ctx, frame, 6, BLACK36, 5000, 32, 3, cfa)[1].any()


def test_t_equal_to_the_threshold_is_not_hot_and_one_above_is(ctx):
    frame = flat()
    frame[8, 9] = 520 + 5000  # site (0, 1): t = 5000
    assert not check(ctx, frame, 2, BLACK, 5000, 32, 4)[1].any()
    assert check(ctx, frame, 2, BLACK, 4999, 32, 4)[1].sum() == 1


def test_q_t_equal_to_256_t_k_is_not_below(ctx):
    frame = flat(level=512 + 500)  # site (0, 0) and (1, 1): t_k = 500
    frame[8, 8] = 512 + 4000  # 32 * 4000 == 256 * 500
    assert not check(ctx, frame, 2, BLACK, 1000, 32, 4)[1].any()
    frame[8, 8] = 512 + 4001
    want, hot = check(ctx, frame, 2, BLACK, 1000, 32, 4)
    assert hot.sum() == 1 and want[8, 8] == 512 + 500
    frame[6, 8] = 512 + 501  # one neighbour a step up: three below, and the largest of THOSE is taken
    assert not check(ctx, frame, 2, BLACK, 1000, 32, 4)[1].any()
    want, hot = check(ctx, frame, 2, BLACK, 1000, 32, 3)
    assert hot.sum() == 1 and want[8, 8] == 512 + 500


def test_samples_below_their_black_level_count_as_zero(ctx):
    frame = flat(level=100)  # every t is 0
    frame[8, 8] = 512 + 1
    want, hot = check(ctx, frame, 2, BLACK, 0, 1, 4)  # 1 * 1 > 256 * 0
    assert hot.sum() == 1 and want[8, 8] == 512  # max t_k = 0, on the centre's level: not the neighbours' raw 100
    frame[8, 8] = 300  # the centre itself below its level: t = 0 is not above a threshold of 0
    assert not check(ctx, frame, 2, BLACK, 0, 255, 3)[1].any()


def test_an_xtrans_centre_with_a_larger_level_of_its_own_ends_at_the_top_of_the_range(ctx):
    """The result of a hot centre is max t_k + black_centre with every such t_k < t_centre (q <= 255), so it stays below the centre's
    own raw value and the clamp at 65535 never binds: the nearest case is a centre at 65535 on a level of 65000 whose neighbours, on
    levels of 0, are just below it -- 65532 -- where a clamp that bound early, or a sum taken in 16 bits, would show."""
    cfa = model.cfa_ids(model.CANONICAL, 0, 0)
    black = [0] * 36
    y, x = 7, 8
    black[(y % 6) * 6 + x % 6] = 65000  # the centre's own level; its neighbours' phases keep 0
    offs = model.neighbour_table(6, cfa)[(y % 6) * 6 + x % 6]
    assert all(black[((y + dy) % 6) * 6 + (x + dx) % 6] == 0 for dy, dx in offs)
    frame = flat(level=130)
    frame[y, x] = 65535  # t = 535
    want, hot = check(ctx, frame, 6, black, 100, 255, 4, cfa)
    assert hot[y, x] and want[y, x] == 65130
    frame = flat(level=532)
    frame[y, x] = 65535  # 255 * 535 = 136425 > 256 * 532 = 136192: below, all four; 532 + 65000
    want, hot = check(ctx, frame, 6, black, 100, 255, 4, cfa)
    assert hot[y, x] and want[y, x] == 65532
    frame = flat(level=533)  # 256 * 533 = 136448: not below
    frame[y, x] = 65535
    assert not check(ctx, frame, 6, black, 100, 255, 3, cfa)[1][y, x]
