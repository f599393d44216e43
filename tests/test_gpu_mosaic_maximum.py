"""The data maximum on the device: r2f_mosaic_maximum against the NumPy model of its definition (tests/levels_model.py), exactly,
on tiny shapes derived from the kernel's load width V and the rows R a block walks per step -- every width at which a row gains a
head, a full vector or a tail, and rows of more than 64 V samples, on which a lane takes a second to a sixth vector: the unrolled
loop, its remainders and the rotation of the level pairs from one of a lane's vectors to the next --, heights around R and the
period, both periods with distinct levels per phase, views that start 1, 2 and 4 samples into an aligned buffer, pitches whose padding holds 0xFFFF, source windows that begin
below the frame's top, row cuts that are no multiple of anything, single largest samples planted where a lane's share begins or
ends (each with a decoy of a larger raw value at a site of a larger black level), the fold into the word, and the refusals."""

import ctypes as C
import zlib

import numpy as np
import pytest

import levels_model as lm
from raw2film_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

V, R = _lib.MOSAIC_MAX_VEC, _lib.MOSAIC_MAX_ROWS
PAD = 0xFFFF


@pytest.fixture(scope="module")
def ctx():
    from raw2film_amd.context import HipContext

    c = HipContext(0)
    yield c
    c.close()


def levels(P):
    """P * P distinct levels, at least 37 apart, in no order along either axis; the largest is not at a corner phase."""
    return [1000 + 37 * ((11 * i + 5) % (P * P)) for i in range(P * P)]


def widths(P):
    return sorted({P, P + 1, V - 1, V, V + 1, 2 * V + 3, 64 * V - 1, 64 * V + 1})


def heights(P):
    return sorted({P, P + 1, R - 1, R + 1, 37})


# Rows on which a lane takes more than one vector.  With nvec the 16-byte vectors of a row, lane l takes vectors l, l + 64, ... (its
# rounds); the kernel folds three rounds per pass of its unrolled loop while l + 128 < nvec, then up to two more.  Aligned (head 0) /
# one sample off (head 7), nvec is: 65 / 64 -- round 1 for lane 0 only, through the first remainder; 129 / 128 -- rounds 0 .. 2
# unrolled for lane 0, two remainders for the others; 193 / 192 -- one unrolled pass, then round 3 as a remainder; 384 / 383 -- two
# unrolled passes, or one and both remainders (lane 63).  Every one ends in a tail.
WIDE = (64 * V + V, 128 * V + 9, 192 * V + V + 3, 384 * V + 5)


_MOSAICS = {}


def mosaic(kind, P, H, W, gy0=0):
    """uint16 rows [gy0, gy0 + H) of a frame.  tight: every sample within 40 of its site's level, so that a level taken from another
    phase moves the answer by tens or hundreds; below: every sample under its level (d = 0); mixed: any 16 bits."""
    key = (kind, P, H, W, gy0)
    if key not in _MOSAICS:
        rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
        plane = lm.black_plane(levels(P), P, H, W, gy0)
        if kind == "tight":
            m = plane + rng.integers(-40, 41, (H, W))
        elif kind == "below":
            m = plane - rng.integers(1, 41, (H, W))
        else:
            m = rng.integers(0, 65536, (H, W))
        _MOSAICS[key] = m.astype(np.uint16)
    return _MOSAICS[key]


def place(rows, pitch=None, offset=0):
    """The rows on the device as a view `offset` samples into an aligned buffer, `pitch` samples apart, padding and slack 0xFFFF."""
    n, W = rows.shape
    pitch = W if pitch is None else pitch
    host = np.full(offset + n * pitch + 8, PAD, np.uint16)
    body = host[offset:offset + n * pitch].reshape(n, pitch)
    body[:, :W] = rows
    buf = torch.from_numpy(host.view(np.int16)).cuda()
    assert buf.data_ptr() % 16 == 0
    return torch.as_strided(buf, (n, W), (pitch, 1), offset)


def measure(ctx, view, gy0, H, P, black, y0, y1, preset=0, pitch=None):
    """The entry point itself on a source window -> (rc, the word afterwards)."""
    word = torch.full((1,), preset, dtype=torch.int32, device="cuda")
    rc = ctx._lib.r2f_mosaic_maximum(ctx._h, view.data_ptr(), gy0, int(view.shape[0]), int(view.stride(0)) if pitch is None else pitch, H,
                                     int(view.shape[1]), P, (C.c_int32 * len(black))(*black), y0, y1, word.data_ptr(), ctx._stream())
    return rc, int(word.item())


@pytest.mark.parametrize("P", [2, 6])
def test_every_width_and_height_equals_the_model(ctx, P):
    black = levels(P)
    for W in widths(P):
        for h in heights(P):
            H, cut = (h, (0, h)) if h >= P else (P + 1, (1, 1 + h))  # (a frame below the period is refused: fewer rows are a cut)
            for kind in ("tight", "mixed"):
                m = mosaic(kind, P, H, W)
                want = lm.data_maximum(m, black, P, cut)
                assert measure(ctx, place(m), 0, H, P, black, *cut) == (0, want), (kind, W, h)
                if kind == "tight":
                    assert 0 < want <= 40
    assert len(set(black)) == P * P


@pytest.mark.parametrize("P", [2, 6])
def test_samples_below_their_black_level_give_zero(ctx, P):
    for W, H in ((2 * V + 3, 37), (64 * V + 1, P + 1)):
        m = mosaic("below", P, H, W)
        assert lm.data_maximum(m, levels(P), P) == 0 and int(m.max()) > 0
        assert measure(ctx, place(m), 0, H, P, levels(P), 0, H) == (0, 0)
        assert measure(ctx, place(m, W + 1, 1), 0, H, P, levels(P), 0, H) == (0, 0)
    # black = 0 everywhere: the plain maximum; black = 65535: 0 whatever the samples
    m = mosaic("mixed", P, 37, 64 * V + 1)
    assert measure(ctx, place(m), 0, 37, P, [0] * (P * P), 0, 37) == (0, int(m.max()))
    assert measure(ctx, place(m), 0, 37, P, [65535] * (P * P), 0, 37) == (0, 0)


@pytest.mark.parametrize("P", [2, 6])
def test_alignment_and_pitch_select_the_loads_not_the_samples(ctx, P):
    """The padding holds 0xFFFF, above every sample's d: a load that strays into it, or a head or tail counted twice or not at all,
    changes the answer."""
    black = levels(P)
    for W in (V - 1, V + 1, 2 * V + 3, 64 * V + 1):
        m = mosaic("tight", P, 37, W)
        want = lm.data_maximum(m, black, P)
        for offset in (0, 1, 2, 4):
            for pitch in (W, W + 1, W + 7):
                assert measure(ctx, place(m, pitch, offset), 0, 37, P, black, 0, 37) == (0, want), (W, offset, pitch)


@pytest.mark.parametrize("P", [2, 6])
def test_the_phase_is_the_frames_whatever_the_window_and_the_cut(ctx, P):
    black, H, W = levels(P), 37, 2 * V + 3
    for gy0 in (0, 1, 5):
        rows = mosaic("tight", P, H - gy0, W, gy0)  # the window holds frame rows [gy0, H)
        view = place(rows, W + 1, 1)
        for y0, y1 in ((gy0, H), (gy0 + 1, gy0 + 2), (H - 1, H), (gy0 + 3, gy0 + 3 + R + 1), (7, 7 + P + 1), (gy0 + 2, H - 3), (9, 9)):
            want = lm.data_maximum(rows, black, P, (y0, y1), gy0)
            assert measure(ctx, view, gy0, H, P, black, y0, y1) == (0, want), (gy0, y0, y1)
    assert measure(ctx, view, 5, H, P, black, 9, 9, preset=77) == (0, 77)  # y0 == y1: nothing read, nothing folded


@pytest.mark.parametrize("P", [2, 6])
def test_rows_of_several_rounds_equal_the_model(ctx, P):
    """Tight mosaics: a level pair used one round early or late puts some sample of the row tens or hundreds above every true d."""
    black, H = levels(P), P + 3
    for W in WIDE:
        m = mosaic("tight", P, H, W)
        want = lm.data_maximum(m, black, P)
        assert 0 < want <= 40
        for offset, pitch in ((0, W + (-W) % V), (1, W + (-W) % V), (0, W + 1), (2, W + 7)):
            assert measure(ctx, place(m, pitch, offset), 0, H, P, black, 0, H) == (0, want), (W, offset, pitch)
        cut = (2, H - 1)
        assert measure(ctx, place(m, W + 1, 1), 0, H, P, black, *cut) == (0, lm.data_maximum(m, black, P, cut)), W


def _head(view):
    return ((16 - view.data_ptr() % 16) % 16) // 2


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("P", [2, 6])
def test_a_single_largest_sample_is_found_wherever_it_lies(ctx, P, offset):
    black, H, W = levels(P), 23, 64 * V + 3
    y0, y1 = 3, 3 + 2 * R + 2  # (its first row odd, its last even: both row phases of a quad)
    base = mosaic("tight", P, H, W)
    table = lm.black_plane(black, P, H, W)
    outside = base.copy()
    outside[y0 - 1], outside[y1] = 65535, 65535  # the rows just outside the cut hold larger samples: they must not count
    pitch = W + 5  # a multiple of V: every row starts as far from a 16-byte boundary as the first
    assert pitch % V == 0
    head = _head(place(base, pitch, offset))
    assert head == (7 if offset else 0)
    nvec = (W - head) // V
    cols = {0, W - 1, V - 1, 64 * V - 1, head + V - 1, head + nvec * V - 1, head + nvec * V, max(head - 1, 0), head}
    decoys = 0
    for y in (y0, y1 - 1):
        for x in sorted(cols):
            m = outside.copy()
            m[y, x] = table[y, x] + 5000
            # a decoy: a larger raw value at a site of the cut whose level is larger still -- smaller after the subtraction
            higher = np.argwhere((table[y0:y1] > table[y, x] + 1))
            if len(higher):
                dy, dx = higher[(7 * x + y) % len(higher)]
                m[y0 + dy, dx] = int(m[y, x]) + 1
                assert m[y0 + dy, dx] > m[y, x] and m[y0 + dy, dx] - table[y0 + dy, dx] < 5000
                decoys += 1
            assert lm.data_maximum(m, black, P, (y0, y1)) == 5000
            assert measure(ctx, place(m, pitch, offset), 0, H, P, black, y0, y1) == (0, 5000), (y, x)
    assert decoys >= len(cols)  # (only a sample at the phase of the largest level has none)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("P", [2, 6])
def test_a_single_largest_sample_is_found_in_a_vector_of_every_round(ctx, P, offset):
    """The planted sample of the test above, in a vector of each round a lane takes of a row of 384 vectors (383 behind a head of
    7) -- at even and odd places of the vector, so in either half of each of its four pairs over the rounds --, and of each row
    length of WIDE in its last round; every one beside a decoy whose raw value is larger and whose level is larger still."""
    black, H = levels(P), 9
    y0, y1 = 2, 7
    for W in WIDE[::-1]:
        base = mosaic("tight", P, H, W).copy()
        base[y0 - 1], base[y1] = 65535, 65535
        table = lm.black_plane(black, P, H, W)
        pitch = W + (-W) % V
        head = _head(place(base, pitch, offset))
        assert head == (7 if offset else 0)
        nvec = (W - head) // V
        rounds = range((nvec + 63) // 64) if W == WIDE[-1] else [(nvec - 1) // 64]
        spots = []
        for r in rounds:
            for lane in sorted({0, (11 * r + 5) % 64, 63}):
                i = 64 * r + lane
                if i < nvec:
                    spots.append((y0 + (r + lane) % (y1 - y0), head + V * i + (3 * r + lane) % V))
        assert len({(x - head) // V // 64 for _, x in spots}) == len(rounds)
        if W == WIDE[-1]:  # all six rounds, every place of a vector
            assert len(rounds) == 6 and {(x - head) % V for _, x in spots} == set(range(V))
        decoys = 0
        for y, x in spots:
            m = base.copy()
            m[y, x] = table[y, x] + 5000
            higher = np.argwhere(table[y0:y1] > table[y, x] + 1)
            if len(higher):
                dy, dx = higher[(7 * x + y) % len(higher)]
                m[y0 + dy, dx] = int(m[y, x]) + 1
                assert m[y0 + dy, dx] > m[y, x] and m[y0 + dy, dx] - table[y0 + dy, dx] < 5000
                decoys += 1
            assert lm.data_maximum(m, black, P, (y0, y1)) == 5000
            assert measure(ctx, place(m, pitch, offset), 0, H, P, black, y0, y1) == (0, 5000), (W, y, x)
        assert decoys >= len(spots) // 2


@pytest.mark.parametrize("P", [2, 6])
def test_the_word_folds_bands_in_any_order(ctx, P):
    black, H, W = levels(P), 37, 2 * V + 3
    m = mosaic("mixed", P, H, W)
    whole = lm.data_maximum(m, black, P)
    view = place(m, W + 7, 2)
    assert measure(ctx, view, 0, H, P, black, 0, H, preset=whole + 1) == (0, whole + 1)  # a word above the data's maximum stays
    assert measure(ctx, view, 0, H, P, black, 0, H, preset=whole - 1) == (0, whole)
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    parts = []
    for y0, y1 in ((30, 37), (5, 30), (0, 5)):  # three uneven bands, the last one first
        assert ctx.mosaic_maximum(view, black, rows=(y0, y1), out=word) is word
        parts.append(lm.data_maximum(m, black, P, (y0, y1)))
    assert int(word.item()) == whole == max(parts)
    # the context's method: a profile or a table, int16 and uint16 tensors as the same bits, the word of its own
    assert ctx.mosaic_maximum(view, black) == whole and ctx.mosaic_maximum(view, black, period=P, rows=(5, 30)) == parts[1]
    assert ctx.mosaic_maximum(view.contiguous().view(torch.uint16), black) == whole
    from raw2film_amd.raw import RawProfile, XTransProfile

    prof = RawProfile("GRBG", black=black) if P == 2 else XTransProfile(black=black)
    assert ctx.mosaic_maximum(view, prof) == whole
    u32 = torch.zeros(1, dtype=torch.uint32, device="cuda")
    assert ctx.mosaic_maximum(view, prof, out=u32) is u32 and int(u32.view(torch.int32).item()) == whole


def test_context_method_refusals(ctx):
    m = place(mosaic("mixed", 2, 37, 19))
    for bad in (dict(mosaic=m.cpu()), dict(mosaic=m[:, ::2]), dict(mosaic=m[:1]), dict(mosaic=m.float()), dict(black=[0] * 5), dict(black=[0] * 4, period=6),
                dict(black=None), dict(out=torch.zeros(2, dtype=torch.int32, device="cuda")), dict(out=torch.zeros(1, dtype=torch.int64, device="cuda")),
                dict(out=torch.zeros(1, dtype=torch.int32)), dict(mosaic=m[:5, :5], black=[0] * 36)):
        kw = {"mosaic": m, "black": [0] * 4, **bad}
        with pytest.raises(ValueError):
            ctx.mosaic_maximum(kw.pop("mosaic"), kw.pop("black"), **kw)
    with pytest.raises(ValueError, match="black level"):
        ctx.mosaic_maximum(m, [0, 0, 70000, 0])


@pytest.mark.parametrize("P", [2, 6])
def test_each_refusal_leaves_the_word_untouched(ctx, P):
    black, H, W = levels(P), 37, 2 * V + 3
    view = place(mosaic("mixed", P, H, W))
    lib, h, s = ctx._lib, ctx._h, ctx._stream()
    word = torch.full((1,), 12345, dtype=torch.int32, device="cuda")
    table = (C.c_int32 * (P * P))(*black)

    def call(src=view.data_ptr(), gy0=0, nrows=H, pitch=W, H=H, W=W, period=P, black=table, y0=0, y1=H, dst=word.data_ptr()):
        return lib.r2f_mosaic_maximum(h, src, gy0, nrows, pitch, H, W, period, black, y0, y1, dst, s)

    bad_levels = [list(black) for _ in range(2)]
    bad_levels[0][P * P - 1], bad_levels[1][1] = 65536, -1
    refused = [dict(period=3), dict(period=0), dict(period=4), dict(H=P - 1, y1=P - 1), dict(W=P - 1, pitch=P - 1), dict(y0=5, y1=4),
               dict(y0=-1), dict(y1=H + 1), dict(pitch=W - 1), dict(src=None), dict(black=None), dict(dst=None),
               dict(black=(C.c_int32 * (P * P))(*bad_levels[0])), dict(black=(C.c_int32 * (P * P))(*bad_levels[1])),
               dict(nrows=H - 1), dict(gy0=1), dict(gy0=2, nrows=10, y0=1, y1=5), dict(gy0=2, nrows=10, y0=5, y1=13), dict(gy0=-1), dict(nrows=-1)]
    for kw in refused:
        assert call(**kw) == _lib.EINVAL, kw
        assert b"mosaic_maximum" in lib.r2f_last_error(h)
    assert lib.r2f_mosaic_maximum(None, view.data_ptr(), 0, H, W, H, W, P, table, 0, H, word.data_ptr(), s) == _lib.EINVAL
    torch.cuda.synchronize()
    assert int(word.item()) == 12345
    assert call(y0=9, y1=9) == _lib.OK and call(y0=H, y1=H) == _lib.OK and int(word.item()) == 12345  # no rows: no launch
    assert call() == _lib.OK and int(word.item()) == max(12345, lm.data_maximum(view.cpu().numpy(), black, P))
