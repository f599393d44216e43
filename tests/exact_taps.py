"""Frames and stencils on which a stencil stage has ONE right answer, bit for bit (no GPU here).

Samples are integers 0 .. 15 and taps are integers -15 .. 15 times 2^-12, with 15 * sum |tap * 2^12| < 2^24 per channel: every
product and every partial sum of the correlation is then an integer below 2^24 in units of 2^-12, exactly representable in
float32.  A direct form must return the integer correlation exactly whatever its tap order, pairing of mirrored columns,
half-weight centre column (w / 2 and x + x are exact too), row partials or FMA contraction; the float64 FFT form returns it to
float64 noise.  A wrong, missing or doubled tap, a wrong reflection, a wrong halo row or a stale LDS column moves an output by a
whole unit, however small the tap -- where the contract tolerance (1e-5 relative at a 1e-3 floor) swallows a tap of relative
weight 1e-6 (tests/test_exact_taps_host.py shows both).

The tap families are the zero patterns no dense box or disc has: the planner (build_stream in raw2film_amd/csrc/r2f_plan.cpp)
emits only the 4-tap chunks between a row step's first and last live one, skips empty row steps, masks the first and last
chunk's dead columns, pads mirrored boxes and splits row steps into LDS phases; the FFT form crops the tap box and moves the
anchor.  Each family returns `(taps, name)`: taps float32 (kh, kw, 1 or 3), anchor (kh // 2, kw // 2) like cv.filter2D.
"""

import numpy as np

SCALE = 4096  # taps are integers / 2^12
SAMPLE_MAX = 15
TAP_MAX = 15


def reflect101(i: int, n: int) -> int:
    """BORDER_REFLECT_101 index, any number of reflections: ... c b | a b c d | c b ..."""
    if n == 1:
        return 0
    p = 2 * n - 2
    i %= p
    return i if i < n else p - i


def frame(rng, H: int, W: int) -> np.ndarray:
    return rng.integers(0, SAMPLE_MAX + 1, (H, W, 3)).astype(np.float32)


def tap_ints(k) -> np.ndarray:
    """The taps in units of 2^-12 (int64); asserts that they are integral and that every partial sum stays below 2^24."""
    k = np.asarray(k)
    assert k.dtype == np.float32 and k.ndim == 3 and k.shape[2] in (1, 3)
    scaled = k.astype(np.float64) * SCALE
    ki = np.rint(scaled).astype(np.int64)
    assert np.array_equal(ki, scaled), "taps are not integers / 4096"
    assert SAMPLE_MAX * int(np.abs(ki).sum(axis=(0, 1)).max()) < 2 ** 24, "partial sums would leave the exact range of float32"
    return ki


def reference(img, k) -> np.ndarray:
    """The reflect-101 correlation of `img` (H, W, 3) with `k`, anchor (kh // 2, kw // 2), in int64 units of 2^-12."""
    ki = tap_ints(k)
    xi = np.asarray(img).astype(np.int64)
    assert np.array_equal(xi, img) and xi.min() >= 0 and xi.max() <= SAMPLE_MAX
    H, W = xi.shape[:2]
    kh, kw, kc = ki.shape
    ay, ax = kh // 2, kw // 2
    rows = np.array([reflect101(y, H) for y in range(-ay, H + kh - 1 - ay)])
    cols = np.array([reflect101(x, W) for x in range(-ax, W + kw - 1 - ax)])
    out = np.zeros((H, W, 3), np.int64)
    tmp = np.empty((H, W), np.int64)
    for c in range(3):
        pad = np.ascontiguousarray(xi[..., c][rows][:, cols])
        kcc = ki[..., c if kc == 3 else 0]
        acc = np.zeros((H, W), np.int64)
        for i, j in zip(*np.nonzero(kcc)):
            np.multiply(pad[i:i + H, j:j + W], kcc[i, j], out=tmp)
            acc += tmp
        out[..., c] = acc
    return out


def source_rows(y0: int, y1: int, above: int, below: int, H: int):
    """Rows [lo, hi) of an H-row frame that outputs [y0, y1) read through taps reaching `above` rows up and `below` rows down
    (plan::stencil_source_rows restated).  above = anchor row - first box row, below = last box row - anchor row, as run_stencil
    derives them: they sum to the box height - 1, and either is negative when the tap box does not hold the anchor row."""
    if H == 1:
        return 0, 1
    lo, hi = y0 - above, y1 - 1 + below
    assert lo <= hi
    p = 2 * (H - 1)
    a, b = reflect101(lo, H), reflect101(hi, H)
    has_first = -(-lo // p) * p <= hi  # a multiple of the period: row 0
    has_last = -(-(lo - (H - 1)) // p) * p + (H - 1) <= hi  # half a period further: row H - 1
    return (0 if has_first else min(a, b)), (H - 1 if has_last else max(a, b)) + 1


def reach(k, c: int = 0):
    """(above, below) of channel c's tap box: what run_stencil hands to stencil_source_rows."""
    nz = np.nonzero(np.asarray(k)[..., c if k.shape[2] == 3 else 0])
    i_lo, i_hi = int(nz[0].min()), int(nz[0].max())
    return k.shape[0] // 2 - i_lo, i_hi - k.shape[0] // 2


def tap_box(k, c: int = 0):
    nz = np.nonzero(np.asarray(k)[..., c if k.shape[2] == 3 else 0])
    return int(nz[0].min()), int(nz[0].max()), int(nz[1].min()), int(nz[1].max())


def row_steps(k, c: int, Q: int, sym: bool = False):
    """build_stream restated for one channel: per non-empty row step m (input row m feeds output rows q of a lane through kernel
    rows m - q) the tuple (entries, live columns of the first chunk, live columns of the last chunk); and the number of skipped
    (empty) row steps.  sym: the mirrored list -- the box padded with zero columns to a half-width of 2 (mod 4), left half only."""
    i_lo, i_hi, j_lo, j_hi = tap_box(k, c)
    box = np.asarray(k)[i_lo:i_hi + 1, j_lo:j_hi + 1, c if k.shape[2] == 3 else 0] != 0
    bh, bw = box.shape
    if sym:
        pad = (2 - ((bw - 1) // 2) % 4) % 4
        box = np.pad(box, ((0, 0), (pad, pad)))
        box = box[:, :(box.shape[1] - 1) // 2 + 1]
    ncols = box.shape[1]
    nch = (ncols + 3) // 4
    box = np.pad(box, ((0, 0), (0, 4 * nch - ncols)))
    steps, skipped = [], 0
    for m in range(bh + Q - 1):
        rows = [m - q for q in range(Q) if 0 <= m - q < bh]
        live = box[rows].any(axis=0).reshape(nch, 4)
        chunks = np.nonzero(live.any(axis=1))[0]
        if len(chunks) == 0:
            skipped += 1
            continue
        steps.append((int(chunks[-1] - chunks[0] + 1), int(live[chunks[0]].sum()), int(live[chunks[-1]].sum())))
    return steps, skipped


# ------------------------------------------------------------------------------------------------ tap families
def _weights(rng, shape, signed):
    v = rng.integers(1, TAP_MAX + 1, shape)
    if signed:
        v = v * rng.choice((-1, 1), shape)
    return v


def _finish(ki, name, signed):
    k = (ki.astype(np.float64) / SCALE).astype(np.float32)
    tap_ints(k)
    return k, f"{name}-{ki.shape[0]}x{ki.shape[1]}x{ki.shape[2]}{'-signed' if signed else ''}"


def _triangle(i, amp):
    if amp <= 0:
        return 0
    i %= 2 * amp
    return i if i <= amp else 2 * amp - i


def _channel_boxes(kh, kw, kc):
    """Three different boxes inside kh x kw (row0, row1, col0, col1, inclusive); the first is the whole stencil."""
    boxes = [(0, kh - 1, 0, kw - 1), (1 if kh > 4 else 0, kh - 1, 0, kw - 2 if kw > 4 else kw - 1),
             (0, kh - 2 if kh > 4 else kh - 1, 2 if kw > 6 else 0, kw - 1)]
    return boxes[:kc]


def ragged(rng, kh, kw, kc=3, signed=False, box=None):
    """Every kernel row has its own first and last non-zero column: the first column walks a triangle wave of amplitude up to 5, the
    last another one, so that across row steps the first and the last 4-tap chunk hold 1, 2, 3 and 4 live columns; row 0 is a
    single tap and the last row two taps in one chunk (row steps of one entry at both ends), and from 20 rows up five rows in the
    middle collapse to one chunk (one-entry row steps for Q = 4 too).  Wide rows are filled to about 12 %.
    box: (row0, row1, col0, col1) for every channel instead of the three built-in boxes (an off-centre box: above != below)."""
    ki = np.zeros((kh, kw, kc), np.int64)
    boxes = [box] * kc if box is not None else _channel_boxes(kh, kw, kc)
    for c, (r0, r1, c0, c1) in enumerate(boxes):
        bh, bw = r1 - r0 + 1, c1 - c0 + 1
        amp_f, amp_l = min(5, (bw - 1) // 2), min(4, (bw - 1) // 2)
        fill = 1.0 if bw <= 12 else 0.12
        for i in range(bh):
            f, l = _triangle(i + c, amp_f), bw - 1 - _triangle(i + 2 + 2 * c, amp_l)
            if i == 0:
                l = f = min(bw - 1, 1 + c)
            elif i == bh - 1 and bh > 2:
                f = (bw - 1) // 4 * 4
                l = bw - 1
            elif bh >= 20 and bh // 2 <= i < bh // 2 + 5:
                f = (bw // 2) // 4 * 4 + (i - bh // 2) % 3
                l = min(bw - 1, f + (i - bh // 2) % 2)
            row = np.zeros(bw, np.int64)
            inner = rng.random(max(l - f - 1, 0)) < fill
            inner[:3] = inner[-3:] = True  # solid ends: the live columns of an end chunk are then the extent's, not the fill's
            row[f + 1:l] = _weights(rng, max(l - f - 1, 0), signed) * inner
            row[f], row[l] = _weights(rng, 2, signed)
            ki[r0 + i, c0:c1 + 1, c] = row
        if bh > 2:  # the box keeps its width whatever the waves do
            ki[r0 + 1, c0, c], ki[r0 + 1, c1, c] = _weights(rng, 2, signed)
    return _finish(ki, "ragged", signed)


def gaps(rng, kh, kw, kc=3, signed=False):
    """Runs of 1, 2, 3, 4 and 5 all-zero kernel rows inside the box (as many as fit, one live row between them, then again), and
    all-zero columns: every fifth one, and from 16 columns up a whole aligned chunk.  Row steps are empty for Q = 2 from a run of 2
    and for Q = 4 from a run of 4."""
    ki = np.zeros((kh, kw, kc), np.int64)
    fill = 1.0 if kh * kw <= 150 else 0.15
    for c in range(kc):
        r0, c0 = (c if kh > 4 else 0), (c if kw > 6 else 0)  # channel c's box starts c rows and columns in
        live_rows = np.ones(kh, bool)
        live_rows[:r0] = False
        i, run = r0 + 1, 1 + c % 2
        while i + run < kh - 1:
            live_rows[i:i + run] = False
            i += run + 1
            run = run % 5 + 1
        live_cols = np.ones(kw, bool)
        live_cols[:c0] = False
        live_cols[c0 + 2:kw - 1:5] = False
        if kw >= 16:
            live_cols[c0 + 4:c0 + 8] = False  # (chunks count from the box's first column)
        live_cols[[c0, kw - 1]] = True
        w = _weights(rng, (kh, kw), signed) * (rng.random((kh, kw)) < fill)
        for i in np.nonzero(live_rows)[0]:  # no live row or column may come out empty
            j = rng.choice(np.nonzero(live_cols)[0])
            w[i, j] = w[i, j] or _weights(rng, (), signed)
        for j in np.nonzero(live_cols)[0]:
            i = rng.choice(np.nonzero(live_rows)[0])
            w[i, j] = w[i, j] or _weights(rng, (), signed)
        ki[..., c] = w * live_rows[:, None] * live_cols[None, :]
    return _finish(ki, "gaps", signed)


def corners(rng, kh, kw, kc=3, signed=False):
    """A box that holds only its four corner taps, its centre and about ten isolated taps."""
    ki = np.zeros((kh, kw, kc), np.int64)
    for c, (r0, r1, c0, c1) in enumerate(_channel_boxes(kh, kw, kc)):
        for i, j in ((r0, c0), (r0, c1), (r1, c0), (r1, c1), ((r0 + r1) // 2, (c0 + c1) // 2)):
            ki[i, j, c] = _weights(rng, (), signed)
        for _ in range(10):
            ki[rng.integers(r0, r1 + 1), rng.integers(c0, c1 + 1), c] = _weights(rng, (), signed)
    return _finish(ki, "corners", signed)


SHIFT_PLACES = ("above", "below", "left", "right", "first", "last")


def shift(rng, kh, kw, places=("above", "left", "first"), cluster=True, signed=False):
    """A single tap, or a 3 x 5 cluster (5 x 3 beside the anchor column), placed so that the tap box does not contain the anchor: a
    pure translation.  One channel per place: box wholly above / below / left / right of the anchor, or the tap at the stencil's
    first (0, 0) or last (kh - 1, kw - 1) corner.  `above` makes run_stencil's `below` negative and the other way round."""
    ay, ax = kh // 2, kw // 2
    ki = np.zeros((kh, kw, len(places)), np.int64)
    for c, place in enumerate(places):
        ch, cw = ((3, 5) if place in ("above", "below") else (5, 3)) if cluster else (1, 1)
        if place in ("first", "last"):
            ch = cw = 1
        ch, cw = min(ch, kh), min(cw, kw)
        if place == "above":
            ch = min(ch, ay)
            i0, j0 = max(0, ay - ch - 1), max(0, min(kw - cw, ax - 1))
        elif place == "below":
            ch = min(ch, kh - 1 - ay)
            i0, j0 = kh - ch, max(0, min(kw - cw, ax - 2))
        elif place == "left":
            cw = min(cw, ax)
            i0, j0 = max(0, min(kh - ch, ay - 1)), max(0, ax - cw - 1)
        elif place == "right":
            cw = min(cw, kw - 1 - ax)
            i0, j0 = max(0, min(kh - ch, ay - 3)), kw - cw
        elif place == "first":
            i0 = j0 = 0
        else:
            assert place == "last", place
            i0, j0 = kh - 1, kw - 1
        assert ch >= 1 and cw >= 1, f"{kh} x {kw} taps have no room {place} of the anchor"
        ki[i0:i0 + ch, j0:j0 + cw, c] = _weights(rng, (ch, cw), signed)
        assert not (i0 <= ay < i0 + ch and j0 <= ax < j0 + cw)
    return _finish(ki, "shift-" + "-".join(places) + ("" if cluster else "-tap"), signed)


def sym_sparse(rng, r, kh=None, kc=3, signed=False):
    """Left-right mirror symmetric bit for bit about the anchor column, box width 2 r + 1 >= 9: ragged rows (the first column of
    the left half walks a triangle wave), zero rows in runs of 1 .. 3, a centre column that is set on some rows only.  This takes
    the paired-tap entry list, whose boxes are padded to r = 2 (mod 4)."""
    assert r >= 4
    kw = 2 * r + 1
    kh = kh or kw
    ki = np.zeros((kh, kw, kc), np.int64)
    fill = 1.0 if r <= 8 else 0.2
    for c in range(kc):
        r0 = c if kh > 6 else 0
        i, run = r0 + 2, 1 + c % 3
        zero = np.zeros(kh, bool)
        zero[:r0] = True
        while i + run < kh - 1:
            zero[i:i + run] = True
            i += run + 2 + c
            run = run % 3 + 1
        for i in np.nonzero(~zero)[0]:
            f = _triangle(int(i) + 2 * c, min(r, 6))
            half = _weights(rng, r + 1, signed) * (rng.random(r + 1) < fill)
            half[:f] = 0
            if f <= r:
                half[f] = half[f] or _weights(rng, (), signed)
            if i % 3 == c % 3:
                half[r] = 0
            if not half.any():
                half[min(f, r - 1)] = _weights(rng, (), signed)
            ki[i, :r + 1, c] = half
        live = np.nonzero(~zero)[0]
        ki[live[0], :, c] = ki[live[-1], :, c] = 0  # the first row the centre tap alone, the last one pair: row steps of one entry
        ki[live[0], r, c], ki[live[-1], r - 2, c] = _weights(rng, 2, signed)
        ki[live[len(live) // 2], 0, c] = _weights(rng, (), signed)  # the box keeps its width
        ki[:, r + 1:, c] = ki[:, :r, c][:, ::-1]
    return _finish(ki, f"sym_sparse-r{r}", signed)


def central_sparse(rng, kh, kw, kc=3, signed=False, fill=0.1):
    """Centrally symmetric about the anchor, odd x odd box, sparse: k[i, j] == k[kh - 1 - i, kw - 1 - j].  The FFT form multiplies by a
    real kernel spectrum."""
    assert kh % 2 == 1 and kw % 2 == 1
    ki = np.zeros((kh, kw, kc), np.int64)
    for c in range(kc):
        w = _weights(rng, (kh, kw), signed) * (rng.random((kh, kw)) < fill)
        w[0, 0] = w[0, 0] or _weights(rng, (), signed)  # every channel keeps the whole box
        w[0, kw - 1] = w[0, kw - 1] or _weights(rng, (), signed)
        flat = w.reshape(-1)
        flat[flat.size // 2 + 1:] = flat[:flat.size // 2][::-1]
        ki[..., c] = flat.reshape(kh, kw)
    assert np.array_equal(ki, ki[::-1, ::-1])
    return _finish(ki, "central_sparse", signed)


def square_sym(rng, R, kc=3, signed=False):
    """(2 R + 1)^2, left-right mirror symmetric, with zero rows and zero columns inside but all four box edges occupied: the
    unrolled direct form (R <= 11)."""
    n = 2 * R + 1
    ki = np.zeros((n, n, kc), np.int64)
    for c in range(kc):
        w = _weights(rng, (n, n), signed) * (rng.random((n, n)) < 0.7)
        w[[0, n - 1], :] = _weights(rng, (2, n), signed)
        w[:, [0, n - 1]] = _weights(rng, (n, 2), signed)
        w[1 + (c % 2):n - 1:3, :] = 0
        cols = np.arange(1, R + 1, 4)
        w[:, cols] = 0
        w[:, R + 1:] = w[:, :R][:, ::-1]
        assert w[0].any() and w[n - 1].any() and w[:, 0].any() and w[:, n - 1].any()
        ki[..., c] = w
    return _finish(ki, f"square_sym-R{R}", signed)
