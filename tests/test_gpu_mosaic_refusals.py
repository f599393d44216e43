"""What the three demosaic entry points refuse, and in which words: r2f_demosaic_u16, r2f_demosaic_f32 and r2f_demosaic_xtrans_u16
on an 8 x 8 Bayer and a 12 x 12 X-Trans mosaic.  Every call below is refused before it launches anything (or, for an empty row
range, returns before it does), so the test runs no kernel; it pins, for each refused call, the code, the exact r2f_last_error text,
which message wins when a call breaks two rules at once (the checks run in a stated order), and that the canary-filled destination
and the source are untouched after all of them.  The texts are the entry points' own, copied from their source."""

import ctypes as C

import pytest

from arena import Arena

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EINVAL = -1
NAN = float("nan")


@pytest.fixture(scope="module")
def ctx():
    from raw2film_amd.context import HipContext

    c = HipContext(0)
    yield c
    c.close()


def bayer(H=8, W=8, half=False, cfa=None):
    from raw2film_amd.raw import RawProfile

    p = RawProfile("RGGB", black=64, multipliers=(2.0, 1.0, 1.5)).plan(H, W, half)
    if cfa is not None:
        p.cfa[:] = cfa
    return p


def xtrans(H=12, W=12, reduced=False, tamper=None):
    from raw2film_amd.raw import XTransProfile

    p = XTransProfile(black=64, multipliers=(2.0, 1.0, 1.5)).plan(H, W, reduced)
    if tamper == "gap":
        p.gap[1][0] = 3  # a table that would index outside the staged tile
    elif tamper == "cfa":
        p.cfa[0], p.cfa[1] = p.cfa[1], p.cfa[0]  # another pattern under the same tables
    elif tamper == "taps":
        p.taps[0][0] ^= 1
    elif tamper == "recip":
        p.recip[0][1] += 1
    return p


# ----------------------------------------------------------------------------------------------------------------- the Bayer tables
B_FIRST = "{what}: a mosaic of at least 2 x 2 samples, a pitch of at least W and a source window are required"
B_NOT_BAYER = "{what}: not a Bayer pattern (r2f_demosaic_plan makes one)"
B_ANOTHER = "{what}: the params are those of another frame size (r2f_demosaic_plan)"
F_DIVISOR = "{what}: a positive divisor and a 4-byte aligned destination are required"

# (what is wrong, the arguments that differ from a good call's, the message).  `params` is a function: planned when the case runs.
BAYER = [
    ("a null source", dict(src=None), B_FIRST),
    ("null params", dict(params=None), B_FIRST),
    ("a null destination", dict(dst=None), B_FIRST),
    ("one row", dict(H=1), B_FIRST),
    ("one column", dict(W=1), B_FIRST),
    ("a side above 2^17", dict(H=(1 << 17) + 1), B_FIRST),
    ("a pitch below W", dict(pitch=7), B_FIRST),
    ("a negative source origin", dict(gy0=-1), B_FIRST),
    ("a negative source row count", dict(nrows=-1), B_FIRST),
    ("a colour id of 3", dict(params=lambda: bayer(cfa=(0, 3, 1, 2))), "{what}: colour id 3 at site 1"),
    ("a negative colour id", dict(params=lambda: bayer(cfa=(0, 1, -1, 2))), "{what}: colour id -1 at site 2"),
    ("two reds", dict(params=lambda: bayer(cfa=(0, 0, 1, 2))), B_NOT_BAYER),
    ("the greens in a row", dict(params=lambda: bayer(cfa=(1, 1, 0, 2))), B_NOT_BAYER),
    ("an odd frame at half size", dict(H=7, params=lambda: bayer(half=True)), "{what}: the half-size form needs an even frame, got 7 x 8"),
    ("an odd width at half size", dict(W=7, pitch=8, params=lambda: bayer(half=True)),
     "{what}: the half-size form needs an even frame, got 8 x 7"),
    ("the params of another frame size", dict(params=lambda: bayer(10, 8)), B_ANOTHER),
    ("half-size params of another frame size", dict(params=lambda: bayer(8, 10, half=True)), B_ANOTHER),
    ("rows that begin before the output", dict(y0=-1, y1=4), "{what}: rows [-1, 4) not inside the output's [0, 8)"),
    ("rows that end behind the output", dict(y0=0, y1=9), "{what}: rows [0, 9) not inside the output's [0, 8)"),
    ("rows that end before they begin", dict(y0=3, y1=2), "{what}: rows [3, 2) not inside the output's [0, 8)"),
    ("rows behind the half-size output", dict(params=lambda: bayer(half=True), y0=0, y1=5),
     "{what}: rows [0, 5) not inside the output's [0, 4)"),
    # the full size reads 4 mosaic rows past its own on either side, clipped to the frame
    ("a source window that ends a row early", dict(y0=1, y1=2, nrows=5),
     "{what}: rows [1, 2) read mosaic rows [0, 6), the source window holds [0, 5)"),
    ("a source window that begins a row late", dict(y0=5, y1=6, gy0=2, nrows=6),
     "{what}: rows [5, 6) read mosaic rows [1, 8), the source window holds [2, 8)"),
    ("a source window a row short of the frame's last", dict(y0=0, y1=8, nrows=7),
     "{what}: rows [0, 8) read mosaic rows [0, 8), the source window holds [0, 7)"),
    # the half size reads the two mosaic rows of each of its own
    ("half size, a source window that ends a row early", dict(params=lambda: bayer(half=True), y0=1, y1=3, gy0=2, nrows=3),
     "{what}: rows [1, 3) read mosaic rows [2, 6), the source window holds [2, 5)"),
    ("half size, a source window that begins a row late", dict(params=lambda: bayer(half=True), y0=1, y1=3, gy0=3, nrows=3),
     "{what}: rows [1, 3) read mosaic rows [2, 6), the source window holds [3, 6)"),
    # two rules at once: the earlier check speaks
    ("a pitch below W and no Bayer pattern", dict(pitch=7, params=lambda: bayer(cfa=(0, 0, 1, 2))), B_FIRST),
    ("a bad colour id and no Bayer pattern", dict(params=lambda: bayer(cfa=(1, 1, 1, 5))), "{what}: colour id 5 at site 3"),
    ("no Bayer pattern and another frame size", dict(params=lambda: bayer(10, 8, cfa=(0, 0, 1, 2))), B_NOT_BAYER),
    ("an odd frame at half size and another frame size", dict(H=7, params=lambda: bayer(10, 8, half=True)),
     "{what}: the half-size form needs an even frame, got 7 x 8"),
    ("another frame size and rows outside", dict(params=lambda: bayer(10, 8), y0=-1, y1=4), B_ANOTHER),
    ("another frame size and a short source window", dict(params=lambda: bayer(10, 8), nrows=0), B_ANOTHER),
    ("rows outside and a short source window", dict(y0=-1, y1=4, nrows=0), "{what}: rows [-1, 4) not inside the output's [0, 8)"),
]

F32_ONLY = [
    ("an empty window", dict(window=(2, 3, 0, 4)), "{what}: the window (2, 3, 0, 4) is empty or not inside the 8 x 8 frame"),
    ("a window with a negative origin", dict(window=(-1, 0, 4, 4)), "{what}: the window (-1, 0, 4, 4) is empty or not inside the 8 x 8 frame"),
    ("a window past the last row", dict(window=(5, 0, 4, 8)), "{what}: the window (5, 0, 4, 8) is empty or not inside the 8 x 8 frame"),
    ("a window past the last column", dict(window=(0, 5, 8, 4)), "{what}: the window (0, 5, 8, 4) is empty or not inside the 8 x 8 frame"),
    ("a window past the half-size frame", dict(params=lambda: bayer(half=True), window=(0, 0, 5, 4)),
     "{what}: the window (0, 0, 5, 4) is empty or not inside the 4 x 4 frame"),
    ("rows outside the window", dict(window=(2, 2, 4, 4), y0=0, y1=5), "{what}: rows [0, 5) not inside the output's [0, 4)"),
    ("a divisor of 0", dict(divisor=0.0), F_DIVISOR),
    ("a negative divisor", dict(divisor=-65535.0), F_DIVISOR),
    ("a NaN divisor", dict(divisor=NAN), F_DIVISOR),
    ("a destination no float can start at", dict(dst_offset=2), F_DIVISOR),
    # rows [3, 4) of a window that begins at row 2 are the frame's row 5
    ("a window's source rows that begin a row late", dict(window=(2, 0, 4, 8), y0=3, y1=4, gy0=2, nrows=6),
     "{what}: rows [3, 4) read mosaic rows [1, 8), the source window holds [2, 8)"),
    ("a window's source rows that end a row early", dict(window=(1, 0, 4, 8), y0=0, y1=1, nrows=5),
     "{what}: rows [0, 1) read mosaic rows [0, 6), the source window holds [0, 5)"),
    ("another frame size and a bad window", dict(params=lambda: bayer(10, 8), window=(2, 3, 0, 4)), B_ANOTHER),
    ("a bad window and rows outside", dict(window=(2, 3, 0, 4), y0=-1, y1=4), "{what}: the window (2, 3, 0, 4) is empty or not inside the 8 x 8 frame"),
    ("rows outside and a bad divisor", dict(y0=-1, y1=4, divisor=0.0), "{what}: rows [-1, 4) not inside the output's [0, 8)"),
    ("a bad divisor and a short source window", dict(divisor=0.0, nrows=0), F_DIVISOR),
    ("a bad divisor and an empty row range", dict(divisor=0.0, y0=2, y1=2), F_DIVISOR),
]

# ---------------------------------------------------------------------------------------------------------------- the X-Trans table
X_FIRST = "{what}: a mosaic of at least 6 x 6 samples, a pitch of at least W and a source window are required"
X_TABLES = "{what}: the params' tables are not those of an admissible pattern (r2f_xtrans_plan makes them)"
X_ANOTHER = "{what}: the params are those of another frame size (r2f_xtrans_plan)"

XTRANS = [
    ("a null source", dict(src=None), X_FIRST),
    ("null params", dict(params=None), X_FIRST),
    ("a null destination", dict(dst=None), X_FIRST),
    ("five rows", dict(H=5), X_FIRST),
    ("five columns", dict(W=5), X_FIRST),
    ("a side above 2^17", dict(W=(1 << 17) + 1, pitch=1 << 18), X_FIRST),
    ("a pitch below W", dict(pitch=11), X_FIRST),
    ("a negative source origin", dict(gy0=-1), X_FIRST),
    ("a negative source row count", dict(nrows=-1), X_FIRST),
    ("a tampered gap", dict(params=lambda: xtrans(tamper="gap")), X_TABLES),
    ("another pattern under the same tables", dict(params=lambda: xtrans(tamper="cfa")), X_TABLES),
    ("a tampered tap mask", dict(params=lambda: xtrans(tamper="taps")), X_TABLES),
    ("a tampered reciprocal", dict(params=lambda: xtrans(tamper="recip")), X_TABLES),
    ("tampered tables at the reduced size", dict(params=lambda: xtrans(reduced=True, tamper="gap")), X_TABLES),
    ("the params of another frame size", dict(params=lambda: xtrans(15, 12)), X_ANOTHER),
    ("reduced params of another frame size", dict(params=lambda: xtrans(12, 15, reduced=True)), X_ANOTHER),
    ("rows that begin before the output", dict(y0=-1, y1=4), "{what}: rows [-1, 4) not inside the output's [0, 12)"),
    ("rows that end behind the output", dict(y0=0, y1=13), "{what}: rows [0, 13) not inside the output's [0, 12)"),
    ("rows that end before they begin", dict(y0=3, y1=2), "{what}: rows [3, 2) not inside the output's [0, 12)"),
    ("rows behind the reduced output", dict(params=lambda: xtrans(reduced=True), y0=0, y1=5),
     "{what}: rows [0, 5) not inside the output's [0, 4)"),
    # the full size reads 3 mosaic rows past its own on either side, clipped to the frame
    ("a source window that begins a row late", dict(y0=5, y1=6, gy0=3, nrows=9),
     "{what}: rows [5, 6) read mosaic rows [2, 9), the source window holds [3, 12)"),
    ("a source window that ends a row early", dict(y0=5, y1=6, gy0=2, nrows=6),
     "{what}: rows [5, 6) read mosaic rows [2, 9), the source window holds [2, 8)"),
    ("a source window a row short at the frame's top", dict(y0=0, y1=2, nrows=4),
     "{what}: rows [0, 2) read mosaic rows [0, 5), the source window holds [0, 4)"),
    ("a source window a row short of the frame's last", dict(y0=0, y1=12, nrows=11),
     "{what}: rows [0, 12) read mosaic rows [0, 12), the source window holds [0, 11)"),
    # the reduced size reads the three mosaic rows of each of its own
    ("reduced size, a source window that begins a row late", dict(params=lambda: xtrans(reduced=True), y0=1, y1=3, gy0=4, nrows=5),
     "{what}: rows [1, 3) read mosaic rows [3, 9), the source window holds [4, 9)"),
    ("reduced size, a source window that ends a row early", dict(params=lambda: xtrans(reduced=True), y0=1, y1=3, gy0=3, nrows=5),
     "{what}: rows [1, 3) read mosaic rows [3, 9), the source window holds [3, 8)"),
    # two rules at once: the earlier check speaks
    ("a pitch below W and tampered tables", dict(pitch=11, params=lambda: xtrans(tamper="gap")), X_FIRST),
    ("tampered tables and another frame size", dict(params=lambda: xtrans(15, 12, tamper="cfa")), X_TABLES),
    ("another frame size and rows outside", dict(params=lambda: xtrans(15, 12), y0=-1, y1=4), X_ANOTHER),
    ("another frame size and a short source window", dict(params=lambda: xtrans(15, 12), nrows=0), X_ANOTHER),
    ("rows outside and a short source window", dict(y0=-1, y1=4, nrows=0), "{what}: rows [-1, 4) not inside the output's [0, 12)"),
]

# entry point -> (its name in messages, the side of the mosaic, the destination's element type, how its params are planned, its table)
ENTRIES = {
    "r2f_demosaic_u16": ("demosaic_u16", 8, torch.int16, bayer, BAYER),
    "r2f_demosaic_f32": ("demosaic_f32", 8, torch.float32, bayer, BAYER + F32_ONLY),
    "r2f_demosaic_xtrans_u16": ("demosaic_xtrans_u16", 12, torch.int16, xtrans, XTRANS),
}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_refused_calls_say_why_and_write_nothing(ctx, entry):
    what, side, dtype, plan, table = ENTRIES[entry]
    src = Arena.holding(torch.arange(side * side, dtype=torch.int16).reshape(side, side).cuda())
    dst = Arena.hwc(side, side, dtype, device="cuda")
    good = plan()

    good_call = dict(src=src.view.data_ptr(), gy0=0, nrows=side, pitch=side, H=side, W=side, params=lambda: good, dst=dst.view.data_ptr(),
                     dst_offset=0, y0=0, y1=4, window=None, divisor=65535.0)

    def call(**args):
        a = {**good_call, **args}
        p = a["params"]() if a["params"] is not None else None
        ref = C.byref(p) if p is not None else None
        d = a["dst"] + a["dst_offset"] if a["dst"] is not None else None
        head = (ctx._h, a["src"], a["gy0"], a["nrows"], a["pitch"], a["H"], a["W"], ref)
        if entry == "r2f_demosaic_f32":
            win = a["window"] or (0, 0, p.out_h if p is not None else side, p.out_w if p is not None else side)
            rc = ctx._lib.r2f_demosaic_f32(*head, *win, a["divisor"], 1.0, d, a["y0"], a["y1"], ctx._stream())
        else:
            rc = getattr(ctx._lib, entry)(*head, d, a["y0"], a["y1"], ctx._stream())
        return rc, ctx._lib.r2f_last_error(ctx._h).decode()

    seen = set()
    for wrong, args, message in table:
        assert wrong not in seen, f"two cases named {wrong!r}"
        seen.add(wrong)
        assert call(**args) == (EINVAL, message.format(what=what)), f"{entry}: {wrong}"
    # an empty row range is no refusal, reads nothing (so it needs no source rows) and launches nothing either
    assert call(y0=2, y1=2, nrows=0)[0] == 0, f"{entry}: an empty row range"
    torch.cuda.synchronize()
    dst.check(None, what=f"refused {entry}")
    src.unchanged(f"refused {entry}")
