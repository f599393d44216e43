"""What the eleven demosaic entry points refuse, and in which words: every r2f_demosaic_* of include/r2f.h on an 8 x 8 Bayer and a
12 x 12 X-Trans mosaic (and one 16 x 16 Bayer mosaic, where step M's extra reach shows).  Every call below is refused before it
launches anything (or, for an empty row range, returns before it does), so the test runs no kernel; it pins, for each refused call,
the code, the exact r2f_last_error text, which message wins when a call breaks two rules at once (the checks run in a stated order:
the mosaic, the params, the frame size, the orientation, the clip, the passes, the window, the rows, the divisor, the source
window), and that the canary-filled destination and the source are untouched after all of them.  The texts are the entry points'
own, copied from their source.  A row whose text differs for the median entry points (their rows of the frame read one more row
either side per pass, and a good call here has one pass) carries that text as a fourth item."""

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
     "{what}: rows [1, 2) read mosaic rows [0, 6), the source window holds [0, 5)",
     "{what}: rows [1, 2) read mosaic rows [0, 7), the source window holds [0, 5)"),
    ("a source window that begins a row late", dict(y0=5, y1=6, gy0=2, nrows=6),
     "{what}: rows [5, 6) read mosaic rows [1, 8), the source window holds [2, 8)",
     "{what}: rows [5, 6) read mosaic rows [0, 8), the source window holds [2, 8)"),
    ("a source window a row short of the frame's last", dict(y0=0, y1=8, nrows=7),
     "{what}: rows [0, 8) read mosaic rows [0, 8), the source window holds [0, 7)"),
    # the half size reads the two mosaic rows of each of its own
    ("half size, a source window that ends a row early", dict(params=lambda: bayer(half=True), y0=1, y1=3, gy0=2, nrows=3),
     "{what}: rows [1, 3) read mosaic rows [2, 6), the source window holds [2, 5)",
     "{what}: rows [1, 3) read mosaic rows [0, 8), the source window holds [2, 5)"),
    ("half size, a source window that begins a row late", dict(params=lambda: bayer(half=True), y0=1, y1=3, gy0=3, nrows=3),
     "{what}: rows [1, 3) read mosaic rows [2, 6), the source window holds [3, 6)",
     "{what}: rows [1, 3) read mosaic rows [0, 8), the source window holds [3, 6)"),
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
     "{what}: rows [3, 4) read mosaic rows [1, 8), the source window holds [2, 8)",
     "{what}: rows [3, 4) read mosaic rows [0, 8), the source window holds [2, 8)"),
    ("a window's source rows that end a row early", dict(window=(1, 0, 4, 8), y0=0, y1=1, nrows=5),
     "{what}: rows [0, 1) read mosaic rows [0, 6), the source window holds [0, 5)",
     "{what}: rows [0, 1) read mosaic rows [0, 7), the source window holds [0, 5)"),
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
     "{what}: rows [5, 6) read mosaic rows [2, 9), the source window holds [3, 12)",
     "{what}: rows [5, 6) read mosaic rows [1, 10), the source window holds [3, 12)"),
    ("a source window that ends a row early", dict(y0=5, y1=6, gy0=2, nrows=6),
     "{what}: rows [5, 6) read mosaic rows [2, 9), the source window holds [2, 8)",
     "{what}: rows [5, 6) read mosaic rows [1, 10), the source window holds [2, 8)"),
    ("a source window a row short at the frame's top", dict(y0=0, y1=2, nrows=4),
     "{what}: rows [0, 2) read mosaic rows [0, 5), the source window holds [0, 4)",
     "{what}: rows [0, 2) read mosaic rows [0, 6), the source window holds [0, 4)"),
    ("a source window a row short of the frame's last", dict(y0=0, y1=12, nrows=11),
     "{what}: rows [0, 12) read mosaic rows [0, 12), the source window holds [0, 11)"),
    # the reduced size reads the three mosaic rows of each of its own
    ("reduced size, a source window that begins a row late", dict(params=lambda: xtrans(reduced=True), y0=1, y1=3, gy0=4, nrows=5),
     "{what}: rows [1, 3) read mosaic rows [3, 9), the source window holds [4, 9)",
     "{what}: rows [1, 3) read mosaic rows [0, 12), the source window holds [4, 9)"),
    ("reduced size, a source window that ends a row early", dict(params=lambda: xtrans(reduced=True), y0=1, y1=3, gy0=3, nrows=5),
     "{what}: rows [1, 3) read mosaic rows [3, 9), the source window holds [3, 8)",
     "{what}: rows [1, 3) read mosaic rows [0, 12), the source window holds [3, 8)"),
    # two rules at once: the earlier check speaks
    ("a pitch below W and tampered tables", dict(pitch=11, params=lambda: xtrans(tamper="gap")), X_FIRST),
    ("tampered tables and another frame size", dict(params=lambda: xtrans(15, 12, tamper="cfa")), X_TABLES),
    ("another frame size and rows outside", dict(params=lambda: xtrans(15, 12), y0=-1, y1=4), X_ANOTHER),
    ("another frame size and a short source window", dict(params=lambda: xtrans(15, 12), nrows=0), X_ANOTHER),
    ("rows outside and a short source window", dict(y0=-1, y1=4, nrows=0), "{what}: rows [-1, 4) not inside the output's [0, 12)"),
]

# ------------------------------------------------------------------------------- the arguments between the params and the destination
# (either pattern: none of these texts names one.  A bad window below is F32_ONLY's empty one.)
ORIENTATION = "{what}: orientation %d is not one of 0 .. 7 (LibRaw's sizes.flip bits)"
BLEND_CLIP = "{what}: clip %d is not inside [1, 65535]"
MEDIAN_CLIP = "{what}: clip %d is neither 0 (no Blend) nor inside [1, 65535]"
PASSES = "{what}: passes %d is not inside [1, R2F_MEDIAN_MAX_PASSES = 4] (LibRaw's med_passes)"

ORIENTED = [  # every entry point that takes an orientation
    ("an orientation of -1", dict(orientation=-1), ORIENTATION % -1),
    ("an orientation of 8", dict(orientation=8), ORIENTATION % 8),
    ("a bad orientation and rows outside", dict(orientation=8, y0=-1, y1=4), ORIENTATION % 8),
    ("a bad orientation and a short source window", dict(orientation=-1, nrows=0), ORIENTATION % -1),
]
BLEND = [  # the blend entry points' clip
    ("a clip of 0", dict(clip=0), BLEND_CLIP % 0),
    ("a clip of 65536", dict(clip=65536), BLEND_CLIP % 65536),
    ("a bad clip and rows outside", dict(clip=0, y0=-1, y1=4), BLEND_CLIP % 0),
]
BLEND_ORIENTED = [("a bad orientation and a bad clip", dict(orientation=8, clip=65536), ORIENTATION % 8)]
BLEND_F32 = [("a bad clip and a bad window", dict(clip=65536, window=(2, 3, 0, 4)), BLEND_CLIP % 65536)]
MEDIAN = [  # the median entry points' clip (0: no Blend) and passes
    ("a clip of -1", dict(clip=-1), MEDIAN_CLIP % -1),
    ("a clip of 65536", dict(clip=65536), MEDIAN_CLIP % 65536),
    ("no pass", dict(passes=0), PASSES % 0),
    ("a pass more than the cap", dict(passes=5), PASSES % 5),
    ("a bad clip and bad passes", dict(clip=-1, passes=0), MEDIAN_CLIP % -1),
    ("bad passes and rows outside", dict(passes=5, y0=-1, y1=4), PASSES % 5),
]
MEDIAN_ORIENTED = [("a bad orientation and a bad clip", dict(orientation=8, clip=65536), ORIENTATION % 8),
                   ("a bad orientation and bad passes", dict(orientation=-1, passes=0), ORIENTATION % -1)]
MEDIAN_F32 = [("a bad clip and a bad window", dict(clip=65536, window=(2, 3, 0, 4)), MEDIAN_CLIP % 65536),
              ("bad passes and a bad window", dict(passes=0, window=(2, 3, 0, 4)), PASSES % 0)]
# step M's reach on a 16 x 16 Bayer mosaic: row 7 with two passes reads rows [5, 10) of the frame, and those read 4 mosaic rows more
MEDIAN_REACH = [("two passes, a source window that begins a row late", dict(side=16, y0=7, y1=8, passes=2, gy0=2, nrows=14),
                 "{what}: rows [7, 8) read mosaic rows [1, 14), the source window holds [2, 16)")]

# entry point -> (its name in messages, the destination's element type, how its params are planned (which says the mosaic's side),
# the arguments it takes between the params and the destination, its table)
SIDES = {bayer: 8, xtrans: 12}
BAYER_F32 = BAYER + F32_ONLY
ENTRIES = {
    "r2f_demosaic_u16": ("demosaic_u16", torch.int16, bayer, (), BAYER),
    "r2f_demosaic_oriented_u16": ("demosaic_oriented_u16", torch.int16, bayer, ("orientation",), BAYER + ORIENTED),
    "r2f_demosaic_blend_u16": ("demosaic_blend_u16", torch.int16, bayer, ("orientation", "clip"), BAYER + ORIENTED + BLEND + BLEND_ORIENTED),
    "r2f_demosaic_median_u16": ("demosaic_median_u16", torch.int16, bayer, ("orientation", "clip", "passes"),
                                BAYER + ORIENTED + MEDIAN + MEDIAN_ORIENTED + MEDIAN_REACH),
    "r2f_demosaic_f32": ("demosaic_f32", torch.float32, bayer, ("window", "decode"), BAYER_F32),
    "r2f_demosaic_blend_f32": ("demosaic_blend_f32", torch.float32, bayer, ("clip", "window", "decode"), BAYER_F32 + BLEND + BLEND_F32),
    "r2f_demosaic_median_f32": ("demosaic_median_f32", torch.float32, bayer, ("clip", "passes", "window", "decode"),
                                BAYER_F32 + MEDIAN + MEDIAN_F32 + MEDIAN_REACH),
    "r2f_demosaic_xtrans_u16": ("demosaic_xtrans_u16", torch.int16, xtrans, (), XTRANS),
    "r2f_demosaic_xtrans_oriented_u16": ("demosaic_xtrans_oriented_u16", torch.int16, xtrans, ("orientation",), XTRANS + ORIENTED),
    "r2f_demosaic_xtrans_blend_u16": ("demosaic_xtrans_blend_u16", torch.int16, xtrans, ("orientation", "clip"),
                                      XTRANS + ORIENTED + BLEND + BLEND_ORIENTED),
    "r2f_demosaic_xtrans_median_u16": ("demosaic_xtrans_median_u16", torch.int16, xtrans, ("orientation", "clip", "passes"),
                                       XTRANS + ORIENTED + MEDIAN + MEDIAN_ORIENTED),
}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_refused_calls_say_why_and_write_nothing(ctx, entry):
    what, dtype, plan, between, table = ENTRIES[entry]
    side, median = SIDES[plan], "passes" in between
    sides = {side} | {args.get("side", side) for _, args, *_ in table}
    sources = {s: Arena.holding(torch.arange(s * s, dtype=torch.int16).reshape(s, s).cuda()) for s in sides}
    dst = Arena.hwc(16, 16, dtype, device="cuda")
    planned = {s: plan(s, s) for s in sources}

    def good_call(s):  # (a good call of a mosaic of s x s samples: one pass, a clip inside both ranges, upright)
        return dict(src=sources[s].view.data_ptr(), gy0=0, nrows=s, pitch=s, H=s, W=s, params=lambda: planned[s], dst=dst.view.data_ptr(),
                    dst_offset=0, y0=0, y1=4, window=None, divisor=65535.0, orientation=0, clip=1000, passes=1)

    def call(side=side, **args):
        a = {**good_call(side), **args}
        p = a["params"]() if a["params"] is not None else None
        ref = C.byref(p) if p is not None else None
        d = a["dst"] + a["dst_offset"] if a["dst"] is not None else None
        a["window"] = a["window"] or (0, 0, p.out_h if p is not None else side, p.out_w if p is not None else side)
        a["decode"] = (a["divisor"], 1.0)
        middle = [v for name in between for v in (a[name] if name in ("window", "decode") else (a[name],))]
        rc = getattr(ctx._lib, entry)(ctx._h, a["src"], a["gy0"], a["nrows"], a["pitch"], a["H"], a["W"], ref, *middle, d, a["y0"], a["y1"],
                                      ctx._stream())
        return rc, ctx._lib.r2f_last_error(ctx._h).decode()

    seen = set()
    for wrong, args, message, *median_message in table:
        assert wrong not in seen, f"two cases named {wrong!r}"
        seen.add(wrong)
        if median and median_message:
            message = median_message[0]
        assert call(**args) == (EINVAL, message.format(what=what)), f"{entry}: {wrong}"
    # an empty row range is no refusal, reads nothing (so it needs no source rows) and launches nothing either; nor does an
    # orientation with nothing else wrong change that
    assert call(y0=2, y1=2, nrows=0)[0] == 0, f"{entry}: an empty row range"
    if "orientation" in between:
        assert call(orientation=5, y0=2, y1=2, nrows=0)[0] == 0, f"{entry}: an empty row range of the oriented frame"
    torch.cuda.synchronize()
    dst.check(None, what=f"refused {entry}")
    for s in sources.values():
        s.unchanged(f"refused {entry}")

