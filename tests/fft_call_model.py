"""The host decisions of one call of the FFT stencil form in plain Python: the window, the real spectrum, the scratch element, the
batches and their walk, the timing classes and bytes.  Written from the launch function as it stood before plan::fft_call existed
(commit 2b3624e: raw2film_amd/csrc/r2f_stencil.hip:163-338, run_stencil_fft, and r2f_plan.cpp:274-325, fft_window / fft_batches;
the line numbers below are that commit's), not from the planner it checks.  What tests/test_fft_call_host.py holds
tests/fft_call_check.cpp's walk of plan::fft_call against, line for line; `cases` is the walk both sides take."""

import itertools
from types import SimpleNamespace as NS

HALATION, MTF = 0, 1  # R2F_KERNEL_HALATION / _MTF: the bit of the option masks


def options(**kw):
    """The option fields a call reads, at r2f_plan.h's defaults."""
    o = NS(window=0, window_max=512, window_rows=0, batch_mib=192, streams=2, even=1,
           fft_s32=1 << MTF, fft_s96=0, fft_s96_auto=1, fft_real=1, fft_mixed_sign=1, fft_cols_walk=1)
    o.__dict__.update(kw)
    return o


def valid(ny, nx, bh, bw):
    """r2f_stencil.hip:204-205 = r2f_plan.cpp:284 = :302-303: vx a multiple of 4."""
    return ny - bh + 1, (nx - bw + 1) & ~3


def fft_window(o, bh, bw, W, H, s32):
    """r2f_plan.cpp:274-297.  (ny, nx), or None when no shape keeps outputs."""
    best = None
    window_max = max(o.window_max, 512) if bw > 200 else o.window_max  # :278
    for y in (256, 512):
        if (y != 512) if bh > 200 else (o.window_rows and y != o.window_rows):  # :280
            continue
        for x in (256, 512, 1024):
            if x > window_max and x != o.window:  # :282
                continue
            if (x < 512 or (o.window >= 512 and x != o.window)) if bw > 200 else (o.window and x != o.window):  # :283
                continue
            vy, vx = valid(y, x, bh, bw)
            if vy < 1 or vx < 4:  # :285
                continue
            n = float(y) * x
            part = n * vy / y
            p2 = 1.3 if y == 512 else 1.0
            e = 4.0 if s32 else 8.0
            nbytes = 4.0 * n + e * n + p2 * (e * n + e * part) + e * part + 4.0 * vy * vx  # :291
            cost = float(((W + vx - 1) // vx) * ((H + vy - 1) // vy)) * nbytes  # :292 (exact in doubles)
            if best is None or cost < best[0]:  # :293, the first of equals
                best = (cost, y, x)
    return None if best is None else best[1:]


def fft_batches(o, ny, nx, bh, bw, W, y0, y1, nch, elem_bytes):
    """r2f_plan.cpp:299-325."""
    b = NS(ny=ny, nx=nx)
    b.vy, b.vx = valid(ny, nx, bh, bw)
    b.gx = (W + b.vx - 1) // b.vx
    b.ntiles = b.gx * ((y1 - y0 + b.vy - 1) // b.vy)
    b.ppc = (b.ntiles + 1) // 2
    b.pairs = b.ppc * nch
    b.img_bytes = ny * nx * elem_bytes
    fft_batch = max(1, (max(o.batch_mib, 1) << 20) // b.img_bytes)  # :312
    b.nstreams = max(1, min(o.streams, 4)) if b.pairs > fft_batch else 1
    b.batch = min(b.pairs, max(1, fft_batch // b.nstreams))
    if o.even:  # :315-321
        nb = (b.pairs + b.batch - 1) // b.batch
        nb = (nb + b.nstreams - 1) // b.nstreams * b.nstreams
        b.batch = (b.pairs + nb - 1) // nb
    b.launches = (b.pairs + b.batch - 1) // b.batch
    b.scratch_bytes = b.batch * b.nstreams * b.img_bytes
    return b


def fft_call(o, bh, bw, ay, ax, nch, which, W, y0, y1, any_mixed, unit_gain, symmetric, epilogue, dyn, curve_set):
    """r2f_stencil.hip:163-338 without its device calls.  None when no window fits (:178-180)."""
    cancelling = any_mixed and o.fft_mixed_sign
    complex64 = bool((o.fft_s32 >> which) & 1) and not cancelling  # :175-177
    win = fft_window(o, bh, bw, W, y1 - y0, complex64)  # :178: priced with complex64 or complex128, never the 12-byte element
    if win is None:
        return None
    c = NS()
    ny, nx = win
    c.kreal = 1 if (o.fft_real and symmetric) else 0  # :207-208
    c.oy, c.ox = (ay, ax) if c.kreal else (0, 0)  # :209-210
    c.element = 2 if (o.fft_s96 >> which) & 1 else (1 if complex64 else 0)  # :250
    if cancelling:  # :251-252
        c.element = 0
    if (c.element == 0 and which == HALATION and epilogue == 1 and dyn and o.fft_s96_auto and c.kreal and unit_gain and ny == 256
            and o.fft_cols_walk and curve_set):  # :258-259
        c.element = 3
    c.elem_bytes = 8 if c.element == 1 else (12 if c.element == 2 else 16)  # :263
    c.timing_offset = 3 if c.element == 1 else 0  # :311-312
    c.b = b = fft_batches(o, ny, nx, bh, bw, W, y0, y1, nch, c.elem_bytes)
    # :316-321: batch i from pair i * batch on, on lane i % nstreams, in that lane's slice of the scratch
    c.batches = [(p0, min(b.batch, b.pairs - p0), i % b.nstreams, (i % b.nstreams) * b.batch * b.img_bytes)
                 for i, p0 in enumerate(range(0, b.pairs, b.batch))]
    full = float(b.img_bytes)  # :324-329, per pair
    part = full * b.vy / ny
    c.pass_bytes = (2.0 * float(ny * nx) * 4 + full, full + part, part + 2.0 * b.vy * b.vx * 4)
    return c


# ------------------------------------------------------------------------------------------------ the walk
BOXES = ((31, 31), (85, 85), (35, 35), (201, 25), (25, 301))
FRAMES = ((300, 520), (12288, 8192))  # H x W


def cases():
    """(label, keyword arguments of fft_call, options) in the order tests/fft_call_check.cpp prints them."""
    # 1: every combination of the facts and switches the element and the real spectrum hang on, for a box that takes 256-row windows
    # and one that needs 512.  The OTHER stencil's mask bit is the complement: reading the wrong bit shows.
    for (bh, bw), bits in itertools.product(((31, 31), (201, 25)), itertools.product((0, 1), repeat=13)):
        s32, s96, mixed, mixed_opt, which, epilogue, dyn, auto, sym, real, unit, walk, curve = bits
        mask = lambda bit: (bit << which) | ((1 - bit) << (1 - which))  # noqa: E731
        o = options(fft_s32=mask(s32), fft_s96=mask(s96), fft_mixed_sign=mixed_opt, fft_s96_auto=auto, fft_real=real, fft_cols_walk=walk)
        yield ("A %d %d " % (bh, bw) + "".join(map(str, bits)),
               dict(bh=bh, bw=bw, ay=bh // 2, ax=bw // 2, nch=2, which=which, W=520, y0=0, y1=300, any_mixed=bool(mixed), unit_gain=bool(unit),
                    symmetric=bool(sym), epilogue=epilogue, dyn=bool(dyn), curve_set=bool(curve)), o)
    # 2: geometries, as the halation of a render (element 3 where the windows have 256 rows) and as the MTF (complex64)
    for (bh, bw), (H, W), rows, batch_mib, streams, even, which in itertools.product(BOXES, FRAMES, range(3), (1, 192), (1, 2, 4), (0, 1),
                                                                                     (HALATION, MTF)):
        y0, y1 = ((0, H), (40, 200), (1058, 2116))[rows]
        o = options(batch_mib=batch_mib, streams=streams, even=even)
        yield ("B %d %d %d %d %d %d %d %d %d %d" % (bh, bw, W, y0, y1, batch_mib, streams, even, which, 3 - which),
               dict(bh=bh, bw=bw, ay=bh // 2, ax=bw // 2, nch=3 - which, which=which, W=W, y0=y0, y1=y1, any_mixed=False, unit_gain=True,
                    symmetric=True, epilogue=1, dyn=True, curve_set=True), o)


def line(label, c):
    """One case as tests/fft_call_check.cpp prints it."""
    if c is None:
        return label + " : no window"
    b = c.b
    h = 0
    for p0, n, lane, off in c.batches:  # a digest of the walk (every batch enters; the first and last are printed too)
        h = (h * 1000003 + p0 * 31 + n * 7 + lane * 3 + off) % (1 << 40)
    first, last = c.batches[0], c.batches[-1]
    return (label + " : %d %d %d %d k %d %d %d e %d %d %d t %d %d %d %d s %d %d %d %d %d" % (
        b.ny, b.nx, b.vy, b.vx, c.kreal, c.oy, c.ox, c.element, c.elem_bytes, c.timing_offset, b.gx, b.ntiles, b.ppc, b.pairs,
        b.nstreams, b.batch, b.launches, b.img_bytes, b.scratch_bytes)
        + " p %s %s %s" % tuple(format(v, ".17g") for v in c.pass_bytes)
        + " w %d %d %d %d %d / %d %d %d %d / %d" % (len(c.batches), *first, *last, h))


def lines():
    return [line(label, fft_call(o, **kw)) for label, kw, o in cases()]
