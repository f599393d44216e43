"""The context calls of one streamed frame per kind of payload, in order and with their row arguments, against the trace this file
builds from the band bounds, the stencils' reaches and the band loop of the commit before bands.py existed
(test_bands_host.parent_schedule): a float frame, a uint16 frame with stops, an exposure="device" frame read through a window with
rows above and below it, a Bayer mosaic.  2368 x 2368, the smallest frame the gate admits, in stream_bands = 4 (six bands with the
taper), LUTs only and with halation, MTF and grain.

The streamed result is the one-piece render's (stream_bands = 0) bit for bit in every case: with LUTs only, and with the stencils on,
which run on the 360 mm format (6.6 px/mm) where halation and MTF are a few taps wide and take the direct form -- there a band's
stencil output is the whole frame's whatever the kind of source (tests/test_gpu_demosaic_stream.py; the FFT form, which anchors its
windows at a band's first row, is tests/test_gpu_stream_fuzz.py's)."""

import numpy as np
import pytest

from helpers import stocks
from test_bands_host import parent_schedule

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N = 2368
POINTWISE = dict(halation=False, sharpness=False, grain=0, exp_kelvin=6000, color_masking=1.0, frame_width=36, frame_height=36,
                 max_scale=None, lens_correction=False, seed=3)
STENCILS = dict(POINTWISE, halation=True, sharpness=True, grain=2, frame_width=360, frame_height=360, halation_green_factor=0.3)
ROW_KEYS = ("y0", "y1", "src_gy0", "in_gy0", "dst_gy0", "rows", "gy0", "H", "window", "identity_done", "clip", "passes")
CTX_CALLS = ("stage_front", "stage_front_split", "stage_halation", "stage_mtf", "decode_u16", "decode_u16_auto", "demosaic",
             "exposure_rows", "exposure_finish")
STOPS = 0.5


def entry(name, args, kw):
    """(name, shape of the first tensor argument, the plain positional arguments, the row keywords)."""
    shape = tuple(args[0].shape) if args and torch.is_tensor(args[0]) else None
    plain = tuple(a for a in args if isinstance(a, (int, float, tuple)))
    return name, shape, plain, {k: kw[k] for k in ROW_KEYS if k in kw}


@pytest.fixture(scope="module")
def proc():
    from raw2film_amd import HipProcessor

    p = HipProcessor(cameras={}, lenses={}, device=0)
    log = p.trace = dict(on=False, inside=0, calls=[], idents=[], bounds=None)

    def tap(name, fn):
        def call(*a, **k):
            if not log["on"] or log["inside"]:  # (what an entry point calls itself is its own business)
                return fn(*a, **k)
            log["calls"].append(entry(name, a, k))
            log["inside"] += 1
            try:
                res = fn(*a, **k)
            finally:
                log["inside"] -= 1
            if name == "stage_front_split":
                log["idents"].append(res)
            return res
        return call

    for name in CTX_CALLS:
        setattr(p.ctx, name, tap(name, getattr(p.ctx, name)))
    for bits, d in list(p._depths.items()):
        p._depths[bits] = d._replace(front=tap("front", d.front), tail=tap("tail", d.tail))
    inner = p._run_bands

    def run_bands(frame, *a, **k):
        log.update(on=True, calls=[], idents=[], bounds=list(frame.bounds))
        try:
            return inner(frame, *a, **k)
        finally:
            log["on"] = False

    p._run_bands = run_bands
    yield p
    p.close()


@pytest.fixture(scope="module")
def frames():
    from raw2film_amd.raw import RawProfile
    from raw2film_amd.synthetic import synthetic_frame

    rows = N + 32  # the square format keeps 2368 of 2400 rows: a window with 16 rows above and 16 below it
    f32 = np.ascontiguousarray(np.kron(synthetic_frame(rows // 8, N // 8, seed=8), np.ones((8, 8, 1), np.float32)))
    u16 = (np.clip(f32, 0.0, 1.0) * 40000.0).astype(np.uint16)
    rng = np.random.default_rng(17)
    y, x = np.mgrid[0:rows, 0:N].astype(np.float32)
    mosaic = np.clip(600 + 9000 * (0.5 + 0.5 * np.sin(x / 230.0) * np.cos(y / 170.0)) + rng.normal(0, 120, (rows, N)), 0, 16383).astype(np.uint16)
    prof = RawProfile("RGGB", black=512, multipliers=(7.9, 4.1, 6.2), matrix=((0.52, 0.27, 0.15), (0.25, 0.68, 0.07), (0.03, 0.12, 0.81)))
    return {"float": (np.ascontiguousarray(f32[:N]), {}),
            "u16": (np.ascontiguousarray(u16[:N]), dict(exposure=STOPS)),
            "device": (u16, dict(exposure="device")),
            "mosaic": (mosaic, dict(raw_profile=prof, half_size=False, exposure=STOPS))}


def expected_trace(proc, kind, src, extra, bounds, settings, idents):
    from raw2film_amd import decode

    hal, mtf, grain = bool(settings["halation"]), bool(settings["sharpness"]), bool(settings["grain"])
    pointwise = not (hal or mtf or grain)
    ha, ma = (proc._halation_reach if hal else (0, 0)), (proc._mtf_reach if mtf else (0, 0))
    H, n, W = bounds[-1], len(bounds) - 1, N
    factor = float(decode.exposure_factor(STOPS))
    load = dict(frame_width=settings["frame_width"], frame_height=settings["frame_height"], max_scale=None, **extra)
    trace = []
    if kind == "device":
        Hf, Wf, root = src.shape[0], src.shape[1], float(decode.exposure_root(None))
        r0, c0, nr, nc = proc.extract_image_data_cpu(src, **load)["u16_window"]
        assert (r0, nr, nc) == (16, N, N) and Hf - r0 - nr == 16
        ub = [0] + [r0 + b for b in bounds[1:-1]] + [Hf]
        trace += [("exposure_rows", (ub[k + 1] - ub[k], Wf, 3), (root,), dict(gy0=ub[k], H=Hf)) for k in range(n)]
        trace.append(("exposure_finish", None, (Hf, Wf, root), {}))
    if kind == "mosaic":
        window = proc.extract_image_data_cpu(src, **load)["demosaic"]["window"]
        assert tuple(window) == (16, 0, N, N)
    fronts = 0
    for stage, b in parent_schedule(n, hal, mtf, pointwise):
        y0, y1 = bounds[b], bounds[b + 1]
        if stage == "front":
            if kind == "u16":
                trace.append(("decode_u16", (y1 - y0, W, 3), (factor,), {}))
            elif kind == "device":
                trace.append(("decode_u16_auto", (y1 - y0, Wf, 3), ((0, c0, y1 - y0, nc),), {}))
            elif kind == "mosaic":
                # (a plain profile: neither Blend nor step M goes along)
                trace.append(("demosaic", tuple(src.shape), (factor,), dict(rows=(y0, y1), window=window, clip=None, passes=0)))
            band = (y1 - y0, W, 3)
            if pointwise:
                trace.append(("front", band, (), dict(y0=y0, y1=y1, in_gy0=y0)))
            elif hal:
                trace.append(("stage_front_split", band, (), dict(y0=y0, y1=y1, in_gy0=y0)))
            else:
                trace.append(("stage_front", band, (1,), dict(y0=y0, y1=y1, in_gy0=y0, dst_gy0=0)))
            fronts += 1
        elif stage == "halation":
            lo, hi = max(y0 - ha[0], 0), min(y1 + ha[1], H)
            trace.append(("stage_halation", (3, hi - lo, W), (), dict(y0=y0, y1=y1, src_gy0=lo, dst_gy0=0, identity_done=idents[fronts - 1])))
        elif stage == "mtf":
            lo, hi = max(y0 - ma[0], 0), min(y1 + ma[1], H)
            trace.append(("stage_mtf", (3, hi - lo, W), (), dict(y0=y0, y1=y1, src_gy0=lo, dst_gy0=0)))
        elif not pointwise:
            trace.append(("tail", (3, H, W), (), dict(y0=y0, y1=y1, src_gy0=0)))
    return trace


@pytest.mark.parametrize("what", ("pointwise", "stencils"))
@pytest.mark.parametrize("kind", ("float", "u16", "device", "mosaic"))
def test_the_calls_of_a_streamed_frame(proc, frames, kind, what):
    neg, prt = stocks()[:2]
    src, extra = frames[kind]
    settings = dict(POINTWISE if what == "pointwise" else STENCILS)
    log = proc.trace
    log["bounds"] = None
    proc.stream_bands, proc.stream_rejected = 4, "unset"
    got = proc.process(src, neg, 6, 0.4, cache=False, print_film=prt, **settings, **extra).copy()
    assert proc.stream_rejected is None and log["bounds"] is not None, f"the frame did not stream: {proc.stream_rejected}"
    bounds, calls, idents = log["bounds"], list(log["calls"]), list(log["idents"])
    assert bounds[0] == 0 and bounds[-1] == N and len(bounds) - 1 > 4, bounds
    want_calls = expected_trace(proc, kind, src, extra, bounds, settings, idents)
    print(f"{kind} {what}: {len(bounds) - 1} bands, {len(calls)} calls recorded, {len(want_calls)} expected")
    for i, (a, b) in enumerate(zip(calls, want_calls)):
        assert a == b, f"call {i}: {a} where the loop of the commit before made {b}"
    assert len(calls) == len(want_calls)
    log["bounds"] = None
    proc.stream_bands = 0
    try:
        want = proc.process(src, neg, 6, 0.4, cache=False, print_film=prt, **settings, **extra)
    finally:
        proc.stream_bands = 16
    assert log["bounds"] is None  # (one piece: no band loop)
    assert got.shape == want.shape == (N, N, 3) and got.dtype == want.dtype == np.uint8
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    print(f"{kind} {what}: {int(np.count_nonzero(d))} of {d.size} samples differ from the one-piece render, by at most {int(d.max())}")
    assert not d.any()
