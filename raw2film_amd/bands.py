"""The host-side plan of a streamed frame (HipProcessor._run_bands runs it): the row bands, the order in which the stages take
them, and how each kind of payload gets its rows into the float frame.  No torch at import, no processor state.

The dependence rule of the schedule: a stencil stage (halation, MTF) reads into the band after its own, so it takes band b once the
stage before it has produced band min(b + 1, n - 1); the tail takes band b once the stage before it has produced band b; every
stage takes every band once, in band order."""

from __future__ import annotations

from typing import Callable, NamedTuple

from . import _lib
from .payload import DEVICE_EXPOSURE, REPAIR_REACH, frame_shape, mosaic_upload_bounds


def plan_bands(H, flags, ha, ma, bands, taper):
    """(row bounds, None) of the bands a frame of H rows streams in, or (None, why it cannot).  `flags`: prepare()'s; `ha`, `ma`:
    (rows above, rows below) the halation / MTF stencils read, (0, 0) for a stage that does not run."""
    if flags & _lib.F_BURN:
        return None, "highlight burn (a function of the whole grained frame)"
    floor_rows = max(2 * max(ha + ma) + 2, 64)  # a band holds its neighbours' halo (and is worth a launch)
    n = min(int(bands), max(H // 512, 2))
    while n > 1 and H // n < floor_rows:
        n -= 1
    if n < 2:
        return None, f"{n} band(s) of {H} rows above the stencils' reach {ha} + {ma}"
    bounds = [H * i // n for i in range(n + 1)]
    # the last bands are the ones nothing hides (their stencil stages, tail and download run behind the last byte of the upload):
    # the final `taper` of them are halved while they stay above the stencils' reach (100 MP: 23.26 -> 22.73 ms with 2)
    cut = [(bounds[i] + bounds[i + 1]) // 2 for i in range(max(n - int(taper), 0), n) if bounds[i + 1] - bounds[i] >= 2 * floor_rows]
    return sorted(set(bounds + cut)), None


def stage_schedule(n, halation, mtf, pointwise):
    """The (stage, band) pairs of a frame of n bands in the order they are queued: "front" (a band's arrival, its decode and S0 + S1),
    "halation" and "mtf" where those stages run, "tail" (the tail and the band's way back).  After every front call each later
    stage, in pipeline order and again until none moves, takes its next band if the module's rule allows it.  A pointwise frame
    (LUTs only: the front call writes the result, "tail" is the hand-back alone) has no stencil stage whatever the flags say."""
    stages = ["front"]
    if halation and not pointwise:
        stages.append("halation")
    if mtf and not pointwise:
        stages.append("mtf")
    stages.append("tail")
    done = [0] * len(stages)  # bands through each stage
    for k in range(n):
        yield "front", k
        done[0] = k + 1
        moved = True
        while moved:
            moved = False
            for i in range(1, len(stages)):
                b = done[i]
                reach = 0 if stages[i] == "tail" else 1  # bands past its own that the stage reads of the one before it
                if b < n and done[i - 1] > min(b + reach, n - 1):
                    yield stages[i], b
                    done[i], moved = b + 1, True


class BandSource(NamedTuple):
    """What the band loop asks of a payload's kind (band_source makes one per streamed frame)."""
    frame: tuple  # (H, W, chans) of the float frame the pipeline renders
    landing: str  # the device buffer the uploads land in: "image" (the float frame itself), "u16" or "mosaic" (int16, of their own)
    landing_shape: tuple
    upload_bounds: Callable  # (band bounds) -> ub: upload k carries the payload tensor's rows ub[k]:ub[k + 1] into the same rows of landing
    queue_all: bool  # a pinned source's uploads are all queued before the first band
    measure: Callable | None  # (ctx, landing, ub, wait): what runs behind the arrivals ahead of every band; wait(k) makes the launching
    #                           stream await upload k, once however often it is called (ub: upload_bounds' answer for the frame's bounds)
    decode: Callable  # (ctx, landing, image, a0, a1): the rows a0:a1 of the float frame from what has landed


class StreamedFrame(NamedTuple):
    """A frame set up for the band loop (HipProcessor._stream_plan makes one, _run_bands takes it)."""
    host: object  # the payload's tensor on the host
    source: BandSource
    params: object  # the frame's r2f_params, already written to the device-side frame block
    bounds: list  # plan_bands' row bounds
    bufs: dict  # the device buffers the frame works in
    halation_reach: tuple  # (rows above, rows below) the stencil reads; (0, 0) for a stage that does not run
    mtf_reach: tuple


def band_source(payload, shape, dtype, repair_count=None) -> BandSource:
    """The BandSource of a payload that stream_rejection has passed.  `shape`, `dtype`: of its tensor, as stream_rejection takes them.
    repair_count: for a mosaic with a `repair` step, the device word its bands add their repaired samples to (None: not counted)."""
    shape = tuple(int(v) for v in shape)
    frame = frame_shape(payload, shape)
    if dtype != "torch.int16":  # a float frame lands where the pipeline reads it
        def clamp(ctx, landing, image, a0, a1):
            image[a0:a1].clamp_(0.0, 65504.0)  # np.clip(image, 0, 65504) of gpu_processor.py:275, band by band

        return BandSource(frame, landing="image", landing_shape=frame, upload_bounds=list, queue_all=False, measure=None,
                          decode=clamp if payload.get("clip_on_device") else lambda ctx, landing, image, a0, a1: None)
    frame, factor = frame[:2] + (3,), payload.get("u16_factor")
    step = payload.get("demosaic")
    if step:  # a Bayer mosaic: band k travels with the mosaic rows its demosaic reads beyond those of the bands before it
        window, params, clip, median = step["window"], step["params"], step.get("clip"), step.get("median", 0)

        # (only a Bayer mosaic streams: stream_rejection has refused the other kind)
        repair, half, rows = step.get("repair"), _lib.MOSAIC_KINDS[_lib.DemosaicParams].reduced(params), int(window[2])
        if repair is not None:
            repair_params = repair.plan(step["profile"], shape[0], shape[1])
            repaired_to = []  # [the mosaic row up to which the bands so far have repaired] (they come in order)

        def repaired(ctx, landing, a1):
            """The context's second mosaic, repaired as far as the demosaic of the window's rows [0, a1) reads: this band adds the
            mosaic rows that no band before it repaired, so every row is repaired exactly once (upload k brought REPAIR_REACH more
            rows than the demosaic reads: what the repair of its last rows reads)."""
            lo, hi = mosaic_upload_bounds([0, a1] if a1 == rows else [0, a1, rows], window, shape[0], half, median)[:2]
            done = repaired_to.pop() if repaired_to else lo
            repaired_to.append(max(hi, done))
            return ctx.mosaic_repair(landing, repair_params, rows=(done, repaired_to[0]), count=repair_count)

        def demosaic(ctx, landing, image, a0, a1):
            if repair is not None:
                landing = repaired(ctx, landing, a1)
            # (clip: a ("blend", clip) profile's level or None; median: a profile's median_passes or 0, step M then reads `median`
            # output rows past the band's ends)
            ctx.demosaic(landing, params, factor, clip=clip, passes=median, window=window, out=image, rows=(a0, a1))

        # A pinned mosaic queues every upload at once.  Its bytes are a third of the RGB frame's, so the render, not the upload, sets
        # the pace; with upload k queued only when band k's turn came the call was no faster than in one piece (100 MP: 15.9 against
        # 15.8 ms, profiles/r17_mosaic_stream_probe.txt).
        return BandSource(frame, landing="mosaic", landing_shape=shape, queue_all=True, measure=None, decode=demosaic,
                          upload_bounds=lambda bounds: mosaic_upload_bounds(bounds, window, shape[0], half, median,
                                                                            REPAIR_REACH if repair is not None else 0))
    if factor == DEVICE_EXPOSURE:
        # the whole uint16 frame goes up (the statistic is the whole frame's), the bands are rows of its window: band k travels as the
        # frame rows ub[k]:ub[k + 1], the first and the last taking the rows above and below the window along
        (Hf, Wf), (r0, c0, _, nc), root = shape[:2], payload["u16_window"], payload["exposure_root"]

        def measure(ctx, landing, ub, wait):
            # every band's row statistic behind its arrival, then the finish: the factor is in the device-side record before the
            # first decode reads it, and the host never learns it in between (the render starts behind the upload in this mode)
            for k in range(len(ub) - 1):
                wait(k)
                ctx.exposure_rows(landing[ub[k]:ub[k + 1]], root, H=Hf, gy0=ub[k])
            ctx.exposure_finish(Hf, Wf, root)

        def decode_window(ctx, landing, image, a0, a1):
            ctx.decode_u16_auto(landing[r0 + a0:r0 + a1], (0, c0, a1 - a0, nc), out=image[a0:a1])

        return BandSource(frame, landing="u16", landing_shape=shape, queue_all=False, measure=measure, decode=decode_window,
                          upload_bounds=lambda bounds: [0] + [b + r0 for b in bounds[1:-1]] + [Hf])

    def decode(ctx, landing, image, a0, a1):
        ctx.decode_u16(landing[a0:a1], factor, out=image[a0:a1])

    return BandSource(frame, landing="u16", landing_shape=shape, upload_bounds=list, queue_all=False, measure=None, decode=decode)
