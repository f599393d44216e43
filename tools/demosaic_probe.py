"""What a Bayer mosaic costs end to end against LibRaw's uint16 RGB frame, and what the demosaic kernels cost on the device
(profiles/r16_demosaic_probe.txt).

    python tools/demosaic_probe.py [--out FILE] [--repeats N] [--rounds R] [--parent DIR]

End to end, for a 24 MP and a 100 MP sensor, full and half size, the source in pageable and in pinned host memory, wall clock around
the call with a device synchronisation on either side:
  (a) process(uint16 RGB frame, exposure=stops, cache=False)        the parent commit (--parent DIR: a built checkout of it)
  (b) the same call                                                 this tree
  (c) process(uint16 mosaic, raw_profile=p, exposure=stops, cache=False, half_size=...)   this tree
Every leg runs in child processes of its own that import their tree's package and load its library; the legs take turns, R rounds
of each, N calls after a warm-up per case and round.  The RGB frame of a case has the size the demosaic gives the mosaic of that
case ((H, W, 3), or (H / 2, W / 2, 3) at half size): what LibRaw would hand over for the same sensor.  Both sources are noise of
the same range -- the calls' times do not depend on the picture, and a 100 MP NumPy demosaic for a matching one would take minutes.
(a) and (b) must agree within the spread the file shows; (c) is read against (b).

Kernels, in this process (device events, median of round medians): r2f_demosaic_u16 full and half size at both sensor sizes, beside
r2f_stream_copy over the same byte count (8 B per mosaic sample at full size: 2 read, 6 written; 3.5 B per sample at half size) in the
same run.

    python tools/demosaic_probe.py --stream [--out FILE] [--repeats N] [--rounds R]

The streamed mosaic (profiles/r17_mosaic_stream_probe.txt), all in this process.  Kernels: r2f_demosaic_f32 against r2f_demosaic_u16
followed by r2f_decode_u16 on the same frame, with the bytes each moves.  Calls: process(mosaic, exposure=stops, cache=False) with
stream_bands = 16 (the mosaic in row bands), with stream_bands = 0 (one piece: what the call did before a mosaic streamed, the
baseline) and process(uint16 RGB) streamed, each from pageable and from pinned memory; the legs take turns call by call, R rounds of N
calls after a warm-up each; a leg's spread over all its calls is the run-to-run spread the comparison is read against.

    python tools/demosaic_probe.py --calls [--out FILE] [--repeats N] [--rounds R] [--parent DIR]

The host cost of a call (profiles/r31_demosaic_call_cost.txt): HipContext.demosaic_u16, demosaic_median_u16 (one pass) and demosaic_f32
on a 64 x 64 mosaic, one tile, which is launch-bound: what the Python method and the C++ entry point spend between the caller and the
launch shows.  Wall clock around a tight loop of N calls (default 2000) with a device synchronisation on either side, after a warm-up
of a tenth as many; this tree and the parent's checkout (--parent DIR) in child processes of their own that take turns, R rounds.  A
leg's range over its rounds is the round-to-round spread the two medians are read against.
Needs a GPU: there is no CPU path.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("R2F_PROBE_PKG", ROOT)  # (a child of the parent's checkout imports its package from there)
if PKG not in sys.path:
    sys.path.insert(0, PKG)

SIZES = (("24 MP", 4000, 6000), ("100 MP", 8192, 12288))
STOPS = 0.5


def spread(xs):
    return f"{min(xs):8.2f} .. {max(xs):8.2f} ms (median {statistics.median(xs):8.2f}, n = {len(xs)})"


def render_kw(prt, H, W):
    fw = max(36.0, W / 341.0)  # ~341 px/mm at most (below max_scale), the frame kept whole
    return dict(print_film=prt, lens_correction=False, seed=5, cache=False, frame_width=fw, frame_height=fw * H / W,
                halation_green_factor=0.3, exposure=STOPS)


def raw_profile():
    from raw2film_amd.raw import RawProfile

    return RawProfile("RGGB", black=512, multipliers=(7.9, 4.1, 6.2), matrix=((0.52, 0.27, 0.15), (0.25, 0.68, 0.07), (0.03, 0.12, 0.81)))


def child(mode, repeats):
    """One turn of one leg: `mode` = "rgb" (any tree) or "mosaic" (this tree) -> JSON {case: [ms, ...]} on stdout."""
    import torch

    from raw2film_amd import HipProcessor, filmstock

    stocks = filmstock.builtin_stocks()
    neg, prt = stocks["Kodak Portra 400"], stocks["Kodak 2383"]
    proc = HipProcessor(device=0, result_buffers=2)
    out = {}
    for label, H, W in SIZES:
        for half in (False, True):
            h, w = (H // 2, W // 2) if half else (H, W)
            rng = np.random.default_rng(H + half)
            if mode == "rgb":
                pageable, extra = rng.integers(0, 40000, (h, w, 3), dtype=np.uint16), {}
            else:
                pageable, extra = rng.integers(0, 16384, (H, W), dtype=np.uint16), dict(raw_profile=raw_profile(), half_size=half)
            pinned = torch.from_numpy(pageable.view(np.int16)).pin_memory().numpy().view(np.uint16)
            kw = dict(render_kw(prt, h, w), **extra)
            times = {"pageable": [], "pinned": []}
            for r in range(repeats + 1):
                for memory, frame in (("pageable", pageable), ("pinned", pinned)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res = proc.process(frame, neg, 6, 0.4, **kw)
                    torch.cuda.synchronize()
                    dt = (time.perf_counter() - t0) * 1e3
                    assert res.shape == (h, w, 3)
                    del res
                    if r:
                        times[memory].append(dt)
            for memory, xs in times.items():
                out[f"{label}, {'half' if half else 'full'} size, {memory}"] = xs
            del pageable, pinned
    proc.close()
    print(json.dumps(out))


def calls_child(calls):
    """One turn of one leg of --calls -> JSON {method: microseconds per call} on stdout."""
    import torch

    from raw2film_amd.context import HipContext

    ctx = HipContext(0)
    m = torch.from_numpy(np.random.default_rng(31).integers(0, 16384, (64, 64), dtype=np.uint16).view(np.int16)).cuda()
    params = raw_profile().plan(64, 64)
    u16, f32 = torch.empty((64, 64, 3), dtype=torch.int16, device="cuda"), torch.empty((64, 64, 3), dtype=torch.float32, device="cuda")
    legs = {"demosaic_u16": lambda: ctx.demosaic_u16(m, params, out=u16),
            "demosaic_median_u16": lambda: ctx.demosaic_median_u16(m, params, 1, out=u16),
            "demosaic_f32": lambda: ctx.demosaic_f32(m, params, 1.5, out=f32)}
    out = {}
    for name, fn in legs.items():
        for _ in range(max(calls // 10, 1)):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out[name] = (time.perf_counter() - t0) * 1e6 / calls
    ctx.close()
    print(json.dumps(out))


def call_cost(parent, rounds, calls, emit):
    legs = [("this tree", ROOT)] + ([("parent", os.path.abspath(parent))] if parent else [])
    res = {}
    for r in range(rounds):
        for name, pkg in (legs if r % 2 == 0 else legs[::-1]):  # (in turn, the other one first in every other round)
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "calls", "--repeats", str(calls)],
                                 env=dict(os.environ, R2F_PROBE_PKG=pkg), capture_output=True, text=True, timeout=300)
            if run.returncode != 0:
                raise RuntimeError(f"{name}: exit {run.returncode}: {run.stderr[-2000:]}")
            for method, us in json.loads(run.stdout.strip().splitlines()[-1]).items():
                res.setdefault(method, {}).setdefault(name, []).append(us)
    emit(f"host cost of a call: a 64 x 64 Bayer mosaic (one tile), `out` given; microseconds per call, wall clock around {calls} calls in a "
         f"tight loop with a device synchronisation on either side; each leg in child processes of its own, {rounds} rounds in turn")
    if not parent:
        emit("  (no --parent checkout given: only this tree was run)")
    for method, by_leg in res.items():
        emit(f"  {method}")
        for name, _ in legs:
            xs = by_leg[name]
            emit(f"    {name:<10s} {min(xs):7.2f} .. {max(xs):7.2f} us (median {statistics.median(xs):7.2f}, n = {len(xs)})")
        if parent:
            t, xs = statistics.median(by_leg["this tree"]), by_leg["parent"]
            emit(f"    this tree's median / the parent's = {t / statistics.median(xs):.3f}; "
                 f"{'inside' if min(xs) <= t <= max(xs) else 'OUTSIDE'} the parent's range over its rounds")
    emit()


def end_to_end(parent, rounds, repeats, emit):
    legs = [("(b) RGB, this tree", ROOT, "rgb"), ("(c) mosaic, this tree", ROOT, "mosaic")]
    if parent:
        legs.insert(0, ("(a) RGB, parent", os.path.abspath(parent), "rgb"))
    res = {}
    for _ in range(rounds):
        for name, pkg, mode in legs:
            env = dict(os.environ, R2F_PROBE_PKG=pkg)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--repeats", str(repeats)], env=env,
                               capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise RuntimeError(f"{name}: exit {r.returncode}: {r.stderr[-2000:]}")
            for case, xs in json.loads(r.stdout.strip().splitlines()[-1]).items():
                res.setdefault(case, {}).setdefault(name, []).extend(xs)
            print(f"[round {_ + 1} of {rounds}: {name} done]", file=sys.stderr, flush=True)
    emit(f"end to end: process(..., exposure={STOPS}, cache=False), full render (halation, MTF, grain, print film), result_buffers=2; "
         f"each leg in child processes of its own, {rounds} rounds in turn, {repeats} calls after a warm-up per case and round; wall clock")
    if not parent:
        emit("  (no --parent checkout given: leg (a) was not run)")
    for case, by_leg in res.items():
        emit(f"  {case}")
        for name, _, _ in legs:
            emit(f"    {name:<24s} {spread(by_leg[name])}")
        b, c = statistics.median(by_leg["(b) RGB, this tree"]), statistics.median(by_leg["(c) mosaic, this tree"])
        emit(f"    (c) / (b) = {c / b:.2f}")
    emit()


def timed(torch, fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(iters):
        start.record()
        fn()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
    return float(np.median(times))


def kernels(rounds, iters, emit):
    import torch

    from raw2film_amd.context import HipContext

    ctx = HipContext(0)
    prof = raw_profile()
    emit(f"kernels ({torch.cuda.get_device_name(0)}): device events, {iters} launches per round median, {rounds} interleaved rounds")
    for label, H, W in SIZES:
        mosaic = torch.randint(0, 16384, (H, W), dtype=torch.int16, device="cuda")
        for half in (False, True):
            params = prof.plan(H, W, half)
            out = torch.empty((params.out_h, params.out_w, 3), dtype=torch.int16, device="cuda")
            nbytes = mosaic.numel() * 2 + out.numel() * 2  # algorithmic: every sample read once, every output written once
            a = torch.empty(nbytes // 2 // 16 * 16, dtype=torch.uint8, device="cuda")  # the copy moves the same bytes: half read, half written
            b = torch.empty_like(a)
            for _ in range(3):
                ctx.demosaic_u16(mosaic, params, out=out)
                ctx.stream_copy(a, b)
            k, c = [], []
            for _ in range(rounds):
                k.append(timed(torch, lambda: ctx.demosaic_u16(mosaic, params, out=out), iters))
                c.append(timed(torch, lambda: ctx.stream_copy(a, b), iters))
            km, cm = float(np.median(k)), float(np.median(c))
            emit(f"  {label} sensor, {'half' if half else 'full'} size: r2f_demosaic_u16 {km:.3f} ms (range {min(k):.3f} .. {max(k):.3f}) = "
                 f"{nbytes / km / 1e6:.0f} GB/s of {nbytes / H / W:.1f} B per sample; r2f_stream_copy of {2 * a.numel() / 1e6:.0f} MB "
                 f"{cm:.3f} ms (range {min(c):.3f} .. {max(c):.3f}) = {2 * a.numel() / cm / 1e6:.0f} GB/s; kernel / copy = {km / cm:.2f}")
            del out, a, b
        del mosaic
        torch.cuda.empty_cache()
    ctx.close()
    emit()


def stream_kernels(rounds, iters, emit):
    import torch

    from raw2film_amd.context import HipContext

    ctx = HipContext(0)
    prof = raw_profile()
    factor = float(np.float32(2.0 ** STOPS))
    emit(f"(a) kernels ({torch.cuda.get_device_name(0)}): device events, {iters} launches per round median, {rounds} interleaved rounds;")
    emit("    bytes are algorithmic (every sample read once, every output written once): fused = 2 B per mosaic sample + 12 B per pixel;")
    emit("    two kernels = 2 B per sample + 6 B per pixel written, then 6 B read + 12 B written")
    for label, H, W in SIZES:
        mosaic = torch.randint(0, 16384, (H, W), dtype=torch.int16, device="cuda")
        for half in (False, True):
            params = prof.plan(H, W, half)
            px = params.out_h * params.out_w
            u16 = torch.empty((params.out_h, params.out_w, 3), dtype=torch.int16, device="cuda")
            f32 = torch.empty((params.out_h, params.out_w, 3), dtype=torch.float32, device="cuda")

            def fused():
                ctx.demosaic_f32(mosaic, params, factor, out=f32)

            def two():
                ctx.demosaic_u16(mosaic, params, out=u16)
                ctx.decode_u16(u16, factor, out=f32)

            for _ in range(3):
                fused(), two()
            a, b = [], []
            for _ in range(rounds):
                a.append(timed(torch, fused, iters))
                b.append(timed(torch, two, iters))
            am, bm = float(np.median(a)), float(np.median(b))
            fused_bytes, two_bytes = 2 * H * W + 12 * px, 2 * H * W + 24 * px
            emit(f"  {label} sensor, {'half' if half else 'full'} size: r2f_demosaic_f32 {am:.3f} ms (range {min(a):.3f} .. {max(a):.3f}), "
                 f"{fused_bytes / 1e6:.0f} MB = {fused_bytes / am / 1e6:.0f} GB/s; r2f_demosaic_u16 + r2f_decode_u16 {bm:.3f} ms (range "
                 f"{min(b):.3f} .. {max(b):.3f}), {two_bytes / 1e6:.0f} MB = {two_bytes / bm / 1e6:.0f} GB/s; fused / two = {am / bm:.2f}")
            del u16, f32
        del mosaic
        torch.cuda.empty_cache()
    ctx.close()
    emit()


def stream_calls(rounds, repeats, emit):
    import torch

    from raw2film_amd import HipProcessor, filmstock

    stocks = filmstock.builtin_stocks()
    neg, prt = stocks["Kodak Portra 400"], stocks["Kodak 2383"]
    proc = HipProcessor(device=0, result_buffers=2)
    emit(f"(b) calls: process(..., exposure={STOPS}, cache=False), full render (halation, MTF, grain, print film), result_buffers=2, one "
         f"process; the legs take turns call by call, {rounds} rounds of {repeats} calls after a warm-up; wall clock with a device "
         "synchronisation on either side")
    legs = (("mosaic, stream_bands = 16", "mosaic", 16), ("mosaic, stream_bands = 0 (baseline)", "mosaic", 0), ("uint16 RGB, streamed", "rgb", 16))
    for label, H, W in SIZES:
        for half in (False, True):
            h, w = (H // 2, W // 2) if half else (H, W)
            rng = np.random.default_rng(H + half)
            src = {"mosaic": rng.integers(0, 16384, (H, W), dtype=np.uint16), "rgb": rng.integers(0, 40000, (h, w, 3), dtype=np.uint16)}
            pinned = {k: torch.from_numpy(v.view(np.int16)).pin_memory().numpy().view(np.uint16) for k, v in src.items()}
            extra = {"mosaic": dict(raw_profile=raw_profile(), half_size=half), "rgb": {}}
            kw = render_kw(prt, h, w)
            times, streamed = {}, {}
            for _ in range(rounds):
                for r in range(repeats + 1):
                    for memory, frames in (("pageable", src), ("pinned", pinned)):
                        for name, kind, bands in legs:
                            proc.stream_bands, proc.stream_rejected = bands, "not asked"
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            res = proc.process(frames[kind], neg, 6, 0.4, **kw, **extra[kind])
                            torch.cuda.synchronize()
                            dt = (time.perf_counter() - t0) * 1e3
                            assert res.shape == (h, w, 3)
                            del res
                            streamed[name] = proc.stream_rejected is None
                            if r:
                                times.setdefault((memory, name), []).append(dt)
            proc.stream_bands = 16
            emit(f"  {label}, {'half' if half else 'full'} size ({2 * H * W / 1e6:.0f} MB of mosaic, {6 * h * w / 1e6:.0f} MB of uint16 RGB)")
            for memory in ("pageable", "pinned"):
                for name, _, bands in legs:
                    assert streamed[name] == (bands > 1), (name, proc.stream_rejected)
                    emit(f"    {memory:<9s} {name:<36s} {spread(times[(memory, name)])}")
                s, o, g = (statistics.median(times[(memory, name)]) for name, _, _ in legs)
                emit(f"    {memory:<9s} streamed / one piece = {s / o:.2f}; streamed mosaic / streamed RGB = {s / g:.2f}")
            del src, pinned
    proc.close()
    emit()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--stream", action="store_true", help="the streamed mosaic's probe (profiles/r17_mosaic_stream_probe.txt)")
    ap.add_argument("--calls", action="store_true", help="the host cost of a call (profiles/r31_demosaic_call_cost.txt)")
    ap.add_argument("--repeats", type=int, default=None, help="calls per case and round (default 5; --calls: 2000 per loop)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit for leg (a)")
    ap.add_argument("--child", default=None, choices=("rgb", "mosaic", "calls"))
    args = ap.parse_args()
    if args.repeats is None:
        args.repeats = 2000 if args.calls else 5
    if args.child:
        return calls_child(args.repeats) if args.child == "calls" else child(args.child, args.repeats)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("demosaic_probe needs a GPU")
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    if args.out is None:
        name = "r31_demosaic_call_cost.txt" if args.calls else "r17_mosaic_stream_probe.txt" if args.stream else "r16_demosaic_probe.txt"
        args.out = os.path.join(ROOT, "profiles", name)
    if args.calls:
        emit("What a demosaic call costs on the host, this tree against the parent commit (tools/demosaic_probe.py --calls)")
        emit()
        call_cost(args.parent, args.rounds, args.repeats, emit)
    elif args.stream:
        emit("A Bayer mosaic streamed in row bands against the same call in one piece (tools/demosaic_probe.py --stream)")
        emit()
        stream_kernels(args.rounds, args.iters, emit)
        stream_calls(args.rounds, args.repeats, emit)
    else:
        emit("Bayer mosaic against LibRaw's uint16 RGB frame (tools/demosaic_probe.py)")
        emit()
        kernels(args.rounds, args.iters, emit)
        end_to_end(args.parent, args.rounds, args.repeats, emit)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
