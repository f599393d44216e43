"""What a deferred profile (raw2film_amd.raw.RawLevels) costs: the data-maximum kernel beside a library reduction and a copy of the
same buffer, the host pass it replaces, and the call with and without it (profiles/r24_levels_probe.txt).

    python tools/levels_probe.py [--out FILE] [--repeats N] [--rounds R] [--sizes 24,100]

All in this process, the legs of each part taking turns; 24 MP (4000 x 6000) and 100 MP (8192 x 12288) mosaics of noise of a
sensor's range (no time here depends on the picture).
  (a) kernels, device events, median of N launches per round: r2f_mosaic_maximum with a Bayer and with an X-Trans table, beside
      torch's own one-pass reduction of the same buffer (amax of the int16 view: 2 B per sample read, one value written) and a
      device-to-device copy of it (2 B read + 2 B written per sample: half its time is what a pure read at the copy's byte rate takes).
      Each result is checked against the NumPy maximum of the same array.
  (b) the host pass: np.max of the pageable array, and the same with the black level subtracted per phase (one strided np.max per
      phase of the period: the cheapest NumPy form), wall clock.
  (c) calls, wall clock around the call with a device synchronisation on either side: process(mosaic, cache=False, exposure=stops)
      with a deferred profile; with the numeric profile it resolves to, in one piece (stream_bands = 0: the parent commit's path for
      that profile, and the route a deferred profile takes); and with the numeric profile streamed in row bands (stream_bands = 16),
      which a deferred profile gives up.  Pageable and pinned sources.  The deferred and the one-piece numeric results are compared
      byte for byte.
Needs a GPU: there is no CPU path.
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = {"24": ("24 MP", 4000, 6000), "100": ("100 MP", 8192, 12288)}
STOPS = 0.5
BLACK = 512
MATRIX = ((0.52, 0.27, 0.15), (0.25, 0.68, 0.07), (0.03, 0.12, 0.81))


def spread(xs):
    return f"{min(xs):8.3f} .. {max(xs):8.3f} ms (median {statistics.median(xs):8.3f}, n = {len(xs)})"


def tables():
    """Distinct levels per phase around BLACK, for both periods."""
    return {2: [BLACK + 3 * i for i in range(4)], 6: [BLACK + i for i in range(36)]}


def host_maximum(mosaic, black, period):
    """max(raw - black[phase], 0) over the frame as period * period strided maxima."""
    best = 0
    for py in range(period):
        for px in range(period):
            best = max(best, int(mosaic[py::period, px::period].max()) - black[py * period + px])
    return best


def device_ms(torch, fn, repeats, stall):
    """Median device time of `repeats` launches of fn, each between its own pair of events.  `stall` queues a few milliseconds of
    other work first, so that the launches and their events are all enqueued while the device is busy: a kernel of tens of
    microseconds is then timed from the end of the launch before it, not from the moment the host got round to launching it."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(repeats)]
    stall()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def kernels(torch, ctx, emit, sizes, rounds, repeats):
    emit(f"(a) kernels ({torch.cuda.get_device_name(0)}): device events, median of {repeats} launches per round, {rounds} rounds in turn, "
         "every batch of launches queued behind ~2 ms of copies")
    big = torch.zeros(1 << 28, dtype=torch.int32, device="cuda"), torch.empty(1 << 28, dtype=torch.int32, device="cuda")

    def stall():
        for _ in range(4):
            big[1].copy_(big[0])

    for label, H, W in sizes:
        host = np.random.default_rng(H).integers(0, 16384, (H, W), dtype=np.uint16)
        dev = torch.from_numpy(host.view(np.int16)).cuda()
        other = torch.empty_like(dev)
        word = torch.zeros(1, dtype=torch.int32, device="cuda")
        legs = {
            "r2f_mosaic_maximum, Bayer table": lambda: ctx.mosaic_maximum(dev, tables()[2], out=word),
            "r2f_mosaic_maximum, X-Trans table": lambda: ctx.mosaic_maximum(dev, tables()[6], out=word),
            "torch amax (int16 view)": lambda: torch.amax(dev),
            "device-to-device copy": lambda: other.copy_(dev),
        }
        for period in (2, 6):  # the results first: the timing is of a kernel that computes the model's value
            got, want = ctx.mosaic_maximum(dev, tables()[period]), host_maximum(host, tables()[period], period)
            if got != want:
                raise RuntimeError(f"{label}, period {period}: the device found {got}, NumPy {want}")
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in legs}
        for _ in range(rounds):
            for name, fn in legs.items():
                times[name].append(device_ms(torch, fn, repeats, stall))
        nbytes = 2.0 * H * W
        emit(f"  {label} ({H} x {W}, {nbytes / 1e6:.0f} MB)")
        ref = statistics.median(times["torch amax (int16 view)"])
        copy = statistics.median(times["device-to-device copy"])
        for name, xs in times.items():
            med = statistics.median(xs)
            note = f"{nbytes / med / 1e9:6.2f} TB/s read" if "copy" not in name else f"{2 * nbytes / med / 1e9:6.2f} TB/s read + written"
            ratio = f", {med / ref:4.2f} x torch amax, {med / (copy / 2):4.2f} x half the copy" if name.startswith("r2f") else ""
            emit(f"      {name:<36s} {med:7.3f} ms (range {min(xs):.3f} .. {max(xs):.3f}), {note}{ratio}")
        del dev, other


def host_pass(emit, sizes, repeats):
    emit(f"(b) the host pass the kernel replaces: wall clock, {repeats} passes after a warm-up, a pageable uint16 array")
    for label, H, W in sizes:
        host = np.random.default_rng(H).integers(0, 16384, (H, W), dtype=np.uint16)
        legs = {"np.max(mosaic)": lambda: int(host.max()), "per phase, Bayer (4 strided maxima)": lambda: host_maximum(host, tables()[2], 2),
                "per phase, X-Trans (36 strided maxima)": lambda: host_maximum(host, tables()[6], 6)}
        times = {name: [] for name in legs}
        for r in range(repeats + 1):
            for name, fn in legs.items():
                t0 = time.perf_counter()
                fn()
                if r:
                    times[name].append((time.perf_counter() - t0) * 1e3)
        emit(f"  {label}")
        for name, xs in times.items():
            emit(f"      {name:<40s} {spread(xs)}")


def calls(torch, emit, sizes, rounds, repeats):
    from raw2film_amd import HipProcessor, filmstock
    from raw2film_amd.raw import RawLevels, RawProfile

    stocks = filmstock.builtin_stocks()
    neg, prt = stocks["Kodak Portra 400"], stocks["Kodak 2383"]
    proc = HipProcessor(device=0, result_buffers=2)
    emit(f"(c) calls: process(mosaic, exposure={STOPS}, cache=False, half_size=False), full render, result_buffers=2; the legs take turns call "
         f"by call, {rounds} rounds of {repeats} calls after a warm-up; wall clock with a device synchronisation on either side")
    for label, H, W in sizes:
        pageable = np.random.default_rng(H).integers(0, 16384, (H, W), dtype=np.uint16)
        pinned = torch.from_numpy(pageable.view(np.int16)).pin_memory().numpy().view(np.uint16)
        d = int(pageable.max()) - BLACK
        deferred = RawProfile("RGGB", black=BLACK, multipliers=RawLevels((1.9, 1.0, 1.5), BLACK + int(d / 0.9)), matrix=MATRIX)
        numeric = deferred.resolve(d)
        fw = max(36.0, W / 341.0)
        kw = dict(print_film=prt, lens_correction=False, seed=5, cache=False, frame_width=fw, frame_height=fw * H / W, halation_green_factor=0.3,
                  exposure=STOPS, half_size=False)
        legs = (("deferred profile (one piece + the pass)", deferred, 16), ("numeric profile, one piece", numeric, 0),
                ("numeric profile, streamed", numeric, 16))
        times = {(name, memory): [] for name, _, _ in legs for memory in ("pageable", "pinned")}
        kept = {}
        for rnd in range(rounds):
            for r in range(repeats + (0 if rnd else 1)):
                for memory, frame in (("pageable", pageable), ("pinned", pinned)):
                    for name, profile, bands in legs:
                        proc.stream_bands = bands
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        res = proc.process(frame, neg, 6, 0.4, raw_profile=profile, **kw)
                        torch.cuda.synchronize()
                        dt = (time.perf_counter() - t0) * 1e3
                        if rnd or r:
                            times[(name, memory)].append(dt)
                        elif memory == "pageable" and name != legs[2][0]:  # (the first results of the two one-piece legs)
                            kept[name] = (res.copy(), proc.last_raw_scale)
                        del res
        a, b = kept[legs[0][0]], kept[legs[1][0]]
        if not np.array_equal(a[0], b[0]) or a[1] != {"data_maximum": d, "maximum_used": d, "adjusted": True} or b[1] is not None:
            raise RuntimeError(f"{label}: the deferred call does not render the resolved profile's bytes ({a[1]}, {b[1]})")
        emit(f"  {label} ({H} x {W}); data maximum {d}, adjusted; deferred == numeric one piece byte for byte")
        for memory in ("pageable", "pinned"):
            emit(f"    {memory}")
            for name, _, _ in legs:
                emit(f"      {name:<42s} {spread(times[(name, memory)])}")
            med = {name: statistics.median(times[(name, memory)]) for name, _, _ in legs}
            emit(f"      the pass + readback: {med[legs[0][0]] - med[legs[1][0]]:+.2f} ms; not streaming: {med[legs[0][0]] - med[legs[2][0]]:+.2f} ms")
        del pageable, pinned
    proc.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_levels_probe.txt"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="24,100")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("tools/levels_probe.py needs a GPU: there is no CPU path")
    from raw2film_amd.context import HipContext

    sizes = [SIZES[s] for s in args.sizes.split(",")]
    lines = []

    def emit(line=""):
        print(line, flush=True)
        lines.append(line)

    emit("A deferred profile's data-maximum pass: the kernel, the host pass it replaces, and the call (tools/levels_probe.py)")
    emit()
    ctx = HipContext(0)
    kernels(torch, ctx, emit, sizes, args.rounds, args.repeats)
    ctx.close()
    emit()
    host_pass(emit, sizes, max(3, args.repeats // 4))
    emit()
    calls(torch, emit, sizes, max(2, args.rounds // 2), max(3, args.repeats // 4))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
