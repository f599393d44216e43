"""What the hot-pixel repair of a mosaic (raw2film_amd.raw.HotPixels, r2f_mosaic_repair) costs: the kernel beside r2f_mosaic_maximum
and a device copy of the same 4 bytes per sample, and the call with and without the keyword (profiles/r30_repair_probe.txt).

    python tools/repair_probe.py [--out FILE] [--repeats N] [--rounds R] [--sizes 24,100]

All in this process, the legs of each part taking turns; 24 MP (4000 x 6000) and 100 MP (8192 x 12288) mosaics.
  (a) kernels, device events, median of N launches per round: r2f_mosaic_repair with a Bayer and with an X-Trans table on a SPARSE
      field (noise of a quarter of a sensor's range with 2 samples in 10 000 stuck near the white level: what the step is for) and on
      a DENSE one (the tests' recipe: a tenth of the samples are candidates that fetch their neighbours), beside r2f_mosaic_maximum
      (2 B per sample read) and a device-to-device copy of the mosaic (2 B read + 2 B written per sample: the repair's floor).  A
      510-row strip of every result is checked against the NumPy model first.
  (b) calls, wall clock around the call with a device synchronisation on either side: process(mosaic, cache=False, exposure=stops)
      of the sparse field with and without raw_repair, in one piece (stream_bands = 0) and streamed in row bands (16), from pageable
      and from pinned memory.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = {"24": ("24 MP", 4000, 6000), "100": ("100 MP", 8192, 12288)}
STOPS = 0.5
BLACK, WHITE = 512, 16383
MATRIX = ((0.52, 0.27, 0.15), (0.25, 0.68, 0.07), (0.03, 0.12, 0.81))
THRESHOLD, RATIO = 6000, 0.125
XTRANS = ("GBGGRG", "RGRBGB", "GBGGRG", "GRGGBG", "BGBRGR", "GRGGBG")


def spread(xs):
    return f"{min(xs):8.3f} .. {max(xs):8.3f} ms (median {statistics.median(xs):8.3f}, n = {len(xs)})"


def sparse(H, W):
    rng = np.random.default_rng(H)
    frame = rng.integers(BLACK, BLACK + 1200, (H, W), dtype=np.uint16)  # (all neighbours below an eighth of a stuck sample)
    n = H * W // 5000
    frame[rng.integers(0, H, n), rng.integers(0, W, n)] = rng.integers(WHITE - 400, WHITE + 1, n, dtype=np.uint16)
    return frame


def dense(H, W):
    rng = np.random.default_rng(H + 1)
    frame = rng.integers(500, 900, (H, W), dtype=np.uint16)
    hot = rng.random((H, W), dtype=np.float32) < 0.1
    frame[hot] = rng.integers(5000, 65536, int(hot.sum()), dtype=np.uint16)
    return frame


def device_ms(torch, fn, repeats, stall):
    """Median device time of `repeats` launches of fn, each between its own pair of events, all queued behind a few milliseconds of
    other work so that a short kernel is timed from the end of the launch before it."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(repeats)]
    stall()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def kernels(torch, ctx, emit, sizes, rounds, repeats):
    import repair_model as model
    from raw2film_amd.raw import HotPixels, RawProfile, XTransProfile

    emit(f"(a) kernels ({torch.cuda.get_device_name(0)}): device events, median of {repeats} launches per round, {rounds} rounds in turn, "
         "every batch of launches queued behind ~2 ms of copies")
    big = torch.zeros(1 << 28, dtype=torch.int32, device="cuda"), torch.empty(1 << 28, dtype=torch.int32, device="cuda")

    def stall():
        for _ in range(4):
            big[1].copy_(big[0])

    profiles = {"Bayer": RawProfile("RGGB", black=(BLACK, BLACK + 3, BLACK + 6, BLACK + 9)),
                "X-Trans": XTransProfile(XTRANS, black=tuple(BLACK + i for i in range(36)))}
    for label, H, W in sizes:
        emit(f"  {label} ({H} x {W}, {2.0 * H * W / 1e6:.0f} MB)")
        for field_name, make, record in (("sparse", sparse, HotPixels(THRESHOLD, RATIO, 4)), ("dense", dense, HotPixels(1000, RATIO, 4))):
            host = make(H, W)
            dev = torch.from_numpy(host.view(np.int16)).cuda()
            other = torch.empty_like(dev)
            word = torch.zeros(1, dtype=torch.int32, device="cuda")
            count = torch.zeros(1, dtype=torch.int32, device="cuda")
            plans = {name: record.plan(p, H, W) for name, p in profiles.items()}
            legs = {f"r2f_mosaic_repair, {name} table": (lambda p=p: ctx.mosaic_repair(dev, p, count=count, out=other)) for name, p in plans.items()}
            legs["r2f_mosaic_maximum, Bayer table"] = lambda: ctx.mosaic_maximum(dev, profiles["Bayer"], out=word)
            legs["device-to-device copy"] = lambda: other.copy_(dev)
            shares = {}
            for name, p in plans.items():  # the results first: the timing is of a kernel that computes the model's bytes (a strip of them)
                count.zero_()
                out = ctx.mosaic_repair(dev, p, count=count, out=other)
                P = 2 if name == "Bayer" else 6
                cfa = None if P == 2 else model.cfa_ids(XTRANS)
                top = H // 2 // 6 * 6  # (a multiple of both periods: the phases of the rows below it are the frame's)
                want, hot = model.repair(host[top:top + 522], P, profiles[name].black, record.threshold, record.q, 4, cfa)
                got = out[top + 6:top + 516].cpu().numpy().view(np.uint16)  # (6 rows in from the cut: the model takes it for the frame's edge)
                if not np.array_equal(got, want[6:516]) or not hot[6:516].any():
                    raise RuntimeError(f"{label}, {field_name}, {name}: the device's strip is not the model's")
                shares[name] = int(count.item()) / (H * W)
            for fn in legs.values():
                fn()
            torch.cuda.synchronize()
            times = {name: [] for name in legs}
            for _ in range(rounds):
                for name, fn in legs.items():
                    times[name].append(device_ms(torch, fn, repeats, stall))
            nbytes = 2.0 * H * W
            copy = statistics.median(times["device-to-device copy"])
            emit(f"    {field_name} field: repaired {', '.join(f'{100 * s:.3f} % ({n})' for n, s in shares.items())}")
            for name, xs in times.items():
                med = statistics.median(xs)
                moved = nbytes if "maximum" in name else 2 * nbytes
                ratio = f", {med / copy:4.2f} x the copy" if "repair" in name else ""
                emit(f"      {name:<36s} {med:7.3f} ms (range {min(xs):.3f} .. {max(xs):.3f}), {moved / med / 1e9:6.2f} TB/s{ratio}")
            del dev, other


def calls(torch, emit, sizes, rounds, repeats):
    from raw2film_amd import HipProcessor, filmstock
    from raw2film_amd.raw import HotPixels, RawProfile

    stocks = filmstock.builtin_stocks()
    neg, prt = stocks["Kodak Portra 400"], stocks["Kodak 2383"]
    proc = HipProcessor(device=0, result_buffers=2)
    emit(f"(b) calls: process(mosaic, exposure={STOPS}, cache=False, half_size=False), full render, result_buffers=2; the legs take turns call "
         f"by call, {rounds} rounds of {repeats} calls after a warm-up; wall clock with a device synchronisation on either side")
    record = HotPixels(THRESHOLD, RATIO, 4)
    for label, H, W in sizes:
        pageable = sparse(H, W)
        pinned = torch.from_numpy(pageable.view(np.int16)).pin_memory().numpy().view(np.uint16)
        mul = tuple(w * 65535.0 / (WHITE - BLACK) for w in (1.9, 1.0, 1.5))
        profile = RawProfile("RGGB", black=BLACK, multipliers=mul, matrix=MATRIX)
        fw = max(36.0, W / 341.0)
        kw = dict(print_film=prt, lens_correction=False, seed=5, cache=False, frame_width=fw, frame_height=fw * H / W, halation_green_factor=0.3,
                  exposure=STOPS, half_size=False, raw_profile=profile)
        legs = (("one piece", 0, None), ("one piece, raw_repair", 0, record), ("streamed", 16, None), ("streamed, raw_repair", 16, record))
        times = {(name, memory): [] for name, _, _ in legs for memory in ("pageable", "pinned")}
        kept, rejected = {}, {}
        for rnd in range(rounds):
            for r in range(repeats + (0 if rnd else 1)):
                for memory, frame in (("pageable", pageable), ("pinned", pinned)):
                    for name, bands, repair in legs:
                        proc.stream_bands = bands
                        proc.stream_rejected = "unset"
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        res = proc.process(frame, neg, 6, 0.4, raw_repair=repair, **kw)
                        torch.cuda.synchronize()
                        dt = (time.perf_counter() - t0) * 1e3
                        if rnd or r:
                            times[(name, memory)].append(dt)
                        elif memory == "pageable":
                            kept[name] = (res.copy(), None if repair is None else proc.last_raw_repair["repaired"])
                            rejected[name] = proc.stream_rejected
                        del res
        one, streamed = kept["one piece, raw_repair"], kept["streamed, raw_repair"]
        same = np.array_equal(one[0], streamed[0])
        emit(f"  {label} ({H} x {W}); repaired {one[1]} one piece, {streamed[1]} streamed; the two results "
             f"{'agree byte for byte' if same else 'differ in ' + str(int((one[0] != streamed[0]).sum())) + ' bytes (the FFT stencils anchor at a band)'}; "
             f"with and without differ: {not np.array_equal(one[0], kept['one piece'][0])}; stream_rejected of the streamed legs: "
             f"{rejected['streamed']!r}, {rejected['streamed, raw_repair']!r}")
        for memory in ("pageable", "pinned"):
            emit(f"    {memory}")
            for name, _, _ in legs:
                emit(f"      {name:<26s} {spread(times[(name, memory)])}")
            med = {name: statistics.median(times[(name, memory)]) for name, _, _ in legs}
            emit(f"      the keyword: {med['one piece, raw_repair'] - med['one piece']:+.2f} ms in one piece, "
                 f"{med['streamed, raw_repair'] - med['streamed']:+.2f} ms streamed")
        del pageable, pinned
    proc.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_repair_probe.txt"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="24,100")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("tools/repair_probe.py needs a GPU: there is no CPU path")
    from raw2film_amd.context import HipContext

    sizes = [SIZES[s] for s in args.sizes.split(",")]
    lines = []

    def emit(line=""):
        print(line, flush=True)
        lines.append(line)

    emit("The hot-pixel repair of a mosaic: the kernel beside the data maximum and a copy, and the call (tools/repair_probe.py)")
    emit()
    ctx = HipContext(0)
    kernels(torch, ctx, emit, sizes, args.rounds, args.repeats)
    ctx.close()
    emit()
    calls(torch, emit, sizes, max(2, args.rounds // 2), max(3, args.repeats // 4))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
