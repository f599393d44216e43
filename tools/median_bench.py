"""Device time of the three median entry points (step M, LibRaw's med_passes) beside their plain siblings at 24 MP and 100 MP, full
and reduced size, n = 1 and n = 4, in the manner of tools/highlight_bench.py: event-timed launches, three untimed launches first,
the median of --iters per round, every kernel taking its turn in every round of one process.  The copy ceiling of the same run
stands beside them: a device-to-device copy of the bytes a plain call moves (the mosaic read once, the frame written once).
Behind the kernels, process(mosaic) with and without median_passes, in one piece and streamed in row bands (the shape of
tools/demosaic_probe.py --stream, profiles/r17_mosaic_stream_probe.txt: pinned mosaic, full render, the legs taking turns).
--lib names further builds of the library (the parent commit's, say): their plain entry points take turns with this tree's in the
same rounds, as tools/ab_libs.py does for the render.

    python tools/median_bench.py [--rounds 6] [--iters 10] [--lib parent.so] [--out profiles/r29_median_probe.txt]

The yardstick is the plain entry point in the same run, not an absolute time.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from raw2film_amd import _lib  # noqa: E402
from raw2film_amd.context import HipContext  # noqa: E402
from raw2film_amd.raw import RawProfile, XTransProfile  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--out", default=None, help="also write the report to this file")
ap.add_argument("--lib", action="append", default=[], help="another build whose plain entry points join the rounds")
ap.add_argument("--repeats", type=int, default=5, help="calls per round of the process() legs")
args = ap.parse_args()
SHAPES = {"24 MP": (4002, 6000), "100 MP": (8190, 12288)}  # (sides that 2 and 3 divide: both reduced forms take the whole mosaic)
PASSES = (1, 4)
MATRIX = ((1.62, -0.41, -0.19), (-0.28, 1.52, -0.22), (0.04, -0.52, 1.49))
MUL = (1.0, 1.0 / 2.1, 1.6 / 2.1)
FACTOR = float(np.float32(2.0 ** 0.5))
ctx = HipContext(0)
# (another build need not export the entry points this tree adds: it is bound without them)
new = {k: _lib._SIGNATURES.pop(k) for k in ("r2f_demosaic_median_u16", "r2f_demosaic_median_f32", "r2f_demosaic_xtrans_median_u16")}
try:
    others = {os.path.basename(os.path.dirname(os.path.abspath(path))) + "/" + os.path.basename(path): HipContext(0, lib_path=path) for path in args.lib}
finally:
    _lib._SIGNATURES.update(new)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(iters):
        start.record()
        fn()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
    return float(np.median(times))


def frame(H, W):
    """A smooth field with sensor-like noise (a 512 x 512 cell, repeated): the medians have something to sort."""
    rng = np.random.default_rng(29)
    y, x = np.mgrid[0:512, 0:512]
    cell = (6000 + 20000 * (0.5 + 0.25 * np.sin(y / 40.0) + 0.25 * np.cos(x / 60.0)) + rng.integers(-600, 600, (512, 512))).astype(np.uint16)
    return np.tile(cell, (-(-H // 512), -(-W // 512)))[:H, :W]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


say(f"# tools/median_bench.py --rounds {args.rounds} --iters {args.iters}: ms per call, the median over the rounds of each round's median "
    "(range over the rounds)")
for label, (H, W) in SHAPES.items():
    m = dev(frame(H, W))
    for reduced in (False, True):
        bayer = RawProfile("RGGB", multipliers=MUL, matrix=MATRIX).plan(H, W, reduced)
        xtrans = XTransProfile(multipliers=MUL, matrix=MATRIX).plan(H, W, reduced)
        legs = {}
        for name, params, plain, median, f32 in (
                ("r2f_demosaic_u16", bayer, ctx.demosaic_u16, ctx.demosaic_median_u16, False),
                ("r2f_demosaic_f32", bayer, lambda m_, p_, out: ctx.demosaic_f32(m_, p_, FACTOR, out=out),
                 lambda m_, p_, n, out: ctx.demosaic_median_f32(m_, p_, n, FACTOR, out=out), True),
                ("r2f_demosaic_xtrans_u16", xtrans, ctx.demosaic_xtrans, ctx.demosaic_xtrans_median, False)):
            oh, ow = int(params.out_h), int(params.out_w)
            out = torch.empty((oh, ow, 3), dtype=torch.float32 if f32 else torch.int16, device="cuda")
            # the copy ceiling: the bytes a plain call moves, as one device-to-device copy (each byte read once and written once)
            moved = (H * W * 2 + out.numel() * out.element_size()) // 2
            a, b = torch.empty(moved, dtype=torch.uint8, device="cuda"), torch.empty(moved, dtype=torch.uint8, device="cuda")
            legs[name] = {"copy": (lambda a=a, b=b: b.copy_(a)), "plain": (lambda plain=plain, params=params, out=out: plain(m, params, out=out))}
            for n in PASSES:
                legs[name][f"n = {n}"] = (lambda median=median, params=params, n=n, out=out: median(m, params, n, out=out))
            for tag, other in others.items():  # the same plain entry point of another build
                method = {"r2f_demosaic_u16": other.demosaic_u16, "r2f_demosaic_xtrans_u16": other.demosaic_xtrans,
                          "r2f_demosaic_f32": lambda m_, p_, out, other=other: other.demosaic_f32(m_, p_, FACTOR, out=out)}[name]
                legs[name][f"plain of {tag}"] = (lambda method=method, params=params, out=out: method(m, params, out=out))
        for fns in legs.values():
            for fn in fns.values():
                for _ in range(3):
                    fn()
        rounds = {(name, leg): [] for name, fns in legs.items() for leg in fns}
        for r in range(args.rounds):
            for name, fns in legs.items():  # interleaved: every leg takes its turn in every round, in reverse order in every other one
                for leg, fn in (list(fns.items()) if r % 2 == 0 else list(fns.items())[::-1]):
                    rounds[(name, leg)].append(timed(fn, args.iters))
        say(f"{label} ({H} x {W}), {'reduced' if reduced else 'full'} size")
        for name, fns in legs.items():
            med = {leg: float(np.median(rounds[(name, leg)])) for leg in fns}
            say(f"  {name}: " + ", ".join(f"{leg} {med[leg]:.3f} ({min(rounds[(name, leg)]):.3f} .. {max(rounds[(name, leg)]):.3f})" for leg in fns)
                + " | x plain: " + ", ".join(f"{leg} {med[leg] / med['plain']:.2f}" for leg in fns if leg.startswith("n"))
                + f" | plain / copy {med['plain'] / med['copy']:.2f}"
                + "".join(f" | plain / {leg} {med['plain'] / med[leg]:.3f}" for leg in fns if leg.startswith("plain of")))
        del legs
        torch.cuda.empty_cache()
    del m
    torch.cuda.empty_cache()

# ---- process(mosaic): with and without median_passes, in one piece and streamed
from raw2film_amd import HipProcessor, filmstock  # noqa: E402

stocks = filmstock.builtin_stocks()
neg, prt = stocks["Kodak Portra 400"], stocks["Kodak 2383"]
proc = HipProcessor(device=0, result_buffers=2)
say("")
say(f"process(pinned mosaic, exposure=0.5, cache=False, half_size=False), full render (halation, MTF, grain, print film), "
    f"result_buffers=2: ms per call, wall clock with a device synchronisation on either side; the legs take turns call by call, "
    f"{args.rounds} rounds of {args.repeats} calls after a warm-up")
for label, (H, W) in (("24 MP", (4000, 6000)), ("100 MP", (8192, 12288))):
    rng = np.random.default_rng(H)
    mosaic = torch.from_numpy(rng.integers(0, 16384, (H, W), dtype=np.uint16).view(np.int16)).pin_memory().numpy().view(np.uint16)
    fw = max(36.0, W / 341.0)
    kw = dict(print_film=prt, lens_correction=False, seed=5, cache=False, frame_width=fw, frame_height=fw * H / W, halation_green_factor=0.3,
              exposure=0.5, half_size=False)
    profiles = {n: RawProfile("RGGB", black=512, multipliers=(7.9, 4.1, 6.2), matrix=((0.52, 0.27, 0.15), (0.25, 0.68, 0.07), (0.03, 0.12, 0.81)),
                              median_passes=n) for n in (0,) + PASSES}
    times = {}
    for _ in range(args.rounds):
        for r in range(args.repeats + 1):
            for n, prof in profiles.items():
                for bands in (16, 0):
                    proc.stream_bands, proc.stream_rejected = bands, "not asked"
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res = proc.process(mosaic, neg, 6, 0.4, raw_profile=prof, **kw)
                    torch.cuda.synchronize()
                    dt = (time.perf_counter() - t0) * 1e3
                    assert res.shape == (H, W, 3) and (proc.stream_rejected is None) == (bands > 1), proc.stream_rejected
                    del res
                    if r:
                        times.setdefault((n, bands), []).append(dt)
    proc.stream_bands = 16
    say(f"  {label} ({H} x {W})")
    for bands in (16, 0):
        base = statistics.median(times[(0, bands)])
        for n in profiles:
            t = times[(n, bands)]
            say(f"    stream_bands = {bands:<2d} median_passes = {n}: {min(t):8.2f} .. {max(t):8.2f} (median {statistics.median(t):8.2f}, n = {len(t)})"
                + (f" = {statistics.median(t) / base:.3f} x median_passes = 0" if n else ""))
    del mosaic
proc.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
