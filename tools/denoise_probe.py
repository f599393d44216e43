"""What the wavelet denoise of a Bayer mosaic (raw_denoise, r2f_mosaic_denoise) costs (profiles/r28_denoise_probe.txt).

    python tools/denoise_probe.py [--out FILE] [--repeats N] [--rounds R] [--sizes 24,100]

All in this process, the legs of each part taking turns; 24 MP (4000 x 6000) and 100 MP (8192 x 12288) mosaics of sensor-like noise on
a ramp.
  (1) each level's launch (r2f_mosaic_denoise_level) beside a device-to-device copy that moves the bytes that launch reads and writes
      (a copy of b / 2 bytes reads b / 2 and writes b / 2), device events, and the ratio.  Per mosaic sample a level moves: level 0
      2 B in (uint16) + 8 B out (D, L); levels 1 .. 3 8 B in (L, D) + 8 B out; level 4 8 B in + 2 B out -- apron re-reads not counted.
  (2) the five launches together (r2f_mosaic_denoise) beside r2f_demosaic_u16, full size, of the same mosaic.
  (3) process(mosaic, cache=False) with and without raw_denoise, pinned and pageable source, wall clock with a device
      synchronisation on either side.
The chain's result is checked against the NumPy model (tests/denoise_model.py) on a 256 x 384 crop-sized frame first.
Needs a GPU: there is no CPU path.
"""

from __future__ import annotations

import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SIZES = {"24": ("24 MP", 4000, 6000), "100": ("100 MP", 8192, 12288)}
BLACK = (512, 515, 509, 512)
MAXIMUM = 16383 - 509
THRESHOLD = 200.0
MATRIX = ((0.52, 0.27, 0.15), (0.25, 0.68, 0.07), (0.03, 0.12, 0.81))
LEVEL_BYTES = (10, 16, 16, 16, 10)  # per mosaic sample, read + written


def frame(H, W):
    rng = np.random.default_rng(H)
    ramp = 600 + 9000 * (np.arange(W, dtype=np.float32) / W)[None, :] * (0.5 + 0.5 * (np.arange(H, dtype=np.float32) / H))[:, None]
    return np.clip(ramp + rng.normal(0, 160, (H, W)).astype(np.float32), 0, 16383).astype(np.uint16)


def device_ms(torch, fn, repeats, stall):
    """Median device time of `repeats` launches of fn, each between its own pair of events, queued behind a few milliseconds of
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
    import denoise_model as model
    from raw2film_amd.raw import RawProfile, WaveletDenoise

    dn = WaveletDenoise(THRESHOLD, MAXIMUM)
    small = frame(256, 384)
    got = ctx.mosaic_denoise(torch.from_numpy(small.view(np.int16)).cuda(), dn.plan(BLACK, 256, 384)).cpu().numpy().view(np.uint16)
    if not np.array_equal(got, model.denoise(small, BLACK, MAXIMUM, THRESHOLD)):
        raise RuntimeError("the device's bytes are not the model's")
    emit(f"(1), (2) kernels ({torch.cuda.get_device_name(0)}): device events, median of {repeats} launches per round, {rounds} rounds in "
         "turn, every batch of launches queued behind ~2 ms of copies; the chain's bytes equal the model's on a 256 x 384 frame")
    big = torch.zeros(1 << 28, dtype=torch.int32, device="cuda"), torch.empty(1 << 28, dtype=torch.int32, device="cuda")

    def stall():
        for _ in range(4):
            big[1].copy_(big[0])

    profile = RawProfile("RGGB", black=BLACK, multipliers=(8.0, 4.1, 6.2), matrix=MATRIX)
    for label, H, W in sizes:
        dev = torch.from_numpy(frame(H, W).view(np.int16)).cuda()
        out = torch.empty_like(dev)
        params = dn.plan(BLACK, H, W)
        need = int(ctx._lib.r2f_mosaic_denoise_workspace_bytes(H, W))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        rgb = torch.empty((H, W, 3), dtype=torch.int16, device="cuda")
        dparams = profile.plan(H, W, False)
        copies = {b: (torch.empty(b * H * W // 2, dtype=torch.uint8, device="cuda"), torch.empty(b * H * W // 2, dtype=torch.uint8, device="cuda"))
                  for b in set(LEVEL_BYTES)}

        def level(lev):
            def run():
                rc = ctx._lib.r2f_mosaic_denoise_level(ctx._h, lev, dev.data_ptr(), W, H, W, C.byref(params), out.data_ptr(), W, ws.data_ptr(),
                                                       need, ctx._stream())
                assert rc == 0, ctx._lib.r2f_last_error(ctx._h)
            return run

        legs = {}
        for lev, b in enumerate(LEVEL_BYTES):
            legs[f"level {lev} (c = {1 << lev:2d})"] = level(lev)
            legs[f"copy of level {lev}'s {b} B/sample"] = (lambda pair: lambda: pair[1].copy_(pair[0]))(copies[b])
        legs["r2f_mosaic_denoise (five launches)"] = lambda: ctx.mosaic_denoise(dev, params, out=out)
        legs["r2f_demosaic_u16, full size"] = lambda: ctx.demosaic_u16(dev, dparams, out=rgb)
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in legs}
        for _ in range(rounds):
            for name, fn in legs.items():
                times[name].append(device_ms(torch, fn, repeats, stall))
        emit(f"  {label} ({H} x {W}, {2.0 * H * W / 1e6:.0f} MB of mosaic, {need / 1e6:.0f} MB of workspace)")
        med = {name: statistics.median(xs) for name, xs in times.items()}
        names = list(legs)
        for lev, b in enumerate(LEVEL_BYTES):
            k, c = names[2 * lev], names[2 * lev + 1]
            emit(f"      {k:<22s} {med[k]:7.3f} ms (range {min(times[k]):.3f} .. {max(times[k]):.3f}), {b * H * W / med[k] / 1e9:5.2f} TB/s of its "
                 f"{b} B/sample; copy of the same bytes {med[c]:7.3f} ms ({b * H * W / med[c] / 1e9:5.2f} TB/s); ratio {med[k] / med[c]:4.2f}")
        chain, dem = med[names[-2]], med[names[-1]]
        emit(f"      {names[-2]:<36s} {chain:7.3f} ms (range {min(times[names[-2]]):.3f} .. {max(times[names[-2]]):.3f}); sum of the levels "
             f"{sum(med[names[2 * lev]] for lev in range(5)):7.3f} ms; {68 * H * W / chain / 1e9:5.2f} TB/s of 68 B/sample")
        emit(f"      {names[-1]:<36s} {dem:7.3f} ms (range {min(times[names[-1]]):.3f} .. {max(times[names[-1]]):.3f}); the denoise takes "
             f"{chain / dem:4.2f} x the demosaic")
        del dev, out, ws, rgb, copies


def calls(torch, emit, sizes, rounds, repeats):
    from raw2film_amd import HipProcessor, filmstock
    from raw2film_amd.raw import RawProfile, WaveletDenoise

    stocks = filmstock.builtin_stocks()
    neg, prt = stocks["Kodak Portra 400"], stocks["Kodak 2383"]
    proc = HipProcessor(device=0, result_buffers=2)
    proc.stream_bands = 0  # (a denoised mosaic takes the one-piece path: both legs take it)
    emit(f"(3) calls: process(mosaic, exposure=0.5, cache=False, half_size=False), full render, one piece, result_buffers=2; the legs take "
         f"turns call by call, {rounds} rounds of {repeats} calls after a warm-up; wall clock with a device synchronisation on either side")
    profile = RawProfile("RGGB", black=BLACK, multipliers=(8.0, 4.1, 6.2), matrix=MATRIX)
    dn = WaveletDenoise(THRESHOLD, MAXIMUM)
    for label, H, W in sizes:
        pageable = frame(H, W)
        pinned = torch.from_numpy(pageable.view(np.int16)).pin_memory().numpy().view(np.uint16)
        fw = max(36.0, W / 341.0)
        kw = dict(print_film=prt, lens_correction=False, seed=5, cache=False, frame_width=fw, frame_height=fw * H / W, halation_green_factor=0.3,
                  exposure=0.5, half_size=False, raw_profile=profile)
        legs = (("without raw_denoise", {}), ("with raw_denoise", {"raw_denoise": dn}))
        times = {(name, memory): [] for name, _ in legs for memory in ("pageable", "pinned")}
        for rnd in range(rounds):
            for r in range(repeats + (0 if rnd else 1)):
                for memory, src in (("pageable", pageable), ("pinned", pinned)):
                    for name, extra in legs:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        res = proc.process(src, neg, 6, 0.4, **kw, **extra)
                        torch.cuda.synchronize()
                        if rnd or r:
                            times[(name, memory)].append((time.perf_counter() - t0) * 1e3)
                        del res
        emit(f"  {label} ({H} x {W})")
        for memory in ("pageable", "pinned"):
            med = {name: statistics.median(times[(name, memory)]) for name, _ in legs}
            for name, _ in legs:
                xs = times[(name, memory)]
                emit(f"      {memory:<9s}{name:<22s} {min(xs):8.3f} .. {max(xs):8.3f} ms (median {med[name]:8.3f}, n = {len(xs)})")
            emit(f"      {memory:<9s}the denoise adds {med[legs[1][0]] - med[legs[0][0]]:+.2f} ms")
        del pageable, pinned
    proc.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_denoise_probe.txt"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="24,100")
    ap.add_argument("--no-calls", action="store_true", help="parts (1) and (2) only")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("tools/denoise_probe.py needs a GPU: there is no CPU path")
    from raw2film_amd.context import HipContext

    sizes = [SIZES[s] for s in args.sizes.split(",")]
    lines = []

    def emit(line=""):
        print(line, flush=True)
        lines.append(line)

    emit("The wavelet denoise of a Bayer mosaic: each level beside its copy, the chain beside the demosaic, the call (tools/denoise_probe.py)")
    emit()
    ctx = HipContext(0)
    kernels(torch, ctx, emit, sizes, args.rounds, args.repeats)
    ctx.close()
    if not args.no_calls:
        emit()
        calls(torch, emit, sizes, max(2, args.rounds // 2), max(3, args.repeats // 4))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
