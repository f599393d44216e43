"""What the X-Trans demosaic kernels cost on the device, beside the Bayer kernel and a copy of their bytes
(profiles/r22_xtrans_probe.txt).

    python tools/xtrans_probe.py [--out FILE] [--rounds R] [--iters N]

For a 24 MP and a 100 MP sensor, in this process (device events, median of round medians, the legs taking turns round by round):
  r2f_demosaic_xtrans_u16   full size and reduced (third) size
  r2f_demosaic_u16          the Bayer kernel, full size and half size, on a mosaic of the same size: the yardstick -- the full-size
                            kernels do comparable LDS work per pixel
  r2f_stream_copy           over the X-Trans kernel's byte count (8 B per mosaic sample at full size: 2 read, 6 written; 2 + 6 / 9 B
                            per sample at reduced size): its floor
Both mosaics are noise of the same range: the kernels' times do not depend on the picture.  Needs a GPU: there is no CPU path.
"""

from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = (("24 MP", 4000, 6000), ("100 MP", 8192, 12288))
MATRIX = ((0.52, 0.27, 0.15), (0.25, 0.68, 0.07), (0.03, 0.12, 0.81))


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
    from raw2film_amd.raw import RawProfile, XTransProfile

    ctx = HipContext(0)
    xtrans = XTransProfile(black=512, multipliers=(7.9, 4.1, 6.2), matrix=MATRIX)
    bayer = RawProfile("RGGB", black=512, multipliers=(7.9, 4.1, 6.2), matrix=MATRIX)
    emit(f"kernels ({torch.cuda.get_device_name(0)}): device events, {iters} launches per round median, {rounds} interleaved rounds")
    for label, H, W in SIZES:
        mosaic = torch.randint(0, 16384, (H, W), dtype=torch.int16, device="cuda")
        for reduced in (False, True):
            xp, bp = xtrans.plan(H, W, reduced), bayer.plan(H, W, reduced)
            xout = torch.empty((xp.out_h, xp.out_w, 3), dtype=torch.int16, device="cuda")
            bout = torch.empty((bp.out_h, bp.out_w, 3), dtype=torch.int16, device="cuda")
            nbytes = mosaic.numel() * 2 + xout.numel() * 2  # algorithmic: every sample read once, every output written once
            a = torch.empty(nbytes // 2 // 16 * 16, dtype=torch.uint8, device="cuda")  # the copy moves the same bytes: half read, half written
            b = torch.empty_like(a)
            legs = {"x": lambda: ctx.demosaic_xtrans(mosaic, xp, out=xout), "b": lambda: ctx.demosaic_u16(mosaic, bp, out=bout),
                    "c": lambda: ctx.stream_copy(a, b)}
            for _ in range(3):
                for fn in legs.values():
                    fn()
            t = {k: [] for k in legs}
            for _ in range(rounds):
                for k, fn in legs.items():
                    t[k].append(timed(torch, fn, iters))
            xm_, bm, cm = (float(np.median(t[k])) for k in "xbc")
            form = "reduced (third) size" if reduced else "full size"
            emit(f"  {label} sensor, {form}: r2f_demosaic_xtrans_u16 {xm_:.3f} ms (range {min(t['x']):.3f} .. {max(t['x']):.3f}) = "
                 f"{nbytes / xm_ / 1e6:.0f} GB/s of {nbytes / H / W:.2f} B per sample")
            emit(f"      r2f_demosaic_u16 (Bayer, {'half' if reduced else 'full'} size) {bm:.3f} ms (range {min(t['b']):.3f} .. {max(t['b']):.3f}); "
                 f"X-Trans / Bayer = {xm_ / bm:.2f}")
            emit(f"      r2f_stream_copy of {2 * a.numel() / 1e6:.0f} MB {cm:.3f} ms (range {min(t['c']):.3f} .. {max(t['c']):.3f}) = "
                 f"{2 * a.numel() / cm / 1e6:.0f} GB/s; X-Trans / copy = {xm_ / cm:.2f}")
            del xout, bout, a, b
        del mosaic
        torch.cuda.empty_cache()
    ctx.close()
    emit()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_xtrans_probe.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("xtrans_probe needs a GPU")
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    emit("The X-Trans demosaic kernels beside the Bayer kernel and a copy of their bytes (tools/xtrans_probe.py)")
    emit()
    kernels(args.rounds, args.iters, emit)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
