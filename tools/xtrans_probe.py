"""What the X-Trans demosaic kernels cost on the device, beside the Bayer kernel and a copy of their bytes
(profiles/r22_xtrans_probe.txt).

    python tools/xtrans_probe.py [--out FILE] [--rounds R] [--iters N] [--lib PATH ...]

For a 24 MP and a 100 MP sensor, in this process (device events, median of round medians, the legs taking turns round by round):
  r2f_demosaic_xtrans_u16   full size and reduced (third) size
  r2f_demosaic_u16          the Bayer kernel, full size and half size, on a mosaic of the same size: the yardstick -- the full-size
                            kernels do comparable LDS work per pixel
  r2f_stream_copy           over the X-Trans kernel's byte count (8 B per mosaic sample at full size: 2 read, 6 written; 2 + 6 / 9 B
                            per sample at reduced size): its floor
Each --lib PATH is another build of the library (say the parent commit's, built with build(out=PATH)) bound beside the in-tree one:
its r2f_demosaic_xtrans_u16, r2f_demosaic_u16 and r2f_demosaic_f32 legs take turns with the in-tree build's, after every leg's output
has been asserted equal to the in-tree build's on the same mosaic; the in-tree median is then held against that build's own range
over the rounds.
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


def kernels(rounds, iters, emit, libs=()):
    import torch

    from raw2film_amd.context import HipContext
    from raw2film_amd.raw import RawProfile, XTransProfile

    # build 0 is the in-tree library; every --lib is one more build whose legs take turns with its own
    ctxs = [HipContext(0)] + [HipContext(0, lib_path=path) for path in libs]
    ctx = ctxs[0]
    xtrans = XTransProfile(black=512, multipliers=(7.9, 4.1, 6.2), matrix=MATRIX)
    bayer = RawProfile("RGGB", black=512, multipliers=(7.9, 4.1, 6.2), matrix=MATRIX)
    factor = 2 ** 0.37
    emit(f"kernels ({torch.cuda.get_device_name(0)}): device events, {iters} launches per round median, {rounds} interleaved rounds")
    for i, path in enumerate(libs):
        emit(f"  build {i + 1}: {path} ({ctxs[i + 1]._lib.r2f_version().decode()}); build 0: the in-tree library")
    for label, H, W in SIZES:
        mosaic = torch.randint(0, 16384, (H, W), dtype=torch.int16, device="cuda")
        for reduced in (False, True):
            xp, bp = xtrans.plan(H, W, reduced), bayer.plan(H, W, reduced)
            outs = [{"x": torch.empty((xp.out_h, xp.out_w, 3), dtype=torch.int16, device="cuda"),
                     "b": torch.empty((bp.out_h, bp.out_w, 3), dtype=torch.int16, device="cuda"),
                     "f": torch.empty((bp.out_h, bp.out_w, 3), dtype=torch.float32, device="cuda")} for _ in ctxs]
            nbytes = mosaic.numel() * 2 + outs[0]["x"].numel() * 2  # algorithmic: every sample read once, every output written once
            a = torch.empty(nbytes // 2 // 16 * 16, dtype=torch.uint8, device="cuda")  # the copy moves the same bytes: half read, half written
            b = torch.empty_like(a)
            legs = {"c": lambda: ctx.stream_copy(a, b)}
            for i, (c, o) in enumerate(zip(ctxs, outs)):
                legs[f"x{i}"] = lambda c=c, o=o: c.demosaic_xtrans(mosaic, xp, out=o["x"])
                legs[f"b{i}"] = lambda c=c, o=o: c.demosaic_u16(mosaic, bp, out=o["b"])
                legs[f"f{i}"] = lambda c=c, o=o: c.demosaic_f32(mosaic, bp, factor, out=o["f"])
            for _ in range(3):
                for fn in legs.values():
                    fn()
            torch.cuda.synchronize()
            for o in outs[1:]:  # before any timing: every build computes the in-tree build's bytes
                for k in "xbf":
                    assert torch.equal(o[k].view(torch.int16), outs[0][k].view(torch.int16)), f"{label} {k} reduced={reduced}: the builds differ"
            t = {k: [] for k in legs}
            for _ in range(rounds):
                for k, fn in legs.items():
                    t[k].append(timed(torch, fn, iters))
            xm_, bm, cm = (float(np.median(t[k])) for k in ("x0", "b0", "c"))
            form = "reduced (third) size" if reduced else "full size"
            emit(f"  {label} sensor, {form}: r2f_demosaic_xtrans_u16 {xm_:.3f} ms (range {min(t['x0']):.3f} .. {max(t['x0']):.3f}) = "
                 f"{nbytes / xm_ / 1e6:.0f} GB/s of {nbytes / H / W:.2f} B per sample")
            emit(f"      r2f_demosaic_u16 (Bayer, {'half' if reduced else 'full'} size) {bm:.3f} ms (range {min(t['b0']):.3f} .. {max(t['b0']):.3f}); "
                 f"X-Trans / Bayer = {xm_ / bm:.2f}")
            emit(f"      r2f_stream_copy of {2 * a.numel() / 1e6:.0f} MB {cm:.3f} ms (range {min(t['c']):.3f} .. {max(t['c']):.3f}) = "
                 f"{2 * a.numel() / cm / 1e6:.0f} GB/s; X-Trans / copy = {xm_ / cm:.2f}")
            emit(f"      r2f_demosaic_f32 (Bayer) {np.median(t['f0']):.3f} ms (range {min(t['f0']):.3f} .. {max(t['f0']):.3f})")
            for i in range(1, len(ctxs)):  # the in-tree build's median against this build's own range over the rounds
                for k, name in (("x", "r2f_demosaic_xtrans_u16"), ("b", "r2f_demosaic_u16"), ("f", "r2f_demosaic_f32")):
                    mine, theirs = round(float(np.median(t[f"{k}0"])), 3), [round(v, 3) for v in t[f"{k}{i}"]]  # (as printed)
                    verdict = "inside" if min(theirs) <= mine <= max(theirs) else "OUTSIDE"
                    emit(f"      build {i} {name} {np.median(theirs):.3f} ms (range {min(theirs):.3f} .. {max(theirs):.3f}), output equal; "
                         f"in-tree {mine:.3f} ms is {verdict} that range")
            del outs, a, b
        del mosaic
        torch.cuda.empty_cache()
    for c in ctxs:
        c.close()
    emit()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_xtrans_probe.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--lib", action="append", default=[], metavar="PATH",
                    help="another build of the library (repeatable): its legs take turns with the in-tree build's, after its outputs "
                         "have been found equal to the in-tree build's")
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
    kernels(args.rounds, args.iters, emit, args.lib)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
