"""What honouring the sensor's orientation inside the demosaic kernels costs on the device, beside the upright kernels and beside
what a caller had to do without it (profiles/r23_orientation_probe.txt).

    python tools/orientation_probe.py [--out FILE] [--rounds R] [--iters N] [--lib PATH ...]

For a 24 MP and a 100 MP sensor and both patterns (Bayer: r2f_demosaic_oriented_u16, X-Trans: r2f_demosaic_xtrans_oriented_u16), in
this process (device events, median of round medians, the legs taking turns round by round):
  upright                   the upright entry point alone (r2f_demosaic_u16 / r2f_demosaic_xtrans_u16): the yardstick this work leaves
                            unchanged
  upright + rot90           the upright entry point followed by torch.rot90(frame, 1, (0, 1)).contiguous(): what a caller has to do
                            for orientation 5 without the oriented entry points -- a second frame and 12 B per pixel more traffic
  orientation 0, 3, 5, 6    the oriented entry point: the upright kernel again, the mirrored class, the turned class both ways
  reduced, orientation 5    the lane-per-pixel kernel of the reduced size storing to the mapped address, beside its upright form
Before any timing every oriented output is asserted equal to the definition applied to the upright frame (flips and a transpose in
torch).  Each --lib PATH is another build of the library (say the parent commit's, built with build(out=PATH)): its upright legs take
turns with the in-tree build's, after their outputs have been asserted equal, and the in-tree median is held against that build's own
range over the rounds.
The mosaics are noise: the kernels' times do not depend on the picture.  Needs a GPU: there is no CPU path.
"""

from __future__ import annotations

import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = (("24 MP", 4000, 6000), ("100 MP", 8192, 12288))
MATRIX = ((0.52, 0.27, 0.15), (0.25, 0.68, 0.07), (0.03, 0.12, 0.81))
ORIENTATIONS = (0, 3, 5, 6)


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


def oriented(frame, o):
    """The definition of include/r2f.h on a device frame."""
    if o & 2:
        frame = frame.flip(0)
    if o & 1:
        frame = frame.flip(1)
    return frame.transpose(0, 1) if o & 4 else frame


def kernels(rounds, iters, emit, libs=()):
    import torch

    from raw2film_amd import _lib
    from raw2film_amd.context import HipContext
    from raw2film_amd.raw import RawProfile, XTransProfile

    ctxs = [HipContext(0)]  # build 0 is the in-tree library
    # another build may be from before the oriented entry points (the parent commit's): only its upright legs are called, so it is
    # bound without the two symbols it cannot have
    new = {k: _lib._SIGNATURES.pop(k) for k in ("r2f_demosaic_oriented_u16", "r2f_demosaic_xtrans_oriented_u16")}
    try:
        ctxs += [HipContext(0, lib_path=path) for path in libs]
    finally:
        _lib._SIGNATURES.update(new)
    ctx = ctxs[0]
    patterns = (("Bayer", "demosaic_u16", RawProfile("RGGB", black=512, multipliers=(7.9, 4.1, 6.2), matrix=MATRIX)),
                ("X-Trans", "demosaic_xtrans", XTransProfile(black=512, multipliers=(7.9, 4.1, 6.2), matrix=MATRIX)))
    emit(f"kernels ({torch.cuda.get_device_name(0)}): device events, {iters} launches per round median, {rounds} interleaved rounds")
    for i, path in enumerate(libs):
        emit(f"  build {i + 1}: {path} ({ctxs[i + 1]._lib.r2f_version().decode()}); build 0: the in-tree library")
    for label, H, W in SIZES:
        mosaic = torch.randint(0, 16384, (H, W), dtype=torch.int16, device="cuda")
        for name, method, profile in patterns:
            for reduced in (False, True):
                p = profile.plan(H, W, reduced)
                shape, turned_shape = (p.out_h, p.out_w, 3), (p.out_w, p.out_h, 3)
                ups = [torch.empty(shape, dtype=torch.int16, device="cuda") for _ in ctxs]
                outs = {o: torch.empty(turned_shape if o & 4 else shape, dtype=torch.int16, device="cuda")
                        for o in (ORIENTATIONS if not reduced else (0, 5))}
                legs = {}
                for i, (c, up) in enumerate(zip(ctxs, ups)):
                    legs[f"u{i}"] = lambda c=c, up=up: getattr(c, method)(mosaic, p, out=up)
                legs["r"] = lambda: torch.rot90(getattr(ctx, method)(mosaic, p, out=ups[0]), 1, (0, 1)).contiguous()
                for o, out in outs.items():
                    if o:
                        legs[f"o{o}"] = lambda o=o, out=out: getattr(ctx, method)(mosaic, p, out=out, orientation=o)
                    else:  # (the context calls the upright entry point for 0: the oriented one through the library)
                        fn = getattr(ctx._lib, "r2f_demosaic_oriented_u16" if name == "Bayer" else "r2f_demosaic_xtrans_oriented_u16")
                        legs["o0"] = lambda out=out, fn=fn: ctx._check(fn(ctx._h, mosaic.data_ptr(), 0, H, W, H, W, C.byref(p), 0, out.data_ptr(), 0,
                                                                          p.out_h, ctx._stream()))
                for _ in range(3):
                    for fn in legs.values():
                        fn()
                torch.cuda.synchronize()
                for up in ups[1:]:  # before any timing: every build computes the in-tree build's upright bytes ...
                    assert torch.equal(up, ups[0]), f"{label} {name} reduced={reduced}: the builds differ"
                for o, out in outs.items():  # ... and every orientation is the definition applied to them
                    assert torch.equal(out, oriented(ups[0], o)), f"{label} {name} reduced={reduced}: orientation {o} is not the definition"
                assert torch.equal(legs["r"](), outs[5]), "upright + rot90 is orientation 5"
                t = {k: [] for k in legs}
                for _ in range(rounds):
                    for k, fn in legs.items():
                        t[k].append(timed(torch, fn, iters))
                med = {k: float(np.median(v)) for k, v in t.items()}
                form = ("reduced (half) size" if name == "Bayer" else "reduced (third) size") if reduced else "full size"
                px = p.out_h * p.out_w
                emit(f"  {label} sensor, {name}, {form} ({p.out_h} x {p.out_w}):")
                emit(f"      upright entry point           {med['u0']:.3f} ms (range {min(t['u0']):.3f} .. {max(t['u0']):.3f})")
                emit(f"      upright + rot90.contiguous()  {med['r']:.3f} ms (range {min(t['r']):.3f} .. {max(t['r']):.3f}): "
                     f"{(med['r'] - med['u0']) * 1e6 / px:.3f} ns per pixel for the turn's 12 B per pixel")
                for o in outs:
                    k = f"o{o}"
                    cls = "upright kernel" if o == 0 else "lane per pixel" if reduced else "turned" if o & 4 else "mirrored"
                    emit(f"      orientation {o} ({cls:14s})   {med[k]:.3f} ms (range {min(t[k]):.3f} .. {max(t[k]):.3f}) = "
                         f"{med[k] / med['u0']:.2f} x upright" + (f", {med[k] / med['r']:.2f} x upright + rot90" if o & 4 else ""))
                for i in range(1, len(ctxs)):
                    mine, theirs = round(med["u0"], 3), [round(v, 3) for v in t[f"u{i}"]]  # (as printed)
                    verdict = "inside" if min(theirs) <= mine <= max(theirs) else "OUTSIDE"
                    emit(f"      build {i} upright entry point {np.median(theirs):.3f} ms (range {min(theirs):.3f} .. {max(theirs):.3f}), output "
                         f"equal; in-tree {mine:.3f} ms is {verdict} that range")
                del ups, outs, legs
                torch.cuda.empty_cache()
        del mosaic
        torch.cuda.empty_cache()
    for c in ctxs:
        c.close()
    emit()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_orientation_probe.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--lib", action="append", default=[], metavar="PATH",
                    help="another build of the library (repeatable): its upright legs take turns with the in-tree build's, after its "
                         "outputs have been found equal to the in-tree build's")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("orientation_probe needs a GPU")
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    emit("The oriented demosaic kernels beside the upright ones and beside upright + rot90 (tools/orientation_probe.py)")
    emit()
    kernels(args.rounds, args.iters, emit, args.lib)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
