"""Device time of the three blend entry points beside their plain siblings at 24 MP and 100 MP, in the manner of
tools/lens_tca_bench.py: event-timed launches, three untimed launches first, the median of --iters per round, every kernel taking its
turn in every round of one process.  Two frames per size: one with no sample above `clip` (the Blend branch is never taken: the
cost of the test itself), one with about 5 % of its pixels blown in compact patches (a wave diverges only where a patch's edge
crosses its row).

    python tools/highlight_bench.py [--rounds 6] [--iters 10]

The yardstick is the plain entry point in the same run, not an absolute time.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from raw2film_amd.context import HipContext  # noqa: E402
from raw2film_amd.raw import RawProfile, XTransProfile  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--iters", type=int, default=10)
args = ap.parse_args()
SHAPES = {"24 MP": (4000, 6000), "100 MP": (8192, 12288)}
MATRIX = ((1.62, -0.41, -0.19), (-0.28, 1.52, -0.22), (0.04, -0.52, 1.49))
MUL = (1.0, 1.0 / 2.1, 1.6 / 2.1)  # a daylight white balance normalised by its largest factor, 16-bit samples
CLIP = int(np.float32(65535.0) * np.float32(1.0 / 2.1))  # 31207
FACTOR = float(np.float32(2.0 ** 0.5))
ctx = HipContext(0)


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


def frames(H, W):
    """(below, blown): a smooth field whose red stays under CLIP, and the same with round patches of saturated samples over about
    5 % of it (a 512 x 512 cell with one disc of radius 65, repeated)."""
    rng = np.random.default_rng(27)
    y, x = np.mgrid[0:512, 0:512]
    cell = (6000 + 20000 * (0.5 + 0.25 * np.sin(y / 40.0) + 0.25 * np.cos(x / 60.0)) + rng.integers(-200, 200, (512, 512))).astype(np.uint16)
    blown = cell.copy()
    blown[(y - 256) ** 2 + (x - 256) ** 2 <= 65 ** 2] = 65535
    reps = (-(-H // 512), -(-W // 512))
    return np.tile(cell, reps)[:H, :W], np.tile(blown, reps)[:H, :W]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


for label, (H, W) in SHAPES.items():
    bayer, xtrans = RawProfile("RGGB", multipliers=MUL, matrix=MATRIX).plan(H, W), XTransProfile(multipliers=MUL, matrix=MATRIX).plan(H, W)
    for kind, mosaic in zip(("nothing above clip", "5 % blown"), frames(H, W)):
        m = dev(mosaic)
        u16 = torch.empty((H, W, 3), dtype=torch.int16, device="cuda")
        f32 = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        pairs = {
            "r2f_demosaic_u16": (lambda: ctx.demosaic_u16(m, bayer, out=u16), lambda: ctx.demosaic_blend_u16(m, bayer, CLIP, out=u16)),
            "r2f_demosaic_f32": (lambda: ctx.demosaic_f32(m, bayer, FACTOR, out=f32), lambda: ctx.demosaic_blend_f32(m, bayer, CLIP, FACTOR, out=f32)),
            "r2f_demosaic_xtrans_u16": (lambda: ctx.demosaic_xtrans(m, xtrans, out=u16), lambda: ctx.demosaic_xtrans_blend(m, xtrans, CLIP, out=u16)),
        }
        changed = {}
        for name, (plain, blend) in pairs.items():
            out = f32 if name.endswith("f32") else u16
            for _ in range(3):
                plain()
            ref = out.clone()
            for _ in range(3):
                blend()
            changed[name] = float((out != ref).any(dim=-1).float().mean())
            del ref
        print(f"{label} ({H} x {W}), {kind}: pixels the blend entry point changed: "
              + ", ".join(f"{n} {100 * c:.2f} %" for n, c in changed.items()), flush=True)
        rounds = {(name, i): [] for name in pairs for i in (0, 1)}
        for _ in range(args.rounds):
            for name, fns in pairs.items():  # interleaved: every kernel takes its turn in every round
                for i, fn in enumerate(fns):
                    rounds[(name, i)].append(timed(fn, args.iters))
        for name in pairs:
            p, b = rounds[(name, 0)], rounds[(name, 1)]
            pm, bm = float(np.median(p)), float(np.median(b))
            print(f"  {name}: plain {pm:.3f} ms (range {min(p):.3f} .. {max(p):.3f}), blend {bm:.3f} ms (range {min(b):.3f} .. {max(b):.3f}) = "
                  f"{bm / pm:.3f} x plain", flush=True)
        del m, u16, f32
        torch.cuda.empty_cache()
