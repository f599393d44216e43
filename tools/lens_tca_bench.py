"""Device time of r2f_lens_correct_tca beside r2f_lens_correct at 24 MP and 100 MP, in the manner of tools/lens_bench.py: event-timed
launches, three untimed launches first, the median of --iters per round, both kernels taking turns in every round of one process,
and the copy ceiling of the same run (r2f_stream_copy).  The profile is lens_bench's ptlens + vignetting; the TCA records are the
tests' `poly3` spec and `identity` (factors exactly 1: the same texels as the plain kernel, at three coordinate chains).

    python tools/lens_tca_bench.py [--rounds 6] [--iters 10]

The yardstick is r2f_lens_correct in the same run, not an absolute time.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from raw2film_amd.context import HipContext  # noqa: E402
from raw2film_amd.lens import LensProfile  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--iters", type=int, default=10)
args = ap.parse_args()
SHAPES = {"24 MP": (4000, 6000), "100 MP": (8192, 12288)}
BASE = dict(distortion="ptlens", coefficients=(0.02, -0.06, 0.01), vignetting=(-0.3, 0.1, -0.02), scale=1.02)
TCA = {"poly3": ("poly3", (1.002, 0.998, 0.01, -0.008, -0.02, 0.015)), "identity": ("linear", (1.0, 1.0))}
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


for label, (H, W) in SHAPES.items():
    img = torch.rand((H, W, 3), device="cuda") * 4
    other = torch.empty_like(img)
    for _ in range(3):
        ctx.stream_copy(img, other)
    copy_ms = min(timed(lambda: ctx.stream_copy(img, other), args.iters) for _ in range(3))
    print(f"{label} ({H} x {W}): copy {copy_ms:.3f} ms = {2 * img.numel() * 4 / copy_ms / 1e6:.0f} GB/s", flush=True)
    del other
    plain = LensProfile(**BASE).plan(H, W)
    calls = {"r2f_lens_correct": lambda: ctx.lens_correct(img, plain)}
    for name, tca in TCA.items():
        params, tca_params = LensProfile(**BASE, tca=tca).plan_tca(H, W)
        calls[f"r2f_lens_correct_tca [{name}]"] = lambda p=params, t=tca_params: ctx.lens_correct(img, p, tca=t)
    outs = {}
    for name, fn in calls.items():
        for _ in range(3):
            outs[name] = fn()
    ref = outs["r2f_lens_correct"].view(torch.int32)
    print(f"  identity bit-identical to r2f_lens_correct: {torch.equal(outs['r2f_lens_correct_tca [identity]'].view(torch.int32), ref)}; "
          f"poly3's green plane bit-identical: {torch.equal(outs['r2f_lens_correct_tca [poly3]'].view(torch.int32)[1], ref[1])}", flush=True)
    del outs, ref
    rounds = {name: [] for name in calls}
    for _ in range(args.rounds):
        for name, fn in calls.items():  # interleaved: every kernel takes its turn in every round
            rounds[name].append(timed(fn, args.iters))
    base = float(np.median(rounds["r2f_lens_correct"]))
    for name, r in rounds.items():
        med = float(np.median(r))
        print(f"  {name}: median of {args.rounds} round medians {med:.3f} ms (range {min(r):.3f} .. {max(r):.3f}) = "
              f"{med / base:.2f} x r2f_lens_correct = {med / copy_ms:.2f} x the copy", flush=True)
    del img
    torch.cuda.empty_cache()
