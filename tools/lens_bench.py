"""Device time of r2f_lens_correct at 24 MP and 100 MP, beside r2f_warp_affine at the same shapes and the copy ceiling of the same
run (r2f_stream_copy, bench.py's roofline.copy_ceiling); with more than one library, an interleaved A/B of their lens kernels in
one process, in the manner of tools/ab_libs.py (builds bind side by side, take turns on the same frame, share clock and drift).

    python tools/lens_bench.py [--rounds 6] [--iters 10] [default | path/to/libr2f_hip.so ...]

The algorithmic traffic of the lens step is 24 B per pixel (12 read, 12 written); the share of the copy ceiling is that over the
kernel's time, against the rate the copy moves its bytes at.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from raw2film_amd import geometry  # noqa: E402
from raw2film_amd.context import HipContext  # noqa: E402
from raw2film_amd.lens import LensProfile  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("libs", nargs="*", default=["default"])
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--iters", type=int, default=10)
args = ap.parse_args()
SHAPES = {"24 MP": (4000, 6000), "100 MP": (8192, 12288)}
PROFILES = {
    "ptlens + vignetting": LensProfile("ptlens", (0.02, -0.06, 0.01), vignetting=(-0.3, 0.1, -0.02), scale=1.02),
    "none (identity map)": LensProfile("none"),
}
ctxs = {name: HipContext(0, lib_path=None if name == "default" else name) for name in args.libs}


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
    first = next(iter(ctxs.values()))
    other = torch.empty_like(img)
    for _ in range(3):
        first.stream_copy(img, other)
    copy_ms = min(timed(lambda: first.stream_copy(img, other), args.iters) for _ in range(3))
    copy_rate = 2 * img.numel() * 4 / copy_ms / 1e6  # GB/s
    m, _ = geometry.rotation_plan(H, W, 3.5)
    for _ in range(3):
        first.warp_affine(img, m)
    warp_ms = min(timed(lambda: first.warp_affine(img, m), args.iters) for _ in range(3))
    print(f"{label} ({H} x {W}): copy {copy_ms:.3f} ms = {copy_rate:.0f} GB/s; r2f_warp_affine {warp_ms:.3f} ms", flush=True)
    results = {}
    for pname, prof in PROFILES.items():
        params = prof.plan(H, W)
        outs = {}
        for name, ctx in ctxs.items():
            for _ in range(3):
                outs[name] = ctx.lens_correct(img, params)
        ref = next(iter(outs.values()))
        same = all(torch.equal(o.view(torch.int32), ref.view(torch.int32)) for o in outs.values())
        rounds = {name: [] for name in ctxs}
        for _ in range(args.rounds):
            for name, ctx in ctxs.items():  # interleaved: every build takes its turn in every round
                rounds[name].append(timed(lambda: ctx.lens_correct(img, params), args.iters))
        for name, r in rounds.items():
            med = float(np.median(r))
            rate = 24.0 * H * W / med / 1e6
            print(f"  r2f_lens_correct [{pname}] {os.path.basename(os.path.dirname(name)) or name}/{os.path.basename(name)}: median of {args.rounds} round "
                  f"medians {med:.3f} ms (range {min(r):.3f} .. {max(r):.3f}) = {rate:.0f} GB/s of algorithmic traffic = "
                  f"{100 * rate / copy_rate:.1f} % of the copy ceiling; {med / warp_ms:.2f} x r2f_warp_affine", flush=True)
        print(f"  results of the builds bit-identical: {same}", flush=True)
    del img, other
    torch.cuda.empty_cache()
