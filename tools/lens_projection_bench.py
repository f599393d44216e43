"""Device time of r2f_lens_correct_projected beside r2f_lens_correct / r2f_lens_correct_tca at 24 MP and 100 MP, in the manner of
tools/lens_tca_bench.py: event-timed launches, three untimed launches first, the median of --iters per round, all kernels taking
turns in every round of one process, and the copy ceiling of the same run (r2f_stream_copy).  Per shape, without a TCA record and
with the tests' `poly3` record:
  - the projected kernel with an identity record (focal 2^20: P is exactly 1, the same texels) against the unprojected kernel;
  - the projected kernel with the fisheye record (focal 2/pi) and with the equisolid record (0.55) at their auto scales, against the
    unprojected kernel with the same profile minus the projection at the same scale -- which gathers from global memory the tiles
    whose box no longer fits, where the projected kernel works in two halves.
The share of blocks on each staging route comes from the host restatement of the kernel's rule (tests/lens_projection_model.py's,
evaluated here strip by strip).

    python tools/lens_projection_bench.py [--rounds 6] [--iters 10] [--lib path/to/other/libr2f_hip.so]

The yardsticks are the unprojected kernels and the copy in the same run, not an absolute time.

--lib binds ANOTHER build of the library beside the in-tree one (the parent commit's, to see whether a kernel moved): every case is
also launched through it, taking turns with the in-tree one inside every round, its output is compared bit for bit (the last line counts the cases that differ, and any makes the exit status 1), and per case the
ratio in-tree / --lib of every round's median is printed.  The spread of those ratios with --lib pointing at a copy of the in-tree
library itself is the noise of the method.  The route shares, which do not depend on the build, are left out of such a run.
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lens_model as lm  # noqa: E402
import lens_projection_model as pm  # noqa: E402
import lens_tca_model as tm  # noqa: E402
from raw2film_amd.context import HipContext  # noqa: E402
from raw2film_amd.lens import LensProfile  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--lib", default=None)
args = ap.parse_args()
SHAPES = {"24 MP": (4000, 6000), "100 MP": (8192, 12288)}
BASE = dict(distortion="ptlens", coefficients=(0.02, -0.06, 0.01), vignetting=(-0.3, 0.1, -0.02))
POLY3 = tm.TCA_SPECS["poly3"]
RECORDS = {"fisheye": ("fisheye", 2.0 / math.pi), "equisolid": ("equisolid", 0.55)}
F = np.float32
ctx = HipContext(0)
other_ctx = HipContext(0, lib_path=args.lib) if args.lib else None
differing = []  # the cases whose output through --lib is not the in-tree library's


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


def route_shares(prof, H, W, scale):
    """The share of 64 x 16 blocks on each route, and of half-passes that gather: the kernel's rule over the whole frame."""
    c = lm.rounded(lm.constants(prof, H, W, scale))
    rec = pm.record(prof)
    tca = None if prof.tca is None else tm.record(prof, F)
    ntx = (W + 63) // 64
    counts = dict(whole=0, halves=0, gather=0)
    big = np.iinfo(np.int64).max
    for y0 in range(0, H, 16):
        rows = min(16, H - y0)
        Y, X = np.meshgrid(np.arange(y0, y0 + rows), np.arange(W), indexing="ij")
        ox, oy, _, _ = pm.offsets(c, rec, X, Y)
        coords = [(F(c.cx) + ox, F(c.cy) + oy)] if tca is None else [tm.channel_coords(c, tca, ch, ox, oy) for ch in range(3)]
        lo = np.full((2, ntx, 2), big, np.int64)   # per half, tile: min ix, min iy
        hi = np.full((2, ntx, 2), -big, np.int64)
        for sx, sy in coords:
            in_x, ix, _ = lm.split_phase(sx, W)
            in_y, iy, _ = lm.split_phase(sy, H)
            inside = in_x & in_y
            for k, a in enumerate((ix, iy)):
                pad_lo = np.full((16, ntx * 64), big, np.int64)
                pad_hi = np.full((16, ntx * 64), -big, np.int64)
                pad_lo[:rows, :W] = np.where(inside, a, big)
                pad_hi[:rows, :W] = np.where(inside, a, -big)
                lo[:, :, k] = np.minimum(lo[:, :, k], pad_lo.reshape(2, 8, ntx, 64).min(axis=(1, 3)))
                hi[:, :, k] = np.maximum(hi[:, :, k], pad_hi.reshape(2, 8, ntx, 64).max(axis=(1, 3)))
        any_half = lo[:, :, 0] <= hi[:, :, 0]
        size = np.where(any_half, (hi[:, :, 0] - lo[:, :, 0] + 8) * (hi[:, :, 1] - lo[:, :, 1] + 8), 0)
        un_lo, un_hi = lo.min(axis=0), hi.max(axis=0)
        whole = ~any_half.any(axis=0) | ((un_hi[:, 0] - un_lo[:, 0] + 8) * (un_hi[:, 1] - un_lo[:, 1] + 8) <= pm.BOX_TEXELS)
        gathers = (size > pm.BOX_TEXELS) & ~whole[None, :]
        counts["whole"] += int(whole.sum())
        counts["gather"] += int(gathers.any(axis=0).sum())
        counts["halves"] += int((~whole & ~gathers.any(axis=0)).sum())
    n = sum(counts.values())
    return {k: v / n for k, v in counts.items()}


for label, (H, W) in SHAPES.items():
    img = torch.rand((H, W, 3), device="cuda") * 4
    other = torch.empty_like(img)
    for _ in range(3):
        ctx.stream_copy(img, other)
    copy_ms = min(timed(lambda: ctx.stream_copy(img, other), args.iters) for _ in range(3))
    print(f"{label} ({H} x {W}): copy {copy_ms:.3f} ms = {2 * img.numel() * 4 / copy_ms / 1e6:.0f} GB/s", flush=True)
    del other
    for tca_name, tca in (("no TCA", None), ("poly3 TCA", POLY3)):
        calls, other_calls, yardstick = {}, {}, {}

        def add(name, prof, base=None):
            params, proj, tca_params = prof.plan_projected(H, W)
            calls[name] = lambda p=params, j=proj, t=tca_params: ctx.lens_correct(img, p, tca=t, projection=j)
            if other_ctx:
                other_calls[name] = lambda p=params, j=proj, t=tca_params: other_ctx.lens_correct(img, p, tca=t, projection=j)
            yardstick[name] = base
            return params.scale

        add("unprojected, scale 1.02", LensProfile(**BASE, scale=1.02, tca=tca))
        add("projected identity, scale 1.02", LensProfile(**BASE, scale=1.02, tca=tca, projection=("fisheye", 2.0 ** 20)), "unprojected, scale 1.02")
        for rname, record in RECORDS.items():
            auto = LensProfile(**BASE, scale="auto", tca=tca, projection=record)
            scale = auto.plan_projected(H, W)[0].scale
            if not other_ctx:
                shares = route_shares(LensProfile(**BASE, scale=scale, tca=tca, projection=record), H, W, scale)
                print(f"  [{tca_name}] {rname} auto scale {scale:.4f}: blocks whole {shares['whole']:.3f}, in two staged halves {shares['halves']:.3f}, "
                      f"with a gathering half {shares['gather']:.3f}", flush=True)
            add(f"unprojected, scale {scale:.3f}", LensProfile(**BASE, scale=scale, tca=tca))
            add(f"projected {rname}, scale {scale:.3f}", LensProfile(**BASE, scale=scale, tca=tca, projection=record), f"unprojected, scale {scale:.3f}")
        outs = {}
        for name, fn in calls.items():
            for _ in range(3):
                outs[name] = fn()
        same = torch.equal(outs["projected identity, scale 1.02"].view(torch.int32), outs["unprojected, scale 1.02"].view(torch.int32))
        print(f"  [{tca_name}] identity bit-identical to the unprojected kernel: {same}", flush=True)
        for name, fn in other_calls.items():
            for _ in range(3):
                out = fn()
            same = torch.equal(out.view(torch.int32), outs[name].view(torch.int32))
            print(f"  [{tca_name}] {name}: bit-identical to {os.path.basename(args.lib)}'s: {same}", flush=True)
            if not same:
                differing.append(f"{label} [{tca_name}] {name}")
            del out
        del outs
        rounds, other_rounds = {name: [] for name in calls}, {name: [] for name in other_calls}
        for _ in range(args.rounds):
            for name, fn in calls.items():  # interleaved: every kernel takes its turn in every round
                rounds[name].append(timed(fn, args.iters))
                if other_ctx:
                    other_rounds[name].append(timed(other_calls[name], args.iters))
        med = {name: float(np.median(r)) for name, r in rounds.items()}
        for name, r in rounds.items():
            against = f" = {med[name] / med[yardstick[name]]:.2f} x {yardstick[name]}" if yardstick[name] else ""
            print(f"  [{tca_name}] {name}: median of {args.rounds} round medians {med[name]:.3f} ms (range {min(r):.3f} .. {max(r):.3f}) = "
                  f"{med[name] / copy_ms:.2f} x the copy{against}", flush=True)
            if other_ctx:
                ratios = [t / o for t, o in zip(r, other_rounds[name])]
                print(f"      in-tree / {os.path.basename(args.lib)} per round: {' '.join(f'{q:.4f}' for q in ratios)}  "
                      f"(min {min(ratios):.4f}, max {max(ratios):.4f})", flush=True)
    del img
    torch.cuda.empty_cache()
if other_ctx:
    print(f"outputs that differ from {os.path.basename(args.lib)}'s: {len(differing)}" + "".join(f"\n  {d}" for d in differing), flush=True)
    sys.exit(1 if differing else 0)
