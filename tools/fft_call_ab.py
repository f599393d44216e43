"""Interleaved A/B of two builds of the library on the FFT stencil stages, in one process (like tools/ab_libs.py): per headline frame
size and build, round by round,
  stage   the eager halation and MTF stage calls (r2f_stage_stencil, render_graph = 0), wall clock with a device synchronise behind each;
  host    the host time of those calls alone (enqueue: what a row shard pays per call);
  render  the graph-replayed r2f_render, event-timed.
Each round notes the median of its iterations; per number the table gives each build's median of round medians and their range, and
whether the second build's median lies inside the first build's own range.

    python tools/fft_call_ab.py [--rounds 7] [--iters 15] [--places abba|baab|ab|ba] [--out FILE] tools/_var/libr2f_parent.so default

(--places: the order in which the builds' contexts are created and take the first turn of the even rounds; abba gives each build two
contexts in mirrored places and pools their rounds.)"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("libs", nargs=2)
ap.add_argument("--configs", default="cfg2_24mp,cfg4_100mp")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=15)
ap.add_argument("--out", default=None)
ap.add_argument("--places", default="abba", choices=("abba", "baab", "ab", "ba"),
                help="the order the builds' contexts are created and take their turns in: the context created first runs slower by up to "
                     "1 % of a render and 3 % of an enqueue whichever build it is, so by default each build gets two contexts, mirrored")
args = ap.parse_args()
from raw2film_amd import HipProcessor, filmstock  # noqa: E402
from raw2film_amd.hip_processor import REC709_TO_XYZ  # noqa: E402
from raw2film_amd.synthetic import CONFIGS, synthetic_frame_device  # noqa: E402

stocks = filmstock.builtin_stocks()
neg, prt = stocks["Kodak Portra 400"], stocks["Kodak 2383"]
text = [f"# tools/fft_call_ab.py --rounds {args.rounds} --iters {args.iters}{' --places ' + args.places} {' '.join(args.libs)}: ms, median of round medians (min..max of the rounds)"]
for config in args.configs.split(","):
    W, H = CONFIGS[config]
    img = synthetic_frame_device(H, W)
    out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    src = torch.rand((3, H, W), dtype=torch.float32, device="cuda") * 2.0 + 0.05
    dst = torch.empty_like(src)
    procs = []
    for lib in (args.libs["ab".index(c)] for c in args.places):
        p = HipProcessor(device=0, lib_path=None if lib == "default" else lib)
        params = p.prepare(neg, 6, 0.4, (W, H), seed=20260630, matrix=REC709_TO_XYZ, print_film=prt, halation_green_factor=0.3,
                           exp_kelvin=6000, color_masking=1.0, halation=True, sharpness=True, grain=2)
        procs.append((lib, p, params))
    names = ["halation stage", "halation host", "mtf stage", "mtf host", "render replay"]
    med = {lib: {n: [] for n in names} for lib in args.libs}
    forms = {}
    for r in range(args.rounds):
        for lib, p, params in (procs if r % 2 == 0 else procs[::-1]):
            ctx = p.ctx
            ctx.set_option("render_graph", 0)
            for which, name in ((0, "halation"), (1, "mtf")):
                stage, host = [], []
                for i in range(args.iters + 2):  # two warm-up calls (spectra, scratch)
                    t0 = time.perf_counter()
                    ctx.stage_stencil(which, src, dst, y0=0, y1=H, H_global=H)
                    t1 = time.perf_counter()
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    if i >= 2:
                        stage.append((t2 - t0) * 1e3), host.append((t1 - t0) * 1e3)
                med[lib][name + " stage"].append(float(np.median(stage)))
                med[lib][name + " host"].append(float(np.median(host)))
                forms[(lib, name)] = [(c["fft"], c["window"]) for c in ctx.stencil_stats(which)]
            ctx.set_option("render_graph", 1)
            for _ in range(3):
                ctx.render(img, params, out_f32=out)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.iters + 1)]
            ev[0].record()
            for i in range(args.iters):
                ctx.render(img, params, out_f32=out)
                ev[i + 1].record()
            torch.cuda.synchronize()
            med[lib]["render replay"].append(float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(args.iters)])))
    text.append(f"## {config}: {W} x {H}; forms (fft, window) per channel: " + "; ".join(f"{k[1]} {v}" for k, v in forms.items() if k[0] == args.libs[0]))
    a, b = args.libs
    for n in names:
        for lib in args.libs:
            m = med[lib][n]
            text.append(f"  {n:15s} {lib:32s} {np.median(m):9.4f}   {min(m):.4f}..{max(m):.4f}   rounds: " + " ".join(f"{x:.4f}" for x in m))
        lo, hi, mb = min(med[a][n]), max(med[a][n]), float(np.median(med[b][n]))
        text.append(f"  {n:15s} -> {b}'s median {mb:.4f} is {'INSIDE' if lo <= mb <= hi else 'OUTSIDE'} {a}'s range {lo:.4f}..{hi:.4f} "
                    f"(range = {100 * (hi - lo) / np.median(med[a][n]):.1f} % of its median)")
    for _, p, _ in procs:
        p.close()
    del img, out, src, dst
    torch.cuda.empty_cache()
print("\n".join(text))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(text) + "\n")
