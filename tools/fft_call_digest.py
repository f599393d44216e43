"""What the FFT stencil form does per call, as text two builds of the library can be compared by: a seeded sweep over both stencils,
every window shape, whole-frame and row-range calls, stencil_fft_batch 1 / 192 and the scratch element options, then full renders
(kernel by kernel with the passes timed, then captured and replayed).  Per case: the stencil_stats FFT words, the launches and
algorithmic bytes kernel_timing counted per class, the frame_scratch_flags, a SHA-256 of the output bytes.

    python tools/fft_call_digest.py --lib tools/_var/libr2f_parent.so [--out profiles/rNN_fft_call_digest.txt]

runs the sweep in one process with the library given and then with the in-tree one, and exits 1 unless the two printouts are the
same.  (Uses nothing of the Python API that either build lacks.)"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import kernels as ok  # noqa: E402
from raw2film_amd import HipProcessor, filmstock  # noqa: E402
from raw2film_amd.hip_processor import REC709_TO_XYZ  # noqa: E402

WINDOWS = [(256, 256), (256, 512), (512, 256), (512, 512), (256, 1024), (512, 1024)]  # tests/test_gpu_fft.py's
SCALE = 12288 / 36.0  # px per mm of the 100 MP headline: an 87-tap halation disc, a 35-tap MTF kernel


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:24]


def fft_words(ctx, which):
    return " ".join("%d:%s:%d" % (c["fft"], "%dx%d" % c["window"] if c["window"] else "-", c["real_spectrum"]) for c in ctx.stencil_stats(which))


def timing(ctx):
    return " ".join("%d/%.17g" % ctx.kernel_timing(cls)[1:] for cls in range(6))


def sweep(lib_path):
    lines = []
    stocks = filmstock.builtin_stocks()
    neg, prt = stocks["Kodak Portra 400"], stocks["Kodak 2383"]
    proc = HipProcessor(device=0, lib_path=lib_path)
    ctx = proc.ctx
    rng = np.random.default_rng(20261020)
    H, W = 600, 1100
    img = rng.uniform(0.05, 2.0, (H, W, 3)).astype(np.float32)
    img[rng.integers(0, H, 40), rng.integers(0, W, 40)] = 500.0
    src = torch.from_numpy(np.ascontiguousarray(np.transpose(img, (2, 0, 1)))).cuda()
    kernels = (ok.compute_halation_kernel(SCALE, halation_green_factor=0.3), ok.mtf_kernel(neg.mtf, SCALE))
    # ---- stage calls
    for which in (0, 1):
        ctx.set_kernel(which, kernels[which])
        for window in WINDOWS:
            ctx.set_option("stencil_fft_window_rows", window[0])
            ctx.set_option("stencil_fft_window", window[1])
            for batch in (1, 192):
                for element in ("default", "scratch32_flipped", "scratch96"):
                    ctx.set_option("stencil_fft_batch", batch)
                    ctx.set_option("stencil_fft_scratch32", (2 ^ (1 << which)) if element == "scratch32_flipped" else 2)
                    ctx.set_option("stencil_fft_scratch96", (1 << which) if element == "scratch96" else 0)
                    ctx.set_option("kernel_timing", 7)
                    for y0, y1 in ((0, H), (137, 411)):
                        dst = torch.zeros((3, y1 - y0, W), dtype=torch.float32, device="cuda")
                        ctx.stage_stencil(which, src, dst, dst_gy0=y0, y0=y0, y1=y1, H_global=H)
                        lines.append(f"stage which={which} window={window[0]}x{window[1]} batch={batch} {element} rows={y0}:{y1} | "
                                     f"{fft_words(ctx, which)} | {timing(ctx)} | flags {ctx.frame_scratch_flags().tolist()} | {sha(dst)}")
    for name, v in (("stencil_fft_window_rows", 0), ("stencil_fft_window", 0), ("stencil_fft_batch", 192), ("stencil_fft_scratch32", 2),
                    ("stencil_fft_scratch96", 0), ("kernel_timing", 0)):
        ctx.set_option(name, v)
    # ---- full renders: the halation chooses its element per window pair on the device
    # (window rows forced to 256 where the frame would take 512: only 256-row windows choose per pair)
    for (H, W), batch, auto, rows in (((700, 1100), 192, 1, 256), ((700, 1100), 1, 1, 256), ((700, 1100), 192, 0, 256), ((700, 1100), 192, 1, 0),
                                      ((333, 2048), 1, 1, 0), ((333, 2050), 1, 1, 0)):
        frame = torch.from_numpy(rng.uniform(0.02, 4.0, (H, W, 3)).astype(np.float32)).cuda()
        frame[::97, ::131] = 3000.0
        fw = 36.0 * W / 12288.0
        params = proc.prepare(neg, 6, 0.4, (W, H), seed=20260630, matrix=REC709_TO_XYZ, print_film=prt, halation_green_factor=0.3,
                              exp_kelvin=6000, color_masking=1.0, frame_width=fw, frame_height=fw * H / W)
        ctx.set_option("stencil_fft_batch", batch)
        ctx.set_option("stencil_fft_scratch96_auto", auto)
        ctx.set_option("stencil_fft_window_rows", rows)
        out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        for step in ("timed", "eager", "captured", "replayed"):
            if step in ("timed", "eager"):  # (an option moves the generation: the three untimed frames share one)
                ctx.set_option("kernel_timing", 7 if step == "timed" else 0)
            ctx.render(frame, params, out_f32=out)
            flags = ctx.frame_scratch_flags()
            lines.append(f"render {H}x{W} batch={batch} auto={auto} rows={rows} {step} | {fft_words(ctx, 0)} | {fft_words(ctx, 1)} | {timing(ctx)} | "
                         f"flags {int(flags.sum())}/{flags.size} {hashlib.sha256(flags.tobytes()).hexdigest()[:12]} | {sha(out)}")
        s = ctx.render_stats()
        lines.append(f"render {H}x{W} batch={batch} auto={auto} rows={rows} stats replays={s['replays']} captures={s['captures']} eager={s['eager']}")
        ctx.set_option("stencil_fft_batch", 192)
        ctx.set_option("stencil_fft_scratch96_auto", 1)
        ctx.set_option("stencil_fft_window_rows", 0)
    proc.close()
    return lines


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="the other build of the library (run first)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    first, second = sweep(args.lib), sweep(None)
    same = first == second
    text = [f"# tools/fft_call_digest.py --lib {args.lib}: {len(first)} cases with that library, then {len(second)} with the in-tree one: "
            + ("the two printouts are identical" if same else "the printouts DIFFER"),
            "# stage lines: stencil_stats per channel (fft:window:real spectrum) | kernel_timing classes 0-5 (launches/algorithmic bytes) | "
            "frame_scratch_flags | SHA-256 of the output", f"## {args.lib}"] + first + ["## in-tree library"] + second
    if not same:
        text += ["## differing lines"] + [f"< {a}\n> {b}" for a, b in zip(first, second) if a != b]
    print("\n".join(text))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(text) + "\n")
    sys.exit(0 if same else 1)
