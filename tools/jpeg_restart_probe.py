"""What restart intervals cost the device JPEG encoder, and whether the encode without them moved: the jpeg_probe.py setup (uint8
noise, the encoder's worst case, and a render of the smooth synthetic frame; 24 MP and 101 MP; quality 100; events on the stream
around HipContext.jpeg_encode with the frame on the device) with builds of the library taking turns in one process as in
ab_libs.py.

    python tools/jpeg_restart_probe.py [--out FILE] [--rounds 6] [--iters 7] [--no-check] [parent.so]

Per round every variant encodes `iters` frames after one untimed one and notes their median; the table gives the median of the
round medians and their range.  Variants: the in-tree library without an interval, with restart_marker_rows=1 and with
restart_marker_blocks=1, and -- when a second library is named, e.g. a build of the parent commit -- that library without an
interval (it knows no other), interleaved with the rest and in reversed order every other round.  Every in-tree file is checked to be
Pillow's, byte for byte, at 24 MP (--no-check: not at all)."""
import argparse
import io
import os
import statistics
import sys

import numpy as np
import torch
from PIL import Image, ImageFile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from raw2film_amd import HipProcessor, filmstock  # noqa: E402
from raw2film_amd.synthetic import synthetic_frame_device  # noqa: E402


def pillow(a, q, **kw):
    ImageFile.MAXBLOCK = max(ImageFile.MAXBLOCK, 8 * a.shape[0] * a.shape[1])
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", quality=q, **kw)
    return buf.getvalue()


def round_median(ctx, dev, q, restart, iters):
    ctx.jpeg_encode(dev, q, restart=restart)  # (warm: scratch sized)
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ctx.jpeg_encode(dev, q, restart=restart)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent", nargs="?", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--quality", type=int, default=100)
    ap.add_argument("--no-check", action="store_true")
    args = ap.parse_args()
    q = args.quality
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    proc = HipProcessor(device=0)
    say(f"# tools/jpeg_restart_probe.py on {torch.cuda.get_device_name(0)}, quality {q}, 4:2:0, standard tables; device ms: median of "
        f"{args.rounds} round medians of {args.iters} encodes (min..max of the round medians)")
    say(f"# in-tree: {proc.ctx._lib.r2f_version().decode()}")
    parent = None
    if args.parent:
        parent = HipProcessor(device=0, lib_path=args.parent)
        say(f"# parent: {parent.ctx._lib.r2f_version().decode()} ({os.path.basename(args.parent)})")
    stocks = filmstock.builtin_stocks()
    neg, prt = stocks["Kodak Portra 400"], stocks["Kodak 2383"]
    kw = dict(print_film=prt, lens_correction=False, frame_width=36, frame_height=24, seed=1)
    say(f"{'frame':<28} {'variant':<26} {'interval':>8} {'intervals':>9} {'file MB':>8} {'device ms':>9}  {'min..max':<17} same bytes")
    for H, W in ((4000, 6000), (8192, 12288)):
        mp = f"{H * W / 1e6:.0f} MP"
        noise_u8 = np.random.default_rng(H).integers(0, 256, (H, W, 3), dtype=np.uint8)
        smooth = proc.process(synthetic_frame_device(H, W, seed=3, kind="smooth").cpu().numpy(), neg, 6, 0.4, **kw)
        for name, u8 in ((f"{mp} uint8 noise", noise_u8), (f"{mp} render of smooth frame", smooth)):
            dev = torch.from_numpy(u8).cuda()
            per_row, n_mcus = -(-W // 16), -(-W // 16) * -(-H // 16)
            variants = [("in-tree, no restart", proc, 0, {})]
            if parent is not None:
                variants.append(("parent, no restart", parent, 0, {}))
            variants += [("in-tree, rows=1", proc, per_row, dict(restart_marker_rows=1)),
                         ("in-tree, blocks=1", proc, 1, dict(restart_marker_blocks=1))]
            med = {v[0]: [] for v in variants}
            for r in range(args.rounds):
                for label, p, restart, _ in (variants if r % 2 == 0 else variants[::-1]):
                    med[label].append(round_median(p.ctx, dev, q, restart, args.iters))
            for label, p, restart, options in variants:
                out, n = p.ctx.jpeg_encode(dev, q, restart=restart)
                got = out[:int(n.item())].cpu().numpy().tobytes()
                same = "-"
                if not args.no_check and H * W < 30e6:
                    same = str(got == pillow(u8, q, **options))
                m = med[label]
                say(f"{name:<28} {label:<26} {restart:8d} {-(-n_mcus // restart) if restart else 0:9d} {len(got) / 1e6:8.2f} "
                    f"{statistics.median(m):9.3f}  {min(m):.3f}..{max(m):.3f}".ljust(112) + f"  {same}")
            del dev
    for p in (proc, parent):
        if p is not None:
            p.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
