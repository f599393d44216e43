"""JPEG export timing: the device encoder (HipProcessor.encode_jpeg) and the whole export (process_jpeg) against what the
reference does -- process() + Pillow's `Image.fromarray(a).save(f, "JPEG", quality=100)` (gui.py:2338-2341) -- at 24 MP and 100 MP,
on uniform uint8 noise (the encoder's worst case) and on renders of the synthetic noise and smooth frames.  Every file is checked to
be Pillow's, byte for byte.

    python tools/jpeg_probe.py [--out FILE] [--quality 100]

Columns: device = the encoder's kernels alone (events on the stream, frame already on the device, median of 7); encode_jpeg = the
call from a device frame to the bytes on the host (the 8-byte length read and the file's download included); Pillow = the host
encode of the same uint8 array (median of 3, one thread); export = process_jpeg from the host float frame, against
process(cache=False) + Pillow (what the reference's export path runs)."""
import argparse
import io
import os
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from raw2film_amd import HipProcessor, filmstock  # noqa: E402
from raw2film_amd.synthetic import synthetic_frame_device  # noqa: E402


def pillow(a, q):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", quality=q)
    return buf.getvalue()


def wall(fn, reps):
    ts, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), out


def device_ms(proc, dev, q, reps=7):
    proc.ctx.jpeg_encode(dev, q)  # (warm: scratch sized)
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        proc.ctx.jpeg_encode(dev, q)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quality", type=int, default=100)
    args = ap.parse_args()
    q = args.quality
    lines = [f"# tools/jpeg_probe.py on {torch.cuda.get_device_name(0)}, quality {q}; times in ms (medians)"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    stocks = filmstock.builtin_stocks()
    neg, prt = stocks["Kodak Portra 400"], stocks["Kodak 2383"]
    proc = HipProcessor(device=0)
    kw = dict(print_film=prt, lens_correction=False, frame_width=36, frame_height=24, seed=1)
    say(f"{'frame':<28} {'file MB':>8} {'raw MB':>7} {'device':>8} {'encode_jpeg':>11} {'Pillow':>8} {'export':>8} "
        f"{'process+Pillow':>14}  same bytes")
    for H, W in ((4000, 6000), (8192, 12288)):
        mp = f"{H * W / 1e6:.0f} MP"
        rng = np.random.default_rng(H)
        noise_u8 = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        rows = [(f"{mp} uint8 noise", noise_u8, None)]
        for kind in ("noise", "smooth"):
            src = synthetic_frame_device(H, W, seed=3, kind=kind).cpu().numpy()
            rows.append((f"{mp} render of {kind} frame", proc.process(src, neg, 6, 0.4, **kw), src))
        for name, u8, src in rows:
            dev = torch.from_numpy(u8).cuda()
            d_ms = device_ms(proc, dev, q)
            e_ms, got = wall(lambda: proc.encode_jpeg(dev, q), 5)
            p_ms, want = wall(lambda: pillow(u8, q), 3)
            same = got == want
            x_ms = r_ms = float("nan")
            if src is not None:
                x_ms, got_x = wall(lambda: proc.process_jpeg(src, neg, 6, 0.4, quality=q, **kw), 3)
                same = same and got_x == want  # (u8 is process(cache=True)'s render of src)
                r_ms, _ = wall(lambda: pillow(proc.process(src, neg, 6, 0.4, cache=False, **kw), q), 3)
            say(f"{name:<28} {len(want) / 1e6:8.2f} {u8.nbytes / 1e6:7.1f} {d_ms:8.2f} {e_ms:11.2f} {p_ms:8.1f} {x_ms:8.1f} "
                f"{r_ms:14.1f}  {same}")
            del dev
    proc.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
