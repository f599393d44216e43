"""JPEG export with progressive=True: what it costs and saves, on the device and in Pillow, at 24 MP and 101 MP.

    python tools/jpeg_progressive_probe.py [--out FILE] [--quality 95]

Per frame (a render of the synthetic noise frame): device = ctx.jpeg_encode from a device frame, wall time (the progressive call
blocks: the transform, the per-scan symbol and run passes, the 40 KB read-back, the tables and headers built on the host, the
packing of the ten scans and the length read back; median of 5), next to the optimized baseline encode of the same frame;
encode_jpeg = the call from a device frame to the bytes on the host; Pillow = the host encode of the same array (one thread);
same = byte for byte.  At 24 MP also the whole export: process_jpeg(progressive=True) against process() followed by Pillow's
progressive save."""
import argparse
import io
import os
import statistics
import sys
import time

import torch
from PIL import Image, ImageFile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from raw2film_amd import HipProcessor, filmstock  # noqa: E402
from raw2film_amd.synthetic import synthetic_frame_device  # noqa: E402

FRAMES = ((4000, 6000), (8192, 12288))


def pillow(a, q, s, o=False, p=False):
    ImageFile.MAXBLOCK = max(ImageFile.MAXBLOCK, 32 * a.shape[0] * a.shape[1])
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", quality=q, subsampling=s, optimize=o, progressive=p)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quality", type=int, default=95)
    args = ap.parse_args()
    q = args.quality
    lines = [f"# tools/jpeg_progressive_probe.py on {torch.cuda.get_device_name(0)}, quality {q}, 4:2:0; times in ms (medians)"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    proc = HipProcessor(device=0)
    stocks = filmstock.builtin_stocks()
    kw = dict(print_film=stocks["Kodak 2383"], lens_correction=False, frame_width=36, frame_height=24, seed=1)
    neg = stocks["Kodak Portra 400"]
    say(f"{'frame':<10} {'options':<12} {'file MB':>8} {'device':>8} {'encode_jpeg':>11} {'Pillow MB':>9} {'Pillow':>8}  same")
    for H, W in FRAMES:
        src = synthetic_frame_device(H, W, seed=3, kind="noise").cpu().numpy()
        u8 = proc.process(src, neg, 6, 0.4, **kw)
        dev = torch.from_numpy(u8).cuda()
        name = f"{H * W / 1e6:.0f} MP"
        for label, o, p in (("optimize", True, False), ("progressive", False, True)):
            d_ms, _ = wall(lambda: proc.ctx.jpeg_encode(dev, q, 2, o, p), 5)
            e_ms, got = wall(lambda: proc.encode_jpeg(dev, q, subsampling=2, optimize=o, progressive=p), 5)
            p_ms, want = wall(lambda: pillow(u8, q, 2, o, p), 1 if H > 5000 else 3)
            say(f"{name:<10} {label:<12} {len(got) / 1e6:8.2f} {d_ms:8.2f} {e_ms:11.2f} {len(want) / 1e6:9.2f} {p_ms:8.1f}  "
                f"{got == want}")
        if H < 5000:
            x_ms, got = wall(lambda: proc.process_jpeg(src, neg, 6, 0.4, quality=q, progressive=True, **kw), 3)
            c_ms, want = wall(lambda: pillow(proc.process(src, neg, 6, 0.4, **kw), q, 2, False, True), 3)
            say(f"{name} export: process_jpeg(progressive=True) {x_ms:.1f} ms, process() + Pillow progressive {c_ms:.1f} ms "
                f"({c_ms / x_ms:.1f}x), same {got == want}")
        del dev
    proc.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
