"""JPEG export options: what subsampling and optimize cost and save, on the device and in Pillow, at 24 MP and 101 MP.

    python tools/jpeg_options_probe.py [--out FILE] [--quality 100] [--ab DIR [--rounds 5] [--ab-only]]

Per frame (a render of the synthetic noise and smooth frames) and option set: device = ctx.jpeg_encode from a device frame, timed
with events on the stream (for optimize this includes the stats pass, the one 8 KB read-back, the tables built on the host and the
bits pass; median of 7); encode_jpeg = the call from a device frame to the bytes on the host; Pillow = the host encode of the same
array with the same options (one thread); same = the device file is Pillow's, byte for byte.
--ab DIR: the default 4:2:0 encode of this tree and of another checkout's package (DIR holds its built raw2film_amd, e.g. the
parent commit's), in child processes that take turns over several rounds on the same frames (device and encode_jpeg medians
of the round medians, and their range)."""
import argparse
import io
import json
import os
import statistics
import subprocess
import sys
import time

import torch
from PIL import Image, ImageFile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("R2F_PROBE_PKG", ROOT)  # (--ab: the child of the other build imports its package from here)
sys.path.insert(0, PKG)
from raw2film_amd import HipProcessor, filmstock  # noqa: E402
from raw2film_amd.synthetic import synthetic_frame_device  # noqa: E402

OPTION_SETS = [("4:2:0", 2, False), ("4:2:2", 1, False), ("4:4:4", 0, False), ("4:2:0 optimize", 2, True),
               ("4:4:4 optimize", 0, True)]


def pillow(a, q, s, o):
    ImageFile.MAXBLOCK = max(ImageFile.MAXBLOCK, 24 * a.shape[0] * a.shape[1])  # (optimize: Pillow's buffer must hold the file)
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", quality=q, subsampling=s, optimize=o)
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


def device_ms(encode, reps=7):
    encode()  # (warm: scratch sized)
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        encode()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def options_table(q, say):
    proc = HipProcessor(device=0)
    frames = [(f"{H * W / 1e6:.0f} MP {kind} render", render(proc, H, W, kind)) for H, W in AB_FRAMES for kind in ("noise", "smooth")]
    say(f"{'frame':<22} {'options':<15} {'file MB':>8} {'device':>8} {'encode_jpeg':>11} {'Pillow MB':>9} {'Pillow':>8}  same")
    for name, u8 in frames:
        dev = torch.from_numpy(u8).cuda()
        reps = 3 if u8.shape[0] < 5000 else 1
        for label, s, o in OPTION_SETS:
            d_ms = device_ms(lambda: proc.ctx.jpeg_encode(dev, q, s, o))
            e_ms, got = wall(lambda: proc.encode_jpeg(dev, q, subsampling=s, optimize=o), 5)
            p_ms, want = wall(lambda: pillow(u8, q, s, o), reps)
            say(f"{name:<22} {label:<15} {len(got) / 1e6:8.2f} {d_ms:8.2f} {e_ms:11.2f} {len(want) / 1e6:9.2f} {p_ms:8.1f}  "
                f"{got == want}")
        del dev
    proc.close()


def render(proc, H, W, kind):
    stocks = filmstock.builtin_stocks()
    kw = dict(print_film=stocks["Kodak 2383"], lens_correction=False, frame_width=36, frame_height=24, seed=1)
    src = synthetic_frame_device(H, W, seed=3, kind=kind).cpu().numpy()
    return proc.process(src, stocks["Kodak Portra 400"], 6, 0.4, **kw)


AB_FRAMES = ((4000, 6000), (8192, 12288))


def ab_child(q):
    """One turn of --ab: the default encode of this process's package on the noise renders -> JSON on stdout."""
    proc = HipProcessor(device=0)
    out = {}
    for H, W in AB_FRAMES:
        dev = torch.from_numpy(render(proc, H, W, "noise")).cuda()
        out[f"{H * W / 1e6:.0f} MP"] = (device_ms(lambda: proc.ctx.jpeg_encode(dev, q), reps=9),  # (the parent's signature)
                                        wall(lambda: proc.encode_jpeg(dev, q), 7)[0])
    proc.close()
    print(json.dumps(out))


def ab(q, other, rounds, say):
    builds = [("this tree", ROOT), ("--ab " + os.path.basename(os.path.normpath(other)), os.path.abspath(other))]
    res = {}
    for _ in range(rounds):
        for name, pkg in builds:
            env = dict(os.environ, R2F_PROBE_PKG=pkg)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--ab-child", "--quality", str(q)], env=env,
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f"{name}: {r.stderr[-2000:]}")
            for frame, (d, e) in json.loads(r.stdout.strip().splitlines()[-1]).items():
                res.setdefault((frame, name), ([], []))
                res[(frame, name)][0].append(d)
                res[(frame, name)][1].append(e)
    for (frame, name), (d, e) in res.items():
        say(f"A/B {frame} noise render, 4:2:0  {name:<22} device {statistics.median(d):6.3f} [{min(d):.3f}, {max(d):.3f}]  "
            f"encode_jpeg {statistics.median(e):7.2f} [{min(e):.2f}, {max(e):.2f}]  ({rounds} rounds)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quality", type=int, default=100)
    ap.add_argument("--ab", default=None)
    ap.add_argument("--ab-only", action="store_true")
    ap.add_argument("--ab-child", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    q = args.quality
    if args.ab_child:
        return ab_child(q)
    lines = [f"# tools/jpeg_options_probe.py on {torch.cuda.get_device_name(0)}, quality {q}; times in ms (medians)"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if not args.ab_only:
        options_table(q, say)
    if args.ab:
        ab(q, args.ab, args.rounds, say)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
