"""Streamed JPEG export timing (process_jpeg / process_preloaded_jpeg with stream=True) against the one-piece export (stream=False)
and against streamed process(cache=False), at 24 MP and 101 MP, on renders of the synthetic noise and smooth frames and on a float32
and a uint16 payload, with and without `file` (written into a temporary directory).  Every file is checked to be Pillow's of the
matching pixel call, byte for byte.  Then the one-piece path's tail, split: the encoder plus the 8-byte length read, the file's
device-to-host copy into pinned memory, and the copy into the bytes object.

    python tools/jpeg_stream_probe.py [--out FILE] [--quality 100] [--sizes 24,101]
    python tools/jpeg_stream_probe.py --once        # one warm streamed 101 MP export into a file (for a kernel trace)

Columns (ms, best of --reps): process = process(cache=False) (streamed, pixels back on the host); export = process_jpeg
stream=False, streamed = stream=True returning bytes, +file = the same into a file (one-piece: the bytes written after the call)."""
import argparse
import io
import os
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from raw2film_amd import HipProcessor, filmstock  # noqa: E402
from raw2film_amd.synthetic import synthetic_frame_device  # noqa: E402

SIZES = {24: (4000, 6000), 101: (8192, 12288)}


def pillow(a, q):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", quality=q)
    return buf.getvalue()


def best(fn, reps):
    ts, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), out


def file_bytes(path):
    with open(path, "rb") as f:
        return f.read()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quality", type=int, default=100)
    ap.add_argument("--sizes", default="24,101")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    q, reps = args.quality, args.reps
    stocks = filmstock.builtin_stocks()
    neg, prt = stocks["Kodak Portra 400"], stocks["Kodak 2383"]
    proc = HipProcessor(device=0)
    kw = dict(print_film=prt, lens_correction=False, frame_width=36, frame_height=24, seed=1)
    tmp = tempfile.mkdtemp(prefix="r2f_jpeg_probe_")
    path = os.path.join(tmp, "export.jpg")

    if args.once:
        src = synthetic_frame_device(*SIZES[101], seed=3, kind="noise").cpu().numpy()
        for _ in range(3):  # (warm: code objects, scratch, staging, the torch allocator)
            proc.process_jpeg(src, neg, 6, 0.4, quality=q, stream=True, file=path, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = proc.process_jpeg(src, neg, 6, 0.4, quality=q, stream=True, file=path, **kw)
        torch.cuda.synchronize()
        print(f"one streamed 101 MP export into a file: {n / 1e6:.2f} MB in {(time.perf_counter() - t0) * 1e3:.1f} ms")
        os.remove(path)
        os.rmdir(tmp)
        proc.close()
        return

    lines = [f"# tools/jpeg_stream_probe.py on {torch.cuda.get_device_name(0)}, quality {q}; times in ms (best of {reps})"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"{'frame':<30} {'file MB':>8} {'process':>8} {'export':>8} {'+file':>8} {'streamed':>9} {'+file':>8}  same bytes "
        "(one-piece, streamed)")
    tails = []
    for mp in (int(s) for s in args.sizes.split(",")):
        H, W = SIZES[mp]
        rows = []
        for kind in ("noise", "smooth"):
            rows.append((f"{mp} MP render of {kind} frame", "array", synthetic_frame_device(H, W, seed=3, kind=kind).cpu().numpy()))
        f32 = rows[0][2]
        rows.append((f"{mp} MP float32 payload", "payload",
                     proc.extract_image_data_cpu(f32, lens_correction=False, frame_width=36, frame_height=24)))
        raw = (np.clip(f32, 0, 1) * 65535).astype(np.uint16)
        rows.append((f"{mp} MP uint16 payload", "payload",
                     proc.extract_image_data_cpu(raw, lens_correction=False, frame_width=36, frame_height=24, exposure=0.5)))
        pre = {k: v for k, v in kw.items() if k not in ("lens_correction", "frame_width", "frame_height")}
        for name, kind, src in rows:
            if kind == "array":
                pix = lambda: proc.process(src, neg, 6, 0.4, cache=False, **kw)  # noqa: E731
                exp = lambda **x: proc.process_jpeg(src, neg, 6, 0.4, quality=q, **kw, **x)  # noqa: E731
            else:
                pix = lambda: proc.process_preloaded(src, neg, 6, 0.4, **pre)  # noqa: E731
                exp = lambda **x: proc.process_preloaded_jpeg(src, neg, 6, 0.4, quality=q, **pre, **x)  # noqa: E731
            pix()
            p_ms, px = best(pix, reps)
            want = pillow(np.array(px), q)  # (the streamed render's pixels)
            proc.stream_bands = 0  # stream=False renders in one piece: its file is Pillow's of the one-piece pixels
            want_one = pillow(np.array(pix()), q)
            proc.stream_bands = 16
            exp(stream=True)  # (warm)

            def one_piece_file():
                with open(path, "wb") as f:
                    f.write(exp())

            e_ms, got_e = best(exp, reps)
            ef_ms, _ = best(one_piece_file, reps)
            same_one = got_e == want_one and file_bytes(path) == want_one
            proc.stream_rejected = "not asked"
            s_ms, got_s = best(lambda: exp(stream=True), reps)
            streamed = proc.stream_rejected is None
            sf_ms, _ = best(lambda: exp(stream=True, file=path), reps)
            same = got_s == want and file_bytes(path) == want
            say(f"{name:<30} {len(want) / 1e6:8.2f} {p_ms:8.1f} {e_ms:8.1f} {ef_ms:8.1f} {s_ms:9.1f} {sf_ms:8.1f}  {same_one} {same}"
                + ("" if streamed else f"  (did not stream: {proc.stream_rejected})"))
            if kind == "array":
                tails.append((name, proc.last_output.clone()))
    os.remove(path)
    os.rmdir(tmp)

    say("")
    say("one-piece path's tail from a device frame (encode_jpeg): encoder + length read, device-to-host copy, bytes object")
    say(f"{'frame':<30} {'file MB':>8} {'enc+sync':>9} {'D2H':>7} {'tobytes':>8} {'total':>7}")
    for name, dev in tails:
        out, length = proc.ctx.jpeg_encode(dev, q)  # (warm: scratch sized)
        n = int(length.item())
        host = torch.empty(n, dtype=torch.uint8, pin_memory=True)
        ts = {"enc": [], "d2h": [], "bytes": []}
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out, length = proc.ctx.jpeg_encode(dev, q)
            n = int(length.item())
            t1 = time.perf_counter()
            host[:n].copy_(out[:n])
            t2 = time.perf_counter()
            b = host[:n].numpy().tobytes()
            t3 = time.perf_counter()
            ts["enc"].append((t1 - t0) * 1e3)
            ts["d2h"].append((t2 - t1) * 1e3)
            ts["bytes"].append((t3 - t2) * 1e3)
            del b
        e, d, c = (min(ts[k]) for k in ("enc", "d2h", "bytes"))
        say(f"{name:<30} {n / 1e6:8.2f} {e:9.2f} {d:7.2f} {c:8.2f} {e + d + c:7.2f}")
        del host
    proc.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
