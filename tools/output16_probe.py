"""What the 16-bit output side costs next to the 8-bit one (profiles/r11_output16_probe.txt).

    python tools/output16_probe.py [--out FILE] [--repeats N] [--ab DIR [--rounds R]] [--commit TEXT]

For a 24 MP and a 100 MP float frame in pinned host memory, interleaved over N repeats after a warm-up round (ranges, not single
figures):
  (a) process(host array, cache=False) at 8 bits -- with --ab DIR also in child processes of another checkout (DIR holds a built
      tree of it, e.g. the parent commit's) that import its package and load its library, in turn with the same child of this tree
  (b) the same call with output_bits=16, and the download of 6 B/px alone (its floor beside the upload)
  (c) device time of the tail kernel with uint8, uint16 and float stores (events around the eager stage calls: r2f_kernel_timing
      counts the FFT passes only), at the frame's W and at W - 2 (rows of a wave at different store phases); the LUTs-only pointwise
      pass at 8 bits (the LDS front kernel) and at 16 (the generic one); the LANCZOS4 way back at 8 and at 16 bits
  (d) r2f_render16 against r2f_render(want_f32) + a torch quantise pass, device to device
  (e) process_tiff(file=...) at 16 bits in one piece and streamed
Needs a GPU: there is no CPU path.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("R2F_PROBE_PKG", ROOT)  # (--ab: the child of the other checkout imports its package from here)
if PKG not in sys.path:
    sys.path.insert(0, PKG)

SIZES = (("24 MP", 4000, 6000), ("100 MP", 8192, 12288))


def spread(xs):
    return f"{min(xs):8.2f} .. {max(xs):8.2f} ms (median {statistics.median(xs):8.2f}, n = {len(xs)})"


def make_frame(torch, H, W):
    """A float32 XYZ-like frame in pinned memory (a small random tile repeated: the generator is not what is measured)."""
    rng = np.random.default_rng(H)
    tile = (rng.random((256, 256, 3), dtype=np.float32) ** 2 * 1.2).astype(np.float32)
    t = torch.empty((H, W, 3), dtype=torch.float32).pin_memory()
    a = t.numpy()
    a[...] = np.tile(tile, (H // 256 + 1, W // 256 + 1, 1))[:H, :W]
    return t, a


def render_kw(prt, H, W):
    fw = max(36.0, W / 341.0)  # ~341 px/mm at most (below max_scale), the frame kept whole
    return dict(print_film=prt, lens_correction=False, seed=5, cache=False, frame_width=fw, frame_height=fw * H / W,
                halation_green_factor=0.3)


def wall(torch, legs, repeats):
    """Every leg in turn, `repeats` times after one untimed round; wall clock with a synchronisation on both sides."""
    times = {k: [] for k in legs}
    for r in range(repeats + 1):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            del out
            if r:
                times[k].append(dt)
    return times


def device(torch, legs, repeats):
    """Every leg in turn between two events on the launch stream."""
    times = {k: [] for k in legs}
    for r in range(repeats + 1):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r:
                times[k].append(e0.elapsed_time(e1))
    return times


def ab_child(repeats):
    """One turn of --ab: process(host array, cache=False) at 8 bits with this process's package -> JSON on stdout.  Only calls that
    the other checkout has too."""
    import torch

    from raw2film_amd import HipProcessor, filmstock

    stocks = filmstock.builtin_stocks()
    neg, prt = stocks["Kodak Portra 400"], stocks["Kodak 2383"]
    proc = HipProcessor(device=0)
    out = {}
    for label, H, W in SIZES:
        _, frame = make_frame(torch, H, W)
        kw = render_kw(prt, H, W)
        out[label] = wall(torch, {"p": lambda: proc.process(frame, neg, 6, 0.4, **kw)}, repeats)["p"]
    proc.close()
    print(json.dumps(out))


def ab(other, rounds, repeats, emit):
    builds = [("this tree", ROOT), ("--ab " + os.path.basename(os.path.normpath(other)), os.path.abspath(other))]
    res = {}
    for _ in range(rounds):
        for name, pkg in builds:
            env = dict(os.environ, R2F_PROBE_PKG=pkg)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--ab-child", "--repeats", str(repeats)], env=env,
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f"{name}: exit {r.returncode}: {r.stderr[-2000:]}")
            for case, xs in json.loads(r.stdout.strip().splitlines()[-1]).items():
                res.setdefault((case, name), []).extend(xs)
    emit(f"(a) process(host array, cache=False) at 8 bits: each build's own package and library in child processes of its own, "
         f"{rounds} rounds in turn, {repeats} calls after a warm-up in each")
    for (case, name), xs in sorted(res.items()):
        emit(f"  {case:<8s} {name:<22s} {spread(xs)}")
    for case in sorted({c for c, _ in res}):
        (_, a), (_, b) = [(n, xs) for (c, n), xs in sorted(res.items()) if c == case]
        emit(f"  {case}: the two ranges {'overlap' if max(min(a), min(b)) <= min(max(a), max(b)) else 'DO NOT overlap'}")
    emit()


def main():
    import torch

    from raw2film_amd import HipProcessor, _lib, filmstock

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_output16_probe.txt"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--ab", default=None, help="a built checkout of another commit (the parent's) for row (a)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--commit", default="", help="what the file says it was measured at")
    ap.add_argument("--ab-child", action="store_true")
    args = ap.parse_args()
    if args.ab_child:
        return ab_child(args.repeats)
    if not torch.cuda.is_available():
        raise SystemExit("output16_probe needs a GPU")
    stocks = filmstock.builtin_stocks()
    neg, prt = stocks["Kodak Portra 400"], stocks["Kodak 2383"]
    proc = HipProcessor(device=0)
    ctx = proc.ctx
    lines = [f"the 16-bit output side next to the 8-bit one ({torch.cuda.get_device_name(0)}){'; ' + args.commit if args.commit else ''}",
             f"full render (halation, MTF, grain, print film) unless stated, float32 frame in pinned host memory; {args.repeats} "
             "interleaved repeats after one warm-up round; wall clock around the call, or device events where it says so", ""]

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def rows(times, notes=None):
        for k, xs in times.items():
            emit(f"  {k:<58s} {spread(xs)}{(notes or {}).get(k, '')}")

    tmp = tempfile.mkdtemp(prefix="r2f_probe_")
    for label, H, W in SIZES:
        pinned_t, frame = make_frame(torch, H, W)
        kw = render_kw(prt, H, W)
        px = H * W
        emit(f"{label} ({H} x {W} x 3 float32, {frame.nbytes / 1e6:.0f} MB up; result {3 * px / 1e6:.0f} MB at 8 bits, {6 * px / 1e6:.0f} MB at 16)")
        # (a) in this process, (b)
        res16 = torch.empty((H, W, 3), dtype=torch.int16).pin_memory()
        dev16 = torch.empty((H, W, 3), dtype=torch.int16, device="cuda")
        t = wall(torch, {"(a) process, 8 bits": lambda: proc.process(frame, neg, 6, 0.4, **kw),
                         "(b) process, output_bits=16": lambda: proc.process(frame, neg, 6, 0.4, output_bits=16, **kw),
                         "(b) download of 6 B/px alone (pinned)": lambda: res16.copy_(dev16, non_blocking=True)}, args.repeats)
        med = statistics.median(t["(b) download of 6 B/px alone (pinned)"])
        rows(t, {"(b) download of 6 B/px alone (pinned)": f"   {6 * px / 1e9 / (med / 1e3):.1f} GB/s"})
        emit(f"  streamed: {proc.stream_rejected is None}")
        # (e)
        path = os.path.join(tmp, "probe.tif")
        t = wall(torch, {"(e) process_tiff(file), 16 bits, one piece": lambda: proc.process_tiff(frame, neg, 6, 0.4, path, **kw),
                         "(e) process_tiff(file), 16 bits, stream=True": lambda: proc.process_tiff(frame, neg, 6, 0.4, path, stream=True, **kw)},
                 args.repeats)
        rows(t)
        emit(f"  file of {os.path.getsize(path) / 1e6:.0f} MB in the temporary directory; streamed: {proc.stream_rejected is None}")
        os.remove(path)
        # (d) device to device
        img = pinned_t.cuda()
        params = proc.prepare(neg, 6, 0.4, (W, H), **{k: v for k, v in kw.items() if k not in ("lens_correction", "cache")})
        f32 = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")

        def quantised():
            ctx.render(img, params, out_f32=f32)
            return (f32 * 65535.0).clamp_(0.0, 65535.0).to(torch.int32).to(torch.int16)

        t = device(torch, {"(d) r2f_render16": lambda: ctx.render16(img, params, out_u16=dev16),
                           "(d) r2f_render(want_f32) + torch quantise": quantised,
                           "(d) r2f_render(want_f32) alone": lambda: ctx.render(img, params, out_f32=f32)}, args.repeats)
        emit("  device events, frame on the device, result left there:")
        rows(t)
        # (c) the tail kernel per store form
        for Wc in (W, W - 2):
            dens = torch.rand((3, H, Wc), dtype=torch.float32, device="cuda") * 3.0
            o8 = torch.empty((H, Wc, 3), dtype=torch.uint8, device="cuda")
            o16 = torch.empty((H, Wc, 3), dtype=torch.int16, device="cuda")
            o32 = torch.empty((H, Wc, 3), dtype=torch.float32, device="cuda")
            g = dict(y0=0, y1=H, H_global=H)
            t = device(torch, {f"(c) tail, uint8 stores, W = {Wc}": lambda: ctx.stage_tail(dens, params, out_u8=o8, **g),
                               f"(c) tail, uint16 stores, W = {Wc}": lambda: ctx.stage_tail16(dens, params, out_u16=o16, **g),
                               f"(c) tail, float stores, W = {Wc}": lambda: ctx.stage_tail(dens, params, out_f32=o32, **g)}, args.repeats)
            rows(t, {k: f"   writes {b * H * Wc / 1e6:.0f} MB" for k, b in zip(t, (3, 6, 12))})
            del dens, o8, o16, o32
        # (c) the LUTs-only pointwise pass, the LANCZOS4 way back
        flat = proc.prepare(neg, 6, 0.4, (W, H), halation=False, sharpness=False, grain=0,
                            **{k: v for k, v in kw.items() if k not in ("lens_correction", "cache")})
        o8 = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
        t = device(torch, {"(c) LUTs only, stage_front -> uint8 (LDS front kernel)": lambda: ctx.stage_front(img, flat, _lib.UPTO_OUTPUT, out_u8=o8),
                           "(c) LUTs only, stage_front16 -> uint16 (generic kernel)": lambda: ctx.stage_front16(img, flat, out_u16=dev16)},
                   args.repeats)
        rows(t)
        sh, sw = round(H * 0.6), round(W * 0.6)
        s8, s16 = o8[:sh, :sw].contiguous(), dev16[:sh, :sw].contiguous()
        t = device(torch, {f"(c) LANCZOS4 {sh} x {sw} -> {H} x {W}, uint8": lambda: ctx.resize_lanczos4_u8(s8, H, W),
                           f"(c) LANCZOS4 {sh} x {sw} -> {H} x {W}, uint16": lambda: ctx.resize_lanczos4_u16(s16, H, W)}, args.repeats)
        rows(t)
        emit()
        del img, f32, o8, dev16, res16, s8, s16, pinned_t, frame
        torch.cuda.empty_cache()
    os.rmdir(tmp)
    proc.close()  # (the children open the GPU one at a time, after this process has let go of its buffers)
    if args.ab:
        ab(args.ab, args.rounds, args.repeats, emit)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
