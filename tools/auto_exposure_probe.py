"""What the auto exposure of the uint16 hand-off costs, on the host and on the device (profiles/r10_auto_exposure_probe.txt).

    python tools/auto_exposure_probe.py [--out FILE] [--repeats N] [--ab DIR [--rounds R]]

For a 24 MP and a 100 MP uint16 frame, in pageable and in pinned host memory, interleaved over N repeats (ranges, not single
figures):
  host measurement alone      decode.auto_exposure(frame, metadata)  -- the single-threaded NumPy pass of exposure=None
  process, host mode          process(u16, metadata=md, cache=False)
  process, device mode        process(u16, metadata=md, exposure="device", cache=False)
  process, stops given        process(u16, exposure=<stops>, cache=False)                 -- the floor: no measurement at all
  row statistic + finish      device time of r2f_exposure_rows over the whole frame and of r2f_exposure_finish (events)
  copy ceiling                the streaming copy kernel over the bytes the row kernel reads, in the same run; the upload of the frame
--ab DIR: the host-mode call of another checkout (DIR holds a built tree of it, e.g. the parent commit's), in child processes of
its own that import its package and load its library; the same child of this tree runs in turn with it, R rounds of each.
Needs a GPU: there is no CPU path.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("R2F_PROBE_PKG", ROOT)  # (--ab: the child of the other checkout imports its package from here)
if PKG not in sys.path:
    sys.path.insert(0, PKG)

META = {"EXIF:FNumber": 5.6, "EXIF:ISO": 200, "EXIF:ExposureTime": 1 / 125}
SIZES = (("24 MP", 4000, 6000), ("100 MP", 8192, 12288))


def spread(xs):
    return f"{min(xs):8.2f} .. {max(xs):8.2f} ms (median {statistics.median(xs):8.2f}, n = {len(xs)})"


def make_frame(H, W):
    rng = np.random.default_rng(H)
    return (rng.random((H, W, 3), dtype=np.float32) ** 3 * 40000).astype(np.uint16)


def render_kw(prt, H, W):
    fw = max(36.0, W / 341.0)  # ~341 px/mm at most (below max_scale), the frame kept whole
    return dict(print_film=prt, lens_correction=False, seed=5, cache=False, frame_width=fw, frame_height=fw * H / W,
                halation_green_factor=0.3)


def ab_child(repeats):
    """One turn of --ab: process(u16, metadata=md) in host mode with this process's package -> JSON on stdout.  Only calls that the
    other checkout has too."""
    import torch

    from raw2film_amd import HipProcessor, filmstock

    stocks = filmstock.builtin_stocks()
    neg, prt = stocks["Kodak Portra 400"], stocks["Kodak 2383"]
    proc = HipProcessor(device=0, result_buffers=2)
    out = {}
    for label, H, W in SIZES:
        pageable = make_frame(H, W)
        pinned = torch.from_numpy(pageable.view(np.int16)).pin_memory().numpy().view(np.uint16)
        kw = render_kw(prt, H, W)
        times = {"pageable": [], "pinned": []}
        for r in range(repeats + 1):
            for memory, frame in (("pageable", pageable), ("pinned", pinned)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = proc.process(frame, neg, 6, 0.4, metadata=META, **kw)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                del res
                if r:
                    times[memory].append(dt)
        for memory, xs in times.items():
            out[f"{label}, {memory}"] = xs
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
    emit(f"A/B of process(u16, metadata=md) in host mode: each build's own package and library in child processes of its own, "
         f"{rounds} rounds in turn, {repeats} calls after a warm-up in each")
    for (case, name), xs in sorted(res.items()):
        emit(f"  {case:<18s} {name:<22s} {spread(xs)}")
    emit()


def main():
    import torch

    from raw2film_amd import HipProcessor, decode, filmstock

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_auto_exposure_probe.txt"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--ab", default=None, help="a built checkout of another commit (the parent's) for the host-mode A/B")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ab-child", action="store_true")
    args = ap.parse_args()
    if args.ab_child:
        return ab_child(args.repeats)
    if not torch.cuda.is_available():
        raise SystemExit("auto_exposure_probe needs a GPU")
    stocks = filmstock.builtin_stocks()
    neg, prt = stocks["Kodak Portra 400"], stocks["Kodak 2383"]
    proc = HipProcessor(device=0, result_buffers=2)
    lines = [f"auto exposure of the uint16 hand-off: host pass against device kernels ({torch.cuda.get_device_name(0)})",
             f"full render (halation, MTF, grain, print film), cache=False, result_buffers=2, metadata root "
             f"{decode.exposure_root(META):.3f}; {args.repeats} interleaved repeats after one warm-up round; wall clock around the call",
             ""]

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    for label, H, W in SIZES:
        pageable = make_frame(H, W)
        pinned_t = torch.from_numpy(pageable.view(np.int16)).pin_memory()
        pinned = pinned_t.numpy().view(np.uint16)
        kw = render_kw(prt, H, W)
        stops = decode.auto_exposure(pageable, metadata=META)
        for memory, frame in (("pageable", pageable), ("pinned", pinned)):
            legs = {"host measurement alone": lambda: decode.auto_exposure(frame, metadata=META),
                    "process, host mode": lambda: proc.process(frame, neg, 6, 0.4, metadata=META, **kw)}
            legs['process, exposure="device"'] = lambda: proc.process(frame, neg, 6, 0.4, metadata=META, exposure="device", **kw)
            legs["process, stops given (floor)"] = lambda: proc.process(frame, neg, 6, 0.4, exposure=stops, **kw)
            times = {k: [] for k in legs}
            for r in range(args.repeats + 1):
                for k, fn in legs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = fn()
                    torch.cuda.synchronize()
                    dt = (time.perf_counter() - t0) * 1e3
                    del out
                    if r:
                        times[k].append(dt)
            emit(f"{label} ({H} x {W} x 3 uint16, {pageable.nbytes / 1e6:.0f} MB), {memory} source; streamed: "
                 f"{proc.stream_rejected is None}")
            for k, xs in times.items():
                emit(f"  {k:<44s} {spread(xs)}")
            emit(f"  device-measured stops {proc.last_auto_exposure!r}, host-measured {stops!r}")
        # the kernels alone, on the frame already on the device, next to the copy ceiling of the same run
        ctx = proc.ctx
        dev = pinned_t.cuda()
        root = decode.exposure_root(META)
        read_bytes = (H + 1) // 2 * W * 3 * 2  # the even rows, every byte of them
        n16 = read_bytes // 16 * 16
        a = torch.empty(n16, dtype=torch.uint8, device="cuda")
        b = torch.empty(n16, dtype=torch.uint8, device="cuda")
        t_rows, t_fin, t_copy, t_up = [], [], [], []
        for r in range(args.repeats + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
            ev[0].record()
            ctx.exposure_rows(dev, root)
            ev[1].record()
            ctx.exposure_finish(H, W, root)
            ev[2].record()
            ctx.stream_copy(a, b)
            ev[3].record()
            ev[4].record()
            dev.copy_(pinned_t, non_blocking=True)
            ev[5].record()
            torch.cuda.synchronize()
            if r:
                t_rows.append(ev[0].elapsed_time(ev[1]))
                t_fin.append(ev[1].elapsed_time(ev[2]))
                t_copy.append(ev[2].elapsed_time(ev[3]))
                t_up.append(ev[4].elapsed_time(ev[5]))
        emit(f"{label}: kernels alone (device events)")
        emit(f"  row statistic, whole frame                   {spread(t_rows)}   reads {read_bytes / 1e6:.0f} MB: "
             f"{read_bytes / 1e9 / (statistics.median(t_rows) / 1e3):.0f} GB/s")
        emit(f"  finish                                       {spread(t_fin)}")
        emit(f"  streaming copy of the same bytes             {spread(t_copy)}   {2 * n16 / 1e9 / (statistics.median(t_copy) / 1e3):.0f} GB/s "
             f"moved (read + write)")
        emit(f"  upload of the frame (pinned)                 {spread(t_up)}   {pageable.nbytes / 1e9 / (statistics.median(t_up) / 1e3):.1f} GB/s")
        emit()
        del dev, a, b
    proc.close()  # (the children open the GPU one at a time, after this process has let go of its buffers)
    if args.ab:
        ab(args.ab, args.rounds, args.repeats, emit)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
