"""One SHA-256 per output path of HipProcessor, at 8 and at 16 bits: the bit-equality check of a change to the Python output side.

    python tools/output_paths_digest.py [--times FILE] [--group prepath] > digest.txt

Every case renders a seeded synthetic frame through the public API only and prints `<case> <dtype> <shape> <sha256>` -- for a file
its length in place of dtype and shape.  Run it on two commits, each in a process of its own, and compare the outputs line for
line.  Non-streamed cases use 96 x 160 and 70 x 257 frames (the odd width takes the 2- and 4-byte edge stores of the uint16
output); streamed cases use 2368 x 2368 x 3, just above the 2 ** 24 samples the gate admits, in four bands, so that the taper and
the stencil lag are exercised; the streamed Bayer mosaics (raw_profile=, stops given) are 2400 x 2368 at full size and 4800 x 4736 at
half size, of which the square format keeps that window.  A streamed case whose frame did not stream prints `stream_rejected` in
place of a digest (one case is made for that: the host gate passes, a preview resolution then keeps the payload from streaming).
The `prepath` group renders the small frames through what runs ahead of the pipeline: the crops and quarter turns, the free
rotation, exposure="device", a LensProfile, a RawProfile mosaic at full and half size, both together, the two-phase API and the
exports of such frames, and one encode_jpeg call with every JPEG keyword set.
--times FILE: wall clock of every case in ms (its first call, tables and allocations included, and a second one), kept out of
the digest."""

from __future__ import annotations

import argparse
import hashlib
import io
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SMALL = ((96, 160), (70, 257))
BIG = 2368
TIMES = []


def digest(name, value):
    if isinstance(value, (bytes, bytearray)):
        print(f"{name} file {len(value)} {hashlib.sha256(value).hexdigest()}", flush=True)
        return
    a = np.ascontiguousarray(value)
    print(f"{name} {a.dtype} {'x'.join(map(str, a.shape))} {hashlib.sha256(a.tobytes()).hexdigest()}", flush=True)


def timed(name, fn, repeat=False):
    t0 = time.perf_counter()
    res = fn()
    t1 = time.perf_counter()
    if repeat:  # (a case whose result does not depend on what ran before: the second call is the steady state)
        fn()
    TIMES.append((name, (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3 if repeat else None))
    return res


def small_cases(proc, torch, neg, prt):
    from raw2film_amd.synthetic import synthetic_frame

    for H, W in SMALL:
        frame = synthetic_frame(H, W, seed=H + W)
        geom = dict(frame_width=36.0 * W / 6000.0, frame_height=36.0 * W / 6000.0 * H / W, lens_correction=False)
        film = dict(print_film=prt, seed=20260630, exp_kelvin=6000, color_masking=1.0, halation_green_factor=0.3)
        kw = dict(geom, **film)
        for bits in (8, 16):
            tag = f"{H}x{W}/{bits}"
            case = lambda name, fn: digest(f"{name} {tag}", timed(f"{name} {tag}", fn))  # noqa: E731
            b = dict(output_bits=bits)
            case("process_cached_first", lambda: proc.process(frame, neg, 6, 0.4, **kw, **b))
            case("process_cached_rerender", lambda: proc.process(frame, neg, 6, 0.4, exp_comp=0.5, **kw, **b))
            case("process_uncached", lambda: proc.process(frame, neg, 6, 0.4, cache=False, **kw, **b))
            digest(f"last_output {tag}", proc.last_output.view(torch.int16 if bits == 16 else torch.uint8).cpu().numpy())
            digest(f"histogram {tag}", proc.generate_histogram())
            payload = proc.extract_image_data_cpu(frame, **geom)
            for fs in ("gpu", "cpu"):
                case(f"process_preloaded_{fs}", lambda: proc.process_preloaded(payload, neg, 6, 0.4, final_scaling=fs, **kw, **b))
                shrunk = dict(payload, final_resolution=(H // 2, W // 2))  # "cpu": INTER_AREA on the finished frame
                case(f"process_preloaded_{fs}_shrunk", lambda: proc.process_preloaded(shrunk, neg, 6, 0.4, final_scaling=fs, **kw, **b))
            case("submit_preloaded", lambda: proc.submit_preloaded(payload, neg, 6, 0.4, final_scaling="cpu", **kw, **b).result())
            case("process_array_host", lambda: proc.process_array(frame, neg, 6, 0.4, colorspace="linear-rec709", **film, **b,
                                                                  frame_width=geom["frame_width"], frame_height=geom["frame_height"]))
            dev = proc.process_array(frame, neg, 6, 0.4, colorspace="linear-rec709", output="device", **film, **b,
                                     frame_width=geom["frame_width"], frame_height=geom["frame_height"])
            digest(f"process_array_device {tag}", dev.view(torch.int16 if bits == 16 else torch.uint8).cpu().numpy())
            for mode in ("Uniform white", "Proportional black", "Fixed"):
                canvas = dict(canvas_mode=mode, canvas_scale=1.25, canvas_ratio=1.4)
                # process() scales the canvas-framed frame back to the frame's own size: INTER_AREA; "gpu" keeps the canvas
                case(f"canvas_{mode.replace(' ', '_')}", lambda: proc.process(frame, neg, 6, 0.4, **kw, **canvas, **b))
                case(f"canvas_{mode.replace(' ', '_')}_preloaded_gpu", lambda: proc.process_preloaded(
                    proc.extract_image_data_cpu(frame, **geom, **canvas), neg, 6, 0.4, final_scaling="gpu", **kw, **canvas, **b))
            # the pipeline runs at 0.6 x and the result goes back up through LANCZOS4
            case("max_scale_round_trip", lambda: proc.process(frame, neg, 6, 0.4, max_scale=0.6 * W / geom["frame_width"], **kw, **b))
            case("preview_resolution", lambda: proc.process(frame, neg, 6, 0.4, resolution=(H // 2, W // 2), **kw, **b))
            case("process_tiff", lambda: proc.process_tiff(frame, neg, 6, 0.4, icc_profile=b"an odd profile.", **kw, **b))
            case("process_tiff_stream_rejected", lambda: proc.process_tiff(frame, neg, 6, 0.4, stream=True, **kw, **b))
            buf = io.BytesIO()
            proc.process_preloaded_tiff(payload, neg, 6, 0.4, buf, final_scaling="cpu", **kw, **b)
            digest(f"process_preloaded_tiff {tag}", buf.getvalue())
        case = lambda name, fn: digest(f"{name} {H}x{W}", timed(f"{name} {H}x{W}", fn))  # noqa: E731
        case("process_jpeg", lambda: proc.process_jpeg(frame, neg, 6, 0.4, 90, **kw))
        case("process_jpeg_stream_rejected", lambda: proc.process_jpeg(frame, neg, 6, 0.4, 90, stream=True, subsampling=0, **kw))
        case("process_preloaded_jpeg", lambda: proc.process_preloaded_jpeg(payload, neg, 6, 0.4, 90, final_scaling="cpu", optimize=True, **kw))


def prepath_cases(proc, torch, neg, prt):
    from raw2film_amd.lens import LensProfile
    from raw2film_amd.raw import RawProfile
    from raw2film_amd.synthetic import synthetic_frame

    lens = LensProfile("ptlens", (0.02, -0.06, 0.01), vignetting=(-0.3, 0.1, -0.02), center=(0.01, -0.006))
    raw = RawProfile("GRBG", black=(64, 60, 66, 64), multipliers=(2.1, 1.0, 1.6),
                     matrix=((1.62, -0.41, -0.19), (-0.28, 1.52, -0.22), (0.04, -0.52, 1.49)))
    film = dict(print_film=prt, seed=20260630, exp_kelvin=6000, color_masking=1.0, halation_green_factor=0.3)
    shapes = {"plain": {}, "zoomed_turned": dict(zoom=1.3, rotate_times=3), "rotated": dict(rotation=3.5, zoom=1.3, rotate_times=1)}
    for H, W in SMALL:
        tag = f"{H}x{W}"
        case = lambda name, fn: digest(f"prepath_{name} {tag}", timed(f"prepath_{name} {tag}", fn, repeat=True))  # noqa: E731
        frame = synthetic_frame(H, W, seed=H + W)
        u16 = np.ascontiguousarray((np.clip(frame, 0.0, 1.0) * 40000.0).astype(np.uint16))
        # a frame wider than the film format, so that the aspect crop cuts columns (and rows when flipped)
        kw = dict(film, frame_width=36.0 * W / 6000.0, frame_height=36.0 * W / 6000.0 * H / W * 1.1)
        for name, src, extra in (("f32", frame, {}), ("u16", u16, dict(exposure=0.5))):
            for shape, g in shapes.items():
                case(f"{name}_{shape}", lambda: proc.process(src, neg, 6, 0.4, cache=False, **g, **extra, **kw))
            case(f"{name}_flip", lambda: proc.process(src, neg, 6, 0.4, cache=False, flip=True, **extra, **kw))
        case("u16_device_exposure", lambda: proc.process(u16, neg, 6, 0.4, cache=False, exposure="device", zoom=1.3, **kw))
        print(f"prepath_u16_device_exposure_stops {tag} {proc.last_auto_exposure!r}", flush=True)
        case("u16_device_exposure_turned", lambda: proc.process(u16, neg, 6, 0.4, cache=False, exposure="device", rotate_times=1, **kw))
        print(f"prepath_u16_device_exposure_turned_rejected {tag} {proc.exposure_rejected!r}", flush=True)
        rng = np.random.default_rng(H * 1000 + W)
        mosaics = {"mosaic_full": (rng.integers(0, 40000, (H, W), dtype=np.uint16), False),
                   "mosaic_half": (rng.integers(0, 40000, (2 * H, 2 * W), dtype=np.uint16), True)}
        steps = [("lens", frame, dict(lens_profile=lens)), ("lens_u16", u16, dict(lens_profile=lens, exposure=0.5))]
        for name, (mosaic, half) in mosaics.items():
            steps.append((name, mosaic, dict(raw_profile=raw, half_size=half, exposure=0.5)))
            steps.append((name + "_lens", mosaic, dict(raw_profile=raw, half_size=half, exposure=0.5, lens_profile=lens)))
        for name, src, extra in steps:
            for shape, g in shapes.items():
                case(f"{name}_{shape}", lambda: proc.process(src, neg, 6, 0.4, cache=False, **g, **extra, **kw))
            load = {k: v for k, v in dict(kw, **extra, zoom=1.3, rotate_times=3).items() if k not in film}
            payload = proc.extract_image_data_cpu(src, **load)
            for fs in ("gpu", "cpu"):
                case(f"{name}_preloaded_{fs}", lambda: proc.process_preloaded(payload, neg, 6, 0.4, final_scaling=fs, **film, **load))
        case("lens_u16_device_exposure", lambda: proc.process(u16, neg, 6, 0.4, cache=False, exposure="device", zoom=1.3, lens_profile=lens, **kw))
        for name, (mosaic, half) in mosaics.items():  # (a mosaic without stops is measured on the device)
            case(f"{name}_device_exposure", lambda: proc.process(mosaic, neg, 6, 0.4, cache=False, raw_profile=raw, half_size=half, zoom=1.3, **kw))
        case("lens_cached_rerender", lambda: (proc.process(frame, neg, 6, 0.4, lens_profile=lens, zoom=1.3, **kw),
                                              proc.process(frame, neg, 6, 0.4, lens_profile=lens, zoom=1.3, exp_comp=0.5, **kw))[1])
        case("lens_chroma_nr_preview", lambda: proc.process(frame, neg, 6, 0.4, cache=False, lens_profile=lens, rotation=3.5, chroma_nr=3,
                                                            resolution=(H // 2, W // 2), **kw))
        case("lens_process_jpeg", lambda: proc.process_jpeg(frame, neg, 6, 0.4, 90, lens_profile=lens, zoom=1.3, rotate_times=3, **kw))
        for bits in (8, 16):
            case(f"lens_process_tiff_{bits}", lambda: proc.process_tiff(frame, neg, 6, 0.4, output_bits=bits, lens_profile=lens,
                                                                         rotation=3.5, zoom=1.3, rotate_times=1, **kw))
        image = proc.process(frame, neg, 6, 0.4, **kw)
        case("encode_jpeg_every_keyword", lambda: proc.encode_jpeg(
            image, 83, subsampling="4:2:2", optimize=True, exif=b"Exif\x00\x00II*\x00\x08\x00\x00\x00\x00\x00\x00\x00\x00\x00", progressive=False,
            icc_profile=b"an odd profile.", xmp=b"<x:xmpmeta/>", comment="a comment", dpi=(300, 299.6), restart_marker_blocks=7,
            restart_marker_rows=1))
        case("encode_jpeg_progressive", lambda: proc.encode_jpeg(image, 83, subsampling=0, progressive=True, icc_profile=b"icc", dpi=(72, 72)))


def streamed_cases(proc, torch, neg, prt):
    from raw2film_amd.raw import RawProfile
    from raw2film_amd.synthetic import synthetic_frame

    small = synthetic_frame(BIG // 8, BIG // 8, seed=8)
    ramp = np.linspace(0.5, 1.5, BIG, dtype=np.float32)[None, :, None]
    pageable = np.ascontiguousarray(np.kron(small, np.ones((8, 8, 1), np.float32)) * ramp)
    pinned_t = torch.from_numpy(pageable).pin_memory()
    pinned = pinned_t.numpy()
    u16 = np.ascontiguousarray((np.clip(pageable, 0.0, 1.0) * 40000.0).astype(np.uint16))
    geom = dict(frame_width=36.0, frame_height=36.0, lens_correction=False)
    film = dict(print_film=prt, seed=20260630, exp_kelvin=6000, color_masking=1.0, halation_green_factor=0.3)
    stencils_on = dict(geom, **film)  # halation, MTF and grain: the stencil lag of the band loop
    pointwise = dict(stencils_on, grain=0, halation=False, sharpness=False)  # LUTs only: the front kernel writes the result
    raw = RawProfile("GRBG", black=(64, 60, 66, 64), multipliers=(2.1, 1.0, 1.6),
                     matrix=((1.62, -0.41, -0.19), (-0.28, 1.52, -0.22), (0.04, -0.52, 1.49)))
    rng = np.random.default_rng(BIG)
    mosaics = {"mosaic_full": (rng.integers(0, 40000, (BIG + 32, BIG), dtype=np.uint16), False),
               "mosaic_half": (rng.integers(0, 40000, (2 * BIG + 64, 2 * BIG), dtype=np.uint16), True)}
    proc.stream_bands = 4

    def streamed(name, fn, repeat=True):
        proc.stream_rejected = "unset"
        res = timed(name, fn, repeat)
        if proc.stream_rejected is not None:
            print(f"{name} stream_rejected {proc.stream_rejected}", flush=True)
        else:
            digest(name, res)

    for bits in (8, 16):
        b = dict(output_bits=bits)
        for what, kw in (("stencils", stencils_on), ("pointwise", pointwise)):
            tag = f"{what}/{bits}"
            streamed(f"streamed_process_pageable {tag}", lambda: proc.process(pageable, neg, 6, 0.4, cache=False, **kw, **b))
            streamed(f"streamed_process_pinned {tag}", lambda: proc.process(pinned, neg, 6, 0.4, cache=False, **kw, **b))
            digest(f"streamed_last_output {tag}", proc.last_output.view(torch.int16 if bits == 16 else torch.uint8).cpu().numpy())
        payload = proc.extract_image_data_cpu(pageable, **geom)
        streamed(f"streamed_process_preloaded {bits}", lambda: proc.process_preloaded(payload, neg, 6, 0.4, **stencils_on, **b))
        streamed(f"streamed_submit_preloaded {bits}", lambda: proc.submit_preloaded(payload, neg, 6, 0.4, **stencils_on, **b).result())
        in_flight = dict(payload, image_array=torch.from_numpy(payload["image_array"]).pin_memory())
        digest(f"submit_preloaded_pinned {bits}", timed(f"submit_preloaded_pinned {bits}", lambda: proc.submit_preloaded(
            in_flight, neg, 6, 0.4, **stencils_on, **b).result()))
        streamed(f"streamed_u16_source {bits}", lambda: proc.process(u16, neg, 6, 0.4, cache=False, exposure=0.5, **stencils_on, **b))
        streamed(f"streamed_u16_device_exposure {bits}", lambda: proc.process(u16, neg, 6, 0.4, cache=False, exposure="device", **pointwise, **b))
        for name, (mosaic, half) in mosaics.items():
            for what, kw in (("stencils", stencils_on), ("pointwise", pointwise)):
                streamed(f"streamed_{name} {what}/{bits}", lambda: proc.process(mosaic, neg, 6, 0.4, cache=False, raw_profile=raw,
                                                                                 half_size=half, exposure=0.5, **kw, **b))
        streamed(f"streamed_process_tiff {bits}", lambda: proc.process_tiff(pageable, neg, 6, 0.4, stream=True, icc_profile=b"icc", **stencils_on, **b))
        streamed(f"streamed_process_preloaded_tiff {bits}", lambda: proc.process_preloaded_tiff(payload, neg, 6, 0.4, stream=True, **pointwise, **b))
    proc.stream_bands = 0  # one piece: the frame comes down into a lent pinned buffer of its depth's pool
    for bits in (8, 16):
        digest(f"one_piece_process_big {bits}", timed(f"one_piece_process_big {bits}", lambda: proc.process(
            pageable, neg, 6, 0.4, cache=False, output_bits=bits, **stencils_on)))
    proc.stream_bands = 4
    digest("one_piece_process_tiff_big 16", timed("one_piece_process_tiff_big 16", lambda: proc.process_tiff(pageable, neg, 6, 0.4, **stencils_on)))
    # the host gate lets the frame through, its payload then does not stream (a preview resolution): extracted once, rendered whole
    streamed("gate_passed_payload_refused", lambda: proc.process(pageable, neg, 6, 0.4, cache=False, resolution=(BIG // 2, BIG // 2), **pointwise))
    digest("gate_passed_payload_refused_last_output", proc.last_output.cpu().numpy())  # (the line above holds the reason, not the pixels)
    streamed("streamed_process_jpeg", lambda: proc.process_jpeg(pageable, neg, 6, 0.4, 90, stream=True, **stencils_on))
    streamed("streamed_process_jpeg_pinned_444", lambda: proc.process_jpeg(pinned, neg, 6, 0.4, 90, stream=True, subsampling=0, **pointwise))
    streamed("streamed_process_preloaded_jpeg", lambda: proc.process_preloaded_jpeg(payload, neg, 6, 0.4, 90, stream=True, **stencils_on))
    digest("one_piece_process_jpeg_big", timed("one_piece_process_jpeg_big", lambda: proc.process_jpeg(pageable, neg, 6, 0.4, 90, **stencils_on)))
    del pinned, pinned_t


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--times", help="write every case's wall clock (first call, second call; ms) into this file")
    ap.add_argument("--skip-streamed", action="store_true", help="the small frames only")
    ap.add_argument("--group", default="all", choices=["all", "small", "prepath"], help="one group of cases only")
    args = ap.parse_args()
    import torch

    from raw2film_amd import HipProcessor, filmstock

    stocks = filmstock.builtin_stocks()
    neg, prt = stocks["Kodak Portra 400"], stocks["Kodak 2383"]
    proc = HipProcessor(device=0)
    if args.group in ("all", "small"):
        small_cases(proc, torch, neg, prt)
    if args.group in ("all", "prepath"):
        prepath_cases(proc, torch, neg, prt)
    if args.group == "all" and not args.skip_streamed:
        streamed_cases(proc, torch, neg, prt)
    proc.close()
    if args.times:
        with open(args.times, "w") as f:
            for name, first, second in TIMES:
                f.write(f"{name:48s} first {first:9.2f} ms" + ("" if second is None else f"   second {second:9.2f} ms") + "\n")


if __name__ == "__main__":
    main()
