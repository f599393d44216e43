"""A Bayer mosaic in the row-band path, the host half (raw2film_amd/payload.py, no GPU): the mosaic rows that travel with each
band (mosaic_upload_bounds) hold what that band's r2f_demosaic_f32 reads, and the two gates let a mosaic through exactly when its
exposure is given in stops, nothing turns it, no lens step follows and its window of the demosaiced frame has 16.7 M samples."""

import numpy as np
import pytest

from raw2film_amd import HipProcessor
from raw2film_amd.lens import LensProfile
from raw2film_amd.payload import host_stream_gate, mosaic_frame_samples, mosaic_upload_bounds, stream_rejection
from raw2film_amd.raw import RawProfile


def rows_read(row0, b0, b1, Hm, half):
    """The mosaic rows r2f_demosaic_f32 reads for the window's rows [b0, b1) (include/r2f.h)."""
    if half:
        return 2 * (row0 + b0), 2 * (row0 + b1)
    return max(row0 + b0 - 4, 0), min(row0 + b1 + 4, Hm)


def windows(Hd):
    """(row0, rows) inside a demosaiced frame of Hd rows: odd and even origins, touching the top, the bottom, both or neither."""
    out = {(0, Hd)}
    for row0 in (0, 1, 2, 3, 5, 8):
        for rows in (1, 2, 7, Hd - row0 - 3, Hd - row0 - 1, Hd - row0):
            if rows >= 1 and row0 + rows <= Hd:
                out.add((row0, rows))
    return sorted(out)


@pytest.mark.parametrize("half", [False, True], ids=["full", "half"])
def test_upload_bounds_hold_what_each_band_reads(half):
    cases = 0
    seen = set()
    for Hm in range(2, 81):
        if half and Hm % 2:
            continue
        Hd = Hm // 2 if half else Hm
        for row0, rows in windows(Hd):
            for n in range(1, 6):
                if n > rows:
                    continue
                bounds = [rows * i // n for i in range(n + 1)]
                window = (row0, 3, rows, 11)
                ub = mosaic_upload_bounds(bounds, window, Hm, half)
                what = (Hm, window, bounds, ub)
                assert len(ub) == n + 1 and all(isinstance(v, int) for v in ub), what
                assert all(a <= b for a, b in zip(ub[:-1], ub[1:])), what
                assert 0 <= ub[0] and ub[-1] <= Hm, what
                if half:
                    assert ub == [2 * (row0 + b) for b in bounds], what
                else:
                    assert ub[0] == max(row0 - 4, 0) and ub[-1] == min(row0 + rows + 4, Hm), what
                    assert ub[1:-1] == [min(row0 + b + 4, Hm) for b in bounds[1:-1]], what
                for k in range(n):
                    lo, hi = rows_read(row0, bounds[k], bounds[k + 1], Hm, half)
                    assert ub[0] <= lo and hi <= ub[k + 1], (what, k, lo, hi)
                # the whole upload is what the whole window reads, no row more
                assert (ub[0], ub[-1]) == rows_read(row0, 0, rows, Hm, half), what
                cases += 1
                seen.add((row0 % 2, row0 == 0 or (not half and row0 < 4), row0 + rows == Hd, n))
    assert cases > 2000
    for odd in (0, 1):
        for n in range(1, 6):
            assert (odd, False, False, n) in seen and (odd, False, True, n) in seen  # (neither edge; the bottom)
    assert any(top and not bottom for _, top, bottom, _ in seen) and any(top and bottom for _, top, bottom, _ in seen)


# ---- the gates
@pytest.fixture(scope="module")
def proc():
    p = HipProcessor.__new__(HipProcessor)
    p.cameras = p.lenses = None
    p.payload_alpha = True
    return p


MOSAIC = np.zeros((2400, 2400), np.uint16)
PROFILE = RawProfile("RGGB")
SQUARE = dict(frame_width=36, frame_height=36, half_size=False, max_scale=None)  # the window is the whole 2400 x 2400 frame: 17.3 M


def payload(proc, **kw):
    return proc.extract_image_data_cpu(MOSAIC, raw_profile=PROFILE, **{**SQUARE, **kw})


def plan_gate(pay, final_scaling="cpu", canvas_mode="No"):
    return stream_rejection(pay, MOSAIC.shape, "torch.int16", False, final_scaling, canvas_mode)


def host_gate(stops=True, rotate_times=0, lens=False, half_size=False, **kw):
    samples = mosaic_frame_samples(MOSAIC, half_size, 1.0, False, 1.0)
    return host_stream_gate(MOSAIC, 16, kw.get("rotation", 0.0), 0, kw.get("canvas_mode", "No"), 0.0, lens, True, stops=stops,
                            rotate_times=rotate_times, frame_samples=samples)


def test_a_large_mosaic_with_stops_passes_both_gates(proc):
    pay = payload(proc, exposure=0.5)
    assert pay["demosaic"]["window"] == (0, 0, 2400, 2400) and isinstance(pay["u16_factor"], float)
    assert plan_gate(pay) is None
    assert plan_gate(payload(proc, exposure=0.5, zoom=1.01)) is None  # (a window with an origin, still above the threshold)
    assert mosaic_frame_samples(MOSAIC, False, 1.0, False, 1.0) == 2400 * 2400 * 3
    assert mosaic_frame_samples(MOSAIC, True, 1.0, False, 1.0) == 1200 * 1200 * 3
    assert mosaic_frame_samples(MOSAIC, False, 1.5, False, 1.0) == 1600 * 2400 * 3
    assert host_gate() is None


def test_each_mosaic_refusal_names_the_demosaic_step_and_its_reason(proc):
    lens = LensProfile("ptlens", (0.02, -0.06, 0.01), scale=1.02)
    cases = {
        "stops": (payload(proc, exposure=None), host_gate(stops=False)),
        "stops ": (payload(proc, exposure="device"), host_gate(stops=False)),
        "rotate_times": (payload(proc, exposure=0.5, rotate_times=1), host_gate(rotate_times=1)),
        "lens": (payload(proc, exposure=0.5, lens_profile=lens), host_gate(lens=True)),
        "16.7 M": (payload(proc, exposure=0.5, half_size=True), host_gate(half_size=True)),
    }
    for reason, (pay, host_why) in cases.items():
        for why in (plan_gate(pay), host_why):
            assert why is not None and why.startswith("the demosaic step") and reason.strip() in why, (reason, why)
            assert "not streamed yet" not in why
    # the defaults of the new keywords mean "stops not given"; four quarter turns are none
    why = host_stream_gate(MOSAIC, 16, 0.0, 0, "No", 0.0, False, True)
    assert why is not None and "demosaic" in why and "stops" in why
    assert host_gate(rotate_times=4) is None and plan_gate(payload(proc, exposure=0.5, rotate_times=4)) is None
    assert "demosaic" in host_stream_gate(MOSAIC, 16, 0.0, 0, "No", 0.0, False, True, stops=True)  # (no window known)


def test_the_generic_refusals_still_apply_to_a_mosaic(proc):
    assert "canvas" in plan_gate(payload(proc, exposure=0.5, canvas_mode="Uniform white", canvas_scale=1.1), canvas_mode="Uniform white")
    assert "canvas" in host_gate(canvas_mode="Uniform white")
    assert plan_gate(payload(proc, exposure=0.5, max_scale=400.0, resolution=(1200, 1200))) is not None  # (a preview scaling)
    pay = payload(proc, exposure=0.5)
    assert plan_gate(dict(pay, final_resolution=(1200, 1200))) == "the finished frame is scaled to (1200, 1200)"
    assert plan_gate(dict(pay, final_resolution=(1200, 1200)), final_scaling="gpu") is None
    assert plan_gate(payload(proc, exposure=0.5, rotation=3.5)) is not None and "rotation" in host_gate(rotation=3.5)
    assert plan_gate(payload(proc, exposure=0.5, chroma_nr=3)) is not None
    assert host_stream_gate(MOSAIC, 1, demosaic=True, stops=True, frame_samples=1 << 25) == "stream_bands = 1"
    assert "host array" in host_stream_gate("frame.npy", 16, demosaic=True, stops=True, frame_samples=1 << 25)
    # frames that are no mosaics pass and fail as before
    assert host_stream_gate(np.zeros((1 << 12, 1 << 12, 3), np.uint16), 16) is None
    assert "16.7 M" in host_stream_gate(np.zeros((1 << 10, 1 << 10, 3), np.uint16), 16)
