"""A Bayer mosaic through the row-band path of HipProcessor: with its exposure in stops, no turn and no lens step, a mosaic just
past the 16.7 M-sample threshold streams -- upload k carries the mosaic rows band k's r2f_demosaic_f32 reads -- and gives the bytes
of the same call in one piece (stream_bands = 0: r2f_demosaic_u16 of the whole mosaic, the cut, r2f_decode_u16), of the model's
uint16 frame through the uint16 RGB route, and the same JPEG and TIFF files; what does not qualify falls back and says why.

Bit for bit throughout.  The stencil case runs its frame on a 360 mm format (6.6 px/mm), where halation and MTF are a few taps wide
and run in the direct form: only there is a band's stencil output the whole frame's bit for bit -- the FFT form anchors its windows
at a band's first row and differs from the one-piece render by an fp32 ulp on a handful of samples, for every kind of source
(tests/test_gpu_stream_fuzz.py bounds that); the mosaic's own share, the demosaic into the float frame, is exact either way and is
what the other cases pin."""

import numpy as np
import pytest

import demosaic_model as dm
from helpers import stocks

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# the square 36 x 36 format keeps 2368 x 2368 of a 2400 x 2368 frame: 16.8 M samples, row0 = 16
KW = dict(halation=False, sharpness=False, grain=0, exp_kelvin=6000, color_masking=1.0, frame_width=36, frame_height=36, max_scale=None,
          lens_correction=False, seed=3, exposure=0.5)
STENCILS = dict(halation=True, sharpness=True, grain=2, frame_width=360, frame_height=360, halation_green_factor=0.3)
PATTERN = "RGGB"
_MOSAICS = {}


def mosaic_of(H, W):
    """An H x W mosaic with image-like statistics (a smooth field plus noise, well inside 14 bits), made once."""
    if (H, W) not in _MOSAICS:
        rng = np.random.default_rng(17)
        y, x = np.mgrid[0:H, 0:W].astype(np.float32)
        base = 600 + 9000 * (0.5 + 0.5 * np.sin(x / 230.0) * np.cos(y / 170.0)) + rng.normal(0, 120, (H, W)).astype(np.float32)
        _MOSAICS[(H, W)] = np.clip(base, 0, 16383).astype(np.uint16)
    return _MOSAICS[(H, W)]


@pytest.fixture(scope="module")
def prof():
    from raw2film_amd.raw import RawProfile

    return RawProfile(PATTERN, black=512, multipliers=(7.9, 4.1, 6.2), matrix=((0.52, 0.27, 0.15), (0.25, 0.68, 0.07), (0.03, 0.12, 0.81)))


@pytest.fixture(scope="module")
def proc():
    from raw2film_amd import HipProcessor

    p = HipProcessor(cameras={}, lenses={}, device=0)
    assert p.stream_bands == 16
    p.band_plans = []
    inner = p._run_bands

    def spy(frame, *a, **k):
        p.band_plans.append(list(frame.bounds))
        return inner(frame, *a, **k)

    p._run_bands = spy
    yield p
    p.close()


def render(proc, src, bands, call="process", **kw):
    """One call with stream_bands = bands -> (its result, copied; stream_rejected after it; the band bounds it ran, or None)."""
    neg, prt, _ = stocks()
    proc.stream_bands, proc.stream_rejected = bands, "unset"
    del proc.band_plans[:]
    try:
        if call == "process":
            out = proc.process(src, neg, 6, 0.4, cache=False, print_film=prt, **kw)
        elif call == "preloaded":
            out = proc.process_preloaded(src, neg, 6, 0.4, final_scaling="cpu", print_film=prt, **kw)
        else:
            out = getattr(proc, call)(src, neg, 6, 0.4, print_film=prt, **kw)
    finally:
        proc.stream_bands = 16
    return (out.copy() if isinstance(out, np.ndarray) else out), proc.stream_rejected, (proc.band_plans[-1] if proc.band_plans else None)


def streamed_and_whole(proc, src, prof, bands=16, min_bands=3, **kw):
    kw = {**KW, **kw}
    got, why, plan = render(proc, src, bands, raw_profile=prof, **kw)
    assert why is None and plan is not None, f"the mosaic did not stream: {why}"
    assert len(plan) - 1 >= min_bands, plan
    want, _, none = render(proc, src, 0, raw_profile=prof, **kw)
    assert none is None  # (one piece: no band loop)
    assert got.shape == want.shape and got.dtype == want.dtype
    diff = int(np.count_nonzero(got != want))
    print(f"streamed against one piece, {kw}: {diff} of {got.size} samples differ")
    assert diff == 0
    return got


FULL, HALF, ZOOMED = (2400, 2368), (4800, 4736), (3120, 3088)


def test_lut_only_settings_pageable_and_pinned(proc, prof):
    m = mosaic_of(*FULL)
    out = streamed_and_whole(proc, m, prof, half_size=False)
    assert out.shape == (2368, 2368, 3) and out.dtype == np.uint8 and out.std() > 1  # (a picture, not a flat field)
    assert not proc._payload_tensor({"image_array": m}).is_pinned()
    pinned = torch.from_numpy(m.view(np.int16)).pin_memory().numpy().view(np.uint16)
    assert proc._payload_tensor({"image_array": pinned}).is_pinned()
    assert np.array_equal(streamed_and_whole(proc, pinned, prof, half_size=False), out)
    # two bands asked for (the taper may halve the last one)
    assert np.array_equal(streamed_and_whole(proc, m, prof, bands=2, min_bands=2, half_size=False), out)


def test_halation_mtf_and_grain_with_a_fixed_seed(proc, prof):
    out = streamed_and_whole(proc, mosaic_of(*FULL), prof, half_size=False, **STENCILS)
    plain, _, _ = render(proc, mosaic_of(*FULL), 0, raw_profile=prof, **{**KW, "half_size": False})
    assert np.count_nonzero(out != plain) > out.size // 2  # (the stages ran)


def test_a_zoomed_window_with_an_odd_origin(proc, prof):
    m = mosaic_of(*ZOOMED)
    pay = proc.extract_image_data_cpu(m, raw_profile=prof, half_size=False, zoom=1.3, exposure=0.5, frame_width=36, frame_height=36,
                                      max_scale=None)
    row0, col0, rows, cols = pay["demosaic"]["window"]
    assert row0 % 2 == 1 and col0 % 2 == 1 and rows * cols * 3 >= 1 << 24, pay["demosaic"]["window"]
    out = streamed_and_whole(proc, m, prof, half_size=False, zoom=1.3)
    assert out.shape == (rows, cols, 3)


def test_half_size(proc, prof):
    out = streamed_and_whole(proc, mosaic_of(*HALF), prof, half_size=True)
    assert out.shape == (2368, 2368, 3)


def test_sixteen_bits(proc, prof):
    out = streamed_and_whole(proc, mosaic_of(*FULL), prof, half_size=False, output_bits=16)
    assert out.dtype == np.uint16


def test_the_models_frame_through_the_uint16_route(proc, prof):
    m = mosaic_of(*FULL)
    got, why, plan = render(proc, m, 16, raw_profile=prof, half_size=False, **KW)
    assert why is None and plan is not None
    rgb = dm.demosaic(m, prof)
    for bands in (16, 0):
        want, _, _ = render(proc, rgb, bands, **KW)
        assert np.array_equal(got, want), bands


def test_the_exports_write_the_one_piece_files(proc, prof):
    m = mosaic_of(*FULL)
    kw = dict(KW, raw_profile=prof, half_size=False)
    a, why, plan = render(proc, m, 16, call="process_jpeg", quality=90, stream=True, **kw)
    assert why is None and plan is not None and len(plan) - 1 >= 3
    b, _, none = render(proc, m, 16, call="process_jpeg", quality=90, **kw)
    assert none is None and isinstance(a, bytes) and a == b
    a, why, plan = render(proc, m, 16, call="process_tiff", output_bits=16, stream=True, **kw)
    assert why is None and plan is not None and len(plan) - 1 >= 3
    b, _, none = render(proc, m, 16, call="process_tiff", output_bits=16, **kw)
    assert none is None and isinstance(a, bytes) and a == b
    # the two-phase API: a pageable payload streams in process_preloaded
    frame, _, _ = render(proc, m, 0, **kw)
    pay = proc.extract_image_data_cpu(m, raw_profile=prof, half_size=False, exposure=0.5, frame_width=36, frame_height=36, max_scale=None)
    got, why, plan = render(proc, pay, 16, call="preloaded", **KW)
    assert why is None and plan is not None and np.array_equal(got, frame)


def test_what_does_not_qualify_falls_back_and_names_the_demosaic_step(proc, prof):
    m = mosaic_of(*FULL)
    for extra in (dict(exposure=None), dict(rotate_times=1)):
        kw = {**KW, "half_size": False, **extra}
        pay = proc.extract_image_data_cpu(m, raw_profile=prof, **{k: kw[k] for k in ("half_size", "exposure", "frame_width", "frame_height",
                                                                                      "max_scale")}, rotate_times=kw.get("rotate_times", 0))
        got, why, plan = render(proc, pay, 16, call="preloaded", **kw)
        assert plan is None and why is not None and why.startswith("the demosaic step"), why
        want, _, _ = render(proc, pay, 0, call="preloaded", **kw)
        assert np.array_equal(got, want)
        whole, _, none = render(proc, m, 16, raw_profile=prof, **kw)  # process(): the host gate refuses ahead of the payload
        assert none is None and np.array_equal(whole, want)
        a, why, plan = render(proc, m, 16, call="process_jpeg", quality=90, stream=True, raw_profile=prof, **kw)
        assert plan is None and why.startswith("the demosaic step") and a == proc.encode_jpeg(want, 90)


def test_the_stream_buffers_serve_frames_of_other_sizes_in_between(proc, prof):
    m, z = mosaic_of(*FULL), mosaic_of(*ZOOMED)
    kw = dict(KW, raw_profile=prof, half_size=False)
    first, why, _ = render(proc, m, 16, **kw)
    assert why is None
    small, _, none = render(proc, np.ascontiguousarray(m[:96, :144]), 16, **kw)
    assert none is None and small.shape == (96, 96, 3)
    other, why, _ = render(proc, z, 16, zoom=1.3, **kw)
    assert why is None and other.shape != first.shape
    again, why, _ = render(proc, m, 16, **kw)
    assert why is None and np.array_equal(again, first)
    again, _, _ = render(proc, np.ascontiguousarray(m[:96, :144]), 16, **kw)
    assert np.array_equal(again, small)
    assert "u16" not in {k for k in proc._stream_bufs if isinstance(k, str)} and tuple(proc._stream_bufs["mosaic"].shape) == FULL
