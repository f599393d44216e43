"""exposure="device", host side (no GPU): what extract_image_data_cpu puts into the payload -- the whole frame as a view, the crop
window, calc_exposure's exponent, the marker in place of the factor --, which payloads fall back to the host measurement, which
values of `exposure` are refused, and the float64 model the GPU tests compare the device with."""

import math

import numpy as np
import pytest

from raw2film_amd import decode, geometry
from raw2film_amd.hip_processor import DEVICE_EXPOSURE, HipProcessor, exposure_on_device
from raw2film_amd.payload import stream_rejection

import exposure_model

META = {"EXIF:FNumber": 5.6, "EXIF:ISO": 200, "EXIF:ExposureTime": 1 / 125}

# the geometry cases of tests/test_processor_host.py (frame shape, frame_width, frame_height, zoom, flip) and a few around them
GEOMETRY = [
    ((400, 640), 36, 24, 2.0, False),
    ((420, 600), 36, 24, 1.3, False),
    ((420, 600), 36, 24, 1.0, False),
    ((400, 600), 5.79, 3.86, 1.0, False),
    ((40, 60), 36, 24, 1.0, False),
    ((1000, 1600), 36, 24, 1.0, False),
    ((640, 400), 36, 24, 1.5, True),
    ((400, 640), 36, 24, 1.0, True),
    ((333, 777), 24, 36, 1.7, False),
    ((501, 500), 6, 6, 3.0, False),
]


@pytest.fixture
def proc():
    p = HipProcessor.__new__(HipProcessor)
    p.payload_alpha = True
    return p


def frame(shape, channels=3, seed=0):
    return np.random.default_rng(seed).integers(0, 65536, shape + (channels,), dtype=np.uint16)


def test_the_payload_is_the_callers_frame(proc):
    u16 = frame((40, 60))
    p = proc.extract_image_data_cpu(u16, exposure="device", metadata=META)
    assert p["image_array"].dtype == np.uint16 and p["image_array"].shape == u16.shape
    assert np.shares_memory(p["image_array"], u16)
    assert p["u16_factor"] == DEVICE_EXPOSURE and p["exposure_rejected"] is None and p["clip_on_device"] is False
    assert p["exposure_root"] == decode.exposure_root(META)
    assert proc.extract_image_data_cpu(u16, exposure="device")["exposure_root"] == 3.0  # (no metadata)
    # a cropped frame still goes up whole, and as the same memory
    wide = frame((400, 900))
    q = proc.extract_image_data_cpu(wide, exposure="device", metadata=META, max_scale=None)
    assert np.shares_memory(q["image_array"], wide) and q["image_array"].shape == wide.shape
    assert q["u16_window"] == (0, 150, 400, 600) and q["pipeline_resolution"] == (600, 400)
    # a source that is not contiguous is made so, whole
    r = proc.extract_image_data_cpu(wide[:, ::2], exposure="device", max_scale=None)
    assert r["image_array"].flags.c_contiguous and np.array_equal(r["image_array"], wide[:, ::2])
    # a float frame ignores exposure= of any kind, as before
    f = proc.extract_image_data_cpu(np.zeros((40, 60, 3), np.float32), exposure="device")
    assert f["u16_factor"] is None and f["u16_window"] is None and f["image_array"].dtype == np.float32


@pytest.mark.parametrize("shape, fw, fh, zoom, flip", GEOMETRY)
def test_the_window_is_the_box_crop_to_frame_selects(proc, shape, fw, fh, zoom, flip):
    u16 = frame(shape, seed=shape[0])
    kw = dict(frame_width=fw, frame_height=fh, zoom=zoom, flip=flip, max_scale=None)
    p = proc.extract_image_data_cpu(u16, exposure="device", metadata=META, **kw)
    r0, c0, nr, nc = p["u16_window"]
    want = geometry.crop_to_frame(u16, fw, fh, zoom, 0, flip)
    assert np.array_equal(u16[r0:r0 + nr, c0:c0 + nc], want) and np.shares_memory(u16[r0:r0 + nr, c0:c0 + nc], want)
    assert u16[r0:r0 + nr, c0:c0 + nc].__array_interface__["data"][0] == want.__array_interface__["data"][0]
    # everything else about the payload is what the stops-given payload says
    given = proc.extract_image_data_cpu(u16, exposure=0.5, **kw)
    assert given["image_array"].shape[:2] == (nr, nc)
    for k in ("final_resolution", "output_resolution", "canvas_resolution", "pipeline_resolution", "chroma_nr", "resize_to", "warp",
              "upscale_to", "clip_on_device"):
        assert p[k] == given[k], k


def test_a_large_payload_streams(proc):
    u16 = np.zeros((2400, 3600, 3), np.uint16)
    p = proc.extract_image_data_cpu(u16, exposure="device", metadata=META, _internal=True)
    assert stream_rejection(p, p["u16_window"][2:] + (3,), "torch.int16", False) is None
    # ... and the messages for one that does not are the old ones, with the marker where the factor was
    small = proc.extract_image_data_cpu(np.zeros((40, 60, 3), np.uint16), exposure="device", _internal=True)
    assert stream_rejection(small, (40, 60, 3), "torch.int16", False) == (
        "a device pre-path, a canvas, or a frame below 16.7 M samples: warp = None, resize_to = None, upscale_to = None, "
        "chroma_nr = 0, canvas_resolution = None, u16_factor = 'device', clip_on_device = False, frame (40, 60, 3) torch.int16")


@pytest.mark.parametrize("kw, names", [(dict(rotate_times=1), "rotate_times = 1"), (dict(rotate_times=3), "rotate_times = 3"),
                                       (dict(rotation=2.5), "rotation = 2.5"),
                                       (dict(rotation=-1.0, rotate_times=2), "rotation = -1.0, rotate_times = 2")])
def test_turned_and_rotated_frames_are_measured_on_the_host(proc, kw, names):
    u16 = (np.random.default_rng(5).uniform(0, 1, (120, 180, 3)) ** 3 * 20000).astype(np.uint16)
    p = proc.extract_image_data_cpu(u16, exposure="device", metadata=META, **kw)
    host = proc.extract_image_data_cpu(u16, exposure=None, metadata=META, **kw)
    assert names in p["exposure_rejected"] and host["exposure_rejected"] is None
    assert p["u16_factor"] == host["u16_factor"] == float(decode.exposure_factor(decode.auto_exposure(u16, metadata=META)))
    assert p["u16_window"] is None and p["exposure_root"] is None
    assert np.array_equal(p["image_array"], host["image_array"]) and (p["warp"] is not None) == ("rotation" in kw)
    # four quarter turns are none
    assert proc.extract_image_data_cpu(u16, exposure="device", rotate_times=4)["u16_factor"] == DEVICE_EXPOSURE


@pytest.mark.parametrize("bad", ["gpu", "", b"device", "Device", "host"])
def test_any_other_string_is_refused_before_any_work(proc, bad):
    u16 = frame((40, 60))
    with pytest.raises(ValueError, match="exposure must be"):
        proc.extract_image_data_cpu(u16, exposure=bad)
    with pytest.raises(ValueError, match="exposure must be"):
        proc.extract_image_data_cpu(np.zeros((40, 60, 3), np.float32), exposure=bad)  # (a float frame too: nothing was looked at)
    with pytest.raises(ValueError, match="exposure must be"):
        HipProcessor.process(proc, "photo.cr3", None, 6, 0.4, exposure=bad)  # (before the RAW path is even refused)
    with pytest.raises(ValueError, match="exposure must be"):
        HipProcessor.process_jpeg(proc, "photo.cr3", None, 6, 0.4, exposure=bad)
    with pytest.raises(ValueError):
        exposure_on_device(bad)
    assert exposure_on_device("device") and not exposure_on_device(None) and not exposure_on_device(0.5)


def test_the_model_is_upstreams_formula_in_float64():
    """The float64 model against the host's float32 evaluation (decode.auto_exposure = upstream's, bit for bit): they agree to the
    float32 evaluation's own error, which grows with the exponent -- and an all-zero sample set is +inf in both."""
    rng = np.random.default_rng(7)
    u16 = (rng.uniform(0, 1, (130, 190, 3)) ** 2.2 * 65535).astype(np.uint16)
    for md, tol in ((None, 1e-5), (META, 1e-5), ({"EXIF:FNumber": 2.02, "EXIF:ISO": 100, "EXIF:ExposureTime": 1e-6}, 1e-3)):
        assert abs(exposure_model.model_stops(u16, md) - decode.auto_exposure(u16, metadata=md)) <= tol
    # by hand: every sample 65535 -> g = 1, m = 1, stops = log2(0.18); one quarter of the samples 65535, the rest 0, root 3
    assert exposure_model.model_stops(np.full((4, 6, 3), 65535, np.uint16)) == math.log2(0.18)
    q = np.zeros((2, 8, 3), np.uint16)
    q[0, 0, 1] = 65535
    assert exposure_model.model_stops(q) == pytest.approx(math.log2(0.18 / 0.25**3), abs=1e-12)
    q[:, :, 1] = 0
    q[1, :, :] = 9  # (unsampled rows and channels do not count)
    q[:, 1::2, :] = 9
    assert exposure_model.model_stops(q) == math.inf
    assert exposure_model.factor_agrees(np.float32(np.inf), math.inf) and not exposure_model.factor_agrees(np.float32(1.0), math.inf)
    s = 0.657791852173465
    assert exposure_model.factor_agrees(decode.exposure_factor(s), s) and not exposure_model.factor_agrees(decode.exposure_factor(s + 1e-6), s)
