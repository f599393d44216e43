"""Host logic of the streamed path and of the result buffers, no GPU needed: the band planner and the qualification of a payload
(hip_processor.plan_bands / payload.stream_rejection), the fresh-array sink under a late page touch, the lease pool under concurrency."""

import gc
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from raw2film_amd import _lib
from raw2film_amd.hip_processor import plan_bands
from raw2film_amd.payload import stream_rejection
from raw2film_amd.results import LEASES, ResultBuffers, ResultSink, touch_pages

torch = pytest.importorskip("torch")

# (H, halation reach, MTF reach, stream_bands, stream_taper, bounds or rejection): bounds as the arithmetic of the commit before the
# planner moved out of HipProcessor._stream_payload produced them
PLANS = [
    (8192, (0, 0), (0, 0), 16, 2, [0, 512, 1024, 1536, 2048, 2560, 3072, 3584, 4096, 4608, 5120, 5632, 6144, 6656, 7168, 7424, 7680,
                                   7936, 8192]),
    (8192, (31, 31), (6, 6), 16, 2, [0, 512, 1024, 1536, 2048, 2560, 3072, 3584, 4096, 4608, 5120, 5632, 6144, 6656, 7168, 7424, 7680,
                                     7936, 8192]),
    (2403, (0, 0), (0, 0), 16, 2, [0, 600, 1201, 1501, 1802, 2102, 2403]),
    (2403, (40, 40), (8, 8), 16, 2, [0, 600, 1201, 1501, 1802, 2102, 2403]),
    (8192, (30, 30), (5, 5), 16, 0, [0, 512, 1024, 1536, 2048, 2560, 3072, 3584, 4096, 4608, 5120, 5632, 6144, 6656, 7168, 7680, 8192]),
    (4096, (0, 0), (0, 0), 8, 20, [0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 2304, 2560, 2816, 3072, 3328, 3584, 3840, 4096]),
    (4096, (300, 300), (0, 0), 16, 2, [0, 682, 1365, 2048, 2730, 3413, 4096]),
    (1000, (400, 400), (0, 0), 16, 2, "1 band(s) of 1000 rows above the stencils' reach (400, 400) + (0, 0)"),
    (8160, (64, 64), (12, 12), 16, 2, [0, 544, 1088, 1632, 2176, 2720, 3264, 3808, 4352, 4896, 5440, 5984, 6528, 7072, 7344, 7616, 7888,
                                       8160]),
    (3000, (0, 0), (0, 0), 2, 0, [0, 1500, 3000]),
    (2049, (0, 0), (0, 0), 23, 3, [0, 512, 768, 1024, 1280, 1536, 1792, 2049]),
    (1400, (10, 10), (3, 3), 16, 2, [0, 350, 700, 1050, 1400]),
    (16384, (0, 0), (0, 0), 5, 1, [0, 3276, 6553, 9830, 13107, 14745, 16384]),
    (6000, (100, 3), (2, 50), 16, 3, [0, 545, 1090, 1636, 2181, 2727, 3272, 3818, 4363, 4636, 4909, 5181, 5454, 5727, 6000]),
    (4000, (0, 0), (0, 0), 1, 2, "1 band(s) of 4000 rows above the stencils' reach (0, 0) + (0, 0)"),
]


@pytest.mark.parametrize("H, ha, ma, bands, taper, want", PLANS)
def test_band_plan(H, ha, ma, bands, taper, want):
    bounds, why = plan_bands(H, _lib.F_HALATION | _lib.F_MTF | _lib.F_GRAIN, ha, ma, bands, taper)
    if isinstance(want, str):
        assert (bounds, why) == (None, want)
        return
    assert why is None and bounds == want
    floor_rows = max(2 * max(ha + ma) + 2, 64)
    assert bounds[0] == 0 and bounds[-1] == H
    assert all(b - a >= floor_rows for a, b in zip(bounds, bounds[1:]))  # (strictly increasing, every band above the reach)
    assert len(bounds) - 1 <= bands + taper


def _payload(**kw):
    p = dict(u16_factor=None, clip_on_device=True, final_resolution=(4096, 4096), canvas_resolution=None, chroma_nr=0, resize_to=None,
             warp=None, upscale_to=None)
    p.update(kw)
    return p


def test_which_payloads_stream():
    shape, f32 = (4096, 4096, 3), "torch.float32"
    assert stream_rejection(_payload(), shape, f32, False) is None
    assert stream_rejection(_payload(u16_factor=0.5), shape, "torch.int16", False) is None
    assert stream_rejection(_payload(final_resolution=(2048, 2048)), shape, f32, False, final_scaling="gpu") is None
    warp = {"m_dst_to_src": None, "window": (0, 0, 4096, 4096), "rotate_times": 0}
    assert stream_rejection(_payload(warp=warp), shape, f32, False) == (
        f"a device pre-path, a canvas, or a frame below 16.7 M samples: warp = {warp!r}, resize_to = None, upscale_to = None, "
        "chroma_nr = 0, canvas_resolution = None, u16_factor = None, clip_on_device = True, frame (4096, 4096, 3) torch.float32")
    pre_path = "a device pre-path, a canvas, or a frame below 16.7 M samples: "
    for payload, shape_, dtype, on_device, canvas_mode in ((_payload(resize_to=(1024, 1024)), shape, f32, False, "No"),
                                                           (_payload(upscale_to=(8192, 8192)), shape, f32, False, "No"),
                                                           (_payload(chroma_nr=2), shape, f32, False, "No"),
                                                           (_payload(canvas_resolution=(5000, 5000)), shape, f32, False, "No"),
                                                           (_payload(), shape, f32, False, "Proportional"),
                                                           (_payload(final_resolution=(2000, 2000)), (2000, 2000, 3), f32, False, "No"),
                                                           (_payload(), shape, f32, True, "No"),
                                                           (_payload(), shape, "torch.int16", False, "No"),  # (no exposure factor)
                                                           (_payload(u16_factor=0.5), shape, f32, False, "No"),
                                                           (_payload(), shape, "torch.float64", False, "No")):
        why = stream_rejection(payload, shape_, dtype, on_device, canvas_mode=canvas_mode)
        assert why.startswith(pre_path), (payload, shape_, dtype, on_device, canvas_mode)
    assert stream_rejection(_payload(final_resolution=(2048, 2048)), shape, f32, False) == "the finished frame is scaled to (2048, 2048)"
    assert plan_bands(4096, _lib.F_BURN | _lib.F_GRAIN, (0, 0), (0, 0), 16, 2) == (None, "highlight burn (a function of the whole grained frame)")


class _Landing:
    """A device-to-host copy's event: synchronize() returns once the test lets the band land."""

    def __init__(self):
        self._landed = threading.Event()

    def land(self):
        self._landed.set()

    def synchronize(self):
        self._landed.wait()


def test_a_fresh_result_is_not_zeroed_by_a_late_page_touch():
    """The fresh-array sink: a band copied out before the touch of its pages has run must not get a zero per page afterwards."""
    H, W = 64, 4096  # (four parts of 16 rows; a page is a third of a row)
    staged = np.random.default_rng(3).integers(1, 256, (H, W, 3), dtype=np.uint8)

    def late_touch(flat, i0, i1):
        time.sleep(0.3 if i0 == 0 else 0.0)  # (the first part's touch comes late)
        touch_pages(flat, i0, i1)

    with ThreadPoolExecutor(max_workers=4) as pool:
        sink = ResultSink(staged, fresh=np.empty((H, W, 3), np.uint8), pool=pool, touch=late_touch)
        bands = [(0, 6), (6, 20), (20, 41), (41, 64)]
        landings = [_Landing() for _ in bands]
        for (y0, y1), landing in zip(bands, landings):
            sink.band_back(landing, y0, y1)
        for landing in reversed(landings):  # the bands come back last first
            landing.land()
            time.sleep(0.01)
        out = sink.finish()
    np.testing.assert_array_equal(out, staged)


def _take(results, shape):
    """A lent result of `shape` as process() hands it out, or None when the caller would get a fresh array."""
    sink = results.sink(shape, staged=False)
    if sink is None:
        return None
    sink.band_back(_Done(), 0, shape[0])
    return sink.finish()


class _Done:
    def synchronize(self):
        pass


def test_lent_buffers_are_neither_lost_nor_over_counted():
    made = []

    def alloc(shape):
        made.append(torch.empty(shape, dtype=torch.uint8))
        return made[-1]

    results = ResultBuffers(alloc)
    A, B = (40, 30, 3), (30, 40, 3)
    theirs = [_take(results, A) for _ in range(2)]  # results a second thread will drop while this one keeps rendering

    def drop():
        while theirs:
            time.sleep(0.0005)
            theirs.pop()

    other = threading.Thread(target=drop)
    other.start()
    lent = 0
    for _ in range(3000):
        out = _take(results, A)
        lent += out is not None
        del out
    other.join()
    gc.collect()
    assert len(made) == LEASES and lent == 3000  # (one of three was always free: this thread drops its result at once)
    back = [_take(results, A) for _ in range(LEASES)]  # every buffer came back, none twice
    assert {a.ctypes.data for a in back} == {t.data_ptr() for t in made} and _take(results, A) is None
    # a lent buffer of a frame given up on comes back too
    del back[0]
    results.sink(A, staged=False).abandon()
    kept = _take(results, A)
    assert kept is not None and _take(results, A) is None
    # another frame size: a count of its own, and the buffers of the old size are let go as they come back
    b_out = [_take(results, B) for _ in range(LEASES)]
    assert all(b is not None for b in b_out) and _take(results, B) is None
    del b_out[:]
    a_out = [_take(results, A) for _ in range(LEASES)]
    assert all(a is not None for a in a_out) and _take(results, A) is None
    del back[:], kept  # (buffers of A lent before the switch) ...
    gc.collect()
    assert _take(results, A) is None  # ... do not join the pool: three of A are out
    del a_out[0]
    again = _take(results, A)
    assert again is not None and _take(results, A) is None
    assert len(made) == 3 * LEASES  # (A, B, A again)
