"""The context's options and its ownership of device resources, on the C ABI: r2f_set_option answers every name and value as the
recorded walk says (tests/golden/option_walk.json, tests/option_walk.py), and a context destroyed with unread launch timings leaves
the next context working and bit-identical."""

import ctypes
import json
import os

import pytest

from helpers import SEED, stocks, synthetic_frame
from option_walk import NAMES, UNKNOWN, VALUES, walk

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "option_walk.json")


def test_set_option_answers_every_name_and_value_as_recorded():
    from raw2film_amd import _lib

    want = json.load(open(GOLDEN))["rows"]
    assert len(NAMES) == 28 and len(want) == (len(NAMES) + 1) * len(VALUES)
    _lib.load()  # (built and loadable)
    got = walk(ctypes.CDLL(_lib.LIB_PATH))  # a handle of its own: walk() sets argtypes
    assert [r[:2] for r in got] == [[n, v] for n in NAMES + [UNKNOWN] for v in VALUES]
    for g, w in zip(got, want):
        assert g == w, (g, w)


def test_a_context_destroyed_with_unread_timings_leaves_the_next_one_bit_identical():
    """kernel_timing = 7 makes every FFT pass launch record an event pair that r2f_kernel_timing would read and destroy; here nobody
    reads them, so r2f_destroy has to.  (That it does is read off r2f_ctx's destructor; what can be observed is that the destroy
    neither faults nor disturbs the next context.)"""
    from raw2film_amd import HipProcessor

    H, W = 160, 256
    neg, prt, _ = stocks()
    kw = dict(print_film=prt, frame_width=36.0 * W / 12288.0, frame_height=36.0 * H / 12288.0, halation_green_factor=0.3,
              exp_kelvin=6000, color_masking=1.0)  # 100 MP pixel pitch: both stencils by FFT
    frame = torch.from_numpy(synthetic_frame(H, W, seed=5)).cuda()
    outs = []
    for timing in (7, 0):
        proc = HipProcessor(device=0)
        proc.ctx.set_option("kernel_timing", timing)
        out = proc.process_array(frame, neg, 6, 0.4, colorspace="linear-rec709", seed=SEED, return_float=True, output="device", **kw).clone()
        assert any(ch["fft"] for ch in proc.ctx.stencil_stats(0)), "the halation did not take the FFT form"
        assert proc.ctx.render_stats()["eager"] >= 1  # (timed frames run kernel by kernel)
        outs.append(out)
        proc.close()  # (the first context's timings were never read)
    assert torch.equal(outs[0], outs[1])
