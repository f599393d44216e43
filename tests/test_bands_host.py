"""The host-side plan of a streamed frame (raw2film_amd/bands.py), no GPU needed: the stage schedule against a transcription of the
band loop of the commit before the schedule moved out of HipProcessor._run_bands and against its data-dependence rule, and the
band source of every kind of payload against the calls that loop made, with CPU tensors and a recording context."""

import itertools
from types import SimpleNamespace

import pytest

from raw2film_amd.bands import band_source, stage_schedule
from raw2film_amd.payload import mosaic_upload_bounds

torch = pytest.importorskip("torch")

FLAGS = list(itertools.product((False, True), repeat=3))  # (halation, mtf, pointwise)


def parent_schedule(n, hal, mtf, pointwise):
    """The (stage, band) order of the commit before: its counter loop, with every call replaced by the pair it stands for."""
    order = []
    dens = sharp = tail = 0
    for k in range(n):
        order.append(("front", k))
        if pointwise:
            order.append(("tail", k))
            continue
        moved = True
        while moved:
            moved = False
            if not hal:
                dens = k + 1
            elif dens < n and k + 1 > min(dens + 1, n - 1):
                order.append(("halation", dens))
                dens, moved = dens + 1, True
            if mtf and sharp < n and dens > min(sharp + 1, n - 1):
                order.append(("mtf", sharp))
                sharp, moved = sharp + 1, True
            if tail < (sharp if mtf else dens):
                order.append(("tail", tail))
                tail, moved = tail + 1, True
    return order


def pairs(text):
    return [(s, int(b)) for s, b in (item.split() for item in text.split(", "))]


def test_the_schedule_is_the_loop_of_the_commit_before():
    for n in range(2, 41):
        for hal, mtf, pointwise in FLAGS:
            assert list(stage_schedule(n, hal, mtf, pointwise)) == parent_schedule(n, hal, mtf, pointwise), (n, hal, mtf, pointwise)
    assert list(stage_schedule(3, True, True, False)) == pairs(
        "front 0, front 1, halation 0, front 2, halation 1, mtf 0, tail 0, halation 2, mtf 1, tail 1, mtf 2, tail 2")
    assert list(stage_schedule(2, True, True, False)) == pairs("front 0, front 1, halation 0, halation 1, mtf 0, tail 0, mtf 1, tail 1")
    assert list(stage_schedule(2, False, False, True)) == pairs("front 0, tail 0, front 1, tail 1")


def test_the_schedule_keeps_the_dependence_rule():
    for n in range(2, 41):
        for hal, mtf, pointwise in FLAGS:
            order = list(stage_schedule(n, hal, mtf, pointwise))
            at = {pair: i for i, pair in enumerate(order)}
            assert len(at) == len(order)  # no pair twice
            stages = ["front"] + ["halation"] * (hal and not pointwise) + ["mtf"] * (mtf and not pointwise) + ["tail"]
            assert {s for s, _ in order} == set(stages)
            for s in stages:  # every stage takes the bands 0 .. n - 1 in order, once each
                assert [b for stage, b in order if stage == s] == list(range(n)), (n, hal, mtf, pointwise, s)
            for before, s in zip(stages, stages[1:]):
                for b in range(n):
                    need = b if s == "tail" else min(b + 1, n - 1)  # a stencil reads into the band after its own
                    assert at[(s, b)] > at[(before, need)], (n, hal, mtf, pointwise, s, b)


class Recorder:
    """A context that records its calls: (name, positional arguments, keywords)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *a, **k: self.calls.append((name, a, k))


def same_view(t, of):
    return t.data_ptr() == of.data_ptr() and t.shape == of.shape and t.stride() == of.stride()


def bounds_of(H, bands):
    """Bounds of plan_bands' shape on a frame far below its 64-row floor: two even bands, the last one halved for three."""
    bounds = [0, H // 2, H]
    return bounds if bands == 2 else bounds[:2] + [(bounds[1] + bounds[2]) // 2, H]


BANDS = (2, 3)
H, W = 50, 12


@pytest.mark.parametrize("bands", BANDS)
@pytest.mark.parametrize("chans", (3, 4))
def test_a_float_frame_is_clamped_in_place_band_by_band(bands, chans):
    bounds = bounds_of(H, bands)
    src = band_source(dict(u16_factor=None, clip_on_device=True), (H, W, chans), "torch.float32")
    assert src.frame == (H, W, chans) and (src.landing, src.landing_shape) == ("image", (H, W, chans))  # (an alpha plane stays)
    assert src.upload_bounds(bounds) == bounds and not src.queue_all and src.measure is None
    before = torch.linspace(-70000.0, 70000.0, W * chans).repeat(H, 1).reshape(H, W, chans)  # (every row leaves the range)
    ctx = Recorder()
    for a0, a1 in zip(bounds, bounds[1:]):
        image = before.clone()  # (a fresh frame per band: a touch of any other row shows, above the band as well as below it)
        src.decode(ctx, image, image, a0, a1)
        assert torch.equal(image[a0:a1], before[a0:a1].clamp(0.0, 65504.0)) and not torch.equal(image[a0:a1], before[a0:a1])
        assert torch.equal(image[:a0], before[:a0]) and torch.equal(image[a1:], before[a1:])
    assert ctx.calls == []
    plain = band_source(dict(u16_factor=None, clip_on_device=False), (H, W, chans), "torch.float32")
    image = before.clone()
    plain.decode(ctx, image, image, 0, H)
    assert torch.equal(image, before) and ctx.calls == [] and plain.measure is None and plain.landing == "image"


@pytest.mark.parametrize("bands", BANDS)
def test_a_uint16_frame_with_a_factor_is_decoded_band_by_band(bands):
    bounds = bounds_of(H, bands)
    src = band_source(dict(u16_factor=1.25, u16_window=None), (H, W, 3), "torch.int16")
    assert src.frame == (H, W, 3) and (src.landing, src.landing_shape) == ("u16", (H, W, 3))
    assert src.upload_bounds(bounds) == bounds and not src.queue_all and src.measure is None
    landing, image, ctx = torch.zeros((H, W, 3), dtype=torch.int16), torch.zeros((H, W, 3)), Recorder()
    for a0, a1 in zip(bounds, bounds[1:]):
        src.decode(ctx, landing, image, a0, a1)
    assert len(ctx.calls) == bands
    for (name, args, kw), a0, a1 in zip(ctx.calls, bounds, bounds[1:]):
        assert name == "decode_u16" and len(args) == 2 and args[1] == 1.25 and set(kw) == {"out"}
        assert same_view(args[0], landing[a0:a1]) and same_view(kw["out"], image[a0:a1])


@pytest.mark.parametrize("bands", BANDS)
def test_a_device_exposure_frame_is_measured_whole_then_decoded_through_its_window(bands):
    Hf, Wf, window = H + 37, W + 9, (11, 5, H, W)  # rows above the window, 26 rows below it
    r0, c0, nr, nc = window
    bounds = bounds_of(nr, bands)
    payload = dict(u16_factor="device", u16_window=window, exposure_root=2.5)
    src = band_source(payload, (Hf, Wf, 3), "torch.int16")
    assert src.frame == (nr, nc, 3) and (src.landing, src.landing_shape) == ("u16", (Hf, Wf, 3)) and not src.queue_all
    ub = src.upload_bounds(bounds)
    assert ub == [0] + [r0 + b for b in bounds[1:-1]] + [Hf]
    landing, image, ctx = torch.zeros((Hf, Wf, 3), dtype=torch.int16), torch.zeros((nr, nc, 3)), Recorder()
    src.measure(ctx, landing, ub, lambda k: ctx.calls.append(("wait", (k,), {})))
    for a0, a1 in zip(bounds, bounds[1:]):
        src.decode(ctx, landing, image, a0, a1)
    names = [c[0] for c in ctx.calls]
    assert names == ["wait", "exposure_rows"] * bands + ["exposure_finish"] + ["decode_u16_auto"] * bands
    for k in range(bands):
        wait, (_, args, kw) = ctx.calls[2 * k], ctx.calls[2 * k + 1]
        assert wait == ("wait", (k,), {})
        assert same_view(args[0], landing[ub[k]:ub[k + 1]]) and args[1:] == (2.5,) and kw == dict(H=Hf, gy0=ub[k])
    assert ctx.calls[2 * bands] == ("exposure_finish", (Hf, Wf, 2.5), {})
    for (_, args, kw), a0, a1 in zip(ctx.calls[2 * bands + 1:], bounds, bounds[1:]):
        assert same_view(args[0], landing[r0 + a0:r0 + a1]) and args[1:] == ((0, c0, a1 - a0, nc),)
        assert set(kw) == {"out"} and same_view(kw["out"], image[a0:a1])


@pytest.mark.parametrize("bands", BANDS)
@pytest.mark.parametrize("half", (False, True))
def test_a_mosaic_travels_with_its_demosaics_reach_and_lands_in_the_float_frame(bands, half):
    window = (7, 3, H, W)  # an odd row0
    Hm, Wm = (2 * (H + 20), 2 * (W + 8)) if half else (H + 20, W + 8)
    bounds = bounds_of(H, bands)
    params = SimpleNamespace(half_size=int(half))
    payload = dict(u16_factor=1.5, u16_window=None, demosaic=dict(params=params, window=window, rotate_times=0))
    src = band_source(payload, (Hm, Wm), "torch.int16")
    assert src.frame == (H, W, 3) and (src.landing, src.landing_shape) == ("mosaic", (Hm, Wm)) and src.measure is None
    assert src.upload_bounds(bounds) == mosaic_upload_bounds(bounds, window, Hm, half)
    landing, image, ctx = torch.zeros((Hm, Wm), dtype=torch.int16), torch.zeros((H, W, 3)), Recorder()
    for a0, a1 in zip(bounds, bounds[1:]):
        src.decode(ctx, landing, image, a0, a1)
    assert len(ctx.calls) == bands
    for (name, args, kw), a0, a1 in zip(ctx.calls, bounds, bounds[1:]):
        assert name == "demosaic" and args[0] is landing and args[1] is params and args[2:] == (1.5,)
        assert set(kw) == {"clip", "passes", "window", "out", "rows"} and kw["window"] == window and kw["out"] is image and kw["rows"] == (a0, a1)
        assert kw["clip"] is None and kw["passes"] == 0  # a plain profile: neither Blend nor step M went along
    # only a mosaic has all its uploads queued ahead of the first band
    others = (band_source(dict(u16_factor=None, clip_on_device=True), (H, W, 3), "torch.float32"),
              band_source(dict(u16_factor=1.0), (H, W, 3), "torch.int16"),
              band_source(dict(u16_factor="device", u16_window=(0, 0, H, W), exposure_root=2.0), (H, W, 3), "torch.int16"))
    assert src.queue_all is True and [o.queue_all for o in others] == [False] * 3


def test_the_frame_is_the_one_the_commit_before_set_up():
    """(H, W, chans) of the float frame: _stream_plan's shape -- the window of the uploaded uint16 frame or of the demosaiced one,
    else the tensor's own -- with _stream_buffers' channels, 3 for a uint16 payload and the tensor's own for a float one."""
    def parent(payload, shape, is_u16):
        if payload.get("u16_window") is not None and len(shape) == 3:
            shape = tuple(int(v) for v in payload["u16_window"][2:]) + shape[2:]
        step = payload.get("demosaic")
        if step and step.get("window") is not None:
            shape = tuple(int(v) for v in step["window"][2:]) + (3,)
        return (int(shape[0]), int(shape[1]), 3 if is_u16 else int(shape[2]))

    params = SimpleNamespace(half_size=0)
    for payload, shape, dtype in (
            (dict(u16_factor=None), (300, 200, 3), "torch.float32"),
            (dict(u16_factor=None, clip_on_device=True), (300, 200, 4), "torch.float32"),
            (dict(u16_factor=0.5, u16_window=None), (300, 200, 3), "torch.int16"),
            (dict(u16_factor="device", u16_window=(10, 20, 250, 160), exposure_root=2.0), (300, 200, 3), "torch.int16"),
            (dict(u16_factor="device", u16_window=(0, 0, 300, 200), exposure_root=2.0), (300, 200, 3), "torch.int16"),
            (dict(u16_factor=0.5, demosaic=dict(params=params, window=(3, 5, 250, 160), rotate_times=0)), (300, 200), "torch.int16")):
        src = band_source(payload, shape, dtype)
        assert src.frame == parent(payload, shape, dtype == "torch.int16"), payload
        assert all(type(v) is int for v in src.frame)
