"""The sensor's orientation in the device demosaic: r2f_demosaic_oriented_u16 and r2f_demosaic_xtrans_oriented_u16 against
orient(model.demosaic(...)) -- the NumPy statement of include/r2f.h applied to the frame of tests/demosaic_model.py /
tests/xtrans_model.py --, byte for byte and without a tolerance: all 8 orientations, the four Bayer patterns and the four X-Trans
layouts, frames that span several tiles with ragged edges both ways and one narrower than a tile, full and reduced size; orientation
0 against the upright entry point; rows of O cut at and next to the tile seams, one call at a time; a pitched source at an odd
element offset; and oriented mosaics through HipProcessor against the same call on the oriented model frame."""

import ctypes as C
import dataclasses
import inspect

import numpy as np
import pytest

import demosaic_model as dm
import xtrans_model as xm
from helpers import stocks

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CANARY = 0xA5A5
# (the model, the context's method, the oriented and the upright entry point, the frames: several tiles with ragged edges both ways,
# and for the Bayer pattern one narrower than a tile)
BAYER = ("bayer", dm, "demosaic_u16", "r2f_demosaic_oriented_u16", "r2f_demosaic_u16", ((70, 134), (38, 50)))
XTRANS = ("xtrans", xm, "demosaic_xtrans", "r2f_demosaic_xtrans_oriented_u16", "r2f_demosaic_xtrans_u16", ((71, 137),))
CASES = [(BAYER, p) for p in dm.PATTERNS] + [(XTRANS, p) for p in xm.PATTERNS]
case_id = lambda c: f"{c[0][0]}-{c[1] if isinstance(c[1], str) else c[1][0]}"  # noqa: E731


def orient(D, o):
    """The NumPy statement of include/r2f.h."""
    E = D
    if o & 2:
        E = E[::-1]
    if o & 1:
        E = E[:, ::-1]
    if o & 4:
        E = E.transpose(1, 0, 2)
    return np.ascontiguousarray(E)


@pytest.fixture(scope="module")
def proc():
    from raw2film_amd import HipProcessor

    p = HipProcessor(cameras={}, lenses={}, device=0)
    yield p
    p.close()


_MODEL = {}


def model(kind, pattern, shape, half):
    """(mosaic, profile, the model's upright frame D), computed once per case and shared by the tests."""
    key = (kind[0], pattern, shape, half)
    if key not in _MODEL:
        mosaic, prof = kind[1].fixture("random", pattern, *shape)
        _MODEL[key] = (mosaic, prof, kind[1].demosaic(mosaic, prof, half_size=half))
    return _MODEL[key]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint16)


def cuts_of(rows):
    """Rows of O at and next to the seams of the 32-row and 64-column tiles."""
    if rows in (70, 71):
        return [0, 1, 33, rows]
    if rows in (134, 137):
        return [0, 5, 64, 65, rows]
    return [0, 1, rows // 2 + 1, rows]


@pytest.mark.parametrize("half", [False, True], ids=["full", "reduced"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_orientation_is_the_definition_applied_to_the_models_frame(proc, case, half):
    kind, pattern = case
    for shape in kind[5]:
        mosaic, prof, D = model(kind, pattern, shape, half)
        params, m = prof.plan(*shape, half), dev(mosaic)
        for o in range(8):
            got = host(getattr(proc.ctx, kind[2])(m, params, orientation=o))
            want = orient(D, o)
            assert got.shape == want.shape == ((D.shape[1], D.shape[0], 3) if o & 4 else D.shape)
            assert np.array_equal(got, want), (shape, o, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("half", [False, True], ids=["full", "reduced"])
@pytest.mark.parametrize("kind", [BAYER, XTRANS], ids=lambda k: k[0])
def test_orientation_0_writes_the_bytes_of_the_upright_entry_point(proc, kind, half):
    ctx = proc.ctx
    pattern = kind[1].PATTERNS[2]
    for shape in kind[5]:
        H, W = shape
        mosaic, prof, D = model(kind, pattern, shape, half)
        params, m = prof.plan(H, W, half), dev(mosaic)
        outs = [torch.full(D.shape, CANARY - 65536, dtype=torch.int16, device="cuda") for _ in range(2)]
        assert getattr(ctx._lib, kind[3])(ctx._h, m.data_ptr(), 0, H, W, H, W, C.byref(params), 0, outs[0].data_ptr(), 0, D.shape[0],
                                          ctx._stream()) == 0, ctx._lib.r2f_last_error(ctx._h)
        assert getattr(ctx._lib, kind[4])(ctx._h, m.data_ptr(), 0, H, W, H, W, C.byref(params), outs[1].data_ptr(), 0, D.shape[0],
                                          ctx._stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1]) and np.array_equal(host(outs[0]), D)


@pytest.mark.parametrize("half", [False, True], ids=["full", "reduced"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_rows_of_the_oriented_frame_one_call_at_a_time_are_the_whole_frames_bytes(proc, case, half):
    kind, pattern = case
    for shape in kind[5]:
        mosaic, prof, D = model(kind, pattern, shape, half)
        params, m = prof.plan(*shape, half), dev(mosaic)
        for o in range(8):
            want = orient(D, o)
            cuts = cuts_of(want.shape[0])
            assert cuts == sorted(set(cuts))
            out = torch.full(want.shape, CANARY - 65536, dtype=torch.int16, device="cuda")
            bands = list(zip(cuts[:-1], cuts[1:]))
            for k in np.random.default_rng(o).permutation(len(bands)):  # (in any order)
                before = out.clone()
                y0, y1 = bands[k]
                assert getattr(proc.ctx, kind[2])(m, params, out=out, rows=(y0, y1), orientation=o) is out
                changed = (out != before).any(dim=2).any(dim=1).cpu().numpy()
                assert not changed[:y0].any() and not changed[y1:].any(), (shape, o, y0, y1)
                assert np.array_equal(host(out[y0:y1]), want[y0:y1]), (shape, o, y0, y1)
            assert np.array_equal(host(out), want), (shape, o)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_a_pitched_source_at_an_odd_offset_selects_the_load_path_not_the_bytes(proc, case):
    kind, pattern = case
    shape = kind[5][0]
    H, W = shape
    for half in (False, True):
        mosaic, prof, D = model(kind, pattern, shape, half)
        params = prof.plan(H, W, half)
        flat = torch.full((H * (W + 3) + 2,), 0x1234, dtype=torch.int16, device="cuda")
        view = torch.as_strided(flat, (H, W), (W + 3, 1), 1)
        view.copy_(dev(mosaic))
        assert view.data_ptr() % 4 == 2 and view.stride(0) == W + 3
        for o in range(8):
            got = host(getattr(proc.ctx, kind[2])(view, params, orientation=o))
            assert np.array_equal(got, orient(D, o)), (half, o)


def test_context_method_arguments(proc):
    shape = BAYER[5][0]
    mosaic, prof, D = model(BAYER, "RGGB", shape, False)
    m = dev(mosaic)
    out = torch.zeros((shape[1], shape[0], 3), dtype=torch.int16, device="cuda")
    assert proc.ctx.demosaic_u16(m, prof, out=out, rows=(5, 9), orientation=5) is out  # (a profile: planned full size; out is O's shape)
    got, want = host(out), orient(D, 5)
    assert np.array_equal(got[5:9], want[5:9]) and not got[:5].any() and not got[9:].any()
    # a profile's own orientation is phase 1's to read: the context takes the argument
    assert np.array_equal(host(proc.ctx.demosaic_u16(m, dataclasses.replace(prof, orientation=5))), D)
    for bad in (-1, 8, 1.5, True, "5"):
        with pytest.raises(ValueError, match="orientation"):
            proc.ctx.demosaic_u16(m, prof, orientation=bad)
    with pytest.raises(ValueError):
        proc.ctx.demosaic_u16(m, prof, out=out, orientation=3)  # (the upright shape is wanted)
    with pytest.raises(ValueError):
        proc.ctx.demosaic_u16(m, prof, out=torch.zeros(shape + (3,), dtype=torch.int16, device="cuda"), orientation=6)
    with pytest.raises(Exception, match="rows"):
        proc.ctx.demosaic_u16(m, prof, out=out, rows=(0, shape[1] + 1), orientation=5)
    proc.ctx.demosaic_u16(m, prof, out=out, rows=(shape[0], shape[1]), orientation=5)  # (rows of O: past D's row count)
    assert "orientation" not in inspect.signature(proc.ctx.demosaic_f32).parameters  # (the fused float form stays upright)


# ---------------------------------------------------------------------------------------------- through the processor
KW = dict(halation=False, sharpness=False, grain=0, exp_kelvin=6000, color_masking=1.0, frame_width=36, frame_height=24, max_scale=None)


def _e2e_mosaic(kind, pattern):
    """The 96 x 144 mosaic of the end-to-end tests of tests/test_gpu_demosaic.py / test_gpu_xtrans.py: image-like statistics (a smooth
    ramp plus noise, well inside 14 bits) and a camera-like profile."""
    from raw2film_amd.raw import RawProfile, XTransProfile

    rng = np.random.default_rng(17)
    y, x = np.mgrid[0:96, 0:144]
    base = 600 + 9000 * (0.5 + 0.5 * np.sin(x / 23.0) * np.cos(y / 17.0)) + rng.normal(0, 120, (96, 144))
    mosaic = np.clip(base, 0, 16383).astype(np.uint16)
    cls = RawProfile if kind is BAYER else XTransProfile
    return mosaic, cls(pattern, black=512, multipliers=(7.9, 4.1, 6.2), matrix=((0.52, 0.27, 0.15), (0.25, 0.68, 0.07), (0.03, 0.12, 0.81)))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_an_oriented_mosaic_through_the_processor_equals_the_oriented_model_frame_through_it(proc, case):
    """Orientation 3 at full size (the mirrored class), 5 at reduced size (a lane per pixel), 6 at full size (the turned class)."""
    from raw2film_amd.lens import LensProfile

    kind, pattern = case
    neg, prt, _ = stocks()
    mosaic, upright = _e2e_mosaic(kind, pattern)
    for o, half in ((3, False), (5, True), (6, False)):
        prof = dataclasses.replace(upright, orientation=o)
        rgb = orient(kind[1].demosaic(mosaic, upright, half_size=half), o)
        assert rgb.dtype == np.uint16 and rgb.shape[:2] == prof.oriented_shape(96, 144, half) and 1000 < rgb.mean() < 60000
        kw = dict(print_film=prt, half_size=half, seed=3, **KW)

        def both(mosaic_kw, rgb_kw, **extra):
            a = proc.process(mosaic, neg, 6, 0.4, raw_profile=prof, **mosaic_kw, **extra, **kw)
            b = proc.process(rgb, neg, 6, 0.4, **rgb_kw, **extra, **kw)
            assert a.shape == b.shape and a.dtype == b.dtype
            assert np.array_equal(a, b), (o, mosaic_kw, extra, int((a != b).sum()))
            return a

        plain = both(dict(exposure=0.5), dict(exposure=0.5))
        assert plain.std() > 1 and (plain.shape[0] > plain.shape[1]) == bool(o & 4)  # (a picture; a portrait one when turned)
        both(dict(exposure=None), dict(exposure="device"))  # measured on the device, on O
        assert proc.exposure_rejected is None
        both(dict(exposure=0.5), dict(exposure=0.5), zoom=1.3, rotate_times=1)
        both(dict(exposure=0.5), dict(exposure=0.5), lens_profile=LensProfile("ptlens", (0.02, -0.06, 0.01), scale=1.02))
        # one export: the same file bytes, and stream=True yields the one-piece bytes with the orientation named
        a = proc.process_jpeg(mosaic, neg, 6, 0.4, quality=90, raw_profile=prof, exposure=0.5, **kw)
        b = proc.process_jpeg(rgb, neg, 6, 0.4, quality=90, exposure=0.5, **kw)
        assert a == b and a == proc.encode_jpeg(plain, 90)
        c = proc.process_jpeg(mosaic, neg, 6, 0.4, quality=90, stream=True, raw_profile=prof, exposure=0.5, **kw)
        assert c == a and "demosaic" in proc.stream_rejected and f"orientation = {o}" in proc.stream_rejected
