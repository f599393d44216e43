"""Lens correction on the device: r2f_lens_correct against the NumPy model of its definition (tests/lens_model.py), bit for bit,
and a lens profile through HipProcessor against the oracle render of the model-corrected, cropped frame."""

import io

import numpy as np
import pytest

import lens_model as lm
from helpers import oracle_inputs, stocks, synthetic_frame
from oracle import stages as st

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def proc():
    from raw2film_amd import HipProcessor

    p = HipProcessor(cameras={}, lenses={}, device=0)
    yield p
    p.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _as_layout(img, layout):
    if layout == "hwc3":
        return img
    if layout == "hwc4":
        return np.concatenate([img, np.full(img.shape[:2] + (1,), 7.0, np.float32)], -1)  # (a fourth channel is ignored)
    return np.ascontiguousarray(img.transpose(2, 0, 1))


_MODEL = {}


def model(name, shape, window=None):
    """The model's result, computed once per case and shared by the layouts."""
    key = (name, shape, window)
    if key not in _MODEL:
        c = lm.rounded(lm.constants(lm.profile(name), *shape))
        _MODEL[key] = lm.correct(lm.frame(*shape), c, window)
    return _MODEL[key]


# A block is 64 x 4 output pixels.  Its source footprint is slightly larger than that tile for the mild distortions, several times
# larger at scale 0.25 (where most blocks of the frame also land wholly outside it), and on 150 x 210 / 96 x 128 the blocks of the
# frame's border straddle each edge; the windows below add blocks that reach past every edge and a window wholly outside.
@pytest.mark.parametrize("layout", ["hwc3", "hwc4", "chw"])
@pytest.mark.parametrize("shape", lm.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_lens_correct_is_bit_identical_to_the_model(proc, shape, layout):
    t = torch.from_numpy(_as_layout(lm.frame(*shape), layout)).cuda()
    for name in lm.PROFILE_SPECS:
        got = proc.ctx.lens_correct(t, lm.profile(name), layout=layout).cpu().numpy().transpose(1, 2, 0)
        want = model(name, shape)
        assert np.array_equal(_bits(got), _bits(want)), (name, shape, layout, int((_bits(got) != _bits(want)).sum()))


@pytest.mark.parametrize("layout", ["hwc3", "hwc4", "chw"])
def test_windows_equal_the_crop_of_the_full_result_and_may_leave_the_frame(proc, layout):
    H, W = 150, 210
    t = torch.from_numpy(_as_layout(lm.frame(H, W), layout)).cuda()
    for name in ("off-centre", "scale-0.25", "vignetting"):
        prof = lm.profile(name)
        full = proc.ctx.lens_correct(t, prof, layout=layout).cpu().numpy()
        for win in ((5, 0, 140, 210), (37, 61, 70, 67), (149, 209, 1, 1)):
            part = proc.ctx.lens_correct(t, prof, win, layout=layout).cpu().numpy()
            assert np.array_equal(_bits(part), _bits(full[:, win[0]:win[0] + win[2], win[1]:win[1] + win[3]])), (name, win)
        for win in ((-9, -70, H + 20, W + 133), (H + 300, -W - 400, 6, 70)):  # straddling every edge; wholly outside
            part = proc.ctx.lens_correct(t, prof, win, layout=layout).cpu().numpy().transpose(1, 2, 0)
            assert np.array_equal(_bits(part), _bits(model(name, (H, W), win))), (name, win)
    outside = proc.ctx.lens_correct(t, lm.profile("none"), (H + 300, -W - 400, 6, 70), layout=layout)
    assert not bool(outside.any())


def test_params_and_profile_are_the_same_call_and_bad_arguments_are_refused(proc):
    t = torch.from_numpy(lm.frame(33, 47)).cuda()
    prof = lm.profile("ptlens")
    a = proc.ctx.lens_correct(t, prof)
    b = proc.ctx.lens_correct(t, prof.plan(33, 47))
    assert torch.equal(a, b) and tuple(a.shape) == (3, 33, 47)
    assert tuple(proc.ctx.lens_correct(t, prof, (3, 4, 0, 9)).shape) == (3, 0, 9)
    bad = prof.plan(33, 47)
    bad.model = 9
    with pytest.raises(Exception, match="model"):
        proc.ctx.lens_correct(t, bad)
    with pytest.raises(ValueError):
        proc.ctx.lens_correct(t.cpu(), prof)


# ---------------------------------------------------------------------------------------------- through the processor
def _xyz(H, W, seed=41):
    return st.apply_matrix3x3(synthetic_frame(H, W, seed=seed), st.REC709_TO_XYZ)


def _u8_close(a, b):  # (test_free_rotation_through_the_processor's comparison)
    d = np.abs(a.astype(int) - b.astype(int))
    return d.max() <= 1 and (d > 0).mean() <= 1e-4


PROFILE_KW = dict(distortion="ptlens", coefficients=(0.02, -0.06, 0.01), vignetting=(-0.3, 0.1, -0.02), scale=1.02)
KW = dict(halation=False, sharpness=False, grain=0, exp_kelvin=6000, color_masking=1.0, frame_width=36, frame_height=24, max_scale=None)


def _oracle(img, profile, rotation=0.0, zoom=1.0, k=0):
    """raw_conversion.crop_rotate_zoom of the model-corrected frame, rendered by the oracle."""
    from raw2film_amd import geometry

    neg, prt, _ = stocks()
    H, W = img.shape[:2]
    corrected = lm.correct(img, lm.rounded(lm.constants(profile, H, W)))
    r0, c0, nr, nc = geometry.crop_box(H, W, 1, 1.5, False)
    pre = np.ascontiguousarray(corrected[r0:r0 + nr, c0:c0 + nc])
    if rotation:
        pre = st.rotate(pre, rotation)
    z = geometry.crop_box(pre.shape[0], pre.shape[1], zoom, 1.5, False)
    pre = np.ascontiguousarray(np.rot90(pre[z[0]:z[0] + z[2], z[1]:z[1] + z[3]], k))
    p = oracle_inputs(neg, prt, max(pre.shape[:2]) / 36, halation=False, mtf=False, grain=0, matrix=False)
    return st.to_uint8(st.render(pre, p))


@pytest.mark.parametrize("geo", [dict(), dict(rotation=3.5, zoom=1.3, rotate_times=1), dict(zoom=1.3, rotate_times=3)],
                         ids=["plain", "rotated", "zoomed-turned"])
def test_profile_through_the_processor(proc, geo):
    from raw2film_amd.lens import LensProfile

    neg, prt, _ = stocks()
    img = _xyz(150, 210, seed=45)
    profile = LensProfile(**PROFILE_KW)
    ref = _oracle(img, profile, geo.get("rotation", 0.0), geo.get("zoom", 1.0), geo.get("rotate_times", 0))
    out = proc.process(img, neg, 6, 0.4, print_film=prt, lens_profile=profile, **geo, **KW)
    assert out.shape == ref.shape
    assert _u8_close(out, ref)
    # the correction is not a no-op on this frame, and lens_correction=False ignores the profile
    plain = proc.process(img, neg, 6, 0.4, print_film=prt, **geo, **KW)
    assert plain.shape == out.shape and not _u8_close(out, plain)
    off = proc.process(img, neg, 6, 0.4, print_film=prt, lens_profile=profile, lens_correction=False, **geo, **KW)
    assert np.array_equal(off, plain)
    # the two-phase API gives the same bytes
    pay = proc.extract_image_data_cpu(img, lens_profile=profile, frame_width=36, frame_height=24, max_scale=None, **geo)
    assert pay["image_array"].shape[:2] == (150, 210)
    two = proc.process_preloaded(pay, neg, 6, 0.4, final_scaling="cpu", print_film=prt, **KW)
    assert np.array_equal(two, out)


def test_profile_on_a_uint16_source(proc):
    from raw2film_amd import decode
    from raw2film_amd.lens import LensProfile

    neg, prt, _ = stocks()
    u16 = (np.random.default_rng(11).uniform(0, 1, (150, 210, 3)) ** 3 * 20000).astype(np.uint16)
    profile = LensProfile(**PROFILE_KW)
    kw = dict(print_film=prt, lens_profile=profile, zoom=1.3, **KW)
    out = proc.process(u16, neg, 6, 0.4, exposure=0.5, **kw)
    ref = _oracle(decode.decode_u16_host(u16, 0.5), profile, zoom=1.3)
    assert out.shape == ref.shape
    assert _u8_close(out, ref)
    # exposure="device" stays valid: the frame is measured and decoded whole, then corrected -- the render of the stops it measured
    auto = proc.process(u16, neg, 6, 0.4, exposure="device", **kw)
    assert proc.exposure_rejected is None
    assert np.array_equal(auto, proc.process(u16, neg, 6, 0.4, exposure=proc.last_auto_exposure, **kw))


def test_process_jpeg_is_encode_jpeg_of_the_process_result(proc):
    from PIL import Image

    from raw2film_amd.lens import LensProfile

    neg, prt, _ = stocks()
    img = _xyz(150, 210, seed=45)
    profile = LensProfile(**PROFILE_KW)
    out = proc.process(img, neg, 6, 0.4, print_film=prt, lens_profile=profile, seed=3, **KW)
    data = proc.process_jpeg(img, neg, 6, 0.4, quality=90, print_film=prt, lens_profile=profile, seed=3, **KW)
    assert data == proc.encode_jpeg(out, 90)
    assert Image.open(io.BytesIO(data)).size == (out.shape[1], out.shape[0])
    # stream=True never streams a lens-corrected frame, and says why
    data2 = proc.process_jpeg(img, neg, 6, 0.4, quality=90, stream=True, print_film=prt, lens_profile=profile, seed=3, **KW)
    assert data2 == data and "lens" in proc.stream_rejected
