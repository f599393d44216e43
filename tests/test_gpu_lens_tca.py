"""Lens correction with TCA on the device: r2f_lens_correct_tca against the NumPy model of its definition
(tests/lens_tca_model.py), bit for bit; against r2f_lens_correct on the device where the definition says the two agree; and a
TCA profile through HipProcessor against the oracle render of the model-corrected, cropped frame.  That red and blue really
sample elsewhere than green in these cases is asserted from the model in tests/test_lens_tca_host.py."""

import ctypes as C
import io

import numpy as np
import pytest

import lens_model as lm
import lens_tca_model as tm
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


# A block is 64 x 16 output pixels.  scale-0.25 is the unstaged path (a footprint four times the tile); `edge` on 150 x 210 stages
# the union of three tap boxes that lie several texels apart, and puts red or blue outside where green is inside.
@pytest.mark.parametrize("layout", ["hwc3", "hwc4", "chw"])
@pytest.mark.parametrize("shape", lm.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_lens_correct_tca_is_bit_identical_to_the_model(proc, shape, layout):
    t = torch.from_numpy(_as_layout(lm.frame(*shape), layout)).cuda()
    for name in lm.PROFILE_SPECS:
        for tca in tm.RENDERED:
            got = proc.ctx.lens_correct(t, tm.profile(name, tca), layout=layout).cpu().numpy().transpose(1, 2, 0)
            want = tm.model(name, tca, shape)
            assert np.array_equal(_bits(got), _bits(want)), (name, tca, shape, layout, int((_bits(got) != _bits(want)).sum()))


@pytest.mark.parametrize("layout", ["hwc3", "chw"])
@pytest.mark.parametrize("shape", lm.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_identity_and_green_equal_the_plain_kernel_on_the_device(proc, shape, layout):
    t = torch.from_numpy(_as_layout(lm.frame(*shape), layout)).cuda()
    for name in lm.PROFILE_SPECS:
        plain = proc.ctx.lens_correct(t, lm.profile(name), layout=layout).view(torch.int32)
        for tca in ("identity", ("poly3", (1, 1, 0, 0, 0, 0))):
            got = proc.ctx.lens_correct(t, tm.profile(name, tca), layout=layout).view(torch.int32)
            assert torch.equal(got, plain), (name, tca, shape, layout)
        for tca in tm.RENDERED:
            got = proc.ctx.lens_correct(t, tm.profile(name, tca), layout=layout).view(torch.int32)
            assert torch.equal(got[1], plain[1]), (name, tca, shape, layout)
            if shape == (150, 210):
                assert not torch.equal(got[0], plain[0]) and not torch.equal(got[2], plain[2])


@pytest.mark.parametrize("layout", ["hwc3", "hwc4", "chw"])
def test_windows_equal_the_crop_of_the_full_result_and_may_leave_the_frame(proc, layout):
    H, W = 150, 210
    t = torch.from_numpy(_as_layout(lm.frame(H, W), layout)).cuda()
    for name, tca in (("off-centre", "poly3"), ("scale-0.25", "linear"), ("vignetting", "edge")):
        prof = tm.profile(name, tca)
        full = proc.ctx.lens_correct(t, prof, layout=layout).cpu().numpy()
        for win in ((5, 0, 140, 210), (37, 61, 70, 67), (149, 209, 1, 1)):
            part = proc.ctx.lens_correct(t, prof, win, layout=layout).cpu().numpy()
            assert np.array_equal(_bits(part), _bits(full[:, win[0]:win[0] + win[2], win[1]:win[1] + win[3]])), (name, tca, win)
        for win in ((-9, -70, H + 20, W + 133), (H + 300, -W - 400, 6, 70)):  # straddling every edge; wholly outside
            part = proc.ctx.lens_correct(t, prof, win, layout=layout).cpu().numpy().transpose(1, 2, 0)
            assert np.array_equal(_bits(part), _bits(tm.model(name, tca, (H, W), win))), (name, tca, win)
    outside = proc.ctx.lens_correct(t, tm.profile("none", "linear"), (H + 300, -W - 400, 6, 70), layout=layout)
    assert not bool(outside.any())


def test_params_and_profile_are_the_same_call_and_bad_arguments_are_refused(proc):
    from raw2film_amd import _lib

    t = torch.from_numpy(lm.frame(33, 47)).cuda()
    prof = tm.profile("ptlens", "poly3")
    params, tca = prof.plan_tca(33, 47)
    a = proc.ctx.lens_correct(t, prof)
    b = proc.ctx.lens_correct(t, params, tca=tca)
    assert torch.equal(a, b) and tuple(a.shape) == (3, 33, 47)
    assert torch.equal(proc.ctx.lens_correct(t, params), proc.ctx.lens_correct(t, lm.profile("ptlens")))  # (no tca: the plain call)
    assert tuple(proc.ctx.lens_correct(t, prof, (3, 4, 0, 9)).shape) == (3, 0, 9)
    with pytest.raises(ValueError, match="tca"):
        proc.ctx.lens_correct(t, prof, tca=tca)
    ctx = proc.ctx
    out = torch.full((3, 33, 47), -7.0, device="cuda")
    pd = ctx.planes(out, 0)

    def call(params, tca, rows=33):
        return ctx._lib.r2f_lens_correct_tca(ctx._h, t.data_ptr(), 0, 33, 47, C.byref(params), C.byref(tca), C.byref(pd), rows, 47, 0, 0,
                                             ctx._stream())

    assert call(params, _lib.LensTcaParams(model=_lib.TCA_NONE)) == _lib.EINVAL and b"r2f_lens_correct" in ctx._lib.r2f_last_error(ctx._h)
    for model in (3, -1):
        assert call(params, _lib.LensTcaParams(model=model)) == _lib.EINVAL
    bad = prof.plan(33, 47)
    bad.model = 9
    assert call(bad, tca) == _lib.EINVAL and b"model" in ctx._lib.r2f_last_error(ctx._h)
    assert call(params, tca, rows=34) == _lib.EINVAL  # rows outside the destination
    assert ctx._lib.r2f_lens_correct_tca(ctx._h, t.data_ptr(), 0, 33, 47, C.byref(params), None, C.byref(pd), 33, 47, 0, 0,
                                         ctx._stream()) == _lib.EINVAL
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())  # a refused call writes nothing
    assert call(params, tca) == _lib.OK
    assert torch.equal(out, a)


# ---------------------------------------------------------------------------------------------- through the processor
def _xyz(H, W, seed=41):
    return st.apply_matrix3x3(synthetic_frame(H, W, seed=seed), st.REC709_TO_XYZ)


def _u8_close(a, b):  # (test_free_rotation_through_the_processor's comparison)
    d = np.abs(a.astype(int) - b.astype(int))
    return d.max() <= 1 and (d > 0).mean() <= 1e-4


PROFILE_KW = dict(distortion="ptlens", coefficients=(0.02, -0.06, 0.01), vignetting=(-0.3, 0.1, -0.02), scale=1.02)
KW = dict(halation=False, sharpness=False, grain=0, exp_kelvin=6000, color_masking=1.0, frame_width=36, frame_height=24, max_scale=None)


def _oracle(img, profile, rotation=0.0, zoom=1.0, k=0):
    """raw_conversion.crop_rotate_zoom of the model-corrected frame, rendered by the oracle (tests/test_gpu_lens.py's, with TCA)."""
    from raw2film_amd import geometry

    neg, prt, _ = stocks()
    H, W = img.shape[:2]
    corrected = tm.correct_tca(img, lm.rounded(lm.constants(profile, H, W)), tm.record(profile, np.float32))
    r0, c0, nr, nc = geometry.crop_box(H, W, 1, 1.5, False)
    pre = np.ascontiguousarray(corrected[r0:r0 + nr, c0:c0 + nc])
    if rotation:
        pre = st.rotate(pre, rotation)
    z = geometry.crop_box(pre.shape[0], pre.shape[1], zoom, 1.5, False)
    pre = np.ascontiguousarray(np.rot90(pre[z[0]:z[0] + z[2], z[1]:z[1] + z[3]], k))
    p = oracle_inputs(neg, prt, max(pre.shape[:2]) / 36, halation=False, mtf=False, grain=0, matrix=False)
    return st.to_uint8(st.render(pre, p))


@pytest.mark.parametrize("geo,tca", [(dict(), "linear"), (dict(rotation=3.5, zoom=1.3, rotate_times=1), "poly3")], ids=["plain", "rotated"])
def test_tca_profile_through_the_processor(proc, geo, tca):
    from raw2film_amd.lens import LensProfile

    neg, prt, _ = stocks()
    img = _xyz(150, 210, seed=45)
    profile = LensProfile(**PROFILE_KW, tca=tm.TCA_SPECS[tca])
    ref = _oracle(img, profile, geo.get("rotation", 0.0), geo.get("zoom", 1.0), geo.get("rotate_times", 0))
    out = proc.process(img, neg, 6, 0.4, print_film=prt, lens_profile=profile, **geo, **KW)
    assert out.shape == ref.shape
    assert _u8_close(out, ref)
    # the TCA step is not a no-op on this frame, and lens_correction=False ignores the whole profile
    without = proc.process(img, neg, 6, 0.4, print_film=prt, lens_profile=LensProfile(**PROFILE_KW), **geo, **KW)
    assert without.shape == out.shape and not _u8_close(out, without)
    off = proc.process(img, neg, 6, 0.4, print_film=prt, lens_profile=profile, lens_correction=False, **geo, **KW)
    assert np.array_equal(off, proc.process(img, neg, 6, 0.4, print_film=prt, **geo, **KW))
    # the two-phase API gives the same bytes
    pay = proc.extract_image_data_cpu(img, lens_profile=profile, frame_width=36, frame_height=24, max_scale=None, **geo)
    assert pay["image_array"].shape[:2] == (150, 210) and "tca" in pay["lens"]
    two = proc.process_preloaded(pay, neg, 6, 0.4, final_scaling="cpu", print_film=prt, **KW)
    assert np.array_equal(two, out)


def test_tca_profile_on_a_uint16_source(proc):
    from raw2film_amd import decode
    from raw2film_amd.lens import LensProfile

    neg, prt, _ = stocks()
    u16 = (np.random.default_rng(11).uniform(0, 1, (150, 210, 3)) ** 3 * 20000).astype(np.uint16)
    profile = LensProfile(**PROFILE_KW, tca=tm.TCA_SPECS["poly3"])
    kw = dict(print_film=prt, lens_profile=profile, zoom=1.3, **KW)
    out = proc.process(u16, neg, 6, 0.4, exposure=0.5, **kw)
    ref = _oracle(decode.decode_u16_host(u16, 0.5), profile, zoom=1.3)
    assert out.shape == ref.shape
    assert _u8_close(out, ref)


def test_tca_profile_behind_a_mosaic_source(proc):
    """A Bayer mosaic demosaiced on the device, then the TCA lens step: the bytes of the same call on the demosaic model's frame."""
    import demosaic_model as dm
    from raw2film_amd.lens import LensProfile
    from raw2film_amd.raw import RawProfile

    neg, prt, _ = stocks()
    y, x = np.mgrid[0:96, 0:144]
    base = 600 + 9000 * (0.5 + 0.5 * np.sin(x / 23.0) * np.cos(y / 17.0)) + np.random.default_rng(17).normal(0, 120, (96, 144))
    mosaic = np.clip(base, 0, 16383).astype(np.uint16)
    raw = RawProfile("RGGB", black=512, multipliers=(7.9, 4.1, 6.2), matrix=((0.52, 0.27, 0.15), (0.25, 0.68, 0.07), (0.03, 0.12, 0.81)))
    rgb = dm.demosaic(mosaic, raw, half_size=False)
    profile = LensProfile(**PROFILE_KW, tca=tm.TCA_SPECS["linear"])
    kw = dict(print_film=prt, exposure=0.5, half_size=False, seed=3, zoom=1.2, **KW)
    a = proc.process(mosaic, neg, 6, 0.4, raw_profile=raw, lens_profile=profile, **kw)
    b = proc.process(rgb, neg, 6, 0.4, lens_profile=profile, **kw)
    assert a.shape == b.shape and np.array_equal(a, b)
    assert not np.array_equal(a, proc.process(rgb, neg, 6, 0.4, lens_profile=LensProfile(**PROFILE_KW), **kw))


def test_process_jpeg_is_encode_jpeg_of_the_process_result(proc):
    from PIL import Image

    from raw2film_amd.lens import LensProfile

    neg, prt, _ = stocks()
    img = _xyz(150, 210, seed=45)
    profile = LensProfile(**PROFILE_KW, tca=tm.TCA_SPECS["linear"])
    out = proc.process(img, neg, 6, 0.4, print_film=prt, lens_profile=profile, seed=3, **KW)
    data = proc.process_jpeg(img, neg, 6, 0.4, quality=90, print_film=prt, lens_profile=profile, seed=3, **KW)
    assert data == proc.encode_jpeg(out, 90)
    assert Image.open(io.BytesIO(data)).size == (out.shape[1], out.shape[0])
    # stream=True never streams a lens-corrected frame, and says why in the lens step's unchanged words
    data2 = proc.process_jpeg(img, neg, 6, 0.4, quality=90, stream=True, print_film=prt, lens_profile=profile, seed=3, **KW)
    why = proc.stream_rejected
    assert data2 == data and "lens" in why
    proc.process_jpeg(img, neg, 6, 0.4, quality=90, stream=True, print_film=prt, lens_profile=LensProfile(**PROFILE_KW), seed=3, **KW)
    assert proc.stream_rejected == why
