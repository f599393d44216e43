"""The projected lens correction on the device: r2f_lens_correct_projected against the NumPy model of its definition
(tests/lens_projection_model.py), bit for bit; against r2f_lens_correct / r2f_lens_correct_tca on the device where the definition
says they agree; and a projected profile through HipProcessor against the oracle render of the model-corrected, cropped frame.  That
the projection really moves the coordinates in these cases, that the fisheye record takes both branches of the stated atan and which
staging route each tile takes are asserted from the model in tests/test_lens_projection_host.py."""

import ctypes as C
import io

import numpy as np
import pytest

import lens_model as lm
import lens_projection_model as pm
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


# A block is 64 x 16 output pixels.  On 150 x 210 the cases reach every staging route: whole tiles (every record at scale 1, the
# fisheye at its auto scale), two halves with a box each (the equisolid record at its auto scale) and global gathers (scale 0.25).
@pytest.mark.parametrize("layout", ["hwc3", "hwc4", "chw"])
@pytest.mark.parametrize("shape", lm.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_lens_correct_projected_is_bit_identical_to_the_model(proc, shape, layout):
    t = torch.from_numpy(_as_layout(lm.frame(*shape), layout)).cuda()
    for name, projection, tca, changes in pm.cases(shape):
        got = proc.ctx.lens_correct(t, pm.profile(name, projection, tca, **changes), layout=layout).cpu().numpy().transpose(1, 2, 0)
        want = pm.model(name, projection, tca, shape, **changes)
        assert np.array_equal(_bits(got), _bits(want)), (name, projection, tca, changes, shape, layout, int((_bits(got) != _bits(want)).sum()))


@pytest.mark.parametrize("layout", ["hwc3", "chw"])
@pytest.mark.parametrize("shape", lm.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_identity_records_equal_the_unprojected_kernels_on_the_device(proc, shape, layout):
    t = torch.from_numpy(_as_layout(lm.frame(*shape), layout)).cuda()
    for name in lm.PROFILE_SPECS:
        plain = proc.ctx.lens_correct(t, lm.profile(name), layout=layout).view(torch.int32)
        with_tca = proc.ctx.lens_correct(t, tm.profile(name, "poly3"), layout=layout).view(torch.int32)
        for kind in pm.TYPES:
            got = proc.ctx.lens_correct(t, pm.profile(name, (kind, pm.IDENTITY_FOCAL)), layout=layout).view(torch.int32)
            assert torch.equal(got, plain), (name, kind, shape, layout)
            got = proc.ctx.lens_correct(t, pm.profile(name, (kind, pm.IDENTITY_FOCAL), "poly3"), layout=layout).view(torch.int32)
            assert torch.equal(got, with_tca), (name, kind, shape, layout)
    if shape == (150, 210):  # a real projection is no identity, with a TCA record or without
        for projection in pm.PROJECTIONS:
            got = proc.ctx.lens_correct(t, pm.profile("ptlens", projection, "poly3"), layout=layout).view(torch.int32)
            unprojected = proc.ctx.lens_correct(t, tm.profile("ptlens", "poly3"), layout=layout).view(torch.int32)
            assert not any(torch.equal(got[ch], unprojected[ch]) for ch in range(3)), projection


@pytest.mark.parametrize("layout", ["hwc3", "hwc4", "chw"])
def test_windows_equal_the_crop_of_the_full_result_and_may_leave_the_frame(proc, layout):
    H, W = 150, 210
    t = torch.from_numpy(_as_layout(lm.frame(H, W), layout)).cuda()
    for name, projection, tca, changes in (("off-centre", "fisheye", "poly3", {}), ("none", "fisheye", None, dict(scale=0.25)),
                                           ("vignetting", "stereographic", "edge", {}), ("none", "equisolid", None, dict(scale="auto"))):
        prof = pm.profile(name, projection, tca, **changes)
        full = proc.ctx.lens_correct(t, prof, layout=layout).cpu().numpy()
        for win in ((5, 0, 140, 210), (37, 61, 70, 67), (149, 209, 1, 1)):
            part = proc.ctx.lens_correct(t, prof, win, layout=layout).cpu().numpy()
            assert np.array_equal(_bits(part), _bits(full[:, win[0]:win[0] + win[2], win[1]:win[1] + win[3]])), (name, projection, tca, win)
            assert np.array_equal(_bits(part.transpose(1, 2, 0)), _bits(pm.model(name, projection, tca, (H, W), win, **changes))), (name, win)
        for win in ((-9, -70, H + 20, W + 133), (H + 300, -W - 400, 6, 70)):  # straddling every edge; wholly outside
            part = proc.ctx.lens_correct(t, prof, win, layout=layout).cpu().numpy().transpose(1, 2, 0)
            assert np.array_equal(_bits(part), _bits(pm.model(name, projection, tca, (H, W), win, **changes))), (name, projection, tca, win)


def test_params_and_profile_are_the_same_call_and_bad_arguments_are_refused(proc):
    from raw2film_amd import _lib

    t = torch.from_numpy(lm.frame(33, 47)).cuda()
    prof = pm.profile("ptlens", "fisheye", "poly3")
    params, proj, tca = prof.plan_projected(33, 47)
    a = proc.ctx.lens_correct(t, prof)
    b = proc.ctx.lens_correct(t, params, tca=tca, projection=proj)
    assert torch.equal(a, b) and tuple(a.shape) == (3, 33, 47)
    no_tca = pm.profile("ptlens", "fisheye")
    assert torch.equal(proc.ctx.lens_correct(t, params, projection=proj), proc.ctx.lens_correct(t, no_tca))
    assert torch.equal(proc.ctx.lens_correct(t, params, tca=tca), proc.ctx.lens_correct(t, tm.profile("ptlens", "poly3")))  # (no projection)
    assert tuple(proc.ctx.lens_correct(t, prof, (3, 4, 0, 9)).shape) == (3, 0, 9)
    with pytest.raises(ValueError, match="projection"):
        proc.ctx.lens_correct(t, prof, projection=proj)
    with pytest.raises(ValueError, match="tca"):
        proc.ctx.lens_correct(t, prof, tca=tca)
    ctx = proc.ctx
    out = torch.full((3, 33, 47), -7.0, device="cuda")
    pd = ctx.planes(out, 0)

    def call(params, proj, tca, rows=33):
        return ctx._lib.r2f_lens_correct_projected(ctx._h, t.data_ptr(), 0, 33, 47, C.byref(params), None if proj is None else C.byref(proj),
                                                   None if tca is None else C.byref(tca), C.byref(pd), rows, 47, 0, 0, ctx._stream())

    none = _lib.LensProjectionParams(type=_lib.PROJ_NONE, inv_focal=1.0)
    assert call(params, none, tca) == _lib.EINVAL
    why = ctx._lib.r2f_last_error(ctx._h)
    assert b"r2f_lens_correct" in why and b"r2f_lens_correct_tca" in why
    for kind in (5, -1):
        assert call(params, _lib.LensProjectionParams(type=kind, inv_focal=1.0), None) == _lib.EINVAL
    assert call(params, None, tca) == _lib.EINVAL
    assert call(params, proj, _lib.LensTcaParams(model=_lib.TCA_NONE)) == _lib.EINVAL and b"TCA" in ctx._lib.r2f_last_error(ctx._h)
    for model in (3, -1):
        assert call(params, proj, _lib.LensTcaParams(model=model)) == _lib.EINVAL
    bad = prof.plan(33, 47)
    bad.model = 9
    assert call(bad, proj, tca) == _lib.EINVAL and b"model" in ctx._lib.r2f_last_error(ctx._h)
    assert call(params, proj, tca, rows=34) == _lib.EINVAL  # rows outside the destination
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())  # a refused call writes nothing
    assert call(params, proj, tca) == _lib.OK
    assert torch.equal(out, a)
    assert call(params, proj, None) == _lib.OK
    assert torch.equal(out, proc.ctx.lens_correct(t, no_tca))


# ---------------------------------------------------------------------------------------------- through the processor
def _xyz(H, W, seed=41):
    return st.apply_matrix3x3(synthetic_frame(H, W, seed=seed), st.REC709_TO_XYZ)


def _u8_close(a, b):  # (test_free_rotation_through_the_processor's comparison)
    d = np.abs(a.astype(int) - b.astype(int))
    return d.max() <= 1 and (d > 0).mean() <= 1e-4


PROFILE_KW = dict(distortion="ptlens", coefficients=(0.02, -0.06, 0.01), vignetting=(-0.3, 0.1, -0.02), scale=0.8)
KW = dict(halation=False, sharpness=False, grain=0, exp_kelvin=6000, color_masking=1.0, frame_width=36, frame_height=24, max_scale=None)


def _corrected(img, profile):
    H, W = img.shape[:2]
    return pm.correct(img, lm.rounded(lm.constants(profile, H, W)), pm.record(profile),
                      None if profile.tca is None else tm.record(profile, np.float32))


def _oracle(img, profile, rotation=0.0, zoom=1.0, k=0):
    """raw_conversion.crop_rotate_zoom of the model-corrected frame, rendered by the oracle (tests/test_gpu_lens_tca.py's, projected)."""
    from raw2film_amd import geometry

    neg, prt, _ = stocks()
    H, W = img.shape[:2]
    corrected = _corrected(img, profile)
    r0, c0, nr, nc = geometry.crop_box(H, W, 1, 1.5, False)
    pre = np.ascontiguousarray(corrected[r0:r0 + nr, c0:c0 + nc])
    if rotation:
        pre = st.rotate(pre, rotation)
    z = geometry.crop_box(pre.shape[0], pre.shape[1], zoom, 1.5, False)
    pre = np.ascontiguousarray(np.rot90(pre[z[0]:z[0] + z[2], z[1]:z[1] + z[3]], k))
    p = oracle_inputs(neg, prt, max(pre.shape[:2]) / 36, halation=False, mtf=False, grain=0, matrix=False)
    return st.to_uint8(st.render(pre, p))


@pytest.mark.parametrize("geo,tca", [(dict(), None), (dict(rotation=3.5, zoom=1.3, rotate_times=1), "poly3")], ids=["plain", "rotated"])
def test_projected_profile_through_the_processor(proc, geo, tca):
    from raw2film_amd.lens import LensProfile

    neg, prt, _ = stocks()
    img = _xyz(150, 210, seed=45)
    profile = LensProfile(**PROFILE_KW, projection=pm.PROJECTIONS["fisheye"], tca=None if tca is None else tm.TCA_SPECS[tca])
    ref = _oracle(img, profile, geo.get("rotation", 0.0), geo.get("zoom", 1.0), geo.get("rotate_times", 0))
    out = proc.process(img, neg, 6, 0.4, print_film=prt, lens_profile=profile, **geo, **KW)
    assert out.shape == ref.shape
    assert _u8_close(out, ref)
    # the projection is not a no-op on this frame, and lens_correction=False ignores the whole profile
    without = proc.process(img, neg, 6, 0.4, print_film=prt, lens_profile=LensProfile(**PROFILE_KW, tca=profile.tca), **geo, **KW)
    assert without.shape == out.shape and not _u8_close(out, without)
    off = proc.process(img, neg, 6, 0.4, print_film=prt, lens_profile=profile, lens_correction=False, **geo, **KW)
    assert np.array_equal(off, proc.process(img, neg, 6, 0.4, print_film=prt, **geo, **KW))
    # the two-phase API gives the same bytes
    pay = proc.extract_image_data_cpu(img, lens_profile=profile, frame_width=36, frame_height=24, max_scale=None, **geo)
    assert pay["image_array"].shape[:2] == (150, 210) and "projection" in pay["lens"] and ("tca" in pay["lens"]) == (tca is not None)
    two = proc.process_preloaded(pay, neg, 6, 0.4, final_scaling="cpu", print_film=prt, **KW)
    assert np.array_equal(two, out)


def test_projected_profile_with_max_scale_round_trip(proc):
    """The `max_scale` pipeline resolution and the LANCZOS4 way back work as they do without a projection: the call's shape is the
    unprojected call's, and its bytes differ."""
    from raw2film_amd.lens import LensProfile

    neg, prt, _ = stocks()
    img = _xyz(150, 210, seed=45)
    kw = dict(KW, max_scale=2.0)
    out = proc.process(img, neg, 6, 0.4, print_film=prt, lens_profile=LensProfile(**PROFILE_KW, projection=pm.PROJECTIONS["fisheye"]), **kw)
    plain = proc.process(img, neg, 6, 0.4, print_film=prt, lens_profile=LensProfile(**PROFILE_KW), **kw)
    assert out.shape == plain.shape and not _u8_close(out, plain)


def test_projected_profile_on_a_uint16_source(proc):
    from raw2film_amd import decode
    from raw2film_amd.lens import LensProfile

    neg, prt, _ = stocks()
    u16 = (np.random.default_rng(11).uniform(0, 1, (150, 210, 3)) ** 3 * 20000).astype(np.uint16)
    profile = LensProfile(**PROFILE_KW, projection=pm.PROJECTIONS["stereographic"], tca=tm.TCA_SPECS["poly3"])
    kw = dict(print_film=prt, lens_profile=profile, zoom=1.3, **KW)
    out = proc.process(u16, neg, 6, 0.4, exposure=0.5, **kw)
    ref = _oracle(decode.decode_u16_host(u16, 0.5), profile, zoom=1.3)
    assert out.shape == ref.shape
    assert _u8_close(out, ref)


def test_projected_profile_behind_a_mosaic_source(proc):
    """A Bayer mosaic demosaiced on the device, then the projected lens step: the bytes of the same call on the demosaic model's frame."""
    import demosaic_model as dm
    from raw2film_amd.lens import LensProfile
    from raw2film_amd.raw import RawProfile

    neg, prt, _ = stocks()
    y, x = np.mgrid[0:96, 0:144]
    base = 600 + 9000 * (0.5 + 0.5 * np.sin(x / 23.0) * np.cos(y / 17.0)) + np.random.default_rng(17).normal(0, 120, (96, 144))
    mosaic = np.clip(base, 0, 16383).astype(np.uint16)
    raw = RawProfile("RGGB", black=512, multipliers=(7.9, 4.1, 6.2), matrix=((0.52, 0.27, 0.15), (0.25, 0.68, 0.07), (0.03, 0.12, 0.81)))
    rgb = dm.demosaic(mosaic, raw, half_size=False)
    profile = LensProfile(**PROFILE_KW, projection=pm.PROJECTIONS["equisolid"])
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
    profile = LensProfile(**PROFILE_KW, projection=pm.PROJECTIONS["fisheye"])
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
