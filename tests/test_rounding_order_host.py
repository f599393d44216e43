"""The power of tests/test_gpu_rounding_order.py, shown without a GPU.  Those tests hold the device equal, bit for bit, to the form of
tests/rounding_model.py in which a product and the sum that takes it round separately.  A kernel that contracted the pair into one fused
multiply-add would differ from that form only where the product's own rounding decides the sum's last bit -- so the inputs have to be
ones where it often does.  Here the model's fused restatement is compared with the separate one on the very inputs the GPU tests use:
it must differ on at least 10 % of the warp's samples and 5 % of the grain's (conditions the inputs were chosen to meet, not
measurements; the shares are printed)."""

import numpy as np
import pytest

from oracle import stages as st
from raw2film_amd import geometry

import rounding_model as rm


def _warp_cases(shape, deg):
    H, W = shape
    m, win = geometry.rotation_plan(H, W, deg)
    return m, (("full", None, (0, 0)), ("window", tuple(win[2:]), tuple(win[:2])))


@pytest.mark.parametrize("kind", rm.WARP_FRAMES)
@pytest.mark.parametrize("shape", rm.WARP_SHAPES)
def test_the_separate_warp_lerp_is_the_oracle_and_a_fused_one_is_not(shape, kind):
    """warp_taps + warp_lerp restate st.warp_affine_linear bit for bit at every angle, shape and window of the GPU test; with fused
    steps the result changes on >= 10 % of the samples at every oblique angle on the (97, 131) frames."""
    img = rm.warp_frame(kind, *shape)
    for deg in rm.WARP_ANGLES:
        m, cases = _warp_cases(shape, deg)
        for name, out_shape, offset in cases:
            if out_shape is not None and 0 in out_shape:
                continue
            ref = st.warp_affine_linear(img, m, out_shape, offset)
            taps = rm.warp_taps(img, m, out_shape, offset)
            sep = rm.warp_lerp(*taps)
            assert np.array_equal(sep, ref), (shape, kind, deg, name)
            assert np.isfinite(ref).all()
            share = rm.differing_share(sep, rm.warp_lerp(*taps, fused=True))
            print(f"warp {kind} {shape} {deg:6.1f} deg {name:6s}: fused != separate on {100 * share:5.1f} % of {ref.size} samples")
            if shape == rm.WARP_POWER_SHAPE and deg in rm.WARP_OBLIQUE:
                assert share >= rm.WARP_MIN_SHARE, (kind, deg, name, share)


def test_the_warp_frames_reach_the_border():
    """Zero border taps are part of the comparison: every oblique angle leaves samples of the full (97, 131) frame outside the source."""
    img = rm.warp_frame("uniform", *rm.WARP_POWER_SHAPE)
    for deg in (5.0, -33.0, 44.0):
        m, _ = _warp_cases(rm.WARP_POWER_SHAPE, deg)
        t00, t01, t10, t11, _, _ = rm.warp_taps(img, m)
        outside = (t00 == 0) & (t01 == 0) & (t10 == 0) & (t11 == 0)
        partly = ((t00 == 0) | (t01 == 0) | (t10 == 0) | (t11 == 0)) & ~outside
        assert outside.all(axis=-1).sum() >= 50 and partly.all(axis=-1).sum() >= 20, (deg, int(outside.sum()), int(partly.sum()))


@pytest.mark.parametrize("mono", [False, True], ids=["colour", "mono"])
@pytest.mark.parametrize("grain_size", rm.GRAIN_SIZES)
@pytest.mark.parametrize("shape", rm.GRAIN_SHAPES)
def test_a_fused_grain_add_differs_from_the_separate_one(shape, grain_size, mono):
    """The GPU test's densities, amplitudes, stencil, seed and rows, with the oracle's field in place of the device's (the same field to
    1e-5; the GPU test states the condition again on the field it reads back): >= 5 % of the samples tell the two forms apart, at least
    1 % clip at 0, and so do samples of the zero column."""
    H, W = shape
    p = rm.grain_inputs(grain_size, mono)
    D = rm.grain_density(H, W)
    G = st.grain_field(H, W, p.seed, p.grain_kernel, mono)
    rows = [("whole", slice(0, H))] + ([("shard", slice(*rm.GRAIN_SHARD))] if H == 37 else [])
    for name, r in rows:
        c = rm.grain_conditions(D[r], G[r])
        print(f"grain {shape} size {grain_size} {'mono' if mono else 'colour'} {name}: fused != separate on {100 * c['share']:.1f} %, "
              f"{100 * c['clipped']:.1f} % clip at 0 ({c['zero_col_clipped']} of the zero column)")
        assert c["share"] >= rm.GRAIN_MIN_SHARE and c["clipped"] >= rm.GRAIN_MIN_CLIPPED and c["zero_col_clipped"] >= 3, (name, c)


def test_the_flat_grain_lut_returns_its_amplitude_exactly():
    """oracle.stages.multi_channel_interp on the flat table: the amplitude itself at any density, in range or not."""
    lut = rm.flat_grain_lut()
    x = np.concatenate([rm.grain_density(37, 53).reshape(-1, 3), [[-1.0, 0.0, 4.0], [5.0, 1e-30, 3.9999]]]).astype(np.float32)
    assert np.array_equal(st.multi_channel_interp(x, lut), np.broadcast_to(rm.GRAIN_AMPLITUDES, x.shape))


def test_grain_add_is_the_oracles_last_line():
    """grain_add on the oracle's own field and factor is st.apply_grain, bit for bit."""
    p = rm.grain_inputs(6.0, False)
    D = rm.grain_density(37, 53)
    G = st.grain_field(37, 53, p.seed, p.grain_kernel, False)
    assert np.array_equal(rm.grain_add(D, G, rm.GRAIN_AMPLITUDES), st.apply_grain(D, p.grain_lut, p.grain_kernel, p.seed, False))
