"""Where a kernel says that a product and the sum that takes it `round separately`, the device against that statement BIT FOR BIT (needs an
MI355X).  The tolerance tests of these sites (2e-5 x 4 absolute for the warp, 1e-5 relative for the grain stage, 1 LSB for the uint16
resamplers) are a hundred times wider than the difference between a separate and a contracted multiply-add; these are not.

  a  warp_affine             == oracle.stages.warp_affine_linear: float32 coordinates, taps, zero border and the two-step lerp
  b  stage_grain             == rounding_model.grain_add on the field stage_grain_field wrote for the same rows (the tail kernel's add)
  c  stage_tail_field        == stage_tail, and == the grain-less tail on rounding_model.grain_add's density (lut3d_kernel's add)
  d  resize_area_u16 / resize_lanczos4_u16 == tests/output16_model.py, which follows OpenCV's stepwise float32 sums

tests/test_rounding_order_host.py shows on the CPU that a contracted step changes 17-49 % of the samples of (a) and 11-12 % of (b); (b)
and (c) state the 5 % condition again on the field they read back.  Values are compared (np.array_equal: +0 == -0); no input is
non-finite."""

import numpy as np
import pytest

from oracle import stages as st
from output16_model import area_u16, lanczos4_u16

import rounding_model as rm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_output16 import frame16, u16  # noqa: E402
from test_gpu_parity import dev, from_planes, setup_ctx, to_planes  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    from raw2film_amd.context import HipContext

    c = HipContext(0)
    yield c
    c.close()


def _same(got, ref, what):
    """Equal values everywhere; the count and the largest difference are printed before the assertion."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = got != ref
    worst = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()) if bad.any() else 0.0
    print(f"{what}: {int(bad.sum())} of {bad.size} samples differ ({100.0 * bad.mean():.2f} %), max |difference| {worst:.3g}")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} samples differ, max |difference| {worst:.3g}"


# ------------------------------------------------------------------------------------------------ a
@pytest.mark.parametrize("kind", rm.WARP_FRAMES)
@pytest.mark.parametrize("shape", rm.WARP_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_warp_affine_equals_the_oracle_bit_for_bit(ctx, shape, kind):
    """Six angles x three layouts x (full frame, rotation_plan's window).  (97, 131) is 3 x 25 workgroups of 64 x 4 lanes with ragged
    edges; (5, 7) and (1, 9) are frames smaller than a workgroup whose every sample has a border tap.  Equality pins the coordinate sums
    (each product and sum rounded to float32), the floor, the choice of taps and the lerp; the border's zeros are compared like any
    sample."""
    from raw2film_amd import geometry

    H, W = shape
    img = rm.warp_frame(kind, H, W)
    for deg in rm.WARP_ANGLES:
        m, win = geometry.rotation_plan(H, W, deg)
        win = tuple(int(v) for v in win)
        ref_full = st.warp_affine_linear(img, m)
        ref_win = st.warp_affine_linear(img, m, win[2:], win[:2]) if win[2] and win[3] else None
        for layout in ("hwc3", "hwc4", "chw"):
            t = dev(rm.with_layout(img, layout))
            _same(from_planes(ctx.warp_affine(t, m, layout=layout)), ref_full, f"warp {kind} {shape} {deg} deg {layout} full")
            gotw = ctx.warp_affine(t, m, win, layout=layout)
            if ref_win is None:
                assert tuple(gotw.shape) == (3, win[2], win[3])
            else:
                _same(from_planes(gotw), ref_win, f"warp {kind} {shape} {deg} deg {layout} window {win}")


# ------------------------------------------------------------------------------------------------ b, c
def _grain_case(ctx, shape, grain_size, mono):
    H, W = shape
    p = rm.grain_inputs(grain_size, mono)
    params = setup_ctx(ctx, p)
    dens = rm.grain_density(H, W)
    F = torch.empty((3, H, W), dtype=torch.float32, device="cuda")
    ctx.stage_grain_field(F, params, y0=0, y1=H, H_global=H)
    stats = ctx.stencil_stats(2)
    print(f"grain stencil {shape} size {grain_size} mono {mono}: " + ", ".join(f"{k} {stats[0][k]}" for k in ("kh", "kw", "unrolled", "separable")))
    # which tail_kernel instantiation ran: the 9 x 9 Gaussian as two 1-D passes of the unrolled R = 4 form, the single tap as the entry list
    assert [(c["unrolled"], c["separable"]) for c in stats] == [(4, 1) if grain_size == 6.0 else (0, 0)] * 3
    return p, params, dens, to_planes(dens), F


def _assert_power(dens, field, what):
    c = rm.grain_conditions(dens, field)
    print(f"{what}: on the device's field a fused add differs on {100 * c['share']:.1f} %, {100 * c['clipped']:.1f} % clip at 0 "
          f"({c['zero_col_clipped']} of the zero column)")
    assert c["share"] >= rm.GRAIN_MIN_SHARE and c["clipped"] >= rm.GRAIN_MIN_CLIPPED and c["zero_col_clipped"] >= 3, (what, c)


@pytest.mark.parametrize("mono", [False, True], ids=["colour", "mono"])
@pytest.mark.parametrize("grain_size", rm.GRAIN_SIZES)
@pytest.mark.parametrize("shape", rm.GRAIN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stage_grain_equals_the_separate_add_on_its_own_field(ctx, shape, grain_size, mono):
    """out = max(D + f32(G * a), 0) with G read back from stage_grain_field (the same params, seed, rows and H_global) and a the flat grain
    LUT's amplitude.  Both entries run tail_kernel: grain_size 6 at 341.33 px/mm is a 9 x 9 Gaussian and takes the separable
    instantiation (two 1-D passes, R = 4), grain_size 1 has no stencil (the single tap of weight 1) and takes the entry-list one (R = 0);
    the add is the same source line in both.  (64, 96): two workgroups, float4 loads and stores.  (37, 53): one ragged workgroup, scalar
    accesses; there also rows [9, 30) alone, from and into buffers whose first row is not the shard's (src_gy0 8, dst_gy0 7)."""
    H, W = shape
    p, params, dens, D, F = _grain_case(ctx, shape, grain_size, mono)
    field = from_planes(F)
    _assert_power(dens, field, f"grain {shape} size {grain_size} mono {mono}")
    out = torch.empty((3, H, W), dtype=torch.float32, device="cuda")
    ctx.stage_grain(D, out, params, y0=0, y1=H, H_global=H)
    got = from_planes(out)
    _same(got, rm.grain_add(dens, field, rm.GRAIN_AMPLITUDES), f"stage_grain {shape} size {grain_size} mono {mono}")
    assert (got[:, rm.GRAIN_ZERO_COLUMN] == 0).any() and (got[:, rm.GRAIN_ZERO_COLUMN] > 0).any()
    if H == 37:
        y0, y1 = rm.GRAIN_SHARD
        Fs = torch.full((3, y1 - 7, W), np.nan, dtype=torch.float32, device="cuda")  # holds global rows 7 ..
        ctx.stage_grain_field(Fs, params, dst_gy0=7, y0=y0, y1=y1, H_global=H)
        fs = from_planes(Fs)[y0 - 7:]
        _assert_power(dens[y0:y1], fs, f"grain shard {shape} size {grain_size} mono {mono}")
        outs = torch.full((3, y1 - 7, W), np.nan, dtype=torch.float32, device="cuda")
        ctx.stage_grain(D[:, 8:y1 + 1], outs, params, src_gy0=8, dst_gy0=7, y0=y0, y1=y1, H_global=H)
        gots = from_planes(outs)
        assert np.isnan(gots[:y0 - 7]).all() and np.isnan(from_planes(Fs)[:y0 - 7]).all()  # rows 7 and 8 are not the shard's
        _same(gots[y0 - 7:], rm.grain_add(dens[y0:y1], fs, rm.GRAIN_AMPLITUDES), f"stage_grain rows [{y0}, {y1}) size {grain_size} mono {mono}")


@pytest.mark.parametrize("mono", [False, True], ids=["colour", "mono"])
@pytest.mark.parametrize("shape", rm.GRAIN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_pointwise_tail_adds_its_field_like_the_fused_tail_and_like_the_model(ctx, shape, mono):
    """stage_tail_field runs lut3d_kernel with has_gfield (one lane per four pixels, W = 96: float4 accesses, W = 53: scalar ones and a
    ragged last lane); stage_tail runs tail_kernel (the separable R = 4 instantiation here) through the same 3-D LUT.  Their results
    are equal bit for bit -- which two kernels that both contracted the add would also be.  So the pointwise kernel is held to the model as
    well: the same kernel with the grain flag off, fed the density rounding_model.grain_add computes from (D, G), runs the identical
    3-D LUT code on what must be the identical density (a contracted add moved 12 % of the densities by an ulp and, behind the stock's
    3-D LUT, 1 % of the output samples).  With test (b) this holds both sites to the separate add."""
    H, W = shape
    p, params, dens, D, F = _grain_case(ctx, shape, 6.0, mono)
    field = from_planes(F)
    _assert_power(dens, field, f"tail {shape} mono {mono}")
    fused = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    ctx.stage_tail(D, params, out_f32=fused, y0=0, y1=H, H_global=H)
    split = torch.empty_like(fused)
    ctx.stage_tail_field(D, F, params, out_f32=split, y0=0, y1=H, H_global=H)
    modelled = torch.empty_like(fused)
    plain = ctx.make_params(matrix=True, grain=False, seed=p.seed)
    ctx.stage_tail(to_planes(rm.grain_add(dens, field, rm.GRAIN_AMPLITUDES)), plain, out_f32=modelled, y0=0, y1=H, H_global=H)
    fused, split, modelled = fused.cpu().numpy(), split.cpu().numpy(), modelled.cpu().numpy()
    assert np.unique(modelled).size > 1000  # the 3-D LUT does not flatten the differences away
    _same(split, fused, f"stage_tail_field vs stage_tail {shape} mono {mono}")
    _same(split, modelled, f"stage_tail_field vs the grain-less tail of the model's density {shape} mono {mono}")
    _same(fused, modelled, f"stage_tail vs the grain-less tail of the model's density {shape} mono {mono}")


# ------------------------------------------------------------------------------------------------ d
AREA_CASES = [((48, 64), (24, 32)), ((48, 63), (16, 21)), ((75, 100), (48, 64)), ((1, 64), (1, 20)), ((64, 1), (20, 1)), ((7, 9), (7, 9)),
              ((68, 102), (4, 6)), ((48, 63), (16, 20))]  # the last: an integer factor down the rows, 3.15 along them
LANCZOS_CASES = [((5, 7), (13, 17)), ((48, 64), (75, 100)), ((48, 63), (16, 20))]  # (the last one shrinks: every tap a new sample)


@pytest.mark.parametrize("src,dst", AREA_CASES)
def test_area_u16_equals_the_model(ctx, src, dst):
    """Every shape of test_gpu_output16.test_area_u16 and one with an integer factor on one axis only (the table path, whose row weights
    are then all equal): float32 products and sums in OpenCV's order, then round half to even."""
    a = frame16(*src, seed=2)
    _same(u16(ctx.resize_area_u16(dev(a.view(np.int16)), *dst)), area_u16(a, *dst), f"area_u16 {src} -> {dst}")


@pytest.mark.parametrize("src,dst", LANCZOS_CASES)
def test_lanczos4_u16_equals_the_model(ctx, src, dst):
    """Every shape of test_gpu_output16.test_lanczos4_u16 and the (48, 63) -> (16, 20) of the area test: eight products per row summed left to right, eight rows top to bottom, each a
    float32 rounding, then saturate_cast<ushort>."""
    a = frame16(*src, seed=1)
    _same(u16(ctx.resize_lanczos4_u16(dev(a.view(np.int16)), *dst)), lanczos4_u16(a, *dst), f"lanczos4_u16 {src} -> {dst}")
