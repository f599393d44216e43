"""Every site that evaluates a 1-D curve on the device, on tables whose axis is NEAR-uniform: a uniform grid with every inner breakpoint
moved by 0.45 x U(-1, 1) of a step (hostile.jittered_axis).  On such a table the planner sets DevCurve::near, and each site makes one
arithmetic guess of the cell and then at most one corrective gather (adj = -1 / +1; r2f_device.h: curve_eval_at, curve_eval_batch with
its wave-wide `any lane needs it` short cut, curve_eval_near_lds with its one-instruction clamp).  The stand-in stocks, the uniform
hostile tables and hostile.curve's wildly uneven axes (near = 0: the exact walk) never take that step on purpose; here a fifth of all
samples do, in both directions.

  site  1  front_kernel, curve cells in LDS          stage_front up to density, generic route (front_fast 0, or W % 4 != 0)
        2  front_kernel, cells in global memory      the same with m = 4096 (196 KB of cells)
        3  fast front kernel                         front_fast 1, W % 4 == 0
        3b fast front kernel, finish_mask            stage_front_split: the halation's identity channel finished in the front kernel
        4  direct stencil epilogue                   stage_halation with stencil_fft 0
        5  single_tap_kernel epilogue                the identity (blue) channel of a colour stock's halation
        6  FFT pass-3 epilogue, cells in LDS         stage_halation in FFT form, stencil_fft_epilogue_lds 1
        7  FFT pass-3 epilogue, cells in global      the same with the option 0, or m = 4096
        8  tail kernel, grain LUT in LDS             stage_grain / stage_tail
        9  tail kernel, grain LUT in global memory   the same with m = 4096
        10 lut3d_kernel with a grain field           stage_grain_field + stage_tail_field

Tables, sample sets, references and bounds are built once in tests/curve_sites.py.  Every test first asserts, through the float32 model of
the look-up (tests/curve_model.py, held equal to the planner by tests/test_curve_host.py), that its table is `near` and that at least
10 % of its in-range samples need the corrective step, at least 2 % in each direction (m = 3 has one inner breakpoint and with it one
direction per table: two tables, one each; the uniform control needs no step outside the rounding of the guess itself).  Only then is the
device result compared with the oracle.  tests/test_curve_host.py shows on the CPU that a look-up without the step misses these bounds on
5 % to 88 % of the in-range samples of every table here (a wrong cell costs about half a cell times the difference of two slopes: 5e-3 at
m = 256, 3e-4 at m = 4096, against bounds of a few 1e-5).  No non-finite samples: tests/test_gpu_hostile.py owns those."""

import numpy as np
import pytest

import curve_sites as cs

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_parity import dev, from_planes, setup_ctx, to_planes  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    from raw2film_amd.context import HipContext

    c = HipContext(0)
    yield c
    c.close()


def _within(got, ref, bound, what):
    """|got - ref| <= bound everywhere; the figure is printed before it is asserted."""
    ratio = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64)) / bound
    print(f"{what}: max |device - oracle| / bound = {float(ratio.max()):.3f}, over on {int((ratio > 1).sum())} of {ratio.size}")
    assert (ratio <= 1).all(), (what, float(ratio.max()), int((ratio > 1).sum()))


# ------------------------------------------------------------------------------------------------ sites 1, 2, 3
@pytest.mark.parametrize("shape", [(64, 96), (37, 53)])
@pytest.mark.parametrize("case", cs.CASES)
def test_front_kernels_take_the_corrective_step(ctx, case, shape):
    """S3 + S4 through stage_front on a flat 2-D LUT: exposures aimed at every breakpoint, past both ends of the axis, spread over the
    axis, and a synthetic frame.  (64, 96): the fast kernel (site 3; m = 4096 exceeds its LDS and takes the generic kernel) and, with
    front_fast 0, the generic one (site 1, m = 4096: site 2) -- the same bits.  (37, 53): the generic kernel whatever front_fast says."""
    H, W = shape
    k = cs.front_case(case, H, W)
    cs.assert_conditions(case, k.lut, k.loge)
    params = setup_ctx(ctx, k.p)
    img = dev(k.img)
    got = {}
    try:
        for fast in ((1, 0) if W % 4 == 0 else (1,)):
            ctx.set_option("front_fast", fast)
            D = torch.empty((3, H, W), dtype=torch.float32, device="cuda")
            ctx.stage_front(img, params, 1, dst=D)
            got[fast] = from_planes(D)
    finally:
        ctx.set_option("front_fast", 1)
    for fast, g in got.items():
        _within(g, k.ref, k.bound, f"front {case} {shape} front_fast {fast}")
        assert np.array_equal(g[0, :5], np.broadcast_to(k.lut[1:, 0], (5, 3)))  # exposure 0 -> log clip -> below the axis: fp[0]
        assert np.array_equal(g[2, :5], np.broadcast_to(k.lut[1:, -1], (5, 3)))  # 180 000 -> above it: fp[m - 1]
    if 0 in got:
        assert np.array_equal(got[1], got[0])


# ------------------------------------------------------------------------------------------------ site 3b
@pytest.mark.parametrize("case", cs.FAST_CASES)
def test_the_identity_channel_finished_by_the_front_kernel_takes_the_corrective_step(ctx, case):
    """stage_front_split on a colour stock's halation (test_identity_halation_channels_are_finished_by_the_front_kernel's set-up): the
    blue channel gets tap weight, log and curve in the fast front kernel (finish_mask 4, curve_eval_at on the LDS cells)."""
    H, W = 64, 96
    k = cs.split_front_case(case, H, W, 166.67)
    cs.assert_conditions(case, k.lut, k.loge)
    params = setup_ctx(ctx, k.p)
    E = torch.full((3, H, W), -1.0, dtype=torch.float32, device="cuda")
    D = torch.full((3, H, W), -1.0, dtype=torch.float32, device="cuda")
    try:
        ctx.set_option("front_fast", 1)
        mask = ctx.stage_front_split(dev(k.img), params, E, D)
    finally:
        ctx.set_option("front_fast", 1)
    assert mask == 4
    _within(D[2].cpu().numpy(), k.ref, k.bound, f"split front {case}")
    assert float(D[:2].max()) == -1.0 and float(E[2].max()) == -1.0  # nothing else was finished, the blue exposure never written


# ------------------------------------------------------------------------------------------------ sites 4, 5, 6, 7
def _halation(ctx, k, params, H, W, want_fft):
    D = torch.empty((3, H, W), dtype=torch.float32, device="cuda")
    ctx.stage_halation(to_planes(k.expo), D, params, y0=0, y1=H, H_global=H)
    assert [c["fft"] for c in ctx.stencil_stats(0)] == want_fft
    return from_planes(D)


def _halation_conditions(case, k):
    cs.assert_conditions(case, k.lut, k.loge[..., :2])  # the channels with a real stencil
    cs.assert_conditions(case, k.lut, k.loge[..., 2:])  # the single tap


@pytest.mark.parametrize("case", cs.CASES)
def test_direct_stencil_and_single_tap_epilogues_take_the_corrective_step(ctx, case):
    """Halation at 166.67 px/mm on (70, 133) with the FFT form off: red and green through the direct stencil's epilogue (site 4), blue
    through single_tap_kernel (site 5; the breakpoint exposures sit in its plane).  The bound is the density curve's own, not widened
    for the stencil sum in the log (measured: the direct stencil uses 0.02 of it, the single tap 0.16)."""
    H, W = 70, 133
    k = cs.halation_case(case, H, W, 166.67)
    _halation_conditions(case, k)
    params = setup_ctx(ctx, k.p)
    try:
        ctx.set_option("stencil_fft", 0)
        got = _halation(ctx, k, params, H, W, [0, 0, 0])
    finally:
        ctx.set_option("stencil_fft", 1)
    _within(got[..., :2], k.ref[..., :2], k.bound[..., :2], f"direct stencil epilogue {case}")
    _within(got[..., 2], k.ref[..., 2], k.bound[..., 2], f"single tap epilogue {case}")


@pytest.mark.parametrize("case", cs.CASES)
def test_fft_epilogues_take_the_corrective_step(ctx, case):
    """Halation at 341.33 px/mm on (300, 417): red and green in FFT form, the curve in pass 3's epilogue -- from LDS through
    curve_eval_near_lds (site 6: stencil_fft_epilogue_lds 1 and the cells fit, m <= 1024) and from global memory through curve_eval_batch
    (site 7: the option 0, or m = 4096).  `Same arithmetic, same results` (r2f_device.h): the same bits.  Bound: the density curve's own,
    not widened (measured: 0.20 of it at the most)."""
    H, W = 300, 417
    k = cs.halation_case(case, H, W, 341.33)
    _halation_conditions(case, k)
    params = setup_ctx(ctx, k.p)
    got = {}
    try:
        for lds in (1, 0):
            ctx.set_option("stencil_fft_epilogue_lds", lds)
            got[lds] = _halation(ctx, k, params, H, W, [1, 1, 0])
    finally:
        ctx.set_option("stencil_fft_epilogue_lds", 1)
    for lds, g in got.items():
        _within(g, k.ref, k.bound, f"FFT epilogue {case} stencil_fft_epilogue_lds {lds}")
    assert np.array_equal(got[1], got[0])


# ------------------------------------------------------------------------------------------------ sites 8, 9, 10
@pytest.mark.parametrize("mono", [False, True])
@pytest.mark.parametrize("m", [256, 4096])
def test_grain_lut_sites_take_the_corrective_step(ctx, m, mono):
    """out = max(D + G * lut(D), 0) with independent amplitudes at every breakpoint of a jittered axis [0, 4] (inside a constant run a
    wrong cell would not show), densities exactly at every breakpoint, one float to either side, at both ends and past them.
    stage_grain and stage_tail run the tail kernel (site 8; m = 4096: site 9), stage_grain_field + stage_tail_field the lut3d kernel
    (site 10) -- bit for bit the fused tail's result.  Bounds: test_grain_lut_with_steps's, and a quarter of them (plus the blend's
    rounding) behind the identity 3-D LUT."""
    H, W = cs.GRAIN_SHAPE
    k = cs.grain_case(m, mono)
    cs.assert_conditions(f"m{m}", k.lut, k.dens)
    params = setup_ctx(ctx, k.p)
    D = to_planes(k.dens)
    G = torch.empty((3, H, W), dtype=torch.float32, device="cuda")
    ctx.stage_grain(D, G, params, y0=0, y1=H, H_global=H)
    got = from_planes(G)
    _within(got, k.ref, k.bound, f"stage_grain m {m} mono {mono}")
    assert (got[1] >= 0).all() and (got[1] == 0).any()
    fused = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    ctx.stage_tail(D, params, out_f32=fused, y0=0, y1=H, H_global=H)
    _within(fused.cpu().numpy(), k.shown, k.shown_bound, f"stage_tail m {m} mono {mono}")
    F = torch.empty((3, H, W), dtype=torch.float32, device="cuda")
    ctx.stage_grain_field(F, params, y0=0, y1=H, H_global=H)
    split = torch.empty_like(fused)
    ctx.stage_tail_field(D, F, params, out_f32=split, y0=0, y1=H, H_global=H)
    _within(split.cpu().numpy(), k.shown, k.shown_bound, f"stage_tail_field m {m} mono {mono}")
    assert np.array_equal(split.cpu().numpy(), fused.cpu().numpy())
