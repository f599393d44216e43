"""The tail kernel's two horizontal grain passes give the same bits.  Needs an MI355X.

A separable grain stencil of radius R <= 4 is filtered along x in registers while the noise is hashed (option grain_xpass_lds = 0,
the default): a lane hashes one 4-column segment and takes its neighbours' samples from the lanes next to it.  grain_xpass_lds = 1
keeps the earlier form, raw noise into LDS and an in-place pass over it.  Both sum the same taps in the same order, so every output
must agree BIT FOR BIT: field, grained density, float, uint8 and uint16 display values, on frames smaller than a tile and than the
halo, one exact tile, ragged frames of several tiles, in row shards, colour and monochrome noise, eagerly and in graph replay.
R = 5 takes the LDS pass under either setting."""

import contextlib

import numpy as np
import pytest

import hostile
from helpers import oracle_inputs, stocks, synthetic_frame

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SCALE = 341.33
SHAPES = ((13, 9), (64, 64), (70, 67), (131, 130), (257, 65))  # (W, H): below a tile and the halo; one tile; ragged, several tiles
RADII = pytest.mark.parametrize("R", [1, 2, 3, 4])
MONO = pytest.mark.parametrize("mono", [False, True], ids=["colour", "mono"])


@pytest.fixture(scope="module")
def ctx():
    from raw2film_amd.context import HipContext
    from test_gpu_parity import setup_ctx

    neg, prt, _ = stocks()
    c = HipContext(0)
    setup_ctx(c, oracle_inputs(neg, prt, SCALE, halation=False, mtf=False, grain=2))  # output LUT, grain LUT: the stage wants them
    yield c
    c.close()


@contextlib.contextmanager
def xpass(ctx, lds):
    ctx.set_option("grain_xpass_lds", lds)
    try:
        yield
    finally:
        ctx.set_option("grain_xpass_lds", 0)


def gaussian_taps(R, shared):
    """(2 R + 1)^2 x 3 taps, u v^T to fp32 rounding like filmstock.grain_kernel's; per channel unless `shared`"""
    ax = np.arange(-R, R + 1)
    sig = np.array([0.35 * R + 0.3, 0.3 * R + 0.4, 0.4 * R + 0.35])
    k = np.exp(-(ax[:, None, None] ** 2 + ax[None, :, None] ** 2) / (2.0 * sig[None, None, :] ** 2))
    k = (k / np.sqrt((k ** 2).sum(axis=(0, 1), keepdims=True))).astype(np.float32)
    return np.repeat(k[..., :1], 3, axis=2) if shared else k


def density(H, W, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.uniform(0.0, 3.0, (3, H, W)).astype(np.float32)).cuda()


def form_taken(ctx):
    stats = ctx.stencil_stats(2)
    assert len({(c["separable"], c["xpass_registers"]) for c in stats}) == 1
    return stats[0]["separable"], stats[0]["xpass_registers"]


def field(ctx, params, H, W, shards=None):
    F = torch.full((3, H, W), float("nan"), dtype=torch.float32, device="cuda")
    for y0, y1 in shards or ((0, H),):
        ctx.stage_grain_field(F, params, dst_gy0=0, y0=y0, y1=y1, H_global=H)
    return F


def tail(ctx, D, params, H, W, shards=None):
    """(float, uint8, uint16) of r2f_stage_tail16 and the grained density of r2f_stage_grain, whole or shard by shard"""
    f32 = torch.full((H, W, 3), float("nan"), dtype=torch.float32, device="cuda")
    u8 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    u16 = torch.zeros((H, W, 3), dtype=torch.uint16, device="cuda")
    G = torch.full((3, H, W), float("nan"), dtype=torch.float32, device="cuda")
    for y0, y1 in shards or ((0, H),):
        ctx.stage_tail16(D, params, out_f32=f32, out_u8=u8, out_u16=u16, y0=y0, y1=y1, H_global=H)
        ctx.stage_grain(D, G, params, y0=y0, y1=y1, H_global=H)
    return f32, u8, u16, G


def same_bits(a, b, what):
    for x, y, name in zip(a, b, ("float", "uint8", "uint16", "grained density")):
        assert not (x.is_floating_point() and torch.isnan(x).any()), (what, name)
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (what, name)


@RADII
@MONO
def test_the_field_alone_is_the_same_bits(ctx, R, mono):
    """to_planes = 2 (r2f_stage_grain_field); per-channel taps for colour noise, shared ones for monochrome noise"""
    ctx.set_kernel(2, gaussian_taps(R, shared=mono))
    params = ctx.make_params(seed=1000 + R, grain=True, grain_mono=mono)
    for W, H in SHAPES:
        with xpass(ctx, 1):
            lds = field(ctx, params, H, W)
            assert form_taken(ctx) == (1, 0)
        reg = field(ctx, params, H, W)
        assert form_taken(ctx) == (1, 1)
        assert not torch.isnan(reg).any()
        assert torch.equal(reg.view(torch.int32), lds.view(torch.int32)), (W, H)


@RADII
@MONO
def test_every_output_of_the_tail_is_the_same_bits(ctx, R, mono):
    ctx.set_kernel(2, gaussian_taps(R, shared=True))  # (fixed_same: monochrome noise then copies channel 0's field)
    params = ctx.make_params(seed=2000 + R, grain=True, grain_mono=mono)
    for W, H in SHAPES:
        D = density(H, W, 10 * R + W)
        with xpass(ctx, 1):
            lds = tail(ctx, D, params, H, W)
        same_bits(tail(ctx, D, params, H, W), lds, (W, H))


def test_radius_five_keeps_the_lds_pass_under_either_setting(ctx):
    ctx.set_kernel(2, gaussian_taps(5, shared=False))
    params = ctx.make_params(seed=5, grain=True)
    W, H = 131, 130
    D = density(H, W, 5)
    with xpass(ctx, 1):
        lds = tail(ctx, D, params, H, W) + (field(ctx, params, H, W),)
        assert form_taken(ctx) == (1, 0)
    reg = tail(ctx, D, params, H, W) + (field(ctx, params, H, W),)
    assert form_taken(ctx) == (1, 0)
    same_bits(reg[:4], lds[:4], "R = 5")
    assert torch.equal(reg[4].view(torch.int32), lds[4].view(torch.int32))


@pytest.mark.parametrize("R", [2, 4])
@MONO
def test_row_shards_are_the_whole_frame_in_both_forms(ctx, R, mono):
    """Two and three shards of the 131 x 130 frame: a hash that saw local, or unclamped, coordinates at a shard's or the frame's
    edge would differ from the whole-frame call."""
    ctx.set_kernel(2, gaussian_taps(R, shared=True))
    params = ctx.make_params(seed=3000 + R, grain=True, grain_mono=mono)
    W, H = 131, 130
    D = density(H, W, R)
    for lds in (0, 1):
        with xpass(ctx, lds):
            whole, whole_field = tail(ctx, D, params, H, W), field(ctx, params, H, W)
            for shards in (((0, 61), (61, H)), ((0, 3), (3, 67), (67, H))):
                same_bits(tail(ctx, D, params, H, W, shards), whole, (lds, shards))
                assert torch.equal(field(ctx, params, H, W, shards).view(torch.int32), whole_field.view(torch.int32)), (lds, shards)


@pytest.mark.parametrize("grain", [2, 1], ids=["colour", "mono"])
def test_render_is_the_same_bits(grain):
    """r2f_render with the stock's own 9 x 9 grain kernel (R = 4), float and uint8, every shape"""
    from raw2film_amd.context import HipContext
    from test_gpu_parity import setup_ctx

    neg, prt, _ = stocks()
    c = HipContext(0)
    try:
        p = oracle_inputs(neg, prt, SCALE, halation=False, mtf=False, grain=grain)
        assert p.grain_kernel.shape[:2] == (9, 9)
        params = setup_ctx(c, p)
        for W, H in SHAPES:
            frame = torch.from_numpy(synthetic_frame(H, W, seed=W)).cuda()
            with xpass(c, 1):
                lds = c.render(frame, params, want_f32=True, want_u8=True)
                assert form_taken(c) == (1, 0)
            reg = c.render(frame, params, want_f32=True, want_u8=True)
            assert form_taken(c) == (1, 1)
            same_bits(reg, lds, (W, H))
    finally:
        c.close()


def test_graph_replay_of_two_seeds_back_to_back_is_the_eager_bits():
    """Canary: a stepped grain LUT of tests/hostile.py, the first `zero` record's seed of the noise extremes and another one; the
    frames rendered eagerly, then alternately on one buffer set by capture and replay."""
    from raw2film_amd.context import HipContext
    from test_gpu_parity import setup_ctx
    from test_noise_extremes_host import of_kind

    neg, prt, _ = stocks()
    W, H = 131, 130
    seeds = (of_kind("zero", "vx")[0]["seed"], 20260630)
    frame = torch.from_numpy(synthetic_frame(H, W, seed=17)).cuda()
    c = HipContext(0)
    try:
        p = oracle_inputs(neg, prt, SCALE, halation=False, mtf=False, grain=2)
        p.grain_lut = hostile.grain_lut(np.random.default_rng(7), 256, amp=0.03)
        setup_ctx(c, p)
        out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        c.set_option("render_graph", 0)
        eager = {}
        for s in seeds:
            c.render(frame, c.make_params(matrix=True, grain=True, seed=s), out_f32=out)
            eager[s] = out.clone()
        assert form_taken(c) == (1, 1)
        assert not torch.equal(eager[seeds[0]], eager[seeds[1]])
        c.set_option("render_graph", 1)
        before = c.render_stats()["replays"]
        for s in seeds + seeds + seeds:
            c.render(frame, c.make_params(matrix=True, grain=True, seed=s), out_f32=out)
            assert torch.equal(out.view(torch.int32), eager[s].view(torch.int32)), s
        assert c.render_stats()["replays"] - before >= 2
    finally:
        c.close()
