"""The Gaussian field at the samples a random frame never reaches (tests/golden/noise_extremes.json, searched by
tools/find_noise_extremes.py): hash components in the clamp max(u, 1e-7) -- hash 0 among them, where the clamp is all that
stands before sqrt(-2 ln 0) --, the first values past it, u == 1.0, the fraction wrap of u1 + uy, the quarter turns.  Both copies
of the noise path are held to them: r2f_stage_noise's kernel and the tail kernel's own hashing into LDS (through
r2f_stage_grain_field, r2f_stage_grain and r2f_render), in every form the grain stencil takes.  Needs an MI355X.

The bound is test_gpu_parity.test_gaussian_field's 1e-5 absolute, asserted against the float64 truth (oracle.truth) and,
separately, against the float32 oracle; the hash is bit-exact.  Every frame is the search's 64 x 256 window or smaller.
Measured on an MI355X over all records: the variates within 2.7e-6 of the truth (the clamped samples, r = 5.68, among them),
the filtered fields within 7.8e-7 of max |field| of the oracle's.

What these tests are for, tried on scratch builds of gaussian_noise(): a clamp constant of 1e-6 and no clamp at all fail here
(the zero, clamped, just-free and edge records) and nowhere else in the suite; (float)(v >> 8) * 2^-24 for the uniform fails
here at nearly every record and in test_gpu_parity too (24 absolute bits lose the small u); dropping floorf from the wrap
changes nothing anywhere, and cannot: s12 - floorf(s12) is exact for s12 in [1, 2) and v_cos_f32, which takes revolutions,
reduces its argument itself."""

import functools

import numpy as np
import pytest

from oracle import stages as st
from oracle import truth

from helpers import assert_close, oracle_inputs, stocks, synthetic_frame
from test_noise_extremes_host import BOUND, H, RECORDS, W, of_kind, record_id

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SCALE = 341.33  # px / mm of the stand-in stock's grain kernels below (test_gpu_parity.test_tail_grain's)
# grain size -> the form its stand-in kernel takes: 9 x 9 two 1-D passes; 17 x 17 fully unrolled once the separable form is
# switched off (test_separable_grain_stencils...: a Gaussian is always rank one); 21 x 21 past the unrolled forms' R <= 9, the
# generic entry list (test_small_square_grain_stencils...)
FORMS = (("separable", 6.0, 9), ("unrolled", 14.0, 17), ("generic", 19.0, 21))
XS, YS = np.arange(W)[None, :], np.arange(H)[:, None]
MONO = pytest.mark.parametrize("mono", [False, True], ids=["colour", "mono"])
PER_RECORD = pytest.mark.parametrize("r", RECORDS, ids=record_id)


@pytest.fixture(scope="module")
def ctx():
    from raw2film_amd.context import HipContext

    c = HipContext(0)
    c.set_grain_lut(grain_lut())  # the field does not use it; the stage wants one
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def from_planes(t):
    return np.transpose(t.cpu().numpy(), (1, 2, 0))


@functools.lru_cache(maxsize=None)
def grain_lut():
    return stocks()[0].get_grain_curve(SCALE, adx=False, bw_grain=False)


@functools.lru_cache(maxsize=None)
def stand_in_kernel(grain_size):
    from raw2film_amd import filmstock

    return filmstock.grain_kernel(1 / SCALE, grain_size / 1000, 0.4)


@functools.lru_cache(maxsize=None)
def window(seed, mono):
    """(truth, oracle) of the variates over the whole window; computed once per seed, never written to."""
    exact, ref = truth.gaussian_noise(XS, YS, seed, mono), st.gaussian_noise(XS, YS, seed, mono)
    exact.setflags(write=False)
    ref.setflags(write=False)
    return exact, ref


def check_variates(got, exact, ref, r, x=None, what=""):
    """finite, and within the bound of the truth and of the oracle: everywhere, and (named separately) at the record's pixel"""
    assert np.isfinite(got).all(), (what, r)
    e_truth, e_ref = np.abs(got - exact), np.abs(got.astype(np.float64) - ref)
    print(f"{what} {record_id(r)}: max |dev - truth| {e_truth.max():.2e}, |dev - oracle| {e_ref.max():.2e}"
          + ("" if x is None else f"; at the record {e_truth[x].max():.2e}, {e_ref[x].max():.2e}"))
    if x is not None:
        assert e_truth[x].max() <= BOUND and e_ref[x].max() <= BOUND, (what, "at the record", r)
    assert e_truth.max() <= BOUND, (what, "truth", r)
    assert e_ref.max() <= BOUND, (what, "oracle", r)


# ------------------------------------------------------------------------------- r2f_stage_noise
@MONO
@PER_RECORD
def test_noise_kernel_at_the_record(ctx, r, mono):
    y, x, seed = r["y"], r["x"], r["seed"]
    params = ctx.make_params(seed=seed, grain_mono=mono)
    h, n = ctx.stage_noise(params, y, y + 1, W)
    got_h = h.cpu().numpy().view(np.uint32)[:, 0, :]
    want_h = np.stack([v[0] for v in st.pcg3d(XS, np.array([[y]]), seed)])
    np.testing.assert_array_equal(got_h, want_h)
    if r["kind"] == "wrap":
        assert (int(got_h[0, x]), int(got_h[1, x])) == (r["hash"], r["hash_y"])
    else:
        assert int(got_h[{"vx": 0, "vy": 1, "vz": 2}[r["component"]], x]) == r["hash"]
    exact, ref = window(seed, mono)
    check_variates(from_planes(n)[0], exact[y], ref[y], r, x, "noise row")


@pytest.mark.parametrize("width", [256, 4096])
@pytest.mark.parametrize("seed", [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF])
def test_hash_at_the_ends_of_the_seed_and_row_ranges(ctx, seed, width):
    """Two-row calls at row 0, across 2^16, across 2^24 (where a coordinate routed through a float stops being exact) and at the
    last pair of rows an int y1 can name; seeds at both ends and across the sign bit."""
    params = ctx.make_params(seed=seed)
    xs = np.arange(width)[None, :]
    for y0 in (0, 65535, (1 << 24) - 1, (1 << 31) - 3):
        h, _ = ctx.stage_noise(params, y0, y0 + 2, width, want_noise=False)
        got = h.cpu().numpy().view(np.uint32)
        want = st.pcg3d(xs, np.arange(y0, y0 + 2, dtype=np.int64)[:, None], seed)
        for c in range(3):
            np.testing.assert_array_equal(got[c], want[c], err_msg=f"seed {seed:#x} rows {y0}.. component {c}")


# ------------------------------------------------------------------------------- the tail kernel's own noise path
def grain_field(ctx, params, y0=0, y1=H):
    F = torch.empty((3, y1 - y0, W), dtype=torch.float32, device="cuda")
    ctx.stage_grain_field(F, params, dst_gy0=y0, y0=y0, y1=y1, H_global=H)
    return F


@MONO
@PER_RECORD
def test_tail_kernel_variates_through_a_one_tap_grain_kernel(ctx, r, mono):
    """K_g = [1]: the field is the variates the tail kernel hashed into LDS."""
    ctx.set_kernel(2, np.ones((1, 1), np.float32))
    params = ctx.make_params(seed=r["seed"], grain=True, grain_mono=mono)
    got = from_planes(grain_field(ctx, params))
    exact, ref = window(r["seed"], mono)
    check_variates(got.reshape(-1, 3), exact.reshape(-1, 3), ref.reshape(-1, 3), r, r["y"] * W + r["x"], "tail, one tap")


@MONO
@PER_RECORD
def test_tail_kernel_grain_field_in_every_stencil_form_and_in_row_shards(ctx, r, mono):
    """The stand-in stock's kernels in the separable, the unrolled and the generic form against oracle.stages.grain_field at
    test_separable_grain_stencils...' tolerance; the rows around the record computed alone are the whole window's, bit for bit.
    The `edge` records lie inside every one of these kernels' radius of the frame border, where the reads clamp."""
    params = ctx.make_params(seed=r["seed"], grain=True, grain_mono=mono)
    y0, y1 = max(r["y"] - 3, 0), min(r["y"] + 4, H)
    try:
        for form, size, n in FORMS:
            k = stand_in_kernel(size)
            assert k.shape == (n, n)
            ctx.set_option("grain_separable", int(form == "separable"))
            ctx.set_kernel(2, k)
            whole = grain_field(ctx, params)
            stats = ctx.stencil_stats(2)
            assert [c["separable"] for c in stats] == [int(form == "separable")] * 3, form
            assert [c["unrolled"] for c in stats] == [0 if form == "generic" else n // 2] * 3, form
            got = from_planes(whole)
            ref = st.grain_field(H, W, r["seed"], k, mono)
            assert np.isfinite(got).all(), form
            err = np.abs(got - ref.astype(np.float64)).max()
            print(f"grain field {form} {record_id(r)}: {err:.2e} of {np.abs(ref).max():.2f}")
            assert err <= 5e-6 * np.abs(ref).max(), form
            assert torch.equal(grain_field(ctx, params, y0, y1), whole[:, y0:y1]), form
    finally:
        ctx.set_option("grain_separable", 1)


def clip_case():
    """A `zero` record whose variate is the most negative of its channel in the window, and the density D (the same everywhere)
    that puts D + G lut(D) below zero at that sample alone: D / lut_c(D) three quarters of the way from the runner-up's |G| to
    the record's (the other channels' tables differ: halfway would leave one of their samples at the contract's floor)."""
    lut = grain_lut()
    for r in of_kind("zero"):
        G = window(r["seed"], False)[0]
        for c in range(3):
            g0 = G[r["y"], r["x"], c]
            if g0 < -5.0 and g0 == G[..., c].min():
                rho = -0.75 * g0 - 0.25 * np.partition(G[..., c].ravel(), 1)[1]
                lo, hi = 0.0, 0.5  # D - rho lut_c(D) changes sign once in between: lut(0) > 0, 0.5 / lut(0.5) > 13
                for _ in range(60):
                    mid = 0.5 * (lo + hi)
                    lo, hi = (mid, hi) if mid - rho * np.interp(mid, lut[0], lut[1 + c]) < 0 else (lo, mid)
                return r, c, np.float32(lo)
    raise AssertionError("the fixture holds no zero record that is its channel's minimum")


def test_a_clamped_sample_next_to_the_clip_at_zero(ctx):
    r, c, D = clip_case()
    lut, k = grain_lut(), np.ones((1, 1), np.float32)
    density = np.full((H, W, 3), D, dtype=np.float32)
    exact = truth.multi_channel_interp(density, lut) * window(r["seed"], False)[0] + np.float64(D)  # before the clip
    here = np.zeros((H, W, 3), dtype=bool)
    here[r["y"], r["x"], c] = True
    # what the case is built for, on the truth: clearly negative there, everything else clear of the contract's floor
    assert exact[here][0] < -1e-3 and exact[~here].min() > 1e-3, (exact[here][0], exact[~here].min())
    ctx.set_kernel(2, k)
    params = ctx.make_params(seed=r["seed"], grain=True)
    out = torch.empty((3, H, W), dtype=torch.float32, device="cuda")
    ctx.stage_grain(dev(np.transpose(density, (2, 0, 1))), out, params, y0=0, y1=H, H_global=H)
    got = from_planes(out)
    assert np.isfinite(got).all()
    assert got[here][0] == 0.0
    ref = st.apply_grain(density, lut, k, r["seed"])
    assert ref[here][0] == 0.0
    e = assert_close(got, ref, 1e-5, 1e-3, "grain next to the clip")
    print(f"clip at zero, {record_id(r)} channel {c}, D = {D:.6f}: max rel err {e:.2e}")


# ------------------------------------------------------------------------------- the seed read from the frame block
def test_render_replays_follow_the_seed_to_the_extreme_samples():
    """r2f_render on one buffer set: eager, captured, replayed.  The zero record's frame is rendered before and after another
    seed's, the second time by replay; then the one record's."""
    from raw2film_amd.context import HipContext
    from test_gpu_parity import setup_ctx

    neg, prt, _ = stocks()
    zero, one = of_kind("zero", "vx")[0], of_kind("one", "vx")[0]
    seeds = [zero["seed"], 20260630, zero["seed"], one["seed"]]
    img = synthetic_frame(H, W, seed=17)
    frame = dev(img)
    ctx = HipContext(0)
    try:
        out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        p = oracle_inputs(neg, prt, SCALE, halation=False, mtf=False, grain=2)
        setup_ctx(ctx, p)  # the tables once: an upload between two frames would drop the graph
        got, refs = [], {}
        for s in seeds:
            p.seed = s
            if s not in refs:
                refs[s] = st.render(img, p)
            ctx.render(frame, ctx.make_params(matrix=True, grain=True, seed=s), out_f32=out)
            got.append(out.cpu().numpy())
        stats = ctx.render_stats()
        assert stats["replays"] >= 2 and stats["eager"] <= 2, stats  # (the third and fourth frame at the least)
        for s, g in zip(seeds, got):
            assert np.isfinite(g).all()
            e = assert_close(g, refs[s], 1e-5, 1e-3, f"render at seed {s}")
            print(f"render at seed {s}: max rel err {e:.2e}")
        np.testing.assert_array_equal(got[0], got[2])
        assert not np.array_equal(got[1], got[2]) and not np.array_equal(got[2], got[3])
    finally:
        ctx.close()
