"""The 16-bit output side on the GPU (output_bits=16): the tail kernels' uint16 stores, the extents they write, the two uint16
resamplers, r2f_render16 and its place in the graph cache, the processor's post-path, streaming, lending and histogram at 16
bits, and the TIFF export.  Expected values: tests/output16_model.py.

Tolerances.  The uint16 samples are compared with the library's own float output with NO tolerance (the same float goes through
the same clip / multiply / truncate).  Against the oracle they may differ by one step: the project's float contract is 1e-5
relative at a 1e-3 floor, 65535 x 1e-5 < 1, and a truncation moves by at most one step when its argument moves by less than one.
The resamplers are compared with the model within one step as well (products and sums are rounded as OpenCV's generic path rounds
them; a tie at the final rounding can fall either way when an intermediate differs in its last bit)."""

import io

import numpy as np
import pytest

from arena import Arena
from helpers import SEED, oracle_inputs, stocks, synthetic_frame
from oracle import stages as st
from output16_model import area_u16, lanczos4_u16, read_tiff, to_uint16

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def to_planes(a):
    return dev(np.ascontiguousarray(np.transpose(a, (2, 0, 1))))


def u16(t):
    return t.cpu().numpy().view(np.uint16)


@pytest.fixture(scope="module")
def ctx():
    from raw2film_amd.context import HipContext

    c = HipContext(0)
    yield c
    c.close()


def wide_inputs(grain):
    """Oracle inputs whose output LUT is stretched to [-0.5, 1.5]: the frame's output spans below 0 to above 1, both clamps fire."""
    neg, prt, _ = stocks()
    p = oracle_inputs(neg, prt, 341.33, halation=False, mtf=False, grain=grain)
    p.lut_3d = (np.asarray(p.lut_3d, np.float32) * np.float32(2.0) - np.float32(0.5)).astype(np.float32)
    return p


def setup_ctx(ctx, p):
    ctx.set_matrix3x3(p.matrix)
    ctx.set_lut2d(p.lut_2d)
    ctx.set_curve1d(p.lut_1d)
    ctx.set_lut3d(p.lut_3d)
    if p.halation_kernel is not None:
        ctx.set_kernel(0, p.halation_kernel)
    if p.mtf_kernel is not None:
        ctx.set_kernel(1, p.mtf_kernel)
    if p.grain_lut is not None:
        ctx.set_grain_lut(p.grain_lut)
        ctx.set_kernel(2, p.grain_kernel if p.grain_kernel is not None else np.ones((1, 1), np.float32))
    return ctx.make_params(matrix=p.matrix is not None, halation=p.halation_kernel is not None, mtf=p.mtf_kernel is not None,
                           grain=p.grain_lut is not None, grain_mono=p.grain_mono, seed=p.seed)


@pytest.fixture(scope="module")
def densities():
    """One density frame per shape (the oracle's, from a frame with speculars), shared by the tail tests and left unchanged."""
    neg, prt, _ = stocks()
    out = {}
    for H in (1, 3, 70):
        for W in (1, 7, 64, 257, 515):
            # (an exposure ramp over the columns: the densities run from the film's base to its shoulder)
            img = synthetic_frame(H, W, seed=31 + H + W) * np.geomspace(1e-3, 30.0, W, dtype=np.float32)[None, :, None]
            p = oracle_inputs(neg, prt, 341.33, halation=False, mtf=False, grain=0)
            st.render(img, p, keep_stages=True)
            out[(H, W)] = np.ascontiguousarray(p.stages["density"])
    return out


def oracle_tail(p, density, burn=None):
    x = np.asarray(density, np.float32)
    if p.grain_lut is not None:
        x = st.apply_grain(x, p.grain_lut, p.grain_kernel, p.seed, p.grain_mono)
    if burn is not None:
        x = st.burn_apply(x, burn["map"], burn["cell"], burn["strength"])
    return st.apply_lut_tetrahedral(x, p.lut_3d, st.LUT3D_SCALE)


# ------------------------------------------------------------------------------- tail
@pytest.mark.parametrize("grain", [0, 2, 1], ids=["nograin", "colour", "mono"])
def test_tail16_every_shape_whole_and_partial_rows(ctx, densities, grain):
    p = wide_inputs(grain)
    params = setup_ctx(ctx, p)
    worst = 0
    for (H, W), dens in densities.items():
        D = to_planes(dens)
        ref = oracle_tail(p, dens)
        assert H * W < 4000 or (ref.min() < 0 and ref.max() > 1), "the frame must drive both clamps"
        f32 = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        u8 = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
        o16 = torch.empty((H, W, 3), dtype=torch.int16, device="cuda")
        ctx.stage_tail16(D, params, out_f32=f32, out_u8=u8, out_u16=o16, y0=0, y1=H, H_global=H)
        got, own = u16(o16), f32.cpu().numpy()
        assert np.array_equal(got, to_uint16(own)), f"{H}x{W}: uint16 is not the library's own float, truncated"
        d = np.abs(got.astype(np.int64) - to_uint16(ref).astype(np.int64))
        print(f"tail16 grain={grain} {H}x{W}: max |u16 - model| = {int(d.max())}, differing {float((d > 0).mean()):.4f}")
        worst = max(worst, int(d.max()))
        assert d.max() <= 1, f"{H}x{W}: {int((d > 1).sum())} samples more than 1 LSB from to_uint16(oracle)"
        # the float and uint8 outputs are r2f_stage_tail's, byte for byte
        f32b, u8b = torch.empty_like(f32), torch.empty_like(u8)
        ctx.stage_tail(D, params, out_f32=f32b, out_u8=u8b, y0=0, y1=H, H_global=H)
        assert torch.equal(f32.view(torch.int32), f32b.view(torch.int32)) and torch.equal(u8, u8b)
        o16_only = torch.empty_like(o16)
        ctx.stage_tail16(D, params, out_u16=o16_only, y0=0, y1=H, H_global=H)
        assert torch.equal(o16, o16_only)
        if H >= 3:  # a partial row range into a buffer that starts at another row (out_gy0 != 0)
            y0, y1, gy0 = 1, H - 1, 1
            part = torch.zeros((H - 1, W, 3), dtype=torch.int16, device="cuda")
            ctx.stage_tail16(D, params, out_u16=part, out_gy0=gy0, y0=y0, y1=y1, H_global=H)
            assert np.array_equal(u16(part)[: y1 - gy0], got[y0:y1]) and not u16(part)[y1 - gy0:].any()
        if grain:  # the field variant: same arithmetic, same results
            G = torch.empty((3, H, W), dtype=torch.float32, device="cuda")
            ctx.stage_grain_field(G, params, y0=0, y1=H, H_global=H)
            o16f, f32f, u8f = torch.empty_like(o16), torch.empty_like(f32), torch.empty_like(u8)
            ctx.stage_tail16(D, params, field=G, out_f32=f32f, out_u8=u8f, out_u16=o16f, y0=0, y1=H, H_global=H)
            assert np.array_equal(u16(o16f), to_uint16(f32f.cpu().numpy()))
            f32g, u8g = torch.empty_like(f32), torch.empty_like(u8)
            ctx.stage_tail_field(D, G, params, out_f32=f32g, out_u8=u8g, y0=0, y1=H, H_global=H)
            assert torch.equal(f32f.view(torch.int32), f32g.view(torch.int32)) and torch.equal(u8f, u8g)
            assert np.abs(u16(o16f).astype(np.int64) - to_uint16(ref).astype(np.int64)).max() <= 1
    assert worst <= 1


@pytest.mark.parametrize("shape", [(70, 257), (70, 515), (70, 64)])
def test_tail16_with_a_burn_map(ctx, densities, shape):
    H, W = shape
    neg = stocks()[0]
    p = wide_inputs(0)
    params = setup_ctx(ctx, p)
    dens = densities[shape]
    cell = st.burn_geometry(H, W, 3.0)[0]
    params.flags |= 32
    params.burn_cell, params.burn_strength, params.burn_d_ref = cell, 0.6, float(neg.d_ref[1])
    D = to_planes(dens)
    bmap = ctx.stage_burn_map(ctx.stage_burn_sums(D, params, y0=0, y1=H, H_global=H), params, W=W, H_global=H)
    f32 = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    o16 = torch.empty((H, W, 3), dtype=torch.int16, device="cuda")
    ctx.stage_tail16(D, params, out_f32=f32, out_u16=o16, y0=0, y1=H, H_global=H, burn_map=bmap)
    assert np.array_equal(u16(o16), to_uint16(f32.cpu().numpy()))
    ref = oracle_tail(p, dens, {"map": bmap.cpu().numpy(), "cell": cell, "strength": 0.6})
    assert np.abs(u16(o16).astype(np.int64) - to_uint16(ref).astype(np.int64)).max() <= 1
    f32b = torch.empty_like(f32)
    ctx.stage_tail(D, params, out_f32=f32b, y0=0, y1=H, H_global=H, burn_map=bmap)
    assert torch.equal(f32.view(torch.int32), f32b.view(torch.int32))


# ------------------------------------------------------------------------------- write extents
@pytest.mark.parametrize("grain", [0, 2], ids=["lut3d_kernel", "tail_kernel"])
@pytest.mark.parametrize("W", [1, 7, 257, 515])
@pytest.mark.parametrize("misalign", [0, 1, 2, 3])
def test_16bit_entries_write_their_rows_and_nothing_else(ctx, grain, W, misalign):
    """Odd widths and every 2-byte phase of the destination: a 6-byte pixel with 8-, 4- and 2-byte stores at the row segments'
    ends is where a store can land outside its rows or leave a sample unwritten."""
    H, y0, y1, gy0 = 70, 3, 68, 2
    p = wide_inputs(grain)
    params = setup_ctx(ctx, p)
    rng = np.random.default_rng(W)
    dens = rng.uniform(0.0, 3.0, size=(H, W, 3)).astype(np.float32)
    D = Arena.holding(to_planes(dens))
    a = Arena.hwc(H - gy0, W, torch.int16, misalign=misalign, device="cuda")
    ctx.stage_tail16(D.view, params, out_u16=a.view, out_gy0=gy0, y0=y0, y1=y1, H_global=H)
    ref = torch.zeros((H - gy0, W, 3), dtype=torch.int16)
    whole = torch.empty((H, W, 3), dtype=torch.int16, device="cuda")
    ctx.stage_tail16(D.view, params, out_u16=whole, y0=0, y1=H, H_global=H)
    ref[:] = whole.cpu()[gy0:]
    a.check([(None, (y0 - gy0, y1 - gy0))], expected=ref, what=f"stage_tail16 W={W} misalign={misalign}")
    assert torch.equal(a.view.cpu()[y0 - gy0:y1 - gy0], ref[y0 - gy0:y1 - gy0])
    D.unchanged("stage_tail16")
    if grain:
        G = torch.empty((3, H, W), dtype=torch.float32, device="cuda")
        ctx.stage_grain_field(G, params, y0=0, y1=H, H_global=H)
        b = Arena.hwc(H - gy0, W, torch.int16, misalign=misalign, device="cuda")
        ctx.stage_tail16(D.view, params, field=G, out_u16=b.view, out_gy0=gy0, y0=y0, y1=y1, H_global=H)
        b.check([(None, (y0 - gy0, y1 - gy0))], expected=ref, what=f"stage_tail_field16 W={W} misalign={misalign}")
    else:  # the fused pointwise pass (r2f_stage_front16): the same store
        img = dev(synthetic_frame(H, W, seed=5))
        c = Arena.hwc(H - gy0, W, torch.int16, misalign=misalign, device="cuda")
        ctx.stage_front16(img, params, out_u16=c.view, out_gy0=gy0, y0=y0, y1=y1, H_global=H)
        ctx.stage_front16(img, params, out_u16=whole, y0=0, y1=H, H_global=H)  # (a sample may really be 0xA5A5: expected=)
        c.check([(None, (y0 - gy0, y1 - gy0))], expected=whole.cpu()[gy0:], what=f"stage_front16 W={W} misalign={misalign}")
        assert torch.equal(c.view.cpu()[y0 - gy0:y1 - gy0], whole.cpu()[y0:y1])


def test_resamplers_write_their_frame_and_nothing_else(ctx):
    rng = np.random.default_rng(3)
    src = dev(rng.integers(0, 65536, size=(48, 63, 3), dtype=np.uint16).view(np.int16))
    for fn, (oh, ow) in ((ctx._lib.r2f_resize_lanczos4_u16, (75, 101)), (ctx._lib.r2f_resize_area_u16, (31, 41))):
        a = Arena.hwc(oh, ow, torch.int16, misalign=1, device="cuda")
        ctx._check(fn(ctx._h, src.data_ptr(), 48, 63, a.view.data_ptr(), oh, ow, ctx._stream()))
        plain = torch.empty((oh, ow, 3), dtype=torch.int16, device="cuda")  # (a sample may really be 0xA5A5: expected=)
        ctx._check(fn(ctx._h, src.data_ptr(), 48, 63, plain.data_ptr(), oh, ow, ctx._stream()))
        a.check([(None, (0, oh))], expected=plain.cpu(), what="resize u16")
        assert torch.equal(a.view.cpu(), plain.cpu())


@pytest.mark.parametrize("grain", [0, 2], ids=["luts_only", "graph_path"])
def test_render16_writes_its_frame_and_nothing_else(ctx, grain):
    """r2f_render16 into canary arenas at an odd width and an odd 2-byte phase, three times (eager, capture, replay): both outputs
    written whole, nothing else touched, the input unchanged."""
    neg, prt, _ = stocks()
    H, W = 37, 53
    params = setup_ctx(ctx, oracle_inputs(neg, prt, 341.33, halation=False, mtf=bool(grain), grain=grain))
    img = Arena.holding(dev(synthetic_frame(H, W, seed=6)))
    a16 = Arena.hwc(H, W, torch.int16, misalign=1, device="cuda")
    a32 = Arena.hwc(H, W, torch.float32, misalign=0, device="cuda")
    plain16 = torch.empty((H, W, 3), dtype=torch.int16, device="cuda")
    plain32 = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    ctx.render16(img.view, params, out_f32=plain32, out_u16=plain16)
    for _ in range(3):
        ctx.render16(img.view, params, out_f32=a32.view, out_u16=a16.view)
    a16.check([(None, (0, H))], expected=plain16.cpu(), what="render16 out_u16")
    a32.check([(None, (0, H))], expected=plain32.cpu(), what="render16 out_f32")
    assert torch.equal(a16.view.cpu(), plain16.cpu()) and torch.equal(a32.view.cpu().view(torch.int32), plain32.cpu().view(torch.int32))
    img.unchanged("render16")


def test_odd_addresses_are_refused(ctx, densities):
    import ctypes as C

    from raw2film_amd import _lib

    p = wide_inputs(0)
    params = setup_ctx(ctx, p)
    D = to_planes(densities[(3, 7)])
    pd = ctx.planes(D, 0)
    raw = torch.empty(3 * 7 * 6 + 2, dtype=torch.uint8, device="cuda")
    rc = ctx._lib.r2f_stage_tail16(ctx._h, C.byref(params), C.byref(pd), None, None, None, raw.data_ptr() + 1, 0, 0, 3, 7, 3, ctx._stream())
    assert rc == _lib.EINVAL and b"2-byte aligned" in ctx._lib.r2f_last_error(ctx._h)
    rc = ctx._lib.r2f_stage_tail16(ctx._h, C.byref(params), C.byref(pd), None, None, None, None, 0, 0, 3, 7, 3, ctx._stream())
    assert rc == _lib.EINVAL
    rc = ctx._lib.r2f_resize_area_u16(ctx._h, raw.data_ptr() + 1, 3, 7, raw.data_ptr(), 1, 1, ctx._stream())
    assert rc == _lib.EINVAL


def test_bad_outputs_are_refused_by_every_entry_that_writes_one(ctx):
    """No output at all, a row range that starts above the output buffer, an odd uint16 address: every case is refused with its
    message before anything is launched."""
    import ctypes as C

    from raw2film_amd import _lib

    H, W = 8, 12
    params = setup_ctx(ctx, wide_inputs(0))
    D = torch.zeros((3, H, W), dtype=torch.float32, device="cuda")
    pd = ctx.planes(D, 0)
    img = dev(synthetic_frame(H, W, seed=7))
    f32 = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    u8 = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    raw = torch.empty(H * W * 6 + 2, dtype=torch.uint8, device="cuda")
    lib, h, s = ctx._lib, ctx._h, ctx._stream()
    # entry -> (call(out_f32, second output, out_gy0, y0), is it a 16-bit entry, what it says about rows above the buffer)
    entries = {
        "r2f_stage_tail": (lambda o32, o, gy0, y0: lib.r2f_stage_tail(h, C.byref(params), C.byref(pd), None, o32, o, gy0, y0, H, W, H, s),
                           False, b"bad geometry"),
        "r2f_stage_tail16": (lambda o32, o, gy0, y0: lib.r2f_stage_tail16(h, C.byref(params), C.byref(pd), None, o32, None, o, gy0, y0, H, W,
                                                                          H, s), True, b"bad geometry"),
        "r2f_stage_front": (lambda o32, o, gy0, y0: lib.r2f_stage_front(h, C.byref(params), img.data_ptr(), 0, 0, H, _lib.UPTO_OUTPUT, None,
                                                                        o32, o, gy0, y0, H, W, H, s), False, b"y0 above the output buffer"),
        "r2f_stage_front16": (lambda o32, o, gy0, y0: lib.r2f_stage_front16(h, C.byref(params), img.data_ptr(), 0, 0, H, o32, o, gy0, y0, H,
                                                                            W, H, s), True, b"y0 above the output buffer"),
    }
    for name, (call, wide, above) in entries.items():
        good = raw.data_ptr() if wide else u8.data_ptr()
        assert call(None, None, 0, 0) == _lib.EINVAL and b"no output buffer" in lib.r2f_last_error(h), name
        for o32, o in ((f32.data_ptr(), None), (None, good), (f32.data_ptr(), good)):
            assert call(o32, o, 3, 2) == _lib.EINVAL and above in lib.r2f_last_error(h), name
        if wide:
            for o32 in (None, f32.data_ptr()):
                assert call(o32, raw.data_ptr() + 1, 0, 0) == _lib.EINVAL and b"2-byte aligned" in lib.r2f_last_error(h), name
        assert call(f32.data_ptr(), good, 0, 0) == 0, name  # (the same arguments with a good output: accepted)
    torch.cuda.synchronize()


def test_one_tail_call_writes_all_three_outputs(ctx, densities):
    """f32, u8 and u16 of ONE r2f_stage_tail16 call are what three calls with one output each write, the integer ones are the float
    one quantised, and the two rows of each buffer above y0 are left alone (out_gy0 = 3, y0 = 5: odd width, 2- and 4-byte edge
    stores)."""
    H, W, gy0, y0, y1 = 70, 257, 3, 5, 70
    params = setup_ctx(ctx, wide_inputs(0))
    D = to_planes(densities[(H, W)])
    kinds = (("out_f32", torch.float32), ("out_u8", torch.uint8), ("out_u16", torch.int16))
    together = {k: Arena.hwc(H - gy0, W, dt, device="cuda") for k, dt in kinds}
    ctx.stage_tail16(D, params, out_gy0=gy0, y0=y0, y1=y1, H_global=H, **{k: a.view for k, a in together.items()})
    written = [(None, (y0 - gy0, y1 - gy0))]
    for k, dt in kinds:
        alone = Arena.hwc(H - gy0, W, dt, device="cuda")
        ctx.stage_tail16(D, params, out_gy0=gy0, y0=y0, y1=y1, H_global=H, **{k: alone.view})
        alone.check(written, expected=alone.view.cpu(), what=f"{k} alone")
        together[k].check(written, expected=alone.view.cpu(), what=f"{k} beside the other two")  # (rows 3 and 4: the canary)
        bits = torch.int32 if dt == torch.float32 else dt
        assert torch.equal(together[k].buf.view(bits), alone.buf.view(bits)), f"{k}: not what the call with only it writes"
    own = together["out_f32"].view.cpu().numpy()[y0 - gy0:]
    assert own.min() < 0 and own.max() > 1, "the frame must drive both clamps"
    assert np.array_equal(u16(together["out_u16"].view)[y0 - gy0:], to_uint16(own))
    assert np.array_equal(together["out_u8"].view.cpu().numpy()[y0 - gy0:], st.to_uint8(own))


# ------------------------------------------------------------------------------- resamplers
def test_lanczos4_tables_one_cache_per_entry_and_a_key_for_the_f32_one(ctx):
    """The float32, uint16 and uint8 LANCZOS4 resizes keep one table cache each: none evicts another's, a repeated float32 call at
    an unchanged geometry uploads nothing (`generation` stays) and a new geometry does.  Every result is compared bit for bit with
    its entry's model; a stale or shared key shows as a wrong image."""
    post = __import__("oracle.post", fromlist=["post"])
    img32 = np.random.default_rng(95).uniform(0, 4, (13, 17, 3)).astype(np.float32)
    img16 = frame16(11, 9, seed=1)
    img8 = np.random.default_rng(9).integers(0, 256, (9, 14, 3)).astype(np.uint8)
    t32, t16, t8 = dev(img32), dev(img16.view(np.int16)), dev(img8)

    def f32(oh, ow):
        got = ctx.resize_lanczos4_f32(t32, oh, ow).cpu().numpy().transpose(1, 2, 0)
        np.testing.assert_array_equal(got, post.resize_lanczos4_f32(img32, oh, ow))
        return got

    def wide():
        np.testing.assert_array_equal(u16(ctx.resize_lanczos4_u16(t16, 20, 33)), lanczos4_u16(img16, 20, 33))

    def narrow():
        np.testing.assert_array_equal(ctx.resize_lanczos4_u8(t8, 25, 19).cpu().numpy(), st.resize_lanczos4_u8(img8, 25, 19))

    first = f32(29, 23)  # (i)
    gen = ctx.generation()
    again = f32(29, 23)  # (ii)
    assert ctx.generation() == gen, "a repeated float32 resize at an unchanged geometry uploaded its tables again"
    assert np.array_equal(first.view(np.int32), again.view(np.int32))
    wide()  # (iii)
    narrow()  # (iv)
    f32(29, 23)  # (v)
    gen = ctx.generation()
    f32(31, 40)  # (vi)
    assert ctx.generation() != gen, "a new geometry must upload its tables"
    f32(29, 23)  # (vii)
    wide(), narrow()  # (viii)


def frame16(H, W, seed):
    """0, 65535, steps and noise: the LANCZOS4 overshoot saturates at both ends."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 65536, size=(H, W, 3), dtype=np.uint16)
    a[:, : W // 3] = 0
    a[:, W // 3: 2 * W // 3] = 65535
    a[H // 2:, : W // 2] = np.where((np.arange(W // 2) // 2 % 2 == 0)[None, :, None], 0, 65535)
    return a


def check_resampler(name, got, ref, saturates=False):
    d = np.abs(got.astype(np.int64) - ref.astype(np.int64))
    print(f"{name}: {got.shape}, differing samples {float((d > 0).mean()):.5f}, max {int(d.max())}")
    assert not saturates or (got.min() == 0 and got.max() == 65535)
    assert d.max() <= 1, f"{name}: {int((d > 1).sum())} samples more than 1 LSB from the model"


@pytest.mark.parametrize("src,dst", [((5, 7), (13, 17)), ((48, 64), (75, 100))])
def test_lanczos4_u16(ctx, src, dst):
    a = frame16(*src, seed=1)
    got = u16(ctx.resize_lanczos4_u16(dev(a.view(np.int16)), *dst))
    ref32 = __import__("oracle.post", fromlist=["post"]).resize_lanczos4_f32(a.astype(np.float32), *dst)
    if src == (48, 64):  # the overshoot leaves [0, 65535] at both ends before the clamp
        assert ref32.min() < 0 and ref32.max() > 65535
    check_resampler("lanczos4_u16", got, lanczos4_u16(a, *dst), saturates=src == (48, 64))


@pytest.mark.parametrize("src,dst,exact", [((48, 64), (24, 32), True), ((48, 63), (16, 21), False), ((75, 100), (48, 64), False),
                                           ((1, 64), (1, 20), False), ((64, 1), (20, 1), False), ((7, 9), (7, 9), False),
                                           ((68, 102), (4, 6), False)])  # 17 x 17 = 289 samples: a bright block's float sum rounds
def test_area_u16(ctx, src, dst, exact):
    a = frame16(*src, seed=2)
    got = u16(ctx.resize_area_u16(dev(a.view(np.int16)), *dst))
    ref = area_u16(a, *dst)
    if exact:  # the integer 2 x 2 path: (a + b + c + d + 2) >> 2, bit for bit
        s = a.astype(np.int64).reshape(dst[0], 2, dst[1], 2, 3).sum(axis=(1, 3))
        assert np.array_equal(got, ((s + 2) >> 2).astype(np.uint16))
    check_resampler("area_u16", got, ref)


# ------------------------------------------------------------------------------- r2f_render16 and the graph cache
def test_render16_replays_its_own_graph_and_never_the_8bit_one(ctx):
    neg, prt, _ = stocks()
    H, W = 96, 131
    p = oracle_inputs(neg, prt, 341.33, halation=False, mtf=True, grain=2)
    params = setup_ctx(ctx, p)
    img = dev(synthetic_frame(H, W, seed=9))
    o16 = torch.empty((H, W, 3), dtype=torch.int16, device="cuda")
    u8 = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    before = ctx.render_stats()
    D, D2 = (torch.empty((3, H, W), dtype=torch.float32, device="cuda") for _ in range(2))
    for i, seed in enumerate((11, 22, 33, 44)):
        params.seed = seed
        ctx.render16(img, params, out_u16=o16)
        got16 = u16(o16).copy()
        ctx.render(img, params, out_u8=u8, want_f32=False)  # alternating on the same input and workspace
        got8 = u8.cpu().numpy()
        # the eager r2f_stage_*16 sequence
        ctx.stage_front(img, params, 1, dst=D, y0=0, y1=H, H_global=H)
        ctx.stage_mtf(D, D2, params, y0=0, y1=H, H_global=H)
        e16, e8 = torch.empty_like(o16), torch.empty_like(u8)
        ctx.stage_tail16(D2, params, out_u8=e8, out_u16=e16, y0=0, y1=H, H_global=H)
        assert np.array_equal(got16, u16(e16)), f"frame {i}: render16 differs from the stage calls"
        assert np.array_equal(got8, e8.cpu().numpy()), f"frame {i}: render after render16 wrote something else"
    after = ctx.render_stats()
    assert after["captures"] - before["captures"] >= 2 and after["replays"] - before["replays"] >= 2  # (one graph per output kind)
    ref = st.render(synthetic_frame(H, W, seed=9), oracle_inputs(neg, prt, 341.33, halation=False, mtf=True, grain=2, seed=44))
    assert np.abs(got16.astype(np.int64) - to_uint16(ref).astype(np.int64)).max() <= 1


def test_render16_luts_only_and_float_beside_it(ctx):
    neg, prt, _ = stocks()
    H, W = 37, 53
    p = oracle_inputs(neg, prt, 341.33, halation=False, mtf=False, grain=0)
    params = setup_ctx(ctx, p)
    img = synthetic_frame(H, W, seed=4)
    f32, o16 = ctx.render16(dev(img), params, want_f32=True)
    assert np.array_equal(u16(o16), to_uint16(f32.cpu().numpy()))
    assert np.abs(u16(o16).astype(np.int64) - to_uint16(st.render(img, p)).astype(np.int64)).max() <= 1


# ------------------------------------------------------------------------------- processor
# (9/16 mm by 3/8 mm: both exact in binary, so the aspect is exactly 96 / 64 and the aspect crop keeps the whole frame)
KW = dict(frame_width=0.5625, frame_height=0.375, halation_green_factor=0.3, exp_kelvin=6000,
          color_masking=1.0, seed=SEED, lens_correction=False)


@pytest.fixture(scope="module")
def proc():
    from raw2film_amd import HipProcessor

    pr = HipProcessor(device=0)
    yield pr
    pr.close()


@pytest.fixture(scope="module")
def frame():
    return st.apply_matrix3x3(synthetic_frame(64, 96, seed=21), st.REC709_TO_XYZ).astype(np.float32)


def test_process_16_against_the_model_and_8_bit_unchanged(proc, frame):
    neg, prt, _ = stocks()
    before = proc.process(frame, neg, 6, 0.4, print_film=prt, **KW)
    out = proc.process(frame, neg, 6, 0.4, print_film=prt, output_bits=16, **KW)
    assert out.dtype == np.uint16 and out.shape == (64, 96, 3) and out.flags.writeable
    scale = 96 / KW["frame_width"]
    ref = st.render(frame, oracle_inputs(neg, prt, scale, matrix=False))
    assert np.abs(out.astype(np.int64) - to_uint16(ref).astype(np.int64)).max() <= 1
    hist = proc.generate_histogram()
    assert np.array_equal(hist, proc.generate_histogram((out // 257).astype(np.uint8)))
    after = proc.process(frame, neg, 6, 0.4, print_film=prt, **KW)
    assert after.dtype == np.uint8 and np.array_equal(before, after)
    with pytest.raises(ValueError, match="RGBA8"):
        proc.process(frame, neg, 6, 0.4, print_film=prt, output_bits=16,
                     dst_texture=torch.empty((32, 48, 4), dtype=torch.uint8, device="cuda"), **KW)


def test_process_16_with_a_canvas(proc, frame):
    from raw2film_amd import geometry

    neg, prt, _ = stocks()
    plain = proc.process(frame, neg, 6, 0.4, print_film=prt, output_bits=16, **KW)
    for mode in ("Uniform white", "Proportional black", "Fixed"):
        kw = dict(KW, canvas_mode=mode, canvas_scale=1.25, max_scale=None)
        shape, color, (oy, ox) = geometry.canvas_layout((64, 96), mode, 1.25, 1.0)
        out = proc.process(frame, neg, 6, 0.4, print_film=prt, output_bits=16, **kw)
        assert out.dtype == np.uint16 and out.shape[:2] == tuple(shape[:2])
        assert np.array_equal(out[oy:oy + 64, ox:ox + 96], plain)
        assert np.array_equal(out[0, 0], np.asarray(color, np.uint16) * 257)


def test_process_16_max_scale_goes_back_up_through_lanczos4(proc, frame):
    neg, prt, _ = stocks()
    kw = dict(KW, max_scale=0.6 * 96 / KW["frame_width"])  # the pipeline runs at 0.6 x and the result is scaled back to 64 x 96
    out = proc.process(frame, neg, 6, 0.4, print_film=prt, output_bits=16, **kw)
    payload = proc.extract_image_data_cpu(frame, lens_correction=False, frame_width=kw["frame_width"], frame_height=kw["frame_height"],
                                          max_scale=kw["max_scale"])
    assert payload["upscale_to"] is not None and out.shape == (64, 96, 3) and out.dtype == np.uint16
    small = proc.process_preloaded(dict(payload, upscale_to=None, final_resolution=None), neg, 6, 0.4, print_film=prt,
                                   output_bits=16, **kw)
    ref = lanczos4_u16(small, 64, 96)
    assert np.abs(out.astype(np.int64) - ref.astype(np.int64)).max() <= 1


def test_process_preloaded_cpu_final_scaling_16(proc, frame):
    neg, prt, _ = stocks()
    payload = proc.extract_image_data_cpu(frame, lens_correction=False, frame_width=KW["frame_width"], frame_height=KW["frame_height"])
    full = proc.process_preloaded(payload, neg, 6, 0.4, print_film=prt, final_scaling="cpu", output_bits=16, **KW)
    small = proc.process_preloaded(dict(payload, final_resolution=(32, 48)), neg, 6, 0.4, print_film=prt, final_scaling="cpu",
                                   output_bits=16, **KW)
    assert small.shape == (32, 48, 3) and small.dtype == np.uint16
    assert np.abs(small.astype(np.int64) - area_u16(full, 32, 48).astype(np.int64)).max() <= 1
    pending = proc.submit_preloaded(payload, neg, 6, 0.4, print_film=prt, final_scaling="cpu", output_bits=16, **KW)
    assert np.array_equal(pending.result(), full) and pending.result().dtype == np.uint16


def test_process_array_16_returns_the_device_tensor(proc, frame):
    neg, prt, _ = stocks()
    kw = {k: v for k, v in KW.items() if k != "lens_correction"}
    t = proc.process_array(frame, neg, 6, 0.4, print_film=prt, output="device", output_bits=16, **kw)
    assert t.is_cuda and t.dtype == torch.uint16 and tuple(t.shape) == (64, 96, 3)
    host = proc.process_array(frame, neg, 6, 0.4, print_film=prt, output_bits=16, **kw)
    assert host.dtype == np.uint16 and np.array_equal(host, t.view(torch.int16).cpu().numpy().view(np.uint16))
    assert np.array_equal(host, proc.process(frame, neg, 6, 0.4, print_film=prt, output_bits=16, **KW))
    with pytest.raises(ValueError):
        proc.process_array(frame, neg, 6, 0.4, return_float=True, output_bits=16)


# ------------------------------------------------------------------------------- streaming, lending, TIFF
BIG = dict(frame_width=36.0, frame_height=36.0 * 1200 / 4800, exp_kelvin=6000, color_masking=1.0, seed=SEED, lens_correction=False)


@pytest.fixture(scope="module")
def big_frame():
    """1200 x 4800 x 3 = 17.3 M samples: above the streaming threshold, at least three bands."""
    small = st.apply_matrix3x3(synthetic_frame(150, 600, seed=8), st.REC709_TO_XYZ).astype(np.float32)
    return np.ascontiguousarray(np.kron(small, np.ones((8, 8, 1), np.float32)) * np.linspace(0.5, 1.5, 4800, dtype=np.float32)[None, :, None])


@pytest.fixture(scope="module")
def streamer():
    from raw2film_amd import HipProcessor

    from raw2film_amd.hip_processor import plan_bands

    pr = HipProcessor(device=0)
    # 1200 rows: two bands of 600 whose halves the taper cuts again -> four bands
    assert len(plan_bands(1200, 0, (0, 0), (0, 0), pr.stream_bands, pr.stream_taper)[0]) - 1 >= 3
    yield pr
    pr.close()


def test_streamed_16_bit_frame_and_lending(streamer, big_frame):
    neg, prt, _ = stocks()
    kw = dict(BIG, halation=False, sharpness=False, print_film=prt)  # grain and LUTs only: pointwise per band, byte-identical
    streamer.stream_rejected = "unset"
    out = streamer.process(big_frame, neg, 6, 0.4, cache=False, output_bits=16, **kw)
    assert streamer.stream_rejected is None, streamer.stream_rejected
    assert out.dtype == np.uint16 and out.shape == (1200, 4800, 3) and out.flags.writeable
    streamer.stream_bands = 0
    whole = streamer.process(big_frame, neg, 6, 0.4, cache=False, output_bits=16, **kw)
    streamer.stream_bands = 16
    assert np.array_equal(out, whole)
    # lending: an 8-bit call between two 16-bit ones hands out 8-bit memory of its own, and the other way round
    keep16 = out.copy()
    out8 = streamer.process(big_frame, neg, 6, 0.4, cache=False, **kw)
    assert out8.dtype == np.uint8 and out8.shape == out.shape and np.array_equal(out, keep16)
    assert not np.shares_memory(out8, out)
    again = streamer.process(big_frame, neg, 6, 0.4, cache=False, output_bits=16, **kw)
    assert again.dtype == np.uint16 and np.array_equal(again, keep16) and not np.shares_memory(again, out8)
    del out8, again
    # with halation and MTF the bands agree with the one-piece render to the FFT form's rounding: within 1 LSB
    kw2 = dict(BIG, print_film=prt, halation_green_factor=0.3)
    a = streamer.process(big_frame, neg, 6, 0.4, cache=False, output_bits=16, **kw2)
    assert streamer.stream_rejected is None, streamer.stream_rejected
    streamer.stream_bands = 0
    b = streamer.process(big_frame, neg, 6, 0.4, cache=False, output_bits=16, **kw2)
    streamer.stream_bands = 16
    d = np.abs(a.astype(np.int64) - b.astype(np.int64))
    print(f"streamed vs one piece with halation and MTF: differing {float((d > 0).mean()):.6f}, max {int(d.max())}")
    assert d.max() <= 1


@pytest.mark.parametrize("bits", [8, 16])
def test_process_tiff_bytes_and_file(proc, frame, bits, tmp_path):
    from PIL import Image

    neg, prt, _ = stocks()
    icc = b"an ICC profile of odd length."
    ref = proc.process(frame, neg, 6, 0.4, print_film=prt, output_bits=bits, **KW)
    data = proc.process_tiff(frame, neg, 6, 0.4, print_film=prt, output_bits=bits, icc_profile=icc, **KW)
    arr, tags, _ = read_tiff(data)
    assert arr.dtype == ref.dtype and np.array_equal(arr, ref) and tags[34675] == icc
    path = str(tmp_path / f"out{bits}.tif")
    n = proc.process_tiff(frame, neg, 6, 0.4, path, print_film=prt, output_bits=bits, icc_profile=icc, **KW)
    assert n == len(data) and open(path, "rb").read() == data
    img = Image.open(path)
    assert img.size == (96, 64) and np.array_equal(np.asarray(img), ref if bits == 8 else (ref >> 8).astype(np.uint8))
    with pytest.raises(ValueError, match="dst_texture"):
        proc.process_tiff(frame, neg, 6, 0.4, print_film=prt, dst_texture=object(), **KW)
    payload = proc.extract_image_data_cpu(frame, lens_correction=False, frame_width=KW["frame_width"], frame_height=KW["frame_height"])
    buf = io.BytesIO()
    proc.process_preloaded_tiff(payload, neg, 6, 0.4, buf, final_scaling="cpu", print_film=prt, output_bits=bits, icc_profile=icc, **KW)
    arr2, tags2, _ = read_tiff(buf.getvalue())
    assert tags2[34675] == icc and np.array_equal(arr2, proc.process_preloaded(payload, neg, 6, 0.4, final_scaling="cpu", print_film=prt,
                                                                                   output_bits=bits, **KW))


def test_process_tiff_streamed_is_the_one_piece_file_of_the_streamed_render(streamer, big_frame, tmp_path):
    from raw2film_amd import tiff

    neg, prt, _ = stocks()
    kw = dict(BIG, print_film=prt, halation_green_factor=0.3)
    pixels = streamer.process(big_frame, neg, 6, 0.4, cache=False, output_bits=16, **kw)
    assert streamer.stream_rejected is None
    path = str(tmp_path / "streamed.tif")
    n = streamer.process_tiff(big_frame, neg, 6, 0.4, path, stream=True, icc_profile=b"icc", **kw)
    assert streamer.stream_rejected is None, streamer.stream_rejected
    want = tiff.encode(pixels, b"icc")
    assert n == len(want) and open(path, "rb").read() == want
    # a frame that cannot stream (a canvas) is exported in one piece, and stream_rejected says why
    small = big_frame[:64, :96]
    data = streamer.process_tiff(small, neg, 6, 0.4, stream=True, canvas_mode="Uniform white", canvas_scale=1.25, **kw)
    assert streamer.stream_rejected is not None
    arr, _, _ = read_tiff(data)
    assert arr.dtype == np.uint16 and np.array_equal(arr, streamer.process(small, neg, 6, 0.4, output_bits=16, canvas_mode="Uniform white",
                                                                             canvas_scale=1.25, **kw))
