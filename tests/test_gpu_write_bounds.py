"""Extent of every write through the C ABI: a call writes rows [y0, y1) of its destination -- or the bytes it was given -- and
nothing else, and leaves nothing of them unwritten.  Needs an MI355X.

Every destination is a view inside a canary-filled allocation with guards round it (tests/arena.py); sources sit in arenas of
their own and must come back unchanged.  One parametrised driver, one table of entry points (CASES).  A case asserts
  1. the arena: nothing outside the entitled region changed, nothing inside was left;
  2. the values: against the oracle at the tolerance the entry's parity test uses (tests/test_gpu_parity.py,
     tests/test_gpu_processor.py, tests/test_gpu_decode.py, tests/test_gpu_histogram.py -- the numbers are copied from there), and
     BIT FOR BIT against the same call into a plain aligned torch.empty destination covering the whole frame, wherever the same
     kernel runs in both (only loads and stores differ between a kernel's vector and scalar paths).  Where the arena's alignment
     selects a different kernel the table says so (`contract_only`) and only the oracle comparison applies;
  3. the return code: R2F_OK, or -- where include/r2f.h states an alignment the layout breaks -- R2F_EINVAL and an untouched arena
     (`refuses`).

Geometry of the row-aware entries: a true shard, rows [y0, y1) with y0 = 37 (not a multiple of 32) of an H_global = y1 + 9 row
frame, into a destination that starts 3 rows above y0 and ends 2 rows below y1; widths either side of the 64-, 128- and 256-pixel
tile and block widths with and without W % 4 == 0, row counts either side of the 32- and 64-row tiles; plane pads of 0, 1 and 4
floats and a base 0 or 1 element past a 16-byte boundary select the vector and the scalar path of each kernel.  FULL: every width
at one row count and every row count at two widths (one odd), 48 geometries; SHORT: 8 of them, for the further variants of an
entry whose first variant ran FULL.

Out of scope: memory the context owns (FFT pass scratch, spectra, JPEG encoder scratch, the exposure-range record) cannot be
wrapped from outside.  Nothing here writes out of bounds on purpose.
"""

import ctypes as C
import functools
from collections import Counter, namedtuple

import numpy as np
import pytest

from oracle import histogram as oh
from oracle import post
from oracle import stages as st

from arena import Arena, guard_elems
from helpers import assert_close, oracle_inputs, stocks, synthetic_frame

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

Y0, ABOVE, BELOW, AFTER = 37, 3, 2, 9
WIDTHS = (1, 3, 4, 5, 63, 64, 65, 68, 127, 128, 129, 255, 256, 257, 260)
ROW_COUNTS = (1, 3, 4, 31, 32, 33, 63, 64, 65)


class Geo(namedtuple("Geo", "W rows misalign pad")):
    y0 = property(lambda s: Y0)
    y1 = property(lambda s: Y0 + s.rows)
    H = property(lambda s: Y0 + s.rows + AFTER)           # H_global: rows after the shard
    gy0 = property(lambda s: Y0 - ABOVE)                   # first global row the destination holds
    rows_alloc = property(lambda s: s.rows + ABOVE + BELOW)
    a = property(lambda s: ABOVE)                          # the shard's rows in the destination's own numbering: [a, b)
    b = property(lambda s: ABOVE + s.rows)
    planes_vec = property(lambda s: s.W % 4 == 0 and s.misalign == 0 and s.pad % 4 == 0)  # planes_vec_ok of r2f_ctx.h
    hwc_vec = property(lambda s: s.W % 4 == 0 and s.misalign == 0)

    def __str__(self):
        return f"W{self.W}-r{self.rows}-m{self.misalign}-p{self.pad}"


def full_matrix():
    geos = []
    for i, W in enumerate(WIDTHS):  # every width at one row count, aligned and misaligned, the pads in turn
        geos += [Geo(W, 33, 0, (0, 4, 1)[i % 3]), Geo(W, 33, 1, (1, 0, 4)[i % 3])]
    for rows in ROW_COUNTS:  # every row count at two widths: one odd (scalar path), one that allows the vector path
        geos += [Geo(65, rows, 0, 0), Geo(128, rows, 0, 0)]
    return geos


FULL = full_matrix()
SHORT = [Geo(5, 33, 1, 1), Geo(65, 33, 0, 0), Geo(128, 33, 0, 0), Geo(128, 33, 1, 4), Geo(257, 4, 0, 1), Geo(260, 65, 0, 4),
         Geo(65, 64, 1, 0), Geo(128, 1, 0, 0)]
assert any(g.planes_vec for g in FULL) and any(not g.planes_vec and g.W % 4 == 0 for g in FULL)
assert any(g.planes_vec for g in SHORT) and any(not g.planes_vec and g.W % 4 == 0 for g in SHORT)

EINVAL = -1
SEED = 77


@pytest.fixture(scope="module")
def ctx():
    from raw2film_amd.context import HipContext

    c = HipContext(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ small helpers
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def planes_np(a):
    return np.ascontiguousarray(np.transpose(a, (2, 0, 1)))


def from_planes(t):
    return np.transpose(t.cpu().numpy(), (1, 2, 0))


def bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b, what):
    assert torch.equal(bits(a), bits(b)), f"{what}: differs from the same call into a plain aligned destination"


def empty(shape, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device="cuda")


def src_planes(g, frame, lo, hi):
    """Rows [lo, hi) of an (H, W, 3) frame as source planes in an arena of their own, laid out like the destination."""
    return Arena.holding(dev(planes_np(frame[lo:hi])), misalign=g.misalign, pad=g.pad)


def dst_planes(g):
    return Arena.planes(g.rows_alloc, g.W, pad=g.pad, misalign=g.misalign, device="cuda")


def rows_of(g, planes=(0, 1, 2)):
    return [(p, (g.a, g.b)) for p in planes]


def check_planes(g, arena, plain, expected, tol, floor, what, planes=(0, 1, 2), bitwise=True, abs_tol=None):
    torch.cuda.synchronize()
    arena.check(rows_of(g, planes), what=what)
    got = arena.view[:, g.a:g.b]
    if bitwise:
        for p in planes:
            same_bits(got[p], plain[p, g.y0:g.y1], f"{what} plane {p}")
    if expected is not None:
        sel = list(planes)
        if abs_tol is not None:
            assert np.abs(from_planes(got)[..., sel] - expected[..., sel]).max() <= abs_tol, what
        else:
            assert_close(from_planes(got)[..., sel], expected[..., sel], tol, floor, what)


def u8_close(got, ref_f32):
    """The parity tests' uint8 rule: at most 1 LSB, on at most 1e-4 of the samples (test_front_stages_and_layouts); frames too small
    for a fraction to mean anything assert the LSB alone, like test_tiny_and_ragged_frames_full_pipeline."""
    d = np.abs(got.astype(int) - st.to_uint8(ref_f32).astype(int))
    assert d.max() <= 1
    if d.size >= 10000:
        assert (d > 0).mean() <= 1e-4


def hwc_outputs(g, outputs, rows=None, W=None):
    rows, W = g.rows_alloc if rows is None else rows, g.W if W is None else W
    af = Arena.hwc(rows, W, torch.float32, misalign=g.misalign, device="cuda") if outputs in ("f32", "both") else None
    au = Arena.hwc(rows, W, torch.uint8, misalign=g.misalign, device="cuda") if outputs in ("u8", "both") else None
    return af, au


def plain_hwc(outputs, H, W):
    return (empty((H, W, 3)) if outputs in ("f32", "both") else None,
            empty((H, W, 3), torch.uint8) if outputs in ("u8", "both") else None)


def check_hwc(g, af, au, pf, pu, ref, what, bitwise=True, a=None, b=None, y0=None, y1=None):
    """af / au: the arenas; pf / pu: the plain call's whole-frame outputs; ref: the oracle's float rows [y0, y1)."""
    a, b = g.a if a is None else a, g.b if b is None else b
    y0, y1 = g.y0 if y0 is None else y0, g.y1 if y1 is None else y1
    torch.cuda.synchronize()
    if af is not None:
        af.check([(None, (a, b))], what=what + " f32")
        if bitwise:
            same_bits(af.view[a:b], pf[y0:y1], what + " f32")
        assert_close(af.view[a:b].cpu().numpy(), ref, 1e-5, 1e-3, what + " f32")
    if au is not None:
        exp = torch.zeros(au.shape, dtype=torch.uint8)
        exp[a:b] = pu[y0:y1].cpu()
        au.check([(None, (a, b))], expected=exp, what=what + " u8")
        if bitwise:
            same_bits(au.view[a:b], pu[y0:y1], what + " u8")
        u8_close(au.view[a:b].cpu().numpy(), ref)


def view_or_none(arena):
    return arena.view if arena is not None else None


@functools.lru_cache(maxsize=None)
def inputs(kind):
    neg, prt, _ = stocks()
    if kind == "luts":
        return oracle_inputs(neg, prt, 100.0, halation=False, mtf=False, grain=0)
    if kind == "split":
        return oracle_inputs(neg, prt, 250.0, mtf=False, grain=0)  # a colour stock: the blue layer's halation is one tap
    if kind == "pipeline":
        return oracle_inputs(neg, prt, 120.0)  # 31-tap halation (FFT form), 13-tap MTF, grain
    if kind in ("grain2", "grain1"):
        return oracle_inputs(neg, prt, 341.33, halation=False, mtf=False, grain=int(kind[-1]), seed=SEED)
    raise KeyError(kind)


def setup_ctx(ctx, p):
    from test_gpu_parity import setup_ctx as parity_setup

    return parity_setup(ctx, p)


class options:
    """Set context options for a case and put the defaults back."""
    DEFAULTS = {"front_fast": 1, "stencil_variant": -1, "stencil_fixed": 1, "stencil_fft_window_rows": 0, "stencil_fft_epilogue_lds": 1,
                "grain_fixed": 1, "grain_separable": 1, "render_graph": 1}

    def __init__(self, ctx, **opts):
        self.ctx, self.opts = ctx, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.ctx.set_option(k, self.DEFAULTS[k])


def layout_of_image(img, layout):
    if layout == "hwc3":
        return img
    if layout == "hwc4":
        return np.concatenate([img, np.ones(img.shape[:2] + (1,), np.float32)], axis=-1)
    return planes_np(img)


# ------------------------------------------------------------------------------------------------ the front
def front_contract_only(g, upto=2, fast=1, **_):
    """The arena's alignment sends the call to the generic pointwise kernel while the plain call takes r2f_front.hip's fast one
    (front_fast_eligible wants the vector path)."""
    vec = g.hwc_vec if upto == 2 else g.planes_vec
    return bool(fast) and g.W % 4 == 0 and not vec


def run_front(ctx, g, upto, layout, fast, outputs="f32"):
    p = inputs("luts")
    params = setup_ctx(ctx, p)
    what = f"stage_front upto {upto} {layout} fast {fast} {outputs} {g}"
    bitwise = not front_contract_only(g, upto, fast)
    img = synthetic_frame(g.H, g.W, seed=3)
    img[g.y0, :2] = 0.0  # S < 1e-12 branch of the 2-D LUT
    lo, hi = g.y0 - 2, g.y1 + 1
    ref = st.render(img[g.y0:g.y1], p, keep_stages=True)
    with options(ctx, front_fast=fast):
        src = Arena.holding(dev(layout_of_image(img[lo:hi], layout)), misalign=g.misalign)
        whole = dev(layout_of_image(img, layout))
        if upto < 2:
            dst, plain = dst_planes(g), empty((3, g.H, g.W))
            ctx.stage_front(src.view, params, upto, in_gy0=lo, dst=dst.view, dst_gy0=g.gy0, y0=g.y0, y1=g.y1, H_global=g.H, layout=layout)
            ctx.stage_front(whole, params, upto, dst=plain, y0=g.y0, y1=g.y1, H_global=g.H, layout=layout)
            expected, floor = (p.stages["exposure"], 1e-4) if upto == 0 else (p.stages["density"], 1e-3)
            check_planes(g, dst, plain, expected, 1e-5, floor, what, bitwise=bitwise)
        else:
            (af, au), (pf, pu) = hwc_outputs(g, outputs), plain_hwc(outputs, g.H, g.W)
            ctx.stage_front(src.view, params, 2, in_gy0=lo, out_f32=view_or_none(af), out_u8=view_or_none(au), out_gy0=g.gy0, y0=g.y0,
                            y1=g.y1, H_global=g.H, layout=layout)
            ctx.stage_front(whole, params, 2, out_f32=pf, out_u8=pu, y0=g.y0, y1=g.y1, H_global=g.H, layout=layout)
            check_hwc(g, af, au, pf, pu, ref, what, bitwise=bitwise)
    src.unchanged(what)


def split_contract_only(g, **_):
    """r2f_stage_front_split falls back to plain r2f_stage_front (mask 0) while the plain call takes the split fast kernel."""
    return g.W % 4 == 0 and not g.planes_vec


def run_front_split(ctx, g):
    p = inputs("split")
    params = setup_ctx(ctx, p)
    what = f"stage_front_split {g}"
    img = synthetic_frame(g.H, g.W, seed=4)
    lo, hi = g.y0 - 2, g.y1 + 1
    st.render(img[g.y0:g.y1], p, keep_stages=True)  # (the blue layer's single tap needs no neighbours: its rows alone will do)
    src = Arena.holding(dev(img[lo:hi]), misalign=g.misalign)
    E, D, pE, pD = dst_planes(g), dst_planes(g), empty((3, g.H, g.W)), empty((3, g.H, g.W))
    mask = ctx.stage_front_split(src.view, params, E.view, D.view, in_gy0=lo, exposure_gy0=g.gy0, density_gy0=g.gy0, y0=g.y0, y1=g.y1,
                                 H_global=g.H, layout="hwc3")
    pmask = ctx.stage_front_split(dev(img), params, pE, pD, y0=g.y0, y1=g.y1, H_global=g.H, layout="hwc3")
    assert mask == (4 if g.planes_vec else 0) and pmask == (4 if g.W % 4 == 0 else 0), (what, mask, pmask)
    assert (mask == pmask) == (not split_contract_only(g))
    written = (0, 1) if mask else (0, 1, 2)
    check_planes(g, E, pE, p.stages["exposure"], 1e-5, 1e-4, what + " exposure", planes=written, bitwise=mask == pmask)
    if mask:
        check_planes(g, D, pD, p.stages["density"], 1e-5, 1e-3, what + " density", planes=(2,), bitwise=mask == pmask)
    else:
        D.check(None, what=what + " density (fallback: not written at all)")
    src.unchanged(what)


# ------------------------------------------------------------------------------------------------ the stencils
def sym_kernel(n, seed):
    rng = np.random.default_rng(seed)
    k = rng.uniform(0.0, 1.0, (n, n, 3)).astype(np.float32)
    k = (k + k[:, ::-1]) / 2
    return k / k.sum(axis=(0, 1), keepdims=True)


def run_stencil(ctx, g, stage, form, variant=-1, fixed=1, window_rows=0, epi_lds=1):
    """form "direct": a 5 x 5 stencil (unrolled with stencil_fixed on the default tile, the entry list otherwise); "fft": 25 x 25 =
    625 taps, past the 400 of the FFT form and past the last unrolled size of either stage."""
    n = 5 if form == "direct" else 25
    which = 0 if stage == "halation" else 1
    what = f"stage_{stage} {form} variant {variant} fixed {fixed} window rows {window_rows} epilogue lds {epi_lds} {g}"
    k = sym_kernel(n, 100 + n)
    rng = np.random.default_rng(g.W * 131 + g.rows)
    frame = rng.uniform(0.01, 2.0, (g.H, g.W, 3)).astype(np.float32)
    r = n // 2
    lo, hi = max(g.y0 - r, 0), min(g.y1 + r, g.H)
    curve = stocks()[0].get_density_curve(push_pull=0.0, color_masking=1.0)
    ref = st.convolve_2d(frame, k)
    if stage == "halation":
        ref = st.multi_channel_interp(st.log_clip(ref), curve)
    with options(ctx, stencil_variant=variant, stencil_fixed=fixed, stencil_fft_window_rows=window_rows, stencil_fft_epilogue_lds=epi_lds):
        ctx.set_kernel(which, k)
        ctx.set_curve1d(curve)
        params = ctx.make_params()

        def call(s, sg, d, dg):
            kw = dict(src_gy0=sg, dst_gy0=dg, y0=g.y0, y1=g.y1, H_global=g.H)
            if stage == "halation":
                ctx.stage_halation(s, d, params, **kw)
            elif stage == "mtf":
                ctx.stage_mtf(s, d, params, **kw)
            else:
                ctx.stage_stencil(which, s, d, **kw)

        src, dst, plain = src_planes(g, frame, lo, hi), dst_planes(g), empty((3, g.H, g.W))
        call(src.view, lo, dst.view, g.gy0)
        call(dev(planes_np(frame)), 0, plain, 0)
        stats = ctx.stencil_stats(which)
        assert [c["fft"] for c in stats] == [int(form == "fft")] * 3, what
        if form == "direct":
            assert [c["unrolled"] for c in stats] == [r if fixed and variant <= 0 else 0] * 3, what
        elif window_rows:
            assert all(c["window"][0] == window_rows for c in stats), (what, stats)
        check_planes(g, dst, plain, ref[g.y0:g.y1], 1e-5, 1e-3, what)
    src.unchanged(what)


# ------------------------------------------------------------------------------------------------ the tail and the grain
def grain_kernel(form):
    if form == "separable":  # a Gaussian: u v^T to fp32 rounding
        ax = np.arange(-2, 3)
        k = np.exp(-(ax[:, None] ** 2 + ax[None, :] ** 2) / (2.0 * 1.1 ** 2))[..., None]
    else:  # mirror symmetric, not rank one: the 2-D forms
        k = np.random.default_rng(5).uniform(0.1, 1.0, (5, 5, 1))
        k = (k + k[:, ::-1]) / 2
    return (k / np.sqrt((k ** 2).sum())).astype(np.float32)[..., 0]


def grain_setup(ctx, form, mono):
    """-> (params, oracle inputs, taps); the context's options are the caller's to set (grain_options)."""
    p = inputs("grain1" if mono else "grain2")
    setup_ctx(ctx, p)
    k = grain_kernel(form)
    ctx.set_kernel(2, k)
    return ctx.make_params(grain=True, grain_mono=mono, seed=SEED), p, k


def grain_options(ctx, form):
    return options(ctx, grain_fixed=0 if form == "list" else 1, grain_separable=1 if form == "separable" else 0)


def assert_grain_form(ctx, form, what):
    s = ctx.stencil_stats(2)[0]
    assert (s["unrolled"], s["separable"]) == {"fixed": (2, 0), "separable": (2, 1), "list": (0, 0)}[form], (what, s)


def density_frame(g):
    return np.random.default_rng(g.W * 17 + g.rows).uniform(0.0, 3.5, (g.H, g.W, 3)).astype(np.float32)


def run_tail(ctx, g, mode, outputs="f32", form=None, mono=False):
    """mode "lut": lut3d_kernel alone; "burn": with a burn map; "grain": the tail kernel in the form `form`."""
    what = f"stage_tail {mode} {form} mono {mono} {outputs} {g}"
    dens = density_frame(g)
    lo, hi = g.y0 - 1, g.y1 + 1
    bmap = bsrc = None
    if mode == "grain":
        params, p, k = grain_setup(ctx, form, mono)
        ref = st.apply_grain(dens[g.y0:g.y1], p.grain_lut, k, SEED, mono, row0=g.y0, H_global=g.H)
    else:
        p = inputs("luts")
        setup_ctx(ctx, p)
        params, ref = ctx.make_params(), dens[g.y0:g.y1]
        if mode == "burn":
            cell, h_lo, w_lo = st.burn_geometry(g.H, g.W, 8.0)
            params = ctx.make_params(burn_strength=0.5, burn_cell=cell, burn_d_ref=1.2)
            blurred = np.random.default_rng(9).uniform(0.0, 1.5, (h_lo, w_lo)).astype(np.float32)
            ref = st.burn_apply(ref, blurred, cell, 0.5, row0=g.y0, H_global=g.H)
            bsrc, bmap = Arena.holding(dev(blurred), misalign=g.misalign), dev(blurred)
    ref = st.apply_lut_tetrahedral(ref, p.lut_3d, 0.25)
    with grain_options(ctx, form or "fixed"):
        src = src_planes(g, dens, lo, hi)
        (af, au), (pf, pu) = hwc_outputs(g, outputs), plain_hwc(outputs, g.H, g.W)
        ctx.stage_tail(src.view, params, src_gy0=lo, out_f32=view_or_none(af), out_u8=view_or_none(au), out_gy0=g.gy0, y0=g.y0, y1=g.y1,
                       H_global=g.H, burn_map=bsrc.view if bsrc else None)
        ctx.stage_tail(dev(planes_np(dens)), params, out_f32=pf, out_u8=pu, y0=g.y0, y1=g.y1, H_global=g.H, burn_map=bmap)
        if mode == "grain":
            assert_grain_form(ctx, form, what)
        check_hwc(g, af, au, pf, pu, ref, what)
    src.unchanged(what)
    if bsrc:
        bsrc.unchanged(what + " burn map")


def run_grain(ctx, g, in_place, form="fixed", mono=False):
    what = f"stage_grain in place {in_place} {form} mono {mono} {g}"
    dens = density_frame(g)
    params, p, k = grain_setup(ctx, form, mono)
    ref = st.apply_grain(dens[g.y0:g.y1], p.grain_lut, k, SEED, mono, row0=g.y0, H_global=g.H)
    kw = dict(y0=g.y0, y1=g.y1, H_global=g.H)
    with grain_options(ctx, form):
        plain = empty((3, g.H, g.W))
        ctx.stage_grain(dev(planes_np(dens)), plain, params, **kw)
        if not in_place:
            src, dst = src_planes(g, dens, g.y0 - 1, g.y1 + 1), dst_planes(g)
            ctx.stage_grain(src.view, dst.view, params, src_gy0=g.y0 - 1, dst_gy0=g.gy0, **kw)
            check_planes(g, dst, plain, ref, 1e-5, 1e-3, what)
            src.unchanged(what)
            return
        # in place: the buffer holds the density; afterwards rows [y0, y1) are the out-of-place call's, every other byte as before
        buf = src_planes(g, dens, g.gy0, g.gy0 + g.rows_alloc)
        ctx.stage_grain(buf.view, buf.view, params, src_gy0=g.gy0, dst_gy0=g.gy0, **kw)
        torch.cuda.synchronize()
        want = buf._snapshot.clone()
        torch.as_strided(want, buf.shape, buf.strides, buf.start)[:, g.a:g.b] = plain[:, g.y0:g.y1]
        diff = bits(buf.buf) != bits(want)
        assert not bool(diff.any()), f"{what}: first difference at {buf.where(int(torch.nonzero(diff)[0]))}"
        assert_close(from_planes(buf.view[:, g.a:g.b]), ref, 1e-5, 1e-3, what)


def run_grain_field(ctx, g, form="fixed", mono=False):
    what = f"stage_grain_field {form} mono {mono} {g}"
    params, p, k = grain_setup(ctx, form, mono)
    ref = st.grain_field(g.rows, g.W, SEED, k, mono, row0=g.y0, H_global=g.H)
    with grain_options(ctx, form):
        dst, plain = dst_planes(g), empty((3, g.H, g.W))
        ctx.stage_grain_field(dst.view, params, dst_gy0=g.gy0, y0=g.y0, y1=g.y1, H_global=g.H)
        ctx.stage_grain_field(plain, params, y0=g.y0, y1=g.y1, H_global=g.H)
        # (test_small_square_grain_stencils_...: 5e-6 of the field's largest value; the noise itself is good to 1e-5 of |n| < 6)
        check_planes(g, dst, plain, ref, None, None, what, abs_tol=5e-6 * max(np.abs(ref).max(), 1.0))


def run_tail_field(ctx, g, outputs="both", mono=False):
    what = f"stage_tail_field {outputs} mono {mono} {g}"
    dens = density_frame(g)
    params, p, k = grain_setup(ctx, "fixed", mono)
    ref = st.apply_lut_tetrahedral(st.apply_grain(dens[g.y0:g.y1], p.grain_lut, k, SEED, mono, row0=g.y0, H_global=g.H), p.lut_3d, 0.25)
    field = empty((3, g.H, g.W))
    ctx.stage_grain_field(field, params, y0=0, y1=g.H, H_global=g.H)
    lo, hi = g.y0 - 1, g.y1 + 1
    src, fsrc = src_planes(g, dens, lo, hi), Arena.holding(field[:, lo:hi].contiguous(), misalign=g.misalign, pad=g.pad)
    (af, au), (pf, pu) = hwc_outputs(g, outputs), plain_hwc(outputs, g.H, g.W)
    ctx.stage_tail_field(src.view, fsrc.view, params, src_gy0=lo, field_gy0=lo, out_f32=view_or_none(af), out_u8=view_or_none(au),
                         out_gy0=g.gy0, y0=g.y0, y1=g.y1, H_global=g.H)
    ctx.stage_tail_field(dev(planes_np(dens)), field, params, out_f32=pf, out_u8=pu, y0=g.y0, y1=g.y1, H_global=g.H)
    check_hwc(g, af, au, pf, pu, ref, what)
    src.unchanged(what)
    fsrc.unchanged(what + " field")


# ------------------------------------------------------------------------------------------------ the burn
def run_burn_sums(ctx, g):
    what = f"stage_burn_sums {g}"
    dens = density_frame(g)
    cell, h_lo, w_lo = st.burn_geometry(g.H, g.W, 8.0)
    params = ctx.make_params(burn_strength=0.5, burn_cell=cell, burn_d_ref=1.2)
    lo, hi = g.y0 - 1, g.y1 + 1
    src = src_planes(g, dens, lo, hi)
    sums = Arena.flat_of(torch.float32, h_lo * w_lo, misalign=g.misalign, device="cuda")
    pd = ctx.planes(src.view, lo)
    rc = ctx._lib.r2f_stage_burn_sums(ctx._h, C.byref(params), C.byref(pd), sums.view.data_ptr(), g.y0, g.y1, g.W, g.H, ctx._stream())
    assert rc == 0, (what, rc)
    plain = ctx.stage_burn_sums(dev(planes_np(dens)), params, y0=g.y0, y1=g.y1, H_global=g.H)
    torch.cuda.synchronize()
    sums.check(torch.ones(h_lo * w_lo, dtype=torch.bool), what=what)  # every cell: a cell no row of the shard touches gets 0
    same_bits(sums.view, plain.reshape(-1), what)
    green = dens[..., 1].copy()
    green[:g.y0], green[g.y1:] = 0.0, 0.0  # the shard's part of the sums: the area weights are linear in the samples
    np.testing.assert_allclose(sums.view.cpu().numpy().reshape(h_lo, w_lo), st.resize_area(green, h_lo, w_lo), rtol=2e-6, atol=0)
    src.unchanged(what)


def run_burn_map(ctx, g):
    from scipy import ndimage

    what = f"stage_burn_map {g}"
    cell, h_lo, w_lo = st.burn_geometry(g.H, g.W, 8.0)
    n = h_lo * w_lo
    params = ctx.make_params(burn_strength=0.5, burn_cell=cell, burn_d_ref=1.2)
    sums_np = np.random.default_rng(g.W).uniform(0.0, 3.0, (h_lo, w_lo)).astype(np.float32)
    src = Arena.holding(dev(sums_np), misalign=g.misalign)
    bmap = Arena.flat_of(torch.float32, n, misalign=g.misalign, device="cuda")
    scratch = Arena.flat_of(torch.float32, 2 * n, misalign=g.misalign, device="cuda")
    rc = ctx._lib.r2f_stage_burn_map(ctx._h, C.byref(params), src.view.data_ptr(), bmap.view.data_ptr(), scratch.view.data_ptr(), g.W, g.H,
                                     ctx._stream())
    assert rc == 0, (what, rc)
    plain = ctx.stage_burn_map(dev(sums_np), params, W=g.W, H_global=g.H)
    torch.cuda.synchronize()
    bmap.check(torch.ones(n, dtype=torch.bool), what=what + " map")
    scratch.check(torch.ones(2 * n, dtype=torch.bool), what=what + " scratch")
    same_bits(bmap.view, plain.reshape(-1), what)
    ref = ndimage.gaussian_filter(np.clip(sums_np - np.float32(1.2), 0, None), sigma=3, truncate=2)  # oracle.stages.burn_map's last two lines
    np.testing.assert_allclose(bmap.view.cpu().numpy().reshape(h_lo, w_lo), ref, rtol=1e-5, atol=1e-6)
    src.unchanged(what)


# ------------------------------------------------------------------------------------------------ chroma NR, range, noise
def run_chroma(ctx, g, which):
    size = 3
    what = f"stage_chroma_nr_{which} {g}"
    xyz = st.apply_matrix3x3(synthetic_frame(g.H, g.W, seed=80), st.REC709_TO_XYZ)
    xyz[g.y0, :1] = 0.0
    tmp, out = empty((3, g.H, g.W)), empty((3, g.H, g.W))
    ctx.stage_chroma_nr_h(dev(xyz), tmp, size, layout="hwc3")
    ctx.stage_chroma_nr_v(tmp, out, size, y0=0, y1=g.H, H_global=g.H)
    ref = st.chroma_nr_filter(xyz, size)
    # (pass 1 has no oracle of its own: its rows are held bit for bit against the plain call's, and the plain call's planes, taken
    # through pass 2, against the oracle -- test_chroma_nr_against_oracle's 5e-6 at a floor of 1e-4)
    assert_close(from_planes(out), ref, 5e-6, 1e-4, what + " plain")
    dst = dst_planes(g)
    if which == "h":
        lo, hi = g.y0 - 2, g.y1 + 1
        src = Arena.holding(dev(xyz[lo:hi]), misalign=g.misalign)
        ctx.stage_chroma_nr_h(src.view, dst.view, size, in_gy0=lo, dst_gy0=g.gy0, y0=g.y0, y1=g.y1, layout="hwc3")
        check_planes(g, dst, tmp, None, None, None, what)
    else:
        lo, hi = g.y0 - size, g.y1 + size
        src = Arena.holding(tmp[:, lo:hi].contiguous(), misalign=g.misalign, pad=g.pad)
        ctx.stage_chroma_nr_v(src.view, dst.view, size, src_gy0=lo, dst_gy0=g.gy0, y0=g.y0, y1=g.y1, H_global=g.H)
        check_planes(g, dst, out, ref[g.y0:g.y1], 5e-6, 1e-4, what)
    src.unchanged(what)


def run_exposure_range(ctx, g):
    """Reads only: the whole arena, planes and guards, must stay as it was."""
    what = f"stage_exposure_range {g}"
    setup_ctx(ctx, inputs("split"))
    frame = np.random.default_rng(g.W).uniform(0.0, 4.0, (g.H, g.W, 3)).astype(np.float32)
    src = src_planes(g, frame, g.gy0, g.gy0 + g.rows_alloc)
    ctx.stage_exposure_range(src.view, src_gy0=g.gy0, y0=g.y0, y1=g.y1, y2=g.y1, y3=g.y1 + BELOW)
    torch.cuda.synchronize()
    src.unchanged(what)


def run_noise(ctx, g, mono=False):
    what = f"stage_noise mono {mono} {g}"
    params = ctx.make_params(seed=SEED, grain_mono=mono)
    hsh = Arena(torch.int32, (3, g.rows, g.W), (g.rows * g.W, g.W, 1), guard=guard_elems(g.W), misalign=g.misalign, device="cuda",
                names=("plane", "row", "column"))
    noi = Arena.planes(g.rows, g.W, misalign=g.misalign, device="cuda")
    rc = ctx._lib.r2f_stage_noise(ctx._h, C.byref(params), hsh.view.data_ptr(), noi.view.data_ptr(), g.y0, g.y1, g.W, ctx._stream())
    assert rc == 0, (what, rc)
    ph, pn = ctx.stage_noise(params, g.y0, g.y1, g.W)
    torch.cuda.synchronize()
    hsh.check(hsh.rows_mask(0, g.rows), what=what + " hash")
    noi.check(noi.rows_mask(0, g.rows), what=what + " noise")
    same_bits(hsh.view, ph, what + " hash")
    same_bits(noi.view, pn, what + " noise")
    ys, xs = np.arange(g.y0, g.y1)[:, None], np.arange(g.W)[None, :]
    if not mono:  # (test_pcg3d_hash_bit_exact pins the colour hash)
        for c, v in enumerate(st.pcg3d(xs, ys, SEED)):
            np.testing.assert_array_equal(hsh.view[c].cpu().numpy().view(np.uint32), v)
    assert np.max(np.abs(from_planes(noi.view) - st.gaussian_noise(xs, ys, SEED, mono))) <= 1e-5  # test_gaussian_field


# ------------------------------------------------------------------------------------------------ whole-frame entries
Whole = namedtuple("Whole", "H W misalign pad")
Whole.__str__ = lambda s: f"{s.H}x{s.W}-m{s.misalign}-p{s.pad}"
RAGGED = [Whole(37, 53, 0, 0), Whole(37, 53, 1, 1), Whole(64, 128, 0, 0), Whole(64, 128, 1, 4), Whole(9, 129, 0, 1), Whole(130, 5, 1, 0)]


def render_contract_only(g, **_):
    """The misaligned input and outputs send the front and tail to their generic / scalar forms; only the fast front kernel records
    the exposure range the halation's scratch element is chosen from, so the frames agree to that element's rounding."""
    return g.W % 4 == 0 and g.misalign != 0


def run_render(ctx, g, outputs, graph):
    p = inputs("pipeline")
    params = setup_ctx(ctx, p)
    what = f"render {outputs} graph {graph} {g}"
    img = synthetic_frame(g.H, g.W, seed=50 + g.H)
    ref = st.render(img, p)
    nbytes = ctx.workspace_bytes(params, g.H, g.W)
    with options(ctx, render_graph=graph):
        src = Arena.holding(dev(img), misalign=g.misalign)
        ws = Arena.flat(nbytes, device="cuda")  # exactly r2f_workspace_bytes, 16-byte aligned as r2f_render demands
        af, au = hwc_outputs(g, outputs, rows=g.H, W=g.W)

        def call(workspace):
            return ctx._lib.r2f_render(ctx._h, C.byref(params), src.view.data_ptr(), 0, af.view.data_ptr() if af else None,
                                       au.view.data_ptr() if au else None, g.H, g.W, workspace.view.data_ptr(), nbytes, ctx._stream())

        if g.misalign:  # r2f_render: "workspace must be 16-byte aligned" -- refused, nothing written anywhere
            bad = Arena.flat(nbytes, misalign=g.misalign, device="cuda")
            assert call(bad) == EINVAL, what
            torch.cuda.synchronize()
            for a in (bad, af, au):
                if a is not None:
                    a.check(None, what=what + " refused")
        before = ctx.render_stats()
        for _ in range(3):  # kernel by kernel, the capture, a replay
            assert call(ws) == 0, (what, ctx._lib.r2f_last_error(ctx._h))
        after = ctx.render_stats()
        assert (after["replays"] > before["replays"]) == bool(graph), (what, before, after)
        pf, pu = ctx.render(dev(img), params, want_f32=outputs != "u8", want_u8=outputs != "f32")
        torch.cuda.synchronize()
        ws.check(torch.ones(nbytes, dtype=torch.bool), require_written=False, what=what + " workspace")
        check_hwc(g, af, au, pf, pu, ref, what, bitwise=not render_contract_only(g), a=0, b=g.H, y0=0, y1=g.H)
    src.unchanged(what)


def run_resize(ctx, g, entry):
    """r2f_resize_area, r2f_warp_affine, r2f_resize_lanczos4_f32: a whole frame in, (3, out_h, out_w) planes out."""
    what = f"{entry} {g}"
    if entry == "resize_area":
        H, W = 2 * g.H - 3, 2 * g.W + 5
    elif entry == "warp_affine":
        H, W = g.H, g.W
    else:
        H, W = max(g.H // 2, 1), max(g.W // 2 + 1, 1)
    img = np.random.default_rng(95).uniform(0, 4, (H, W, 3)).astype(np.float32)
    src = Arena.holding(dev(img), misalign=g.misalign)
    dst = Arena.planes(g.H, g.W, pad=g.pad, misalign=g.misalign, device="cuda")
    pd = ctx.planes(dst.view, 0)
    if entry == "resize_area":
        rc = ctx._lib.r2f_resize_area(ctx._h, src.view.data_ptr(), 0, H, W, C.byref(pd), g.H, g.W, ctx._stream())
        plain = ctx.resize_area(dev(img), g.H, g.W)
    elif entry == "warp_affine":
        from raw2film_amd import geometry

        m, _ = geometry.rotation_plan(H, W, 5.0)
        m64 = np.ascontiguousarray(np.asarray(m, dtype=np.float64).reshape(6))
        rc = ctx._lib.r2f_warp_affine(ctx._h, src.view.data_ptr(), 0, H, W, m64.ctypes.data, C.byref(pd), g.H, g.W, 0, 0, ctx._stream())
        plain = ctx.warp_affine(dev(img), m)
    else:
        rc = ctx._lib.r2f_resize_lanczos4_f32(ctx._h, src.view.data_ptr(), 0, H, W, C.byref(pd), g.H, g.W, ctx._stream())
        plain = ctx.resize_lanczos4_f32(dev(img), g.H, g.W)
    assert rc == 0, (what, rc)
    torch.cuda.synchronize()
    dst.check(dst.rows_mask(0, g.H), what=what)
    same_bits(dst.view, plain, what)
    got = from_planes(dst.view)
    if entry == "resize_area":  # test_resize_area_against_oracle
        assert_close(got, np.stack([st.resize_area(img[..., c], g.H, g.W) for c in range(3)], axis=-1), 2e-6, 1e-6, what)
    elif entry == "warp_affine":  # test_warp_affine_matches_oracle_on_every_layout
        assert np.abs(got - st.warp_affine_linear(img, m)).max() <= 2e-5 * 4, what
    else:  # test_gpu_processor.py: bit for bit
        np.testing.assert_array_equal(got, post.resize_lanczos4_f32(img, g.H, g.W))
    src.unchanged(what)


def run_resize_u8(ctx, g, entry):
    what = f"{entry} {g}"
    H, W = (2 * g.H - 3, 2 * g.W + 5) if entry == "resize_area_u8" else (max(g.H // 2, 1), max(g.W // 2 + 1, 1))
    img = np.random.default_rng(g.H).integers(0, 256, (H, W, 3), dtype=np.uint8)
    src = Arena.holding(dev(img), misalign=g.misalign)
    dst = Arena.hwc(g.H, g.W, torch.uint8, misalign=g.misalign, device="cuda")
    fn = ctx._lib.r2f_resize_area_u8 if entry == "resize_area_u8" else ctx._lib.r2f_resize_lanczos4_u8
    rc = fn(ctx._h, src.view.data_ptr(), H, W, dst.view.data_ptr(), g.H, g.W, ctx._stream())
    assert rc == 0, (what, rc)
    plain = (ctx.resize_area_u8 if entry == "resize_area_u8" else ctx.resize_lanczos4_u8)(dev(img), g.H, g.W)
    torch.cuda.synchronize()
    dst.check(dst.rows_mask(0, g.H), expected=plain.cpu(), what=what)
    same_bits(dst.view, plain, what)
    ref = post.resize_area_u8(img, g.H, g.W) if entry == "resize_area_u8" else st.resize_lanczos4_u8(img, g.H, g.W)
    np.testing.assert_array_equal(dst.view.cpu().numpy(), ref)  # both pinned bit for bit in tests/test_gpu_processor.py
    src.unchanged(what)


def run_decode(ctx, g, channels):
    from raw2film_amd import decode

    what = f"decode_u16 {channels} channels {g}"
    u16 = np.random.default_rng(g.W).integers(0, 65536, (g.H, g.W, channels), dtype=np.uint16)
    src = Arena.holding(dev(u16.view(np.int16)), misalign=g.misalign)  # (int16 tensors are read as the same bits)
    dst = Arena.hwc(g.H, g.W, torch.float32, misalign=g.misalign, device="cuda")
    factor = decode.exposure_factor(0.75)
    rc = ctx._lib.r2f_decode_u16(ctx._h, src.view.data_ptr(), g.H, g.W, channels, float(np.float32(65535.0)), float(np.float32(factor)),
                                 dst.view.data_ptr(), ctx._stream())
    assert rc == 0, (what, rc)
    plain = ctx.decode_u16(dev(u16.view(np.int16)), factor)
    torch.cuda.synchronize()
    dst.check(dst.rows_mask(0, g.H), what=what)
    same_bits(dst.view, plain, what)
    np.testing.assert_array_equal(dst.view.cpu().numpy(), post.decode_u16(u16, 0.75))  # tests/test_gpu_decode.py: bit for bit
    src.unchanged(what)


def run_blit(ctx, g, offset):
    """offset: bytes past a 16-byte boundary.  r2f_blit_rgba8 wants its destination 4-byte aligned."""
    from raw2film_amd import _lib, geometry

    what = f"blit_rgba8 offset {offset} {g}"
    H, W, dh, dw = g.H, g.W, g.H + 11, g.W + 7
    img = np.random.default_rng(3).uniform(-0.1, 1.1, (H, W, 3)).astype(np.float32)
    t = geometry.blit_transform((W, H), (dw, dh), pipeline_resolution=(W, H), output_resolution=(W, H), canvas_resolution=(W + 3, H + 5),
                                canvas_color=(128, 128, 128))
    src = Arena.holding(dev(img), misalign=g.misalign)
    dst = Arena.hwc(dh, dw, torch.uint8, misalign=offset, channels=4, device="cuda")
    bt = _lib.Blit(t["scale_x"], t["scale_y"], t["offset_x"], t["offset_y"], t["canvas_min_x"], t["canvas_min_y"], t["canvas_max_x"],
                   t["canvas_max_y"], (C.c_float * 3)(*t["canvas_color"]))
    rc = ctx._lib.r2f_blit_rgba8(ctx._h, src.view.data_ptr(), H, W, dst.view.data_ptr(), dh, dw, C.byref(bt), ctx._stream())
    torch.cuda.synchronize()
    if offset % 4:
        assert rc == EINVAL, (what, rc)
        dst.check(None, what=what + " refused")
        return
    assert rc == 0, (what, rc)
    plain = ctx.blit_rgba8(dev(img), torch.zeros((dh, dw, 4), dtype=torch.uint8, device="cuda"), t)
    dst.check(dst.rows_mask(0, dh), expected=plain.cpu(), what=what)  # transparent pixels are written too (0, 0, 0, 0)
    same_bits(dst.view, plain, what)
    got, ref = dst.view.cpu().numpy(), post.blit_rgba8(img, dh, dw, t)
    np.testing.assert_array_equal(got[..., 3], ref[..., 3])
    d = np.abs(got.astype(int) - ref.astype(int))
    assert d.max() <= 1 and (d > 0).mean() <= 1e-3  # test_preview_blit_into_a_destination_texture
    src.unchanged(what)


def run_histogram(ctx, g, offset):
    """offset: bytes past a 16-byte boundary for the image (r2f_histogram_u8 wants it 16-byte aligned) and the RGBA images
    (r2f_histogram_render wants those 4-byte aligned); the counts sit `misalign` words past one."""
    from raw2film_amd import histogram

    what = f"histogram offset {offset} {g}"
    img = np.clip(np.random.default_rng(8).normal(120, 40, (g.H, g.W, 3)), 0, 255).astype(np.uint8)
    src = Arena.holding(dev(img), misalign=offset)
    counts = Arena.flat_of(torch.int32, 3 * 256, misalign=g.misalign, device="cuda")
    rc = ctx._lib.r2f_histogram_u8(ctx._h, src.view.data_ptr(), g.H, g.W, counts.view.data_ptr(), ctx._stream())
    torch.cuda.synchronize()
    if offset % 16:
        assert rc == EINVAL, (what, rc)
        counts.check(None, what=what + " counts, refused")
    else:
        assert rc == 0, (what, rc)
        counts.check(torch.ones(768, dtype=torch.bool), what=what + " counts")
        np.testing.assert_array_equal(counts.view.cpu().numpy().reshape(3, 256), oh.counts(img))  # tests/test_gpu_histogram.py
    src.unchanged(what)
    # the bar image and the widget texture from counts in an arena of their own
    height, th, tw = 100, 37, 131
    ref_counts = oh.counts(img).astype(np.int32)
    csrc = Arena.holding(dev(ref_counts.reshape(-1)), misalign=g.misalign)
    image = Arena.hwc(height, 256, torch.uint8, misalign=offset, channels=4, device="cuda")
    target = Arena.hwc(th, tw, torch.uint8, misalign=offset, channels=4, device="cuda")
    mix = np.ascontiguousarray(np.asarray(histogram.MIX_TABLE, dtype=np.uint8).reshape(8, 4))
    rc = ctx._lib.r2f_histogram_render(ctx._h, csrc.view.data_ptr(), mix.ctypes.data, height, image.view.data_ptr(), target.view.data_ptr(),
                                       th, tw, ctx._stream())
    torch.cuda.synchronize()
    if offset % 4:
        assert rc == EINVAL, (what, rc)
        image.check(None, what=what + " image, refused")
        target.check(None, what=what + " target, refused")
        return
    assert rc == 0, (what, rc)
    ptarget = torch.zeros((th, tw, 4), dtype=torch.uint8, device="cuda")
    pimage = ctx.histogram_render(dev(ref_counts), histogram.MIX_TABLE, height, target=ptarget)
    torch.cuda.synchronize()
    image.check(image.rows_mask(0, height), expected=pimage.cpu(), what=what + " image")
    target.check(target.rows_mask(0, th), expected=ptarget.cpu(), what=what + " target")
    same_bits(image.view, pimage, what + " image")
    same_bits(target.view, ptarget, what + " target")
    ref_img, ref_tgt, _ = post.histogram_render(ref_counts, histogram.MIX_TABLE, height, (th, tw))
    got = image.view.cpu().numpy()  # test_histogram_texture_from_device_counts: a bar may be one pixel taller or shorter
    assert (got != ref_img).any(axis=2).sum(axis=0).max() <= 1 and (got != ref_img).any(axis=2).any(axis=0).mean() <= 0.05
    assert (target.view.cpu().numpy() != ref_tgt).any(axis=2).mean() <= 0.01
    csrc.unchanged(what + " counts")


def jpeg_frame(H, W):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    smooth = np.stack([127.5 + 127.5 * np.sin(xx / 9.0) * np.cos(yy / 7.0), 255.0 * xx / max(W - 1, 1), 128 + 127 * np.cos((xx + yy) / 5.0)], -1)
    noise = np.random.default_rng(H * W).integers(-40, 40, (H, W, 3))
    return np.clip(smooth + noise, 0, 255).astype(np.uint8)


def run_jpeg(ctx, g, sampling, optimize=False, progressive=False, rows=False, quality=85):
    """out_cap is the documented bound: nothing past it, nothing round *out_len; the file equals the unpadded call's byte for byte
    (which tests/test_gpu_jpeg*.py hold against Pillow's).  Bytes between the file's end and out_cap are not promised."""
    from raw2film_amd import _lib

    what = f"jpeg sampling {sampling} optimize {optimize} progressive {progressive} rows {rows} {g}"
    img = jpeg_frame(g.H, g.W)
    src = Arena.holding(dev(img), misalign=g.misalign)
    cap = ctx.jpeg_bound_bytes_opts(g.H, g.W, quality, sampling, optimize, True) if progressive else ctx.jpeg_bound_bytes(g.H, g.W, sampling)
    out = Arena.flat(cap, misalign=g.misalign, device="cuda")
    length = Arena.flat_of(torch.int64, 1, device="cuda")
    assert length.view.data_ptr() % 8 == 0
    opts = _lib.JpegOpts(quality, sampling, int(optimize), int(progressive))
    args = (out.view.data_ptr(), cap, length.view.data_ptr(), ctx._stream())
    if rows:
        mcu = 16 if sampling == 2 else 8
        rc = (ctx._lib.r2f_jpeg_rows_begin(ctx._h, g.H, g.W, quality, *args) if sampling == 2 else
              ctx._lib.r2f_jpeg_rows_begin_ex(ctx._h, g.H, g.W, C.byref(opts), *args))
        y = 0
        while rc == 0 and y < g.H:
            y1 = min(y + (2 * mcu if y else mcu), g.H)
            rc = ctx._lib.r2f_jpeg_rows(ctx._h, src.view.data_ptr(), 3 * g.W, y, y1, ctx._stream())
            y = y1
    elif sampling == 2 and not optimize and not progressive:
        rc = ctx._lib.r2f_jpeg_encode(ctx._h, src.view.data_ptr(), g.H, g.W, 3 * g.W, quality, *args)
    else:
        rc = ctx._lib.r2f_jpeg_encode_ex(ctx._h, src.view.data_ptr(), g.H, g.W, 3 * g.W, C.byref(opts), *args)
    assert rc == 0, (what, rc, ctx._lib.r2f_last_error(ctx._h))
    torch.cuda.synchronize()
    out.check(torch.ones(cap, dtype=torch.bool), require_written=False, what=what + " file")
    length.check(torch.ones(1, dtype=torch.bool), what=what + " length word")
    n = int(length.view.cpu()[0])
    pout, plen = ctx.jpeg_encode(dev(img), quality, sampling, optimize, progressive)
    pn = int(plen.cpu()[0])
    assert 0 < n <= cap and n == pn, (what, n, pn)
    assert torch.equal(out.view[:n], pout[:n]), what
    src.unchanged(what)


# ------------------------------------------------------------------------------------------------ the table
Case = namedtuple("Case", "entry variant run kwargs geo contract_only")


def table():
    """(entry point, variant, runner, arguments, geometries, contract_only): contract_only(geo, **arguments) names the cases in which
    the bitwise comparison with the plain call is replaced by the contract (None: never)."""
    rows = []

    def add(entry, variant, run, kwargs, geos, contract_only=None):
        rows.append((entry, variant, run, kwargs, geos, contract_only))

    first = True
    for upto in (0, 1, 2):  # r2f_stage_front: the three upto values x the three layouts x front_fast
        for layout in ("hwc3", "hwc4", "chw"):
            for fast in (1, 0):
                add("r2f_stage_front", f"upto{upto}-{layout}-fast{fast}", run_front, dict(upto=upto, layout=layout, fast=fast),
                    FULL if first or (upto == 2 and layout == "hwc3" and fast == 1) else SHORT, front_contract_only)
                first = False
    for outputs in ("u8", "both"):
        add("r2f_stage_front", f"upto2-hwc3-fast1-{outputs}", run_front, dict(upto=2, layout="hwc3", fast=1, outputs=outputs), SHORT,
            front_contract_only)
    add("r2f_stage_front_split", "split", run_front_split, {}, FULL, split_contract_only)
    for stage in ("halation", "mtf"):
        add(f"r2f_stage_{stage}", "direct-unrolled", run_stencil, dict(stage=stage, form="direct"), FULL)
        for v in (0, 1, 2):
            add(f"r2f_stage_{stage}", f"direct-list-variant{v}", run_stencil, dict(stage=stage, form="direct", variant=v, fixed=0), SHORT)
        add(f"r2f_stage_{stage}", "fft-256", run_stencil, dict(stage=stage, form="fft", window_rows=256), FULL)
        add(f"r2f_stage_{stage}", "fft-512", run_stencil, dict(stage=stage, form="fft", window_rows=512), SHORT)
        add(f"r2f_stage_{stage}", "fft-256-epilogue-global", run_stencil, dict(stage=stage, form="fft", window_rows=256, epi_lds=0), SHORT)
    add("r2f_stage_stencil", "direct-unrolled", run_stencil, dict(stage="stencil", form="direct"), FULL)
    add("r2f_stage_stencil", "fft", run_stencil, dict(stage="stencil", form="fft"), SHORT)
    add("r2f_stage_tail", "lut-f32", run_tail, dict(mode="lut", outputs="f32"), FULL)
    add("r2f_stage_tail", "lut-u8", run_tail, dict(mode="lut", outputs="u8"), SHORT)
    add("r2f_stage_tail", "lut-both", run_tail, dict(mode="lut", outputs="both"), SHORT)
    add("r2f_stage_tail", "burn", run_tail, dict(mode="burn", outputs="both"), SHORT)
    first = True
    for form in ("fixed", "separable", "list"):
        for mono in (False, True):
            add("r2f_stage_tail", f"grain-{form}-{'mono' if mono else 'colour'}", run_tail,
                dict(mode="grain", outputs="both", form=form, mono=mono), FULL if first else SHORT)
            first = False
    add("r2f_stage_tail", "grain-fixed-colour-f32", run_tail, dict(mode="grain", outputs="f32", form="fixed"), SHORT)
    add("r2f_stage_tail", "grain-fixed-colour-u8", run_tail, dict(mode="grain", outputs="u8", form="fixed"), SHORT)
    add("r2f_stage_grain", "out-of-place", run_grain, dict(in_place=False), FULL)
    add("r2f_stage_grain", "in-place", run_grain, dict(in_place=True), FULL)
    add("r2f_stage_grain", "in-place-separable-mono", run_grain, dict(in_place=True, form="separable", mono=True), SHORT)
    add("r2f_stage_grain_field", "fixed", run_grain_field, {}, FULL)
    add("r2f_stage_grain_field", "separable", run_grain_field, dict(form="separable"), SHORT)
    add("r2f_stage_grain_field", "list-mono", run_grain_field, dict(form="list", mono=True), SHORT)
    add("r2f_stage_tail_field", "both", run_tail_field, {}, FULL)
    add("r2f_stage_tail_field", "f32-mono", run_tail_field, dict(outputs="f32", mono=True), SHORT)
    add("r2f_stage_tail_field", "u8", run_tail_field, dict(outputs="u8"), SHORT)
    add("r2f_stage_burn_sums", "sums", run_burn_sums, {}, FULL)
    add("r2f_stage_burn_map", "map", run_burn_map, {}, FULL)
    add("r2f_stage_chroma_nr_h", "h", run_chroma, dict(which="h"), FULL)
    add("r2f_stage_chroma_nr_v", "v", run_chroma, dict(which="v"), FULL)
    add("r2f_stage_exposure_range", "range", run_exposure_range, {}, FULL)
    add("r2f_stage_noise", "colour", run_noise, {}, FULL)
    add("r2f_stage_noise", "mono", run_noise, dict(mono=True), SHORT)
    for outputs in ("f32", "u8", "both"):
        for graph in (1, 0):
            add("r2f_render", f"{outputs}-graph{graph}", run_render, dict(outputs=outputs, graph=graph),
                RAGGED if outputs == "both" else RAGGED[:4], render_contract_only)
    for entry in ("resize_area", "warp_affine", "resize_lanczos4_f32"):
        add(f"r2f_{entry}", entry, run_resize, dict(entry=entry), RAGGED)
    for entry in ("resize_lanczos4_u8", "resize_area_u8"):
        add(f"r2f_{entry}", entry, run_resize_u8, dict(entry=entry), RAGGED)
    for ch in (3, 4):
        add("r2f_decode_u16", f"{ch}ch", run_decode, dict(channels=ch), RAGGED)
    for offset in (0, 4, 1):
        add("r2f_blit_rgba8", f"offset{offset}", run_blit, dict(offset=offset), RAGGED[:3])
    for offset in (0, 4, 1):
        add("r2f_histogram_u8 + r2f_histogram_render", f"offset{offset}", run_histogram, dict(offset=offset), RAGGED[:3])
    for sampling in (0, 1, 2):
        add("r2f_jpeg_encode" if sampling == 2 else "r2f_jpeg_encode_ex", f"s{sampling}", run_jpeg, dict(sampling=sampling), RAGGED[:4])
        add("r2f_jpeg_encode_ex", f"s{sampling}-optimize", run_jpeg, dict(sampling=sampling, optimize=True), RAGGED[:4])
        add("r2f_jpeg_encode_ex", f"s{sampling}-progressive", run_jpeg, dict(sampling=sampling, progressive=True), RAGGED[:4])
        add("r2f_jpeg_rows_begin + r2f_jpeg_rows" if sampling == 2 else "r2f_jpeg_rows_begin_ex + r2f_jpeg_rows", f"s{sampling}-rows", run_jpeg,
            dict(sampling=sampling, rows=True), RAGGED[:4])
    return [Case(e, v, r, kw, g, co) for e, v, r, kw, geos, co in rows for g in geos]


CASES = table()


def refuses(case):
    """Cases in which the entry refuses the layout with R2F_EINVAL (alignment stated in include/r2f.h) and must leave the arena alone."""
    if case.run is run_blit or case.run is run_histogram:
        return case.kwargs["offset"] % (16 if case.run is run_histogram else 4) != 0
    return case.run is run_render and case.geo.misalign != 0  # (the misaligned WORKSPACE; the frame itself is then rendered)


def test_the_table_covers_what_it_says(capsys):
    per_entry = Counter(c.entry for c in CASES)
    contract = [f"{c.entry}[{c.variant}-{c.geo}]" for c in CASES if c.contract_only and c.contract_only(c.geo, **c.kwargs)]
    refused = [f"{c.entry}[{c.variant}-{c.geo}]" for c in CASES if refuses(c)]
    with capsys.disabled():
        print(f"\nwrite-bounds battery: {len(CASES)} cases")
        for e, n in sorted(per_entry.items()):
            print(f"  {e}: {n}")
        print(f"  bitwise comparison replaced by the contract in {len(contract)} cases: {' '.join(contract)}")
        print(f"  layout refused (R2F_EINVAL, arena untouched) in {len(refused)} cases: {' '.join(refused)}")
    for entry in per_entry:  # every row-aware entry: every width, every row count at an odd and an even width, both vector outcomes
        geos = {c.geo for c in CASES if c.entry == entry and isinstance(c.geo, Geo)}
        if geos:
            assert {g.W for g in geos} >= set(WIDTHS), entry
            assert {g.rows for g in geos if g.W == 65} >= set(ROW_COUNTS) and {g.rows for g in geos if g.W == 128} >= set(ROW_COUNTS), entry
            assert {g.planes_vec for g in geos} == {True, False}, entry


@pytest.mark.parametrize("case", CASES, ids=[f"{c.entry.split(' ')[0]}-{c.variant}-{c.geo}" for c in CASES])
def test_write_bounds(ctx, case):
    case.run(ctx, case.geo, **case.kwargs)
