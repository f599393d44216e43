"""Every stencil form on the device against exact integer sums (tests/exact_taps.py) on sparse, ragged and shifted taps.

Integer samples 0 .. 15 and taps that are integers / 4096 make every product and partial sum exact in float32: the direct forms
(entry list, mirrored entry list, unrolled) must return the int64 correlation bit for bit whatever their tap order, and the float64
FFT form must return it to float64 noise (bound 2^-10 of a unit, derived: a tap error costs a whole unit; the oracle's own fp64 FFT
route is off by 2e-12).  All calls go through stage_stencil (no epilogue), and every test asserts from stencil_stats that the form
it is about actually ran.  Why this exists next to the oracle tests: tests/test_exact_taps_host.py, the teeth test.

Measured on an MI355X: every direct form bit-equal; the complex128 FFT form at most 5.7e-12 of a unit off over 900 launches (bound
2^-10 = 9.8e-4); complex64 and 12-byte scratch at most 1 float32 ulp from the complex128 result (bound 3).  What these tests found
when they were written: (1) stencil_source_rows named rows nobody reads for a tap box that does not hold the anchor row, so the
entry points refused a caller's exact source window ("rows [0, 22) not inside the buffer's [17, 22)": a tap 21 rows above the
anchor, outputs [0, 5) of 150 rows); (2) the one-shot column pass and the column walk of the FFT form, stated bit-identical,
differed in 78 of 375 300 outputs (by up to 5.7e-13 of a unit, all where the exact result is 0) on centrally symmetric 45 x 61
taps of both signs, 256 x 256 windows, first at (y 1, x 205, channel 2): 5.68e-13 against 7.96e-13 of a unit, exact 0.  The compiler
had fused the complex products differently in the two kernels; r2f_fft_math.h now states the fusion itself."""

import numpy as np
import pytest

import exact_taps as et
from helpers import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TILES = {0: (128, 64), 1: (64, 32), 2: (128, 32)}  # tile width x height of the direct kernel's three variants
FFT_BOUND = 2.0 ** -10  # of a unit of 2^-12
WINDOWS = [(256, 256), (256, 512), (512, 256), (512, 512), (256, 1024), (512, 1024)]  # = tests/test_gpu_fft.py's: rows x columns


@pytest.fixture()
def ctx():
    from raw2film_amd.context import HipContext

    c = HipContext(0)
    yield c
    c.close()


def planes(a):
    return torch.from_numpy(np.ascontiguousarray(np.transpose(a, (2, 0, 1)))).cuda()


def units(t):
    """A (3, rows, W) device result in units of 2^-12, float64, (rows, W, 3)."""
    return np.transpose(t.cpu().numpy(), (1, 2, 0)).astype(np.float64) * et.SCALE


def options(ctx, **opts):
    for name, v in opts.items():
        ctx.set_option(name, v)


DIRECT = dict(stencil_fft=0, stencil_fft_mixed_sign=0)
FFT = dict(stencil_fft=1, stencil_fft_scratch32=0, stencil_fft_min_taps=1, stencil_fixed=0)

_frames, _refs = {}, {}


def frame_of(shape):
    if shape not in _frames:
        _frames[shape] = et.frame(np.random.default_rng(shape[0] * 7919 + shape[1]), *shape)
    return _frames[shape]


def reference_of(name, k, shape):
    """Computed once per stencil and frame, shared, never written to."""
    key = (name, shape, hash(k.tobytes()))
    if key not in _refs:
        ref = et.reference(frame_of(shape), k)
        ref.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


def whole(ctx, which, img, k):
    H, W = img.shape[:2]
    ctx.set_kernel(which, k)
    dst = torch.zeros((3, H, W), dtype=torch.float32, device="cuda")
    ctx.stage_stencil(which, planes(img), dst, y0=0, y1=H, H_global=H)
    return units(dst)


def banded(ctx, which, img, k, bands, reach):
    """Rows [y0, y1) of every band from an allocation that holds exactly the rows source_rows names; a row short is refused."""
    H, W = img.shape[:2]
    above, below = reach
    ctx.set_kernel(which, k)
    out = torch.zeros((3, H, W), dtype=torch.float32, device="cuda")
    for y0, y1 in bands:
        lo, hi = et.source_rows(y0, y1, above, below, H)
        ctx.stage_stencil(which, planes(img[lo:hi]), out, src_gy0=lo, y0=y0, y1=y1, H_global=H)
        for lo2, hi2 in ((lo + 1, hi), (lo, hi - 1)):
            if hi2 > lo2:
                with pytest.raises(Exception, match="not inside"):
                    ctx.stage_stencil(which, planes(img[lo2:hi2]), out, src_gy0=lo2, y0=y0, y1=y1, H_global=H)
    return units(out)


def first_difference(got, ref):
    bad = np.argwhere(got != ref)
    y, x, c = bad[0]
    return f"{len(bad)} of {ref.size} outputs differ; first at (y {y}, x {x}, channel {c}): got {got[y, x, c]!r}, want {ref[y, x, c]}"


def assert_exact(got, ref, what):
    assert np.array_equal(got, ref), f"{what}: {first_difference(got, ref)}"


def assert_fft_exact(got, ref, what):
    """The complex128 FFT form: the integer after rounding, and within 2^-10 of it before."""
    assert np.array_equal(np.rint(got), ref), f"{what}: {first_difference(np.rint(got), ref)}"
    worst = float(np.abs(got - ref).max())
    print(f"fft form, {what}: max |got - reference| = {worst:.3e} units of 2^-12")
    assert worst <= FFT_BOUND, f"{what}: {worst:.3e} units off, the tap pattern is right"
    return worst


def stats(ctx, which, key):
    return [c[key] for c in ctx.stencil_stats(which)]


def stencil_of(family, size, signed):
    rng = np.random.default_rng(1000 * size[0] + size[1] + (500 if signed else 0))
    if family == "shift_a":
        return et.shift(rng, *size, places=("above", "left", "first"), cluster=not signed, signed=signed)
    if family == "shift_b":
        return et.shift(rng, *size, places=("below", "right", "last"), cluster=signed, signed=signed)
    return getattr(et, family)(rng, *size, signed=signed)


PLAIN = ["ragged", "gaps", "corners", "shift_a", "shift_b"]


# ------------------------------------------------------------------------------------------------ direct forms
@pytest.mark.parametrize("signed", [False, True], ids=["nonneg", "signed"])
@pytest.mark.parametrize("size", [(9, 9), (6, 9), (43, 43), (87, 87)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("family", PLAIN)
def test_entry_list_returns_the_integer_sums(ctx, family, size, signed):
    k, name = stencil_of(family, size, signed)
    options(ctx, **DIRECT)
    phases, ran = set(), 0
    for variant in (0, 1, 2):
        ctx.set_option("stencil_variant", variant)
        tw, th = TILES[variant]
        for shape in ((96, 160), (70, 133), (20, 24), (1, 40), (33, 1), (3 * th + 5, 3 * tw + 7)):
            img, ref = frame_of(shape), reference_of(name, k, shape)
            for kb in (160, 80, 48):
                ctx.set_option("stencil_lds_kb", kb)
                try:
                    got = whole(ctx, 1, img, k)
                except Exception as e:  # a variant whose tile rows cannot hold the stencil refuses it; the others run
                    assert "fit" in str(e), e
                    continue
                assert stats(ctx, 1, "fft") == [0] * 3 and stats(ctx, 1, "unrolled") == [0] * 3 and stats(ctx, 1, "sym") == [0] * 3
                assert stats(ctx, 1, "q") == [4] * 3
                assert [b for b in stats(ctx, 1, "kh")] == [et.tap_box(k, c)[1] - et.tap_box(k, c)[0] + 1 for c in range(3)]
                phases |= set(stats(ctx, 1, "phases"))
                ran += 1
                assert_exact(got, ref, f"{name}, variant {variant}, frame {shape}, {kb} KiB")
    assert ran >= 18 * 2, ran  # at least two variants took it
    if size[0] >= 43 and not family.startswith("shift"):
        assert 1 in phases and len(phases) > 1, phases  # the same stencil in one and in several LDS phases


@pytest.mark.parametrize("signed", [False, True], ids=["nonneg", "signed"])
@pytest.mark.parametrize("r", [4, 5, 6, 7, 43])
def test_mirrored_entry_list_returns_the_integer_sums_and_the_plain_lists_bits(ctx, r, signed):
    k, name = et.sym_sparse(np.random.default_rng(r + 100 * signed), r, signed=signed)
    options(ctx, **DIRECT, stencil_fixed=0)
    for shape in ((96, 160), (70, 133), (20, 24), (197, 391)):
        img, ref = frame_of(shape), reference_of(name, k, shape)
        for kb in (160, 48):
            options(ctx, stencil_lds_kb=kb, stencil_sym=1)
            paired = whole(ctx, 1, img, k)
            assert stats(ctx, 1, "sym") == [1] * 3 and stats(ctx, 1, "fft") == [0] * 3 and stats(ctx, 1, "unrolled") == [0] * 3
            assert all((w - 1) // 2 % 4 == 2 for w in stats(ctx, 1, "kw"))  # every box padded to r = 2 (mod 4)
            ctx.set_option("stencil_sym", 0)
            plain = whole(ctx, 1, img, k)
            assert stats(ctx, 1, "sym") == [0] * 3 and stats(ctx, 1, "fft") == [0] * 3 and stats(ctx, 1, "unrolled") == [0] * 3
            assert_exact(paired, ref, f"{name} mirrored, frame {shape}, {kb} KiB")
            assert_exact(plain, ref, f"{name} plain, frame {shape}, {kb} KiB")
            assert np.array_equal(paired, plain)


@pytest.mark.parametrize("signed", [False, True], ids=["nonneg", "signed"])
@pytest.mark.parametrize("kc", [3, 1], ids=["per-channel", "shared"])
@pytest.mark.parametrize("R", range(1, 12))
def test_unrolled_form_returns_the_integer_sums(ctx, R, kc, signed):
    k, name = et.square_sym(np.random.default_rng(R + 50 * kc + 500 * signed), R, kc=kc, signed=signed)
    options(ctx, **DIRECT, stencil_fixed=1)  # (the FFT form off: 21 x 21 and 23 x 23 run unrolled too)
    shape = (150, 203)
    img, ref = frame_of(shape), reference_of(name, k, shape)
    got = whole(ctx, 1, img, k)
    assert stats(ctx, 1, "unrolled") == [R] * 3 and stats(ctx, 1, "fft") == [0] * 3
    assert_exact(got, ref, f"{name} unrolled, whole frame")
    got = banded(ctx, 1, img, k, ((0, 41), (41, 42), (42, shape[0])), (R, R))
    assert stats(ctx, 1, "unrolled") == [R] * 3
    assert_exact(got, ref, f"{name} unrolled, row ranges")
    ctx.set_option("stencil_fixed", 0)
    assert_exact(whole(ctx, 1, img, k), ref, f"{name}, entry list")
    assert stats(ctx, 1, "unrolled") == [0] * 3 and stats(ctx, 1, "sym") == [1 if R >= 4 else 0] * 3


def band_stencils(signed):
    """Shared taps (one reach for the three channels: the source window is then exact for all of them)."""
    rng = np.random.default_rng(77 + signed)
    out = [et.shift(rng, 43, 43, places=(p,), cluster=c, signed=signed) for p, c in
           (("first", False), ("last", False), ("above", True), ("below", True), ("left", True))]
    out.append(et.shift(rng, 87, 87, places=("first",), signed=signed))  # 43 rows up: further than most bands are tall
    out.append(et.shift(rng, 87, 87, places=("last",), signed=signed))
    out.append(et.ragged(rng, 25, 31, 1, signed=signed, box=(2, 20, 3, 29)))  # above 10, below 8
    out.append(et.ragged(rng, 43, 31, 1, signed=signed, box=(23, 40, 0, 30)))  # wholly below the anchor row: above -2, below 19
    return out


BANDS_H = 150
BANDS = ((0, 5), (5, 37), (37, 38), (38, 101), (101, BANDS_H - 5), (BANDS_H - 5, BANDS_H))  # no multiple of a tile height; first row, one row, last rows


def test_the_band_cases_hold_what_they_are_for():
    """(no device work) Some band touches the top edge and reads, reflected, rows below its own last one; one mirrored."""
    top = bottom = negative = 0
    for k, name in band_stencils(False):
        above, below = et.reach(k)
        negative += above < 0 or below < 0
        assert above != below
        for y0, y1 in BANDS:
            lo, hi = et.source_rows(y0, y1, above, below, BANDS_H)
            top += y0 == 0 and y0 - above < 0 and hi > y1
            bottom += y1 == BANDS_H and y1 - 1 + below > BANDS_H - 1 and lo < y0
    assert top >= 1 and bottom >= 1 and negative >= 6


@pytest.mark.parametrize("signed", [False, True], ids=["nonneg", "signed"])
def test_direct_row_ranges_from_exact_source_windows(ctx, signed):
    options(ctx, **DIRECT)
    shape = (BANDS_H, 133)
    for k, name in band_stencils(signed):
        img, ref = frame_of(shape), reference_of(name, k, shape)
        for variant in (0, 1):
            ctx.set_option("stencil_variant", variant)
            got = banded(ctx, 1, img, k, BANDS, et.reach(k))
            assert stats(ctx, 1, "fft") == [0] * 3 and stats(ctx, 1, "unrolled") == [0] * 3
            assert_exact(got, ref, f"{name}, variant {variant}, bands from exact windows")


# ------------------------------------------------------------------------------------------------ FFT form
def force_window(ctx, window):
    options(ctx, stencil_fft_window_rows=window[0], stencil_fft_window=window[1])


@pytest.mark.parametrize("signed", [False, True], ids=["nonneg", "signed"])
@pytest.mark.parametrize("shape", [(300, 417), (64, 64), (1, 7), (9, 1), (173, 344), (200, 1100)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("size", [(45, 61), (87, 87)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("family", PLAIN)
def test_fft_form_returns_the_integer_sums_in_every_window(ctx, family, size, shape, signed):
    k, name = stencil_of(family, size, signed)
    options(ctx, **FFT)
    img, ref = frame_of(shape), reference_of(name, k, shape)
    for window in WINDOWS:
        force_window(ctx, window)
        got = whole(ctx, 0, img, k)
        assert stats(ctx, 0, "fft") == [1] * 3 and stats(ctx, 0, "window") == [window] * 3
        assert_fft_exact(got, ref, f"{name}, frame {shape}, window {window}")


@pytest.mark.parametrize("family, size, window", [("corners", (301, 25), (512, 256)), ("corners", (25, 301), (256, 512)),
                                                  ("corners", (399, 399), (512, 512)), ("shift_a", (301, 25), (256, 256)),
                                                  ("shift_b", (301, 25), (256, 256)), ("shift_a", (25, 301), (256, 256)),
                                                  ("shift_b", (25, 301), (256, 256))])
def test_fft_form_on_boxes_over_200_taps_and_on_translations_that_far(ctx, family, size, window):
    """A box over 200 taps on an axis takes the 512-point window there whatever is forced; a small box 150 rows or columns away
    from the anchor stays in the forced 256 x 256 one."""
    options(ctx, **FFT)
    force_window(ctx, (256, 256))
    shape = (230, 240)
    for signed in (False, True):
        k, name = stencil_of(family, size, signed)
        got = whole(ctx, 1, frame_of(shape), k)
        assert stats(ctx, 1, "fft") == [1] * 3
        assert stats(ctx, 1, "window")[0] == window, stats(ctx, 1, "window")
        assert_fft_exact(got, reference_of(name, k, shape), f"{name}, frame {shape}")


@pytest.mark.parametrize("signed", [False, True], ids=["nonneg", "signed"])
def test_real_spectrum_on_centrally_symmetric_sparse_taps(ctx, signed):
    k, name = et.central_sparse(np.random.default_rng(31 + signed), 45, 61, signed=signed)
    moved = k.copy()  # one tap off its mirror position: the complex spectrum
    i, j = np.argwhere(k[:22, :, 1] != 0)[3]
    j2 = j + 1 if j + 1 < k.shape[1] and k[i, j + 1, 1] == 0 else j - 1
    moved[i, j2, 1], moved[i, j, 1] = moved[i, j2, 1] + moved[i, j, 1], 0
    assert not np.array_equal(moved, moved[::-1, ::-1])
    options(ctx, **FFT)
    shape = (300, 417)
    img = frame_of(shape)
    for window in ((256, 256), (256, 512), (512, 512)):
        force_window(ctx, window)
        walks = []
        for walk in (0, 1):
            ctx.set_option("stencil_fft_cols_walk", walk)
            got = whole(ctx, 0, img, k)
            assert stats(ctx, 0, "fft") == [1] * 3 and stats(ctx, 0, "real_spectrum") == [1] * 3 and stats(ctx, 0, "window") == [window] * 3
            assert_fft_exact(got, reference_of(name, k, shape), f"{name}, real spectrum, window {window}, cols_walk {walk}")
            walks.append(got)
            got = whole(ctx, 0, img, moved)
            assert stats(ctx, 0, "fft") == [1] * 3 and stats(ctx, 0, "real_spectrum") == [0] * 3
            assert_fft_exact(got, reference_of(name + "-moved", moved, shape), f"{name}, one tap moved, window {window}, cols_walk {walk}")
        if window[0] == 256:  # the column walk against one workgroup per pair: the same arithmetic, so the same bits
            assert np.array_equal(walks[0], walks[1]), f"cols_walk 1 against 0, window {window}: {first_difference(walks[1], walks[0])}"


@pytest.mark.parametrize("signed", [False, True], ids=["nonneg", "signed"])
@pytest.mark.parametrize("rows", [256, 512])
def test_fft_row_ranges_from_exact_source_windows(ctx, rows, signed):
    options(ctx, **FFT, stencil_fft_window_rows=rows)
    shape = (BANDS_H, 133)
    for k, name in band_stencils(signed):
        img, ref = frame_of(shape), reference_of(name, k, shape)
        outs = []
        for batch in (1, 3):
            ctx.set_option("stencil_fft_batch", batch)
            got = banded(ctx, 0, img, k, BANDS, et.reach(k))
            assert stats(ctx, 0, "fft") == [1] * 3 and all(w[0] == rows for w in stats(ctx, 0, "window"))
            assert_fft_exact(got, ref, f"{name}, bands from exact windows, {rows}-row windows, batch {batch}")
            outs.append(got)
        assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("family", ["ragged", "gaps"])
def test_cheaper_scratch_elements_stay_inside_their_stated_bounds(ctx, family):
    """complex64 scratch and the forced 12-byte element are not held to exactness (their rounding is relative to the window's
    magnitude): against the complex128 result of the same call, tests/test_gpu_fft.py's bounds -- at most 3 fp32 ulps, and 1e-6 at
    the 1e-3 floor."""
    k, name = stencil_of(family, (87, 87), False)
    shape = (300, 417)
    img = frame_of(shape)
    options(ctx, **FFT)
    c128 = whole(ctx, 1, img, k) / et.SCALE
    assert stats(ctx, 1, "fft") == [1] * 3
    assert_fft_exact(c128 * et.SCALE, reference_of(name, k, shape), f"{name}, complex128 scratch")
    for what, opts in (("complex64 scratch", dict(stencil_fft_scratch32=2)), ("12-byte scratch", dict(stencil_fft_scratch96=2))):
        options(ctx, **FFT)
        options(ctx, stencil_fft_scratch96=0)
        options(ctx, **opts)
        got = whole(ctx, 1, img, k) / et.SCALE
        assert stats(ctx, 1, "fft") == [1] * 3
        ulps = np.abs(got - c128) / np.spacing(np.abs(c128).astype(np.float32)).astype(np.float64)
        print(f"{name}, {what}: {ulps.max():.2f} ulps, rel {rel_err(got, c128, 1e-3):.3e}")
        assert ulps.max() <= 3 and rel_err(got, c128, 1e-3) <= 1e-6, (what, ulps.max())


# ------------------------------------------------------------------------------------------------ direct against FFT
@pytest.mark.parametrize("signed", [False, True], ids=["nonneg", "signed"])
@pytest.mark.parametrize("n", [21, 23, 25])
def test_whichever_form_the_hand_over_picks_meets_its_criterion(ctx, n, signed):
    """Sparse taps at the sizes around the direct / FFT hand-over, under the settings test_small_square_stencils_unrolled_direct_form
    steers the choice with (stencil_fixed, stencil_fft, the halation or the MTF slot)."""
    k, name = et.ragged(np.random.default_rng(n + signed), n, n, signed=signed)
    shape = (150, 203)
    img, ref = frame_of(shape), reference_of(name, k, shape)
    seen = set()
    for which in (0, 1):
        for fixed, fft in ((1, 1), (0, 1), (1, 0), (0, 0)):
            options(ctx, stencil_fixed=fixed, stencil_fft=fft)
            got = whole(ctx, which, img, k)
            ran = stats(ctx, which, "fft")
            assert stats(ctx, which, "unrolled") == [0] * 3  # (ragged taps are not mirror symmetric)
            if not fft:
                assert ran == [0] * 3
            elif signed:
                assert ran == [1] * 3  # taps of both signs take the float64 form whatever their size
            for c in range(3):  # (the three boxes differ by a row or a column: around 400 taps the channels part ways)
                what = f"{name}, slot {which}, stencil_fixed {fixed}, stencil_fft {fft}, channel {c}: {'fft' if ran[c] else 'direct'} form"
                seen.add(ran[c])
                g, r = got[..., c:c + 1], ref[..., c:c + 1]
                if not ran[c]:
                    assert_exact(g, r, what)
                elif which == 1 and not signed:  # the MTF slot's complex64 scratch: test_gpu_fft.py's bounds for it
                    ulps = np.abs(g - r) / et.SCALE / np.spacing(np.abs(r / et.SCALE).astype(np.float32)).astype(np.float64)
                    print(f"{what}, complex64 scratch: {ulps.max():.2f} ulps")
                    assert ulps.max() <= 3 and rel_err(g / et.SCALE, r / et.SCALE, 1e-3) <= 1e-6, what
                else:
                    assert_fft_exact(g, r, what)
    assert seen == {0, 1}
