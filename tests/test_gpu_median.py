"""Step M (the median filter of the colour differences, LibRaw's med_passes) in the device demosaics, byte for byte against the
NumPy model (tests/median_model.py) through each of the three entry points: r2f_demosaic_median_u16 and
r2f_demosaic_xtrans_median_u16 at full and reduced size, four phases of either pattern, n in {1, 2, 4}, with and without Blend; one
ragged tile, 2 x 3 ragged tiles and a 3 x 2-tile frame whose aprons cross a seam both ways; the smallest frames; all eight
orientations; r2f_demosaic_median_f32 in windows with an odd origin off the tile grid; and row ranges cut at 1, 31, 32, 33 and at
single rows, each call given only the source window its reach allows -- one row fewer is refused with the rows named.  The
fixtures' conditions (every pass changes at least 10 % of the interior, the result differs from the plain demosaic at half the
pixels at least) are asserted in tests/test_median_host.py; the second is asserted on the model's output here as well."""

import ctypes as C

import numpy as np
import pytest

import demosaic_model as dm
import highlight_model as hm
import median_model as mm
import xtrans_model as xm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PASSES = (1, 2, 4)
BAYER_SHAPES = (hm.ONE_TILE, hm.BAYER_FRAME, (70, 130))  # one ragged tile, 2 x 3 of them, 3 x 2 of them
XTRANS_SHAPES = (hm.ONE_TILE, hm.XTRANS_FRAME, (71, 131))
XPATTERNS = xm.PATTERNS  # four phases of the array: shifts (0, 0), (1, 0), (0, 1), (1, 1)


@pytest.fixture(scope="module")
def ctx():
    from raw2film_amd.context import HipContext

    c = HipContext(0)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint16)


def case(xtrans, kind, pattern, shape, reduced):
    """(mosaic, profile, clip) whose demosaiced frame has `shape`: the reduced form's mosaic has 2 (3) times those sides."""
    k = (3 if xtrans else 2) if reduced else 1
    return (hm.xtrans_case if xtrans else hm.bayer_case)(kind, pattern, (k * shape[0], k * shape[1]))


def run(ctx, xtrans, m, params, n, clip=None, **kw):
    return host((ctx.demosaic_xtrans_median if xtrans else ctx.demosaic_median_u16)(m, params, n, clip=clip, **kw))


def check_against_model(ctx, xtrans, pattern, n, reduced, shapes):
    for i, shape in enumerate(shapes):
        mosaic, prof, clip = case(xtrans, ("equal", "wb")[i & 1], pattern, shape, reduced)
        params, m = prof.plan(*mosaic.shape, reduced), dev(mosaic)
        plain = hm.demosaic(mosaic, prof, None, half_size=reduced, xtrans=xtrans)
        for c in (None, clip):
            want = mm.demosaic(mosaic, prof, n, c, half_size=reduced, xtrans=xtrans)
            assert want.shape[:2] == shape
            if c is None:
                assert np.count_nonzero((want != plain).any(axis=-1)) >= 0.5 * shape[0] * shape[1]  # (step M is no no-op here)
            got = run(ctx, xtrans, m, params, n, c)
            assert got.shape == want.shape and np.array_equal(got, want), (pattern, n, reduced, shape, c, int((got != want).sum()))


@pytest.mark.parametrize("reduced", [False, True], ids=["full", "half"])
@pytest.mark.parametrize("n", PASSES)
@pytest.mark.parametrize("pattern", dm.PATTERNS)
def test_bayer_median_equals_the_model(ctx, pattern, n, reduced):
    check_against_model(ctx, False, pattern, n, reduced, BAYER_SHAPES)


@pytest.mark.parametrize("reduced", [False, True], ids=["full", "third"])
@pytest.mark.parametrize("n", PASSES)
@pytest.mark.parametrize("pattern", XPATTERNS, ids=["shift00", "shift10", "shift01", "shift11"])
def test_xtrans_median_equals_the_model(ctx, pattern, n, reduced):
    check_against_model(ctx, True, pattern, n, reduced, XTRANS_SHAPES)


@pytest.mark.parametrize("n", PASSES)
def test_the_smallest_frames(ctx, n):
    """A side of 2 has no interior (the plain entry point's bytes); a side of 3 has one interior row; the X-Trans minimum."""
    for xtrans, shape, reduced in ((False, (4, 6), False), (False, (3, 64 + 3), False), (False, (2, 6), False), (False, (4, 6), True),
                                   (False, (8, 134), True), (True, (6, 6), False), (True, (7, 8), False), (True, (9, 12), True)):
        pattern = xm.PATTERNS[1] if xtrans else "GRBG"
        mosaic, prof, clip = (hm.xtrans_case if xtrans else hm.bayer_case)("equal", pattern, shape)
        params, m = prof.plan(*shape, reduced), dev(mosaic)
        for c in (None, clip):
            want = mm.demosaic(mosaic, prof, n, c, half_size=reduced, xtrans=xtrans)
            got = run(ctx, xtrans, m, params, n, c)
            assert np.array_equal(got, want), (xtrans, shape, reduced, n, c)
        if min(want.shape[:2]) < 3:
            plain = (ctx.demosaic_xtrans if xtrans else ctx.demosaic_u16)(m, params)
            assert np.array_equal(run(ctx, xtrans, m, params, n), host(plain))


@pytest.mark.parametrize("reduced", [False, True], ids=["full", "reduced"])
@pytest.mark.parametrize("xtrans", [False, True], ids=["bayer", "xtrans"])
def test_all_eight_orientations(ctx, xtrans, reduced):
    for n, shape in ((1, hm.ONE_TILE), (4, hm.XTRANS_FRAME if xtrans else hm.BAYER_FRAME)):
        mosaic, prof, clip = case(xtrans, "equal", xm.PATTERNS[1] if xtrans else "GBRG", shape, reduced)
        params, m = prof.plan(*mosaic.shape, reduced), dev(mosaic)
        for c in (None, clip):
            want = mm.demosaic(mosaic, prof, n, c, half_size=reduced, xtrans=xtrans)
            for o in range(8):
                got, ref = run(ctx, xtrans, m, params, n, c, orientation=o), hm.orient(want, o)
                assert got.shape == ref.shape and np.array_equal(got, ref), (xtrans, reduced, n, c, o, int((got != ref).sum()))
        # bands of the oriented frame compose to it (a turned band is columns of D: a ring of columns beyond it is read)
        for o in (3, 5):
            ref = hm.orient(want, o)
            out = torch.zeros(ref.shape, dtype=torch.int16, device="cuda")
            rows = ref.shape[0]
            for y0, y1 in ((0, 1), (1, 33), (33, rows - 2), (rows - 2, rows)):
                (ctx.demosaic_xtrans_median if xtrans else ctx.demosaic_median_u16)(m, params, n, clip=clip, out=out, rows=(y0, y1), orientation=o)
            assert np.array_equal(host(out), ref), (xtrans, reduced, n, o)


def decode(u16, factor, divisor=65535.0):
    """r2f_decode_u16's expression: two correctly rounded fp32 operations and the clamp."""
    return np.minimum(u16.astype(np.float32) / np.float32(divisor) * np.float32(factor), np.float32(65504.0))


@pytest.mark.parametrize("reduced", [False, True], ids=["full", "half"])
@pytest.mark.parametrize("n", PASSES)
def test_the_float_epilogue_equals_the_models_decoded_window(ctx, n, reduced):
    factor = float(np.float32(2.0 ** 0.5))
    for pattern, kind, shape in (("RGGB", "equal", hm.BAYER_FRAME), ("GBRG", "wb", (70, 130))):
        mosaic, prof, clip = case(False, kind, pattern, shape, reduced)
        params, m = prof.plan(*mosaic.shape, reduced), dev(mosaic)
        oh, ow = shape
        for c in (None, clip):
            frame = mm.demosaic(mosaic, prof, n, c, half_size=reduced)
            # odd row0 / col0 that are no tile multiples; a window edge is no border: the median reads the frame beyond it
            for window in ((0, 0, oh, ow), (3, 65, oh - 7, ow - 67), (1, 5, oh - 2, ow - 9), (33, 63, 2, 3)):
                r0, c0, nr, nc = window
                want = decode(frame[r0:r0 + nr, c0:c0 + nc], factor)
                out = torch.full((nr, nc, 3), -1.0, dtype=torch.float32, device="cuda")
                for y0, y1 in ((0, nr // 3), (nr // 3, nr - nr // 4), (nr - nr // 4, nr)):
                    ctx.demosaic_median_f32(m, params, n, factor, clip=c, window=window, out=out, rows=(y0, y1))
                got = out.cpu().numpy()
                assert np.array_equal(got, want), (pattern, n, reduced, c, window, int((got != want).sum()))


CUTS = (0, 1, 31, 32, 33, 34, 35)  # rows [0, 1), [1, 31), [31, 32), [32, 33), [33, 34), [34, 35) and the rest


@pytest.mark.parametrize("reduced", [False, True], ids=["full", "reduced"])
@pytest.mark.parametrize("xtrans", [False, True], ids=["bayer", "xtrans"])
@pytest.mark.parametrize("n", PASSES)
def test_row_ranges_compose_from_the_source_window_their_reach_allows(ctx, n, xtrans, reduced):
    shape = (71, 131) if xtrans else (70, 130)
    mosaic, prof, clip = case(xtrans, "wb", xm.PATTERNS[3] if xtrans else "BGGR", shape, reduced)
    H, W = mosaic.shape
    params, m = prof.plan(H, W, reduced), dev(mosaic)
    want = mm.demosaic(mosaic, prof, n, clip, half_size=reduced, xtrans=xtrans)
    fn = ctx._lib.r2f_demosaic_xtrans_median_u16 if xtrans else ctx._lib.r2f_demosaic_median_u16
    reach, reduction = (3 if xtrans else 4), ((3 if xtrans else 2) if reduced else 0)
    out = torch.zeros(want.shape, dtype=torch.int16, device="cuda")
    cuts = CUTS + (shape[0],)
    for y0, y1 in zip(cuts, cuts[1:]):
        lo, hi = mm.source_rows(y0, y1, n, shape[0], H, reach, reduction)
        rows = m[lo:hi].clone()  # this call's share of the mosaic and nothing else

        def call(gy0, nrows):
            return fn(ctx._h, rows.data_ptr(), gy0, nrows, W, H, W, C.byref(params), 0, clip, n, out.data_ptr(), y0, y1, ctx._stream())

        assert call(lo, hi - lo) == 0, ctx._lib.r2f_last_error(ctx._h)
        for gy0, nrows in ((lo, hi - lo - 1), (lo + 1, hi - lo - 1)):  # one row fewer at either end
            assert call(gy0, nrows) == -1
            message = ctx._lib.r2f_last_error(ctx._h).decode()
            assert f"read mosaic rows [{lo}, {hi})" in message and f"holds [{gy0}, {gy0 + nrows})" in message, message
    torch.cuda.synchronize()
    assert np.array_equal(host(out), want), (n, xtrans, reduced, int((host(out) != want).sum()))


def test_refusals_launch_nothing(ctx):
    mosaic, prof, _ = hm.bayer_case("equal", "RGGB", hm.ONE_TILE)
    xmosaic, xprof, _ = hm.xtrans_case("equal", xm.PATTERNS[0], hm.ONE_TILE)
    H, W = hm.ONE_TILE
    p, xp, m, xmo = prof.plan(H, W), xprof.plan(H, W), dev(mosaic), dev(xmosaic)
    out = torch.full((H, W, 3), 7, dtype=torch.int16, device="cuda")
    fout = torch.full((H, W, 3), 7.0, dtype=torch.float32, device="cuda")
    lib, h, s = ctx._lib, ctx._h, ctx._stream()

    def bayer(clip=0, n=2, o=0):
        return lib.r2f_demosaic_median_u16(h, m.data_ptr(), 0, H, W, H, W, C.byref(p), o, clip, n, out.data_ptr(), 0, H, s)

    def xtrans(clip=0, n=2, o=0):
        return lib.r2f_demosaic_xtrans_median_u16(h, xmo.data_ptr(), 0, H, W, H, W, C.byref(xp), o, clip, n, out.data_ptr(), 0, H, s)

    def f32(clip=0, n=2):
        return lib.r2f_demosaic_median_f32(h, m.data_ptr(), 0, H, W, H, W, C.byref(p), clip, n, 0, 0, H, W, 65535.0, 1.0, fout.data_ptr(), 0, H, s)

    for call in (bayer, xtrans, f32):
        for n in (0, 5, -1, 2 ** 31 - 1):
            assert call(n=n) == -1
            assert b"R2F_MEDIAN_MAX_PASSES" in lib.r2f_last_error(h) and b"med_passes" in lib.r2f_last_error(h)
        for clip in (-1, 65536):
            assert call(clip=clip) == -1
            assert b"clip" in lib.r2f_last_error(h)
    assert bayer(o=8) == -1 and xtrans(o=-1) == -1
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((fout == 7.0).all())
    for bad in (0, 5, 1.0, True, None):
        for method, mo, pp in ((ctx.demosaic_median_u16, m, p), (ctx.demosaic_xtrans_median, xmo, xp)):
            with pytest.raises(ValueError, match="med_passes"):
                method(mo, pp, bad)
        with pytest.raises(ValueError, match="med_passes"):
            ctx.demosaic_median_f32(m, p, bad, 1.0)
    for bad in (0, -1, 65536, 1.5, True):
        with pytest.raises(ValueError, match="clip"):
            ctx.demosaic_median_u16(m, p, 2, clip=bad)
    with pytest.raises(TypeError):  # the float entry point has no orientation
        ctx.demosaic_median_f32(m, p, 2, 1.0, orientation=5)
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((fout == 7.0).all())
