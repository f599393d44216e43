"""tests/exact_taps.py on the CPU: the premise (integer samples and dyadic taps make the correlation exact in float32, whatever the
order), the reason for it (the contract tolerance passes a misplaced small tap that the exact criterion rejects at most outputs),
the source-row rule for tap boxes beside the anchor, and the planner's entry lists for every family through r2f_plan_stencil."""

import ctypes

import numpy as np
import pytest

import exact_taps as et
from helpers import assert_close
from oracle import stages as st


def families(signed):
    """Every family once, at odd sizes (the oracle's direct method wants them)."""
    rng = np.random.default_rng(2026 + signed)
    out = [et.ragged(rng, 43, 43, signed=signed), et.ragged(rng, 9, 9, signed=signed), et.ragged(rng, 87, 87, signed=signed),
           et.ragged(rng, 25, 31, 1, signed=signed, box=(2, 20, 3, 29)),
           et.gaps(rng, 43, 43, signed=signed), et.gaps(rng, 9, 9, signed=signed), et.gaps(rng, 87, 87, signed=signed),
           et.corners(rng, 43, 43, signed=signed), et.corners(rng, 9, 9, signed=signed),
           et.shift(rng, 43, 43, ("above", "left", "first"), signed=signed), et.shift(rng, 43, 43, ("below", "right", "last"), signed=signed),
           et.shift(rng, 9, 9, ("above", "left", "first"), cluster=False, signed=signed),
           et.shift(rng, 9, 9, ("below", "right", "last"), signed=signed),
           et.central_sparse(rng, 45, 61, signed=signed)]
    out += [et.sym_sparse(rng, r, signed=signed) for r in (4, 5, 6, 7, 43)]
    out += [et.square_sym(rng, R, signed=signed) for R in (1, 2, 5, 11)]
    return out


ALL = families(False) + families(True)


@pytest.mark.parametrize("k, name", ALL, ids=[n for _, n in ALL])
def test_the_families_are_exact_in_float32_in_any_order(k, name):
    rng = np.random.default_rng(len(name))
    img = et.frame(rng, 70, 133)
    ref = et.reference(img, k)
    assert np.abs(ref).max() < 2 ** 24
    direct = st.convolve_2d(img, k, method="direct").astype(np.float64) * et.SCALE
    assert np.array_equal(direct, ref), name
    # float32 accumulation over the taps in a shuffled order: exact too
    H, W = img.shape[:2]
    kh, kw, kc = k.shape
    pad = np.pad(img, ((kh // 2, kh - 1 - kh // 2), (kw // 2, kw - 1 - kw // 2), (0, 0)), mode="reflect")
    for c in range(3):
        kcc = k[..., c if kc == 3 else 0]
        taps = np.argwhere(kcc != 0)
        rng.shuffle(taps)
        acc = np.zeros((H, W), np.float32)
        for i, j in taps:
            acc += kcc[i, j] * pad[i:i + H, j:j + W, c]
        assert acc.dtype == np.float32 and np.array_equal(acc.astype(np.float64) * et.SCALE, ref[..., c]), (name, c)


def test_reference_reflects_more_than_once_on_frames_smaller_than_the_stencil():
    rng = np.random.default_rng(5)
    k, _ = et.ragged(rng, 43, 43, signed=True)
    for shape in ((20, 24), (1, 40), (33, 1), (1, 1)):
        img = et.frame(rng, *shape)
        fft = st.convolve_2d(img, k).astype(np.float64) * et.SCALE  # (the oracle's FFT route pads by repeated reflection as well)
        assert np.array_equal(np.rint(fft), et.reference(img, k)), shape


def test_the_contract_tolerance_passes_a_misplaced_small_tap_that_the_exact_criterion_rejects():
    """The written reason for this file.  A normalised dense 87 x 87 stencil over uniform(0, 2) input, as
    test_generic_stencil_reflect101 uses: the model's smallest tap lands one column off and assert_close(..., 1e-5, 1e-3) still
    passes against the unmodified oracle.  The same edit to an exact-family stencil changes the reference at most outputs."""
    rng = np.random.default_rng(87)
    k = rng.uniform(0, 1, (87, 87, 3)).astype(np.float32)
    k /= k.sum(axis=(0, 1), keepdims=True)
    img = rng.uniform(0.0, 2.0, (70, 133, 3)).astype(np.float32)

    def misplace(k):
        """Move the smallest non-zero tap of every channel one column (onto a neighbour that is zero if there is one)."""
        out = k.copy()
        for c in range(k.shape[2]):
            mag = np.where(k[..., c] != 0, np.abs(k[..., c]), np.inf)
            i, j = np.unravel_index(np.argmin(mag), mag.shape)
            j2 = j + 1 if j + 1 < k.shape[1] else j - 1
            out[i, j2, c] += out[i, j, c]
            out[i, j, c] = 0
        return out

    wrong = misplace(k)
    assert not np.array_equal(wrong, k)
    assert_close(st.convolve_2d(img, wrong), st.convolve_2d(img, k), 1e-5, 1e-3, "a tap one column off")  # passes: the blind spot
    for signed in (False, True):
        ke, _ = et.ragged(np.random.default_rng(1), 87, 87, signed=signed)
        imge = et.frame(rng, 70, 133)
        moved = et.reference(imge, misplace(ke)) != et.reference(imge, ke)
        assert moved.mean() > 0.5, moved.mean()


def test_source_rows_against_brute_force_with_tap_boxes_beside_the_anchor():
    rng = np.random.default_rng(11)
    cases = [(1, 0, 1, 3, -2), (5, 0, 1, 43, -41), (5, 4, 5, -41, 43), (50, 0, 1, 43, -41), (50, 49, 50, -41, 43), (2, 0, 2, -7, 9)]
    for _ in range(4000):
        H = int(rng.integers(1, 60))
        y0 = int(rng.integers(0, H))
        y1 = int(rng.integers(y0 + 1, H + 1))
        taps = int(rng.integers(1, 130))  # taller than the frame as often as not
        above = int(rng.integers(-130, 131)) if rng.random() < 0.5 else int(rng.integers(0, taps))
        cases.append((H, y0, y1, above, taps - 1 - above))
    negative = 0
    for H, y0, y1, above, below in cases:
        lo, hi = et.source_rows(y0, y1, above, below, H)
        seen = {et.reflect101(y + d, H) for y in range(y0, y1) for d in range(-above, below + 1)}
        assert 0 <= lo < hi <= H and min(seen) == lo and max(seen) == hi - 1, (H, y0, y1, above, below, lo, hi)
        if above >= 0 and below >= 0:
            assert lo <= y0 and hi >= y1
        negative += above < 0 or below < 0
    assert negative > 1000


# ---- the planner on every family (the library's plan-only export checks its entry list, masks included, against the taps)
def _plan(k, c, Q, TW, TH, budget, allow_sym):
    from raw2film_amd import _lib

    lib = _lib.load()
    k = np.ascontiguousarray(k)
    out = (ctypes.c_int * 8)()
    rc = lib.r2f_plan_stencil(k.ctypes.data, k.shape[0], k.shape[1], k.shape[2], c, Q, TW, TH, budget, allow_sym, out)
    return rc, dict(zip(("entries", "rowsteps", "phases", "sym", "kh", "kw", "rs", "lds_rows"), out))


@pytest.mark.parametrize("k, name", ALL, ids=[n for _, n in ALL])
def test_the_planner_reproduces_every_family_and_the_families_hit_what_they_are_for(k, name):
    from raw2film_amd import _lib

    phases_seen, tallest = set(), 0
    for Q, TW, TH in ((4, 128, 64), (4, 64, 32), (2, 64, 32)):
        for allow_sym in (0, 1):
            for c in range(3):
                for kb in (160, 80, 48, 16):
                    rc, p = _plan(k, c, Q, TW, TH, kb * 1024, allow_sym)
                    assert rc in (_lib.OK, _lib.ETOOLARGE), (name, Q, allow_sym, c, kb, rc)  # never EHIP: the list reproduces its taps
                    if rc == _lib.ETOOLARGE:
                        continue
                    phases_seen.add(p["phases"])
                    tallest = max(tallest, p["kh"])
                    assert (p["lds_rows"] * p["rs"] + 16) * 4 <= kb * 1024
                    steps, skipped = et.row_steps(k, c, Q, sym=bool(p["sym"]))
                    # the restated row steps are the library's: the claims below then speak about what the device walks
                    assert (p["entries"], p["rowsteps"]) == (sum(s[0] for s in steps), len(steps)), (name, Q, allow_sym, c, kb)
                    assert p["rowsteps"] + skipped == p["kh"] + Q - 1
                    if name.startswith("sym_sparse"):
                        assert p["sym"] == allow_sym and (p["kw"] - 1) // 2 % 4 == (2 if allow_sym else (k.shape[1] // 2) % 4)
                    if name.startswith("shift") or name.startswith("corners") or name.startswith("gaps-9x9"):
                        assert p["sym"] == 0
    assert len(phases_seen) > 1 or tallest < 40, (name, phases_seen)  # the small budgets split the tall boxes into phases


@pytest.mark.parametrize("signed", [False, True])
def test_the_families_hold_the_row_steps_they_promise(signed):
    rng = np.random.default_rng(7 + signed)
    for Q in (2, 4):
        for sizes in (((9, 9), (6, 9)), ((43, 43),), ((87, 87),)):  # (a 6-row box has too few row steps of Q = 4 rows to show all alone)
            firsts, lasts, single = set(), set(), 0
            for size in sizes:
                k, name = et.ragged(rng, *size, signed=signed)
                for c in range(3):
                    steps, _ = et.row_steps(k, c, Q)
                    firsts |= {s[1] for s in steps}
                    lasts |= {s[2] for s in steps}
                    single += sum(s[0] == 1 for s in steps)
                if size[0] >= 20:
                    assert any(s == (1, 1, 1) for c in range(3) for s in et.row_steps(k, c, Q)[0]), name  # a row step of one tap
            assert firsts == {1, 2, 3, 4} and lasts == {1, 2, 3, 4} and single >= 2, (name, Q, firsts, lasts, single)
        for size in ((43, 43), (87, 87)):
            k, name = et.gaps(rng, *size, signed=signed)
            for c in range(3):
                steps, skipped = et.row_steps(k, c, Q)
                assert skipped >= (3 if Q == 2 else 1) and len(steps) > skipped, (name, Q, c, skipped)
                assert any(s[0] >= 3 for s in steps)
        for places in (("above", "left", "first"), ("below", "right", "last")):
            k, name = et.shift(rng, 43, 43, places, cluster=False, signed=signed)
            for c in range(3):
                steps, skipped = et.row_steps(k, c, Q)
                assert steps == [(1, 1, 1)] * Q and skipped == 0, name
                above, below = et.reach(k, c)
                assert above + below == 0 and (places[c] in ("left", "right") or above != 0)
        k, name = et.shift(rng, 87, 87, ("first", "last", "above"), signed=signed)
        assert [et.reach(k, c) for c in range(3)] == [(43, -43), (-43, 43), (4, -2)]
        for r in (4, 5, 6, 7, 43):
            k, name = et.sym_sparse(rng, r, signed=signed)
            assert np.array_equal(k, k[:, ::-1]) and k.shape[1] == 2 * r + 1
            counts, single = set(), 0
            for c in range(3):
                steps, skipped = et.row_steps(k, c, Q, sym=True)
                assert skipped >= 1 or Q == 4, (name, Q, c)
                counts |= {s[1] for s in steps} | {s[2] for s in steps}
                single += sum(s[0] == 1 for s in steps)
            # partly live end chunks of more than one kind (the mirrored form evaluates by these masks), one-entry row steps
            assert len(counts - {4}) >= 2 and single >= 1, (name, Q, counts, single)
    for R in range(1, 12):
        k, name = et.square_sym(rng, R, signed=signed)
        for c in range(3):
            assert et.tap_box(k, c) == (0, 2 * R, 0, 2 * R) and np.array_equal(k, k[:, ::-1])
            kc = k[..., c]
            assert (R == 1 or (~kc.any(axis=1)).any()) and (~kc.any(axis=0)).any(), name
    k, _ = et.central_sparse(rng, 45, 61, signed=signed)
    assert np.array_equal(k, k[::-1, ::-1]) and all(et.tap_box(k, c) == (0, 44, 0, 60) for c in range(3))
