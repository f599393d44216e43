"""The curve look-up on near-uniform axes, without a GPU.

The device evaluates the density curve and the grain LUT by guessing the cell arithmetically and, on a table the planner marked `near`
(r2f_plan.cpp, curve_cells), correcting the guess by at most ONE cell (r2f_device.h: curve_eval_at, curve_eval_batch,
curve_eval_near_lds).  Three things are held here:
  * tests/curve_check.cpp, built with AddressSanitizer and UndefinedBehaviorSanitizer from the translation unit the library links and
    run as a child process, searches jittered, reordered and float32-collapsed axes for a `near` flag that claims too much: wherever
    the planner says near, the guess plus one step must be the cell np.interp uses, for every breakpoint, its float neighbours and
    20 000 random arguments per axis;
  * tests/curve_model.py (the NumPy float32 restatement the GPU tests rely on to know their table's route) equals the planner:
    flag, x0, x1, inv_step and every cell, bit for bit;
  * for the exact tables and sample sets of tests/test_gpu_curve_sites.py: the model's look-up stays inside the tests' bounds of
    np.interp in float64, and the same look-up WITHOUT the corrective step misses them on at least 5 % of the in-range samples --
    those GPU tests would notice a site that stopped correcting."""

import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

from oracle import stages as st

import curve_model
import curve_sites as cs
import hostile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def curve_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("curve_check") / "curve_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "curve_check.cpp"), os.path.join(ROOT, "raw2film_amd", "csrc", "r2f_plan.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


def _run(binary, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([binary, *map(str, args)], capture_output=True, text=True, env=env, timeout=600)


@pytest.mark.parametrize("seed", [1, 2, 3, 20261019])
def test_a_near_flag_never_claims_more_than_one_corrective_step_can_mend(curve_check, seed):
    cases = 2500
    res = _run(curve_check, "search", seed, cases)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    words = res.stdout.split()
    assert words[1] == "cases," and words[-1] == "violations" and int(words[0]) == cases and int(words[-2]) == 0, res.stdout
    # two of the six jitters are under half a step, where the order holds and the guess at a breakpoint is floor(k + jitter u), k - 1 or k;
    # float32 collapses some of those axes (origin 1000 on a span of 1e-3, origin 3e5): a fifth of all cases at the very least are `near`
    assert int(words[2]) >= cases // 5, res.stdout


# ------------------------------------------------------------------------------------------------ the generators
def test_jittered_axes_keep_their_ends_and_their_order_and_leave_the_other_modes_alone():
    for m in (2, 3, 16, 256, 4096):
        for jitter in (0.1, 0.45, 0.49):
            c = hostile.curve(np.random.default_rng(m), m, axis="jitter", jitter=jitter)
            g = hostile.grain_lut(np.random.default_rng(m), m, steps=None, axis="jitter", jitter=jitter)
            for lut, lo, hi in ((c, -4.0, 1.5), (g, 0.0, 4.0)):
                assert lut.shape == (4, m) and lut.dtype == F32
                assert lut[0, 0] == F32(lo) and lut[0, -1] == F32(hi) and (np.diff(lut[0]) > 0).all()
                if m > 2:  # every inner breakpoint within jitter of a step of its grid position (and some of them moved)
                    off = (lut[0].astype(np.float64) - np.linspace(lo, hi, m)) / ((hi - lo) / (m - 1))
                    assert np.abs(off[1:-1]).max() <= jitter + 1e-3 and np.abs(off[1:-1]).max() > 0
            assert g[1:].min() >= 0.01 and g[1:].max() <= 0.06
            if m >= 256:  # independent amplitudes: no constant runs for a wrong cell to hide in
                assert (np.diff(g[1:], axis=1) != 0).all()
    with pytest.raises(AssertionError):
        hostile.curve(np.random.default_rng(0), 16, axis="jitter", jitter=0.5)
    # the streams of the callers there were before (recorded from the generators as they stood)
    r = np.random.default_rng(5)
    a, b, c = hostile.curve(r, 37, max_slope=6.0), hostile.curve(r, 64, uniform=True, monotone=True), hostile.grain_lut(r, 256, amp=0.03)
    assert [zlib.crc32(t.tobytes()) for t in (a, b, c)] == [1262806043, 3550394820, 3496029558] and r.uniform() == 0.7431297197222991


# ------------------------------------------------------------------------------------------------ the model against the planner
def _sweep():
    tables = []
    for m in (2, 3, 4, 16, 17, 255, 256, 1024, 4096):
        rng = np.random.default_rng(m)
        tables.append(hostile.curve(rng, m, uniform=True))
        tables.append(hostile.grain_lut(rng, max(m, 8)))
        for jitter in (0.1, 0.45, 0.49):
            tables.append(hostile.curve(rng, m, axis="jitter", jitter=jitter))
        tables.append(hostile.grain_lut(rng, m, steps=None, axis="jitter"))
        tables.append(hostile.curve(rng, m, max_slope=6.0))  # hostile.curve's own uneven axes: the exact walk
        if m <= 256:  # float32 is coarse up here: 6e-5 between neighbours, a tenth of the smallest gap at m = 256
            tables.append(hostile.curve(rng, m, x_lo=1000.0, x_hi=1000.5, axis="jitter"))
        else:  # ... and coarser than the gaps: sorted draws, abscissae repeat
            t = hostile.curve(rng, m, uniform=True).copy()
            t[0] = np.sort((1000.0 + 0.5 * rng.uniform(size=m)).astype(F32))
            tables.append(t)
    for m in (3, 4, 64):  # a repeated abscissa: at either end, in the middle
        for k in (0, m // 2, m - 2):
            t = hostile.curve(np.random.default_rng(k), m, uniform=True).copy()
            t[0, k + 1] = t[0, k]
            tables.append(t)
    two = hostile.curve(np.random.default_rng(9), 2, uniform=True).copy()
    two[0, 1] = two[0, 0]  # an empty range
    tables.append(two)
    tables += [np.asarray(cs.density_curve(c)) for c in cs.CASES] + [np.asarray(cs.grain_table(m)) for m in (256, 4096)]
    return tables


def test_the_model_equals_the_planner_flag_scales_and_cells(curve_check, tmp_path):
    tables = _sweep()
    path, cells_path = str(tmp_path / "tables.bin"), str(tmp_path / "cells.bin")
    with open(path, "wb") as f:
        f.write(np.int32(len(tables)).tobytes())
        for t in tables:
            f.write(np.int32(t.shape[1]).tobytes())
            f.write(np.ascontiguousarray(t, dtype=F32).tobytes())
    res = _run(curve_check, "flags", path, cells_path)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    lines = res.stdout.split("\n")[:-1]
    assert len(lines) == len(tables)
    cells = np.fromfile(cells_path, dtype=F32)
    at = 0
    seen = set()
    for t, line in zip(tables, lines):
        near, x0, x1, inv = line.split()
        k = curve_model.cells(t)
        what = (t.shape[1], line)
        assert int(near) == curve_model.is_near(t), what
        assert [int(w, 16) for w in (x0, x1, inv)] == [int(F32(k[n]).view(np.uint32)) for n in ("x0", "x1", "inv_step")], what
        n = 3 * (t.shape[1] - 1) * 4
        assert np.array_equal(cells[at:at + n].view(np.uint32), k["cells"].ravel().view(np.uint32)), what
        at += n
        seen.add(int(near))
        if (np.diff(t[0]) == 0).any() and t.shape[1] >= 3:
            assert int(near) == 0, what
    assert at == cells.size and seen == {0, 1}
    # the routes the GPU tests count on
    assert all(curve_model.is_near(cs.density_curve(c)) == 1 for c in cs.CASES) and all(curve_model.is_near(cs.grain_table(m)) == 1 for m in (256, 4096))
    assert curve_model.is_near(hostile.curve(np.random.default_rng(200 + 256), 256, max_slope=6.0)) == 0


def test_the_model_lands_in_the_cell_np_interp_uses():
    """guess + corrective step == upper_bound - 1 on `near` tables (what curve_check searches, here for the model itself), and the step
    is taken: about jitter / 2 of uniformly spread arguments need it, split between the two directions."""
    rng = np.random.default_rng(77)
    for m in (16, 64, 256, 1024, 3000):
        t = hostile.curve(rng, m, axis="jitter", jitter=0.45)
        assert curve_model.is_near(t) == 1
        x = np.concatenate([rng.uniform(-4.0, 1.5, 50000).astype(F32), t[0], np.nextafter(t[0], F32(-9)), np.nextafter(t[0], F32(9))])
        adj = curve_model.corrective(t, x)
        assert np.array_equal(curve_model.guess(t, x) + adj, curve_model.true_cell(t, x))
        share = (adj[:50000] != 0).mean()
        assert 0.17 <= share <= 0.29 and (adj == -1).mean() >= 0.05 and (adj == 1).mean() >= 0.05, (m, share)  # 0.45 / 2 = 0.225
        u = hostile.curve(rng, m, uniform=True)
        assert (curve_model.corrective(u, x[:50000]) != 0).mean() <= 1e-3


# ------------------------------------------------------------------------------------------------ teeth of the GPU tests' bounds
def _teeth(case, lut, x, bound):
    """x (..., 3) arguments, bound (..., 3): the model inside, the model without its corrective step outside on >= 5 % in range."""
    c = cs.assert_conditions(case, lut, x)
    ref = cs.interp64(lut, x)
    good = np.abs(cs.model_eval(lut, x, True).astype(np.float64) - ref)
    assert (good <= bound).all(), (case, float((good / bound).max()))
    inr = (x > lut[0, 0]) & (x < lut[0, -1])
    bad = np.abs(cs.model_eval(lut, x, False).astype(np.float64) - ref) > bound
    if case[0] == "u":  # the control: nothing to correct, nothing to notice
        assert not bad.any()
        return
    assert bad[inr].mean() >= 0.05, (case, float(bad[inr].mean()), c["down"], c["up"])
    assert not bad[~inr].any()  # (outside the axis the end rule answers, whatever the cell)


@pytest.mark.parametrize("shape", [(64, 96), (37, 53)])
@pytest.mark.parametrize("case", cs.CASES)
def test_front_samples_tell_a_missing_corrective_step(case, shape):
    k = cs.front_case(case, *shape)
    _teeth(case, k.lut, k.loge, k.bound)
    # the aimed samples are there: every inner breakpoint (or, where the frame is too small, as many as fit) has an argument within
    # 4 ulp + 1e-7 of it (float32(10 ** xp) is good to 6e-8 of itself, 2.6e-8 of its log; a ten-thousandth of a cell at m = 4096), and
    # both ends of the axis are passed
    xp = k.lut[0]
    tol = 4.0 * np.spacing(np.abs(xp[1:-1])) + F32(1e-7)
    lo, hi = xp[1:-1] - tol, xp[1:-1] + tol
    x = np.sort(k.loge[..., 0].ravel())
    hit = np.searchsorted(x, hi, side="right") > np.searchsorted(x, lo, side="left")
    assert hit.sum() >= min(len(xp) - 2, k.n_aimed - 2), (case, int(hit.sum()))
    assert x[0] < xp[0] and x[-1] > xp[-1]


@pytest.mark.parametrize("case", cs.FAST_CASES)
def test_split_front_samples_tell_a_missing_corrective_step(case):
    k = cs.split_front_case(case, 64, 96, 166.67)
    _teeth(case, k.lut, np.repeat(k.loge, 3, axis=-1), np.repeat(k.bound[..., None], 3, axis=-1))


@pytest.mark.parametrize("shape,scale", [((70, 133), 166.67), ((300, 417), 341.33)])
@pytest.mark.parametrize("case", cs.CASES)
def test_halation_samples_tell_a_missing_corrective_step(case, shape, scale):
    k = cs.halation_case(case, *shape, scale)
    cs.assert_conditions(case, k.lut, k.loge[..., :2])  # each site's own samples: the channels with a real stencil, the single tap
    cs.assert_conditions(case, k.lut, k.loge[..., 2:])
    _teeth(case, k.lut, k.loge, k.bound)


@pytest.mark.parametrize("mono", [False, True])
@pytest.mark.parametrize("m", [256, 4096])
def test_grain_samples_tell_a_missing_corrective_step(m, mono):
    k = cs.grain_case(m, mono)
    c = cs.assert_conditions(f"m{m}", k.lut, k.dens)
    xp = k.lut[0]
    for probe in (xp[1:-1], np.nextafter(xp[1:-1], F32(-9)), np.nextafter(xp[1:-1], F32(9)), xp[:1], xp[-1:]):
        assert np.isin(probe, k.dens).all()
    assert (k.dens < 0).any() and (k.dens > 4).any() and (k.dens[1] == 0).all() and np.isfinite(k.dens).all()
    assert (k.dens[~k.clip_rows] >= cs.GRAIN_LOW).all()
    field = st.grain_field(*cs.GRAIN_SHAPE, k.p.seed, k.p.grain_kernel, mono)
    ref = k.ref.astype(np.float64)

    def grained(correct):
        return np.maximum(k.dens + field * cs.model_eval(k.lut, k.dens, correct), F32(0.0))

    good, broken = grained(True), grained(False)
    assert (np.abs(good - ref) <= k.bound).all()
    inr = (k.dens > xp[0]) & (k.dens < xp[-1])
    bad = np.abs(broken - ref) > k.bound
    assert bad[inr].mean() >= 0.05, (float(bad[inr].mean()), c["down"], c["up"])
    # ... and through the identity 3-D LUT of the tail kernels
    shown = lambda d: np.minimum(d.astype(np.float64), 4.0) / 4.0  # noqa: E731
    assert (np.abs(shown(good) - k.shown) <= k.shown_bound).all()
    assert (np.abs(shown(broken) - k.shown) > k.shown_bound)[inr].mean() >= 0.05
