"""The device's 1-D curve look-up (raw2film_amd/csrc/r2f_device.h: curve_eval_at, curve_eval_batch, curve_eval_near_lds) and the
planner that feeds it (r2f_plan.cpp, curve_cells) restated in NumPy float32 -- test infrastructure, nothing in the product imports it.

A (4, m) table (row 0 = abscissae xp, rows 1..3 = values) becomes m - 1 cells {xp[i], xp[i+1], fp[i], slope[i]} per channel.  A
look-up GUESSES the cell from a uniform grid, clamp(int((x - x0) * inv_step), 0, m - 2), and then corrects the guess against the cell's
own bounds.  On a table the planner marked `near` (the guess is never more than one cell off) the correction is ONE step,
adj = -1 / 0 / +1, instead of a walk.  `evaluate(..., correct=False)` leaves that step out: the look-up a site with a broken corrective
gather would make.  tests/test_curve_host.py holds this model equal to the library's planner and shows that the bounds of
tests/test_gpu_curve_sites.py tell the two apart; the GPU tests use the model to state, BEFORE they look at a device result, which route
their table takes and how many of their samples need the step in each direction."""

from __future__ import annotations

import numpy as np

F32 = np.float32


def cells(lut) -> dict:
    """plan::curve_cells: x0, x1, inv_step = float32(m - 1) / float32(x1 - x0) (0 on an empty range) and the (3, m - 1, 4) float32 cells;
    slopes taken in double and rounded once, 0 across a repeated abscissa."""
    lut = np.asarray(lut, dtype=F32)
    m = lut.shape[1]
    xp = lut[0]
    rng = F32(xp[-1] - xp[0])
    inv_step = F32(m - 1) / rng if rng > 0 else F32(0.0)
    dx = np.diff(xp.astype(np.float64))
    out = np.empty((3, m - 1, 4), dtype=F32)
    for c in range(3):
        df = np.diff(lut[1 + c].astype(np.float64))
        out[c, :, 0] = xp[:-1]
        out[c, :, 1] = xp[1:]
        out[c, :, 2] = lut[1 + c, :-1]
        out[c, :, 3] = np.where(dx != 0, df / np.where(dx != 0, dx, 1.0), 0.0).astype(F32)
    return {"m": m, "x0": xp[0], "x1": xp[-1], "inv_step": F32(inv_step), "cells": out}


def _guess(x0, inv_step, last, x):
    x = np.asarray(x, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        gf = (x - F32(x0)) * F32(inv_step)  # float32 difference, float32 product: no contraction possible
        # the planner's float clamp ahead of the cast (the device casts first and clamps the integer: the same for every finite x)
        gf = np.where(gf > 0, np.minimum(gf, F32(last)), F32(0.0))
    return gf.astype(np.int64)  # truncation, like (int)


def guess(lut, x) -> np.ndarray:
    """The first guess of the cell of x."""
    k = cells(lut)
    return _guess(k["x0"], k["inv_step"], k["m"] - 2, x)


def true_cell(lut, x) -> np.ndarray:
    """upper_bound(xp, x) - 1 clamped to the cells: the cell np.interp uses, and where the exact walk of a table that is not `near` ends."""
    xp = np.asarray(lut, dtype=F32)[0]
    return np.clip(np.searchsorted(xp, np.asarray(x, dtype=F32), side="right") - 1, 0, len(xp) - 2)


def is_near(lut) -> int:
    """The planner's rule for DevCurve::near: no inner breakpoint repeats a neighbour, and at every inner breakpoint k and at the float
    just below it the guess is within one cell of the true cell (k and k - 1)."""
    lut = np.asarray(lut, dtype=F32)
    xp = lut[0]
    m = len(xp)
    if m < 3:
        return 1
    k = cells(lut)
    last = m - 2
    idx = np.arange(1, m - 1)
    if (xp[idx] == xp[idx - 1]).any() or (xp[idx] == xp[idx + 1]).any():
        return 0
    at = _guess(k["x0"], k["inv_step"], last, xp[idx])
    below = _guess(k["x0"], k["inv_step"], last, np.nextafter(xp[idx], F32(-np.inf)))
    ok = (np.abs(at - np.minimum(idx, last)) <= 1) & (np.abs(below - (idx - 1)) <= 1)
    return int(ok.all())


def _adj(k, i, x):
    last = k["m"] - 2
    c = k["cells"][0][i]
    return np.where((x < c[..., 0]) & (i > 0), -1, np.where((x >= c[..., 1]) & (i < last), 1, 0))


def corrective(lut, x) -> np.ndarray:
    """adj of every x: the one corrective step the device takes on a `near` table (-1, 0 or +1)."""
    k = cells(lut)
    x = np.asarray(x, dtype=F32)
    return _adj(k, _guess(k["x0"], k["inv_step"], k["m"] - 2, x), x)


def evaluate(lut, ch: int, x, correct: bool = True) -> np.ndarray:
    """curve_eval_at on channel ch: guess, the corrective step (one step on a `near` table, the walk's end otherwise; none at all with
    correct=False), fma(slope, x - xp, fp) in float32, then the end rule !(x > x0) -> f_first, x >= x1 -> f_last."""
    lut = np.asarray(lut, dtype=F32)
    k = cells(lut)
    x = np.asarray(x, dtype=F32)
    i = _guess(k["x0"], k["inv_step"], k["m"] - 2, x)
    if correct:
        i = i + _adj(k, i, x) if is_near(lut) else true_cell(lut, x)
    c = k["cells"][ch][i]
    # (the product of two float32 is exact in double; the sum is rounded to double and then to float32 -- an fma but for a double rounding)
    v = (c[..., 3].astype(np.float64) * (x - c[..., 0]).astype(np.float64) + c[..., 2].astype(np.float64)).astype(F32)
    return np.where(~(x > k["x0"]), lut[1 + ch, 0], np.where(x >= k["x1"], lut[1 + ch, -1], v)).astype(F32)
