"""Tables, sample sets, references and bounds shared by tests/test_gpu_curve_sites.py (the device's curve look-up sites on jittered
near-uniform axes) and tests/test_curve_host.py (the proof, without a GPU, that those tests would notice a site that stopped taking its
corrective step).  Everything here is NumPy and the oracle; each case is built once (lru_cache) and must not be modified by its users.

A case names its table: "m3lo" / "m3hi" (m = 3, the inner breakpoint moved down / up: with ONE inner breakpoint a table can only ever
need the corrective step in one direction -- +1 when it moved down, -1 when it moved up -- so m = 3 takes two tables to see both), "m256",
"m1024", "m4096" (jitter 0.45) and "u1024" (the exactly uniform control)."""

from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from oracle import stages as st

import curve_model
import hostile
from helpers import oracle_inputs, stocks, synthetic_frame

F32 = np.float32
JITTER = 0.45
CASES = ("m3lo", "m3hi", "m256", "m1024", "m4096", "u1024")
FAST_CASES = ("m3lo", "m3hi", "m256", "m1024", "u1024")  # (m = 4096: 196 KB of cells, no kernel keeps them in LDS)
# seeds chosen on the CPU so that the MODEL alone meets the input conditions below on every sample set that uses the table
_CURVE_SEEDS = {"m3lo": 34, "m3hi": 10, "m256": 256, "m1024": 1024, "m4096": 4096, "u1024": 11}
_GRAIN_SEEDS = {256: 5256, 4096: 9096}


def case_m(case: str) -> int:
    return int(case.lstrip("mu").rstrip("lohi"))


@functools.lru_cache(maxsize=None)
def density_curve(case: str) -> np.ndarray:
    """(4, m) density curve on [-4, 1.5]: monotone, slopes <= 1.5 (the roughness the end-to-end contract bears, hostile.roughen)."""
    rng = np.random.default_rng(_CURVE_SEEDS[case])
    kw = dict(v_lo=0.08, v_hi=3.6, max_slope=1.5, monotone=True)
    lut = hostile.curve(rng, case_m(case), uniform=True, **kw) if case[0] == "u" else hostile.curve(rng, case_m(case), axis="jitter", jitter=JITTER, **kw)
    lut.setflags(write=False)
    return lut


@functools.lru_cache(maxsize=None)
def grain_table(m: int) -> np.ndarray:
    """(4, m) grain LUT on a jittered axis [0, 4], an independent amplitude uniform(0.01, 0.06) at every breakpoint."""
    lut = hostile.grain_lut(np.random.default_rng(_GRAIN_SEEDS[m]), m, steps=None, amp=0.06, axis="jitter", jitter=JITTER)
    lut.setflags(write=False)
    return lut


# ------------------------------------------------------------------------------------------------ input conditions
def conditions(lut, x) -> dict:
    """What the model says of the look-ups at x (any shape): near flag, number of in-range samples (x0 < x < x1), and the share of
    those that take the corrective step down (-1) and up (+1)."""
    lut = np.asarray(lut)
    x = np.asarray(x, dtype=F32).ravel()
    x = x[(x > lut[0, 0]) & (x < lut[0, -1])]
    adj = curve_model.corrective(lut, x)
    n = max(x.size, 1)
    return {"near": curve_model.is_near(lut), "n": int(x.size), "down": float((adj == -1).sum()) / n, "up": float((adj == 1).sum()) / n,
            "x": x, "adj": adj}


def assert_conditions(case: str, lut, x) -> dict:
    """The conditions every test states of its inputs before it looks at a device result."""
    c = conditions(lut, x)
    m = lut.shape[1]
    assert c["near"] == 1, f"{case}: the model says this table is not `near`"
    assert c["n"] >= 500, (case, c["n"])
    if case[0] == "u":
        # the uniform control: a corrective step only where the guess's own rounding decides -- d = x - x0, d * inv_step and inv_step are
        # each good to 2^-24 relative, and linspace rounds a breakpoint by half an ulp of itself: together under 4 ulp of the axis range
        off = c["x"][c["adj"] != 0].astype(np.float64)
        xp = lut[0].astype(np.float64)
        dist = np.min(np.abs(off[:, None] - xp[None, :]), axis=1) if off.size else np.zeros(0)
        assert (dist <= 4.0 * np.spacing(F32(lut[0, -1] - lut[0, 0]))).all(), (case, float(dist.max()))
    elif m == 3:
        # one inner breakpoint: only the direction it moved against (see the module docstring)
        assert (c["up"] > 0 and c["down"] == 0) if case == "m3lo" else (c["down"] > 0 and c["up"] == 0), (case, c["down"], c["up"])
    else:
        assert c["down"] + c["up"] >= 0.10 and c["down"] >= 0.02 and c["up"] >= 0.02, (case, c["down"], c["up"])
    return c


# ------------------------------------------------------------------------------------------------ bounds
def local_slope(lut, x) -> np.ndarray:
    """max |slope| of the curve's cell at x and of its two neighbours, per channel of x (..., 3) (test_gpu_hostile._local_slope)."""
    xp = lut[0].astype(np.float64)
    dx = np.diff(xp)
    out = np.zeros(x.shape)
    for c in range(3):
        s = np.where(dx > 0, np.abs(np.diff(lut[1 + c].astype(np.float64))) / np.maximum(dx, 1e-300), 0.0)
        i = np.clip(np.searchsorted(xp, x[..., c].astype(np.float64), side="right") - 1, 0, len(xp) - 2)
        out[..., c] = np.maximum(np.maximum(s[np.maximum(i - 1, 0)], s[i]), s[np.minimum(i + 1, len(s) - 1)])
    return out


def density_bound(lut, loge, ref) -> np.ndarray:
    """test_density_curve_on_a_non_uniform_axis's bound: the contract plus the steepest slope around x times 4 ulp of the log (the
    device's v_log_f32-based log10 and NumPy's differ by an ulp or two)."""
    return 1e-5 * np.maximum(np.abs(ref), 1e-3) + local_slope(lut, loge) * 4.0 * np.spacing(np.abs(loge).astype(F32))


def interp64(lut, x) -> np.ndarray:
    """np.interp in float64 on the float32 arguments x (..., 3), not rounded."""
    xp = lut[0].astype(np.float64)
    return np.stack([np.interp(x[..., c].astype(np.float64), xp, lut[1 + c].astype(np.float64)) for c in range(3)], axis=-1)


def model_eval(lut, x, correct: bool) -> np.ndarray:
    return np.stack([curve_model.evaluate(lut, c, x[..., c], correct) for c in range(3)], axis=-1)


# ------------------------------------------------------------------------------------------------ sample sets
def _edge_rows(img):
    """The three edge rows of test_gpu_hostile._frame."""
    img[0, :5] = 0.0  # S < 1e-12 -> 0 (lut_2d.wgsl:24)
    img[1, :5] = 1e-9
    img[2, :5] = 60000.0
    return img


def _breakpoint_exposures(lut, room: int) -> np.ndarray:
    """float32(10 ** xp[k]) for every inner breakpoint k (an ulp or two off the breakpoint, on either side, once the log is taken
    again), one exposure below 10 ** x0 and one above 10 ** x1.  Where the frame has no room for all of them, an evenly strided subset."""
    xp = lut[0].astype(np.float64)
    e = (10.0 ** xp[1:-1]).astype(F32)
    ends = np.array([0.5 * 10.0 ** xp[0], 2.0 * 10.0 ** xp[-1]], dtype=F32)
    if e.size + 2 > room:
        e = e[np.round(np.linspace(0, e.size - 1, room - 2)).astype(int)]
    return np.concatenate([ends, e])


def _log_uniform(lut, seed: int, shape) -> np.ndarray:
    """Exposures whose log10 is uniform over the axis and a little beyond: every cell sees arguments all across it."""
    rng = np.random.default_rng(seed)
    return (10.0 ** rng.uniform(float(lut[0, 0]) - 0.1, float(lut[0, -1]) + 0.1, shape)).astype(F32)


def _place(lut, H: int, W: int, seed: int):
    """Where the aimed samples go: flat pixel range [3 W, 3 W + n) after the edge rows, at most 70 % of the frame's rows with them; then
    H // 4 rows of log-uniform exposures; the rest stays the synthetic frame."""
    e = _breakpoint_exposures(lut, (int(0.7 * H) - 3) * W)
    r0 = 3 + -(-e.size // W)
    r1 = r0 + H // 4
    assert r1 <= H
    return e, slice(3 * W, 3 * W + e.size), slice(r0, r1), _log_uniform(lut, seed, (r1 - r0, W, 3))


@functools.lru_cache(maxsize=None)
def front_case(case: str, H: int, W: int):
    """Sites 1-3: a flat 2-D LUT of ones and no matrix, so every channel's exposure is X + Y + Z (to an ulp); pixels (e/4, e/4, e/2)
    sum to e exactly (_place says where they go)."""
    lut = density_curve(case)
    neg, prt, _ = stocks()
    p = oracle_inputs(neg, prt, 100.0, halation=False, mtf=False, grain=0, matrix=False)
    p.lut_2d = np.ones((8, 8, 3), dtype=F32)
    p.lut_1d = lut
    img = _edge_rows(synthetic_frame(H, W, seed=300 + case_m(case)))
    e, aimed, rows, spread = _place(lut, H, W, 301 + case_m(case))
    img.reshape(-1, 3)[aimed] = np.stack([e / 4, e / 4, e / 2], axis=-1)
    img[rows] = spread / 3  # (three equal parts: every channel's exposure is the first channel's draw, to an ulp)
    img[rows, :, 1:] = img[rows, :, :1]
    loge = st.log_clip(st.apply_2d_lut(img, p.lut_2d))
    ref = st.multi_channel_interp(loge, lut)
    return SimpleNamespace(case=case, p=p, lut=lut, img=img, loge=loge, ref=ref, bound=density_bound(lut, loge, ref), n_aimed=int(e.size))


def _halation_inputs(case: str, H: int, W: int, scale: float):
    lut = density_curve(case)
    neg, prt, _ = stocks()
    p = oracle_inputs(neg, prt, scale, mtf=False, grain=0)
    p.lut_1d = lut
    img = _edge_rows(synthetic_frame(H, W, seed=500 + case_m(case)))
    expo = st.apply_2d_lut(st.apply_matrix3x3(img, p.matrix), p.lut_2d)
    # the blue channel of a colour stock's halation is one tap (effects.py:248-263): its argument of the log is the exposure itself
    e, aimed, rows, spread = _place(lut, H, W, 501 + case_m(case))
    expo.reshape(-1, 3)[aimed, 2] = e
    expo[rows] = spread
    return p, lut, img, expo, int(e.size)


@functools.lru_cache(maxsize=None)
def halation_case(case: str, H: int, W: int, scale: float):
    """Sites 4-7: exposure planes of a synthetic frame through the colour stock's own matrix and 2-D LUT, breakpoint exposures in the
    blue plane (the single-tap channel), the halation stage as test_gpu_parity.test_halation_stage calls it.  The log's argument is a
    stencil sum both sides round differently; the density curve's own bound holds all the same (the device uses a fifth of it), so it is
    not widened."""
    p, lut, img, expo, n_aimed = _halation_inputs(case, H, W, scale)
    loge = st.log_clip(st.halation(expo, p.halation_kernel))
    ref = st.multi_channel_interp(loge, lut)
    return SimpleNamespace(case=case, p=p, lut=lut, expo=expo, loge=loge, ref=ref, n_aimed=n_aimed, bound=density_bound(lut, loge, ref))


@functools.lru_cache(maxsize=None)
def split_front_case(case: str, H: int, W: int, scale: float):
    """Site 3b: the frame of halation_case's kind through a flat 2-D LUT (exposure = X + Y + Z), so the breakpoint exposures reach the
    identity channel the front kernel finishes; the reference is the oracle's density of that channel."""
    lut = density_curve(case)
    neg, prt, _ = stocks()
    p = oracle_inputs(neg, prt, scale, mtf=False, grain=0, matrix=False)
    p.lut_2d = np.ones((8, 8, 3), dtype=F32)
    p.lut_1d = lut
    img = _edge_rows(synthetic_frame(H, W, seed=700 + case_m(case)))
    e, aimed, rows, spread = _place(lut, H, W, 701 + case_m(case))
    img.reshape(-1, 3)[aimed] = np.stack([e / 4, e / 4, e / 2], axis=-1)
    img[rows] = spread / 3
    img[rows, :, 1:] = img[rows, :, :1]
    expo = st.apply_2d_lut(img, p.lut_2d)
    blue = st.correlate_reflect101(expo[..., 2], p.halation_kernel[..., 2])
    loge = np.repeat(st.log_clip(blue)[..., None], 3, axis=-1)  # (three copies: the bound helpers take (..., 3))
    ref = st.multi_channel_interp(loge, lut)
    return SimpleNamespace(case=case, p=p, lut=lut, img=img, loge=loge[..., 2:], ref=ref[..., 2], bound=density_bound(lut, loge, ref)[..., 2],
                           n_aimed=int(e.size))


GRAIN_SHAPE = (100, 140)
GRAIN_LOW = 0.35  # densities from here up stay 5 sigma x 0.06 off the clip at 0 (test_grain_lut_with_steps)


@functools.lru_cache(maxsize=None)
def grain_case(m: int, mono: bool):
    """Sites 8-10: densities in, out = max(D + G * lut(D), 0).  Rows: 0 a ramp 0.35 ... 4, 1 exact zeros, then the AIMED samples -- every
    inner breakpoint exactly, nextafter on both sides, x0, x1, one below 0 and one above 4 -- sorted, those under 0.35 (next to the clip)
    in rows of their own, then uniform(0.35, 4).  The 3-D LUT is the identity on [0, 4] (17 texels a side: every index product is exact),
    so the display value of the tail kernels is the grained density / 4 and the density bounds carry over."""
    H, W = GRAIN_SHAPE
    lut = grain_table(m)
    neg, prt, _ = stocks()
    p = oracle_inputs(neg, prt, 166.67, halation=False, mtf=False, grain=1 if mono else 2)
    p.grain_lut = lut
    g = np.arange(17, dtype=np.float64) / 16.0
    p.lut_3d = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).astype(F32)
    rng = np.random.default_rng(800 + m + int(mono))
    dens = rng.uniform(GRAIN_LOW, 4.0, (H, W, 3)).astype(F32)
    dens[0] = np.linspace(GRAIN_LOW, 4, W, dtype=F32)[:, None]
    dens[1] = 0.0
    xp = lut[0]
    aimed = np.sort(np.concatenate([xp[1:-1], np.nextafter(xp[1:-1], F32(-np.inf)), np.nextafter(xp[1:-1], F32(np.inf)),
                                    np.array([xp[0], xp[-1], -0.25, 4.5], dtype=F32)]))
    low, high = aimed[aimed < GRAIN_LOW], aimed[aimed >= GRAIN_LOW]
    per_row = 3 * W
    low = np.concatenate([low, np.full(-low.size % per_row, 0.2, dtype=F32)])
    high = np.concatenate([high, rng.uniform(GRAIN_LOW, 4.0, -high.size % per_row).astype(F32)])
    r_low, r_high = low.size // per_row, high.size // per_row
    assert 2 + r_low + r_high <= int(0.7 * H)
    dens[2:2 + r_low] = low.reshape(r_low, W, 3)
    dens[2 + r_low:2 + r_low + r_high] = high.reshape(r_high, W, 3)
    clip_rows = np.zeros(H, dtype=bool)
    clip_rows[1:2 + r_low] = True
    ref = st.apply_grain(dens, lut, p.grain_kernel, p.seed, mono)
    # test_grain_lut_with_steps's bounds: 1e-5 relative at the 1e-3 floor away from the clip; 3e-7 absolute on the zero-density row (the
    # field is good to 4e-6, times an amplitude of 0.06), which the rows of aimed samples under 0.35 share where 1e-5 of them is less
    bound = 1e-5 * np.maximum(np.abs(ref.astype(np.float64)), 1e-3)
    bound[clip_rows] = np.maximum(1e-5 * np.abs(ref[clip_rows].astype(np.float64)), 3e-7)
    bound[1] = 3e-7
    shown = st.apply_lut_tetrahedral(ref, p.lut_3d, 0.25)
    # display = min(density, 4) / 4 through four products and three sums of non-negative terms: a quarter of the bound + 4 ulp
    shown_bound = 0.25 * bound + 4.0 * np.spacing(np.abs(shown).astype(F32))
    return SimpleNamespace(m=m, mono=mono, p=p, lut=lut, dens=dens, ref=ref, bound=bound, shown=shown, shown_bound=shown_bound,
                           clip_rows=clip_rows, n_aimed=int(aimed.size))
