"""The two places where the device states that a product and a sum `round separately`, as plain NumPy float32 -- and, beside each, the
restatement a contracting compiler would make of it (the product kept exact inside a fused multiply-add), so that a test can show its
inputs tell the two apart.  Used by tests/test_gpu_rounding_order.py (the device against the separate form, bit for bit) and
tests/test_rounding_order_host.py (the proof, without a GPU, that those inputs have power).

  warp_lerp   the two-step bilinear lerp of warp_affine_kernel: top = t00 + ax * (t01 - t00), bot likewise, out = top + ay * (bot - top);
              taps and weights come from warp_taps, which restates oracle.stages.warp_affine_linear's coordinate code line by line (the
              host test holds warp_lerp(*warp_taps(...)) equal to that function)
  grain_add   the grain stage given its field: max(D + f32(G * a), 0)   (oracle.stages.apply_grain's last line)

The `separate` form is the definition.  The `fused` form does each `x + w * d` step in float64 -- the product of two float32 values is
exact there -- and rounds once (the differences t01 - t00 are float32 roundings of their own in both forms: no instruction fuses them).

Everything the two test modules share is built here once (lru_cache) and must not be modified by its users."""

from __future__ import annotations

import functools

import numpy as np

F32 = np.float32
F64 = np.float64


# ------------------------------------------------------------------------------------------------ warp
def warp_taps(img, m_dst_to_src, out_shape=None, offset=(0, 0)):
    """(t00, t01, t10, t11, ax, ay) of oracle.stages.warp_affine_linear: float32 source coordinates from separately rounded products
    and sums, the four taps (zero outside the frame) and the two lerp weights."""
    img = np.asarray(img, dtype=F32)
    H, W = img.shape[:2]
    oh, ow = (H, W) if out_shape is None else out_shape
    m = np.asarray(m_dst_to_src, dtype=F64).astype(F32)
    xf = (np.arange(ow) + offset[1]).astype(F32)[None, :]
    yf = (np.arange(oh) + offset[0]).astype(F32)[:, None]
    sx = (xf * m[0, 0] + yf * m[0, 1]) + m[0, 2]
    sy = (xf * m[1, 0] + yf * m[1, 1]) + m[1, 2]
    x0f, y0f = np.floor(sx), np.floor(sy)
    ax, ay = (sx - x0f)[..., None], (sy - y0f)[..., None]
    x0 = np.clip(x0f, -2, W + 1).astype(np.int64)
    y0 = np.clip(y0f, -2, H + 1).astype(np.int64)

    def tap(yy, xx):
        ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        v = img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1), :3]
        return np.where(ok[..., None], v, F32(0))

    return tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1), ax, ay


def _step(x, w, d, fused: bool):
    """x + w * d on float32 arrays: the product rounded, then the sum -- or, fused, both in float64 and one rounding."""
    x, w, d = np.asarray(x, F32), np.asarray(w, F32), np.asarray(d, F32)
    if fused:
        return (x.astype(F64) + w.astype(F64) * d.astype(F64)).astype(F32)
    return (x + (w * d).astype(F32)).astype(F32)


def warp_lerp(t00, t01, t10, t11, ax, ay, fused: bool = False):
    top = _step(t00, ax, (t01 - t00).astype(F32), fused)
    bot = _step(t10, ax, (t11 - t10).astype(F32), fused)
    return _step(top, ay, (bot - top).astype(F32), fused)


# ------------------------------------------------------------------------------------------------ grain
def grain_add(D, G, a, fused: bool = False):
    """max(D + f32(G * a), 0); D, G: (..., 3) float32, a: the per-channel amplitude (3,) or an array like D."""
    return np.maximum(_step(D, G, np.broadcast_to(np.asarray(a, F32), np.shape(D)), fused), F32(0))


def differing_share(a, b) -> float:
    """Share of the samples whose VALUES differ (+0 and -0 are one value)."""
    return float((np.asarray(a) != np.asarray(b)).mean())


# ------------------------------------------------------------------------------------------------ the inputs of the GPU tests
WARP_ANGLES = (0.3, 5.0, -33.0, 44.0, 90.0, 180.0)
WARP_OBLIQUE = (0.3, 5.0, -33.0, 44.0)  # at 90 and 180 degrees the weights are (all but) 0: nothing for a fused step to change
WARP_SHAPES = ((97, 131), (5, 7), (1, 9))
WARP_FRAMES = ("uniform", "mixed")
WARP_POWER_SHAPE = (97, 131)  # where the share condition is stated (the small shapes have a few dozen samples, many of them border)
WARP_MIN_SHARE = 0.10

GRAIN_SHAPES = ((64, 96), (37, 53))
GRAIN_SHARD = (9, 30)  # rows [y0, y1) of the (37, 53) frame
GRAIN_SCALE = 341.33  # px/mm: grain_size 6 is a 9 x 9 blob, grain_size 1 is finer than a pixel (a single tap of weight 1)
GRAIN_SIZES = (6.0, 1.0)
GRAIN_SEED = 4711
GRAIN_AMPLITUDES = (F32(0.04) * np.array([0.93, 0.73, 1.14], dtype=F32)).astype(F32)
GRAIN_MIN_SHARE = 0.05
GRAIN_MIN_CLIPPED = 0.01
GRAIN_ZERO_COLUMN = 5


@functools.lru_cache(maxsize=None)
def warp_frame(kind: str, H: int, W: int) -> np.ndarray:
    """"uniform": uniform(0, 4).  "mixed": 10 ** N(0, 4 / 3) kept inside [1e-4, 1e4] (three sigma), a quarter of the samples negated:
    differences that cancel, differences that do not, and products of every size; all finite."""
    rng = np.random.default_rng(8 + 1000 * H + W)
    if kind == "uniform":
        img = rng.uniform(0, 4, (H, W, 3)).astype(F32)
    else:
        img = (10.0 ** np.clip(rng.normal(0.0, 4.0 / 3.0, (H, W, 3)), -4.0, 4.0)).astype(F32)
        img = np.where(rng.random((H, W, 3)) < 0.25, -img, img).astype(F32)
    assert np.isfinite(img).all()
    img.setflags(write=False)
    return img


def with_layout(img, layout: str) -> np.ndarray:
    H, W = img.shape[:2]
    if layout == "hwc3":
        return np.ascontiguousarray(img)
    if layout == "hwc4":
        return np.concatenate([img, np.ones((H, W, 1), F32)], axis=-1)
    return np.ascontiguousarray(img.transpose(2, 0, 1))


@functools.lru_cache(maxsize=None)
def flat_grain_lut() -> np.ndarray:
    """(4, 16) on the axis [0, 4], every channel constant at its amplitude: y0 + t * (y1 - y0) with y1 == y0 is y0 whatever t is, so the
    look-up returns the amplitude exactly and only the add is under test.  The amplitudes are not dyadic: their products round."""
    lut = np.empty((4, 16), F32)
    lut[0] = np.linspace(0.0, 4.0, 16, dtype=F32)
    lut[1:] = GRAIN_AMPLITUDES[:, None]
    assert all(np.frexp(float(a))[0] != 0.5 for a in GRAIN_AMPLITUDES)
    lut.setflags(write=False)
    return lut


@functools.lru_cache(maxsize=None)
def grain_density(H: int, W: int) -> np.ndarray:
    """uniform(0, 0.25) -- the grain term is about 0.04 x N(0, 1), so the sum's rounding step is near the product's and a good many
    samples go below 0 and clip -- with one column of exact zeros."""
    rng = np.random.default_rng(600 + H + W)
    dens = rng.uniform(0.0, 0.25, (H, W, 3)).astype(F32)
    dens[:, GRAIN_ZERO_COLUMN] = 0.0
    dens.setflags(write=False)
    return dens


def grain_inputs(grain_size: float, mono: bool):
    """oracle_inputs for the grain tests: the stand-in stock's 3-D LUT, this module's flat grain LUT, the grain stencil of `grain_size`
    microns at GRAIN_SCALE (None -> the single tap of weight 1 the device substitutes)."""
    from helpers import oracle_inputs, stocks

    neg, prt, _ = stocks()
    p = oracle_inputs(neg, prt, GRAIN_SCALE, halation=False, mtf=False, grain=1 if mono else 2, seed=GRAIN_SEED, grain_size=grain_size)
    p.grain_lut = flat_grain_lut()
    if p.grain_kernel is None:
        p.grain_kernel = np.ones((1, 1), F32)
    return p


def grain_conditions(D, G) -> dict:
    """What the separate model alone says of the inputs: the share of samples a fused add would change, and the share that clips at 0."""
    sep, fus = grain_add(D, G, GRAIN_AMPLITUDES), grain_add(D, G, GRAIN_AMPLITUDES, fused=True)
    unclipped = _step(D, G, np.broadcast_to(GRAIN_AMPLITUDES, np.shape(D)), False)
    return {"share": differing_share(sep, fus), "clipped": float((unclipped < 0).mean()), "zero_col_clipped": int((unclipped[:, GRAIN_ZERO_COLUMN] < 0).sum())}
