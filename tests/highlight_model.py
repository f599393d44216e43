"""NumPy restatement of include/r2f.h's highlight modes: Scale with a highlight mode (r2f_raw_scale_plan_highlight) and Blend
(mosaic::blend_pixel, between the interpolation and step C of either demosaic).  Every fp32 operation is its own rounded NumPy
float32 step, written from the definition's matrices T and I as they stand -- the zeros and ones are multiplied out here, not
simplified away as the kernel's text does.  Composes with demosaic_model.py, xtrans_model.py and levels_model.py.

`blend(..., fused=True)` is the restatement a contracting compiler would make of it (each product that feeds a sum kept exact, one
rounding for the pair): what tests/test_highlight_host.py shows the bit-for-bit tests can tell apart.

Plain module, no fixtures of pytest's; `patches()`, `bayer_case()` and `xtrans_case()` make the mosaics the GPU tests share."""

from __future__ import annotations

import zlib

import numpy as np

import demosaic_model as dm
import levels_model as lm
import xtrans_model as xm

CLIP, UNCLIP, BLEND = 0, 1, 2
F = np.float32
SQRT3, HALF_SQRT3 = F(float.fromhex("0x1.bb67aep+0")), F(float.fromhex("0x1.bb67aep-1"))
T = np.array([[1, 1, 1], [SQRT3, -SQRT3, 0], [-1, -1, 2]], dtype=F)
I = np.array([[1, HALF_SQRT3, -0.5], [1, -HALF_SQRT3, -0.5], [1, 0, 1]], dtype=F)
assert float(SQRT3) == float(F(1.7320508)) and float(HALF_SQRT3) == float(F(0.8660254))


def scale(white_balance, white_level, thr, black, d, mode):
    """(mul[3] as doubles, maximum_used, adjusted, clip), or None for what the definition refuses (m < 1, an unknown mode, clip < 1).
    clip is 0 for modes 0 and 1."""
    if mode not in (CLIP, UNCLIP, BLEND):
        return None
    base = lm.scale(white_balance, white_level, thr, black, d)
    if base is None:
        return None
    if mode == CLIP:
        return (*base, 0)
    _, m_eff, adjusted = base
    wb = [float(v) for v in white_balance]
    hi = max(wb)
    mul = tuple(v / hi * 65535.0 / m_eff for v in wb)
    clip = 0
    if mode == BLEND:
        clip = min(int(np.trunc(F(65535.0) * F(v / hi))) for v in wb)  # one fp32 multiply per channel
        if clip < 1:
            return None
    return mul, m_eff, adjusted, clip


def _dot3(m, k, v, fused):
    """((m[k][0] v[0]) + m[k][1] v[1]) + m[k][2] v[2], each operation rounded to fp32; fused: a product that feeds a sum is exact."""
    if not fused:
        acc = m[k, 0] * v[0]
        acc = acc + m[k, 1] * v[1]
        return acc + m[k, 2] * v[2]
    d = [x.astype(np.float64) for x in v]  # (a product of two floats is exact in double, and so is one rounding of product + sum)
    acc = (np.float64(m[k, 0]) * d[0]).astype(F)
    acc = (acc.astype(np.float64) + np.float64(m[k, 1]) * d[1]).astype(F)
    return (acc.astype(np.float64) + np.float64(m[k, 2]) * d[2]).astype(F)


def blend(planes, clip, stats=None, fused=False):
    """Blend of (3, ...) integer planes in [0, 65535] -> int64 planes of the same shape.  stats: the classes of pixels met."""
    p = np.asarray(planes).astype(np.int64)
    assert p.shape[0] == 3 and p.min(initial=0) >= 0 and p.max(initial=0) <= 65535 and 1 <= clip <= 65535
    above = (p > clip).sum(axis=0)
    hit = above > 0
    out = p.copy()
    if stats is not None:
        for n in (1, 2, 3):
            stats[f"above_{n}"] = stats.get(f"above_{n}", 0) + int((above == n).sum())
        stats["at_clip"] = stats.get("at_clip", 0) + int(((p == clip).any(axis=0) & ~hit).sum())
        stats["pixels"] = stats.get("pixels", 0) + int(hit.size)
        stats["blended"] = stats.get("blended", 0) + int(hit.sum())
    if not hit.any():
        return out
    v = p[:, hit]
    cam = [[v[c].astype(F) for c in range(3)], [np.minimum(v[c].astype(F), F(clip)) for c in range(3)]]
    with np.errstate(divide="ignore", invalid="ignore"):
        lab = [[_dot3(T, k, cam[i], fused) for k in range(3)] for i in range(2)]
        if fused:
            s = []
            for i in range(2):
                a, b = lab[i][1].astype(np.float64), lab[i][2].astype(np.float64)
                s.append(((a * a).astype(F).astype(np.float64) + b * b).astype(F))  # fma(b, b, fl(a a))
        else:
            s = [lab[i][1] * lab[i][1] + lab[i][2] * lab[i][2] for i in range(2)]
        assert all(x.dtype == F for x in s)
        zero = s[0] == 0
        ratio = np.where(zero, F(1), np.sqrt(np.where(zero, F(1), s[1] / np.where(zero, F(1), s[0])).astype(F))).astype(F)
    if stats is not None:
        stats["sum0_zero"] = stats.get("sum0_zero", 0) + int(zero.sum())
    l0 = [lab[0][0], lab[0][1] * ratio, lab[0][2] * ratio]
    assert all(x.dtype == F for x in l0)
    res = np.empty_like(v)
    for c in range(3):
        acc = _dot3(I, c, l0, fused) / F(3.0)
        assert acc.dtype == F and np.isfinite(acc).all()
        res[c] = np.clip(np.trunc(acc).astype(np.int64), 0, 65535)
    out[:, hit] = res
    return out


def blend_pixel(v, clip, fused=False):
    """One pixel: (v0, v1, v2) -> a tuple of three ints."""
    return tuple(int(x) for x in blend(np.array(v, dtype=np.int64).reshape(3, 1), clip, fused=fused)[:, 0])


def planes(mosaic, c, xtrans):
    """The three integer planes ahead of step C (B / B'), from either model: (3, out_h, out_w) int64."""
    m = xm if xtrans else dm
    S = m.scale(np.asarray(mosaic), c)
    if xtrans:
        return m.reduced_planes(S, c) if c.reduced else m.planes(S, c)
    return m.half_planes(S, c) if c.half_size else m.planes(S, c)


def demosaic(mosaic, profile_or_constants, clip, half_size=False, xtrans=False, stats=None):
    """Either demosaic's definition with Blend ahead of step C: uint16 (H, W) -> uint16 (out_h, out_w, 3).  clip=None: no Blend."""
    m = xm if xtrans else dm
    H, W = mosaic.shape
    c = profile_or_constants if hasattr(profile_or_constants, "cfa") else m.constants(profile_or_constants, H, W, half_size)
    p = planes(mosaic, c, xtrans)
    if clip is not None:
        p = blend(p, clip, stats)
    return m.colour(p, c)


def orient(D, o):
    """The oriented frame O of include/r2f.h from the demosaiced frame D."""
    E = D
    if o & 2:
        E = E[::-1]
    if o & 1:
        E = E[:, ::-1]
    if o & 4:
        E = E.transpose(1, 0, 2)
    return np.ascontiguousarray(E)


# ---- fixtures
WB = (2.1, 1.0, 1.6)
TILE_W, TILE_H = dm.TILE_W, dm.TILE_H
ONE_TILE = (TILE_H + 6, TILE_W + 6)  # one ragged tile: (38, 70), even sides, 2 and 1 modulo 3
BAYER_FRAME = (2 * TILE_H - 6, 3 * TILE_W - 10)  # 2 x 3 ragged tiles, even sides: (58, 182)
XTRANS_FRAME = (2 * TILE_H - 5, 3 * TILE_W - 7)  # 2 x 3 ragged tiles, sides 2 modulo 3: (59, 185)
CLIP_EQUAL = 30200


def patches(H, W, tag, clip, low=2000, high=24000, share=0.45):
    """A uint16 (H, W) mosaic: a smooth field in [low, high), below `clip`, plus compact elliptic patches over about `share` of it.
    Patches cycle through five kinds: every sample exactly `clip`; samples scattered 400 either side of `clip` (one, two or three
    channels of a pixel end above it); a uniform 45000; samples around 52000; a uniform 65535 -- uniform patches leave equal channels
    under equal multipliers."""
    rng = np.random.default_rng(zlib.crc32(f"highlight/{tag}/{H}x{W}".encode()))
    y, x = np.mgrid[0:H, 0:W]
    field = low + (high - low) * (0.5 + 0.25 * np.sin(y / 5.0) + 0.25 * np.cos(x / 7.0))
    m = (field + rng.integers(-300, 300, (H, W))).clip(0, high)
    kinds = ((clip, 0), (clip, 400), (45000, 0), (52000, 3000), (65535, 0))
    n = max(5, int(share * H * W / 120))
    for i in range(n):
        cy, cx, ry, rx = rng.integers(0, H), rng.integers(0, W), rng.integers(4, 9), rng.integers(5, 11)
        inside = ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1
        level, spread = kinds[i % len(kinds)]
        m[inside] = (level + (rng.integers(-spread, spread + 1, (H, W)) if spread else 0))[inside] if spread else level
    return m.clip(0, 65535).astype(np.uint16)


def bayer_case(kind, pattern, shape):
    """(mosaic, numeric RawProfile, clip).  "equal": equal multipliers and no black level, so that every class of pixel occurs (three
    equal channels above clip among them); "wb": the multipliers and the clip level that Scale with mode 2 yields for WB on a 16-bit
    sensor -- green never exceeds clip there, as on a camera."""
    from raw2film_amd.raw import RawProfile

    if kind == "equal":
        return patches(*shape, f"bayer/{pattern}", CLIP_EQUAL), RawProfile(pattern, matrix=dm.CAMERA), CLIP_EQUAL
    mul, _, _, clip = scale(WB, 65535, 0.0, (64, 60, 66, 64), 0, BLEND)
    return patches(*shape, f"bayer/wb/{pattern}", clip), RawProfile(pattern, black=(64, 60, 66, 64), multipliers=mul, matrix=dm.CAMERA), clip


def xtrans_case(kind, pattern, shape):
    """bayer_case for an X-Trans pattern."""
    from raw2film_amd.raw import XTransProfile

    if kind == "equal":
        return patches(*shape, f"xtrans/{''.join(pattern)}", CLIP_EQUAL), XTransProfile(pattern, matrix=xm.CAMERA), CLIP_EQUAL
    mul, _, _, clip = scale(WB, 65535, 0.0, (1024,) * 36, 0, BLEND)
    return patches(*shape, f"xtrans/wb/{''.join(pattern)}", clip), XTransProfile(pattern, black=1024, multipliers=mul, matrix=xm.CAMERA), clip


CLASSES = ("above_1", "above_2", "above_3", "sum0_zero", "at_clip")
MIN_BLENDED = 0.10
