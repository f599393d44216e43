"""NumPy restatement of include/r2f.h's step M: the median filter of the colour differences (LibRaw's med_passes), between B / B'
and Blend of either demosaic.  `passes` is the definition on whole (3, out_h, out_w) integer planes -- the fifth of the nine
shifted difference planes sorted along their own axis --, `passes_slow` the same read pixel by
pixel with sorted().  Composes with highlight_model.py (planes, blend, orient) and the two demosaic models' `colour`.

Plain module, no fixtures of pytest's."""

from __future__ import annotations

import numpy as np

import demosaic_model as dm
import highlight_model as hm
import xtrans_model as xm

MAX_PASSES = 4


def one_pass(p):
    """I_{k-1} -> I_k: (3, h, w) int64 planes in [0, 65535].  A frame with a side below 3 has no interior and is returned as it is."""
    p = np.asarray(p).astype(np.int64)
    _, h, w = p.shape
    out = p.copy()
    if h < 3 or w < 3:
        return out
    g = p[1]
    for c in (0, 2):
        d = p[c] - g
        nine = np.stack([d[1 + j:h - 1 + j, 1 + i:w - 1 + i] for j in (-1, 0, 1) for i in (-1, 0, 1)])
        med = np.sort(nine, axis=0)[4]
        out[c, 1:-1, 1:-1] = np.clip(med + g[1:-1, 1:-1], 0, 65535)
    return out


def passes(p, n, stats=None):
    """I_0 -> I_n.  stats: per pass the share of interior pixels it changed (`changed`), and over all passes how often the clamp
    engaged at either end per channel (`clamp_low`, `clamp_high`, `interior`: counts)."""
    assert isinstance(n, int) and 0 <= n <= MAX_PASSES
    p = np.asarray(p).astype(np.int64)
    assert p.shape[0] == 3 and p.min(initial=0) >= 0 and p.max(initial=0) <= 65535
    for _ in range(n):
        q = one_pass(p)
        if stats is not None and p.shape[1] >= 3 and p.shape[2] >= 3:
            inner = (slice(None), slice(1, -1), slice(1, -1))
            stats.setdefault("changed", []).append(float((q[inner] != p[inner]).any(axis=0).mean()))
            g = p[1]
            _, h, w = p.shape
            for c in (0, 2):
                d = p[c] - g
                nine = np.stack([d[1 + j:h - 1 + j, 1 + i:w - 1 + i] for j in (-1, 0, 1) for i in (-1, 0, 1)])
                raw = np.sort(nine, axis=0)[4] + g[1:-1, 1:-1]
                stats["clamp_low"] = stats.get("clamp_low", 0) + int((raw < 0).sum())
                stats["clamp_high"] = stats.get("clamp_high", 0) + int((raw > 65535).sum())
                stats["interior"] = stats.get("interior", 0) + int(raw.size)
        p = q
    return p


def passes_slow(p, n):
    """`passes` read from the definition one pixel at a time: sorted() of the nine differences, the fifth, plus green, clamped."""
    p = [[[int(v) for v in row] for row in plane] for plane in np.asarray(p)]
    h, w = len(p[0]), len(p[0][0])
    g = p[1]
    for _ in range(n):
        nxt = [[row[:] for row in plane] for plane in p]  # (every pass reads only the pass before it)
        for c in (0, 2):
            for y in range(1, h - 1):
                for x in range(1, w - 1):
                    nine = sorted(p[c][y + j][x + i] - g[y + j][x + i] for j in (-1, 0, 1) for i in (-1, 0, 1))
                    nxt[c][y][x] = min(max(nine[4] + g[y][x], 0), 65535)
        p = nxt
    return np.array(p, dtype=np.int64)


def demosaic(mosaic, profile_or_constants, n, clip=None, half_size=False, xtrans=False, stats=None):
    """Either demosaic's definition with step M and then Blend ahead of step C: uint16 (H, W) -> uint16 (out_h, out_w, 3).
    clip=None: no Blend; n = 0: highlight_model.demosaic."""
    m = xm if xtrans else dm
    H, W = mosaic.shape
    c = profile_or_constants if hasattr(profile_or_constants, "cfa") else m.constants(profile_or_constants, H, W, half_size)
    p = passes(hm.planes(mosaic, c, xtrans), n, stats)
    if clip is not None:
        p = hm.blend(p, clip)
    return m.colour(p, c)


def source_rows(y0, y1, n, out_h, H, reach, reduction):
    """The mosaic rows [lo, hi) that rows [y0, y1) of D read (include/r2f.h, step M's reach): reduction = 0 for the full size."""
    a, b = max(y0 - n, 0), min(y1 + n, out_h)
    if reduction:
        return reduction * a, reduction * b
    return max(a - reach, 0), min(b + reach, H)
