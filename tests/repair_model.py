"""The hot-pixel repair of a mosaic (include/r2f.h: r2f_mosaic_repair) restated in NumPy: the neighbour rule N, step T, the hot test
H.  The references of tests/test_repair_host.py, tests/test_gpu_repair*.py.  Written from the header's text, with whole-array
operations, not from the C++.

    repair(raw, P, black, threshold, q, min_neighbours, cfa=None) -> (out uint16 (H, W), replaced: bool (H, W))

black: P * P levels per phase (y % P) * P + x % P; cfa: the 36 colour ids of an X-Trans pattern (rows of 6), for P = 6.
"""

from __future__ import annotations

import numpy as np

CANONICAL = ("GBGGRG", "RGRBGB", "GBGGRG", "GRGGBG", "BGBRGR", "GRGGBG")
BAYER = ((-2, 0), (0, 2), (2, 0), (0, -2))  # up, right, down, left
LATERAL = {1: (0, 1), 2: (0, 1, -1, 2)}  # a over -r < a <= r, in the header's order


def cfa_ids(pattern=CANONICAL, dy=0, dx=0):
    """The 6 x 6 colour ids (R, G, B = 0, 1, 2) of `pattern` shifted cyclically: the array of a frame whose (0, 0) is the pattern's (dy, dx)."""
    ids = np.array([["RGB".index(c) for c in row] for row in pattern], np.int32)
    return np.roll(ids, (-dy, -dx), (0, 1))


def shifted_pattern(dy, dx):
    """The six strings of the canonical pattern shifted by (dy, dx), as an XTransProfile takes them."""
    return tuple("".join("RGB"[v] for v in row) for row in cfa_ids(CANONICAL, dy, dx))


def candidates(d, r):
    """Ring r's candidates of quadrant d (0 .. 3 = up, right, down, left), in order."""
    return [((-r, a), (a, r), (r, -a), (-a, -r))[d] for a in LATERAL[r]]


def neighbour_table(P, cfa=None):
    """[phase][d] -> (dy, dx), or None where ring 2 holds no sample of the centre's colour."""
    if P == 2:
        return [list(BAYER) for _ in range(4)]
    cfa = np.asarray(cfa).reshape(6, 6)
    table = []
    for py in range(6):
        for px in range(6):
            row = []
            for d in range(4):
                hit = None
                for r in (1, 2):
                    for dy, dx in candidates(d, r):
                        if hit is None and cfa[(py + dy) % 6, (px + dx) % 6] == cfa[py, px]:
                            hit = (dy, dx)
                row.append(hit)
            table.append(row)
    return table


def black_plane(black, P, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.asarray(black, np.int64)[(yy % P) * P + xx % P]


def repair(raw, P, black, threshold, q, min_neighbours, cfa=None):
    raw = np.asarray(raw)
    assert raw.dtype == np.uint16 and raw.ndim == 2 and P in (2, 6) and len(black) == P * P
    H, W = raw.shape
    table = neighbour_table(P, cfa)
    assert all(n is not None for row in table for n in row), "the planner refuses this pattern"
    levels = black_plane(black, P, H, W)
    t = np.maximum(raw.astype(np.int64) - levels, 0)  # T
    yy, xx = np.mgrid[0:H, 0:W]
    phase = (yy % P) * P + xx % P
    inside = np.ones((H, W), bool)
    below_n = np.zeros((H, W), np.int64)
    best = np.zeros((H, W), np.int64)
    tp = np.pad(t, 2)  # (a neighbour outside the frame: its centre is never hot, whatever this zero says)
    for d in range(4):
        dy = np.array([table[p][d][0] for p in range(P * P)])[phase]
        dx = np.array([table[p][d][1] for p in range(P * P)])[phase]
        ny, nx = yy + dy, xx + dx
        inside &= (ny >= 0) & (ny < H) & (nx >= 0) & (nx < W)
        tk = tp[ny + 2, nx + 2]
        below = q * t > 256 * tk  # H
        below_n += below
        best = np.where(below, np.maximum(best, tk), best)
    hot = inside & (t > threshold) & (below_n >= min_neighbours)
    out = np.where(hot, np.clip(best + levels, 0, 65535), raw).astype(np.uint16)
    return out, hot


def field(shape, seed, black=(512, 520, 500, 512)):
    """The random field of the GPU tests: a background uniform in [500, 900) with a tenth of the samples replaced by uniform
    values in [5000, 65536)."""
    rng = np.random.default_rng(seed)
    frame = rng.integers(500, 900, shape)
    hot = rng.random(shape) < 0.1
    return np.where(hot, rng.integers(5000, 65536, shape), frame).astype(np.uint16)
