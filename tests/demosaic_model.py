"""NumPy restatement of the Bayer demosaic's definition (include/r2f.h, r2f_demosaic_u16): step A (black / scale), B0 (border
ring), B1 (green), B2 / B3 (red and blue), B' (half size) and C (matrix, clip).

Two forms of step B: `planes` is vectorised and pass-parallel (every pass reads the planes the passes before it left);
`planes_sequential` is a literal per-pixel evaluation in place, pass after pass, pixel after pixel in reading order, for tiny
frames.  The definition says that the two agree; tests/test_demosaic_host.py checks it.  The constants come straight from the
RawProfile here, not from the planner: the planner's are compared with them.

Plain module, no fixtures of pytest's; `fixture()` makes the mosaics and profiles the tests share."""

from __future__ import annotations

import zlib
from types import SimpleNamespace

import numpy as np

from raw2film_amd.raw import RawProfile

R, G, B = 0, 1, 2
PATTERNS = ("RGGB", "BGGR", "GRBG", "GBRG")
TILE_W, TILE_H = 64, 32  # R2F_DEMOSAIC_TILE_W / _H


def constants(profile: RawProfile, H: int, W: int, half_size: bool = False):
    """The definition's constants from the profile: cfa[4], int black[4], float32 mul[4], float32 M[3][3], the output's size."""
    cfa = tuple("RGB".index(c) for c in profile.pattern)
    return SimpleNamespace(cfa=cfa, black=np.array([int(b) for b in profile.black], dtype=np.int64),
                           mul=np.array(profile.multipliers, dtype=np.float64).astype(np.float32),
                           M=np.array(profile.matrix, dtype=np.float64).astype(np.float32), half_size=bool(half_size),
                           out_h=H // 2 if half_size else H, out_w=W // 2 if half_size else W)


def from_params(p):
    """The same record from an r2f_demosaic_params."""
    return SimpleNamespace(cfa=tuple(p.cfa), black=np.array(list(p.black), dtype=np.int64), mul=np.array(list(p.mul), dtype=np.float32),
                           M=np.array(list(p.M), dtype=np.float32).reshape(3, 3), half_size=bool(p.half_size), out_h=int(p.out_h),
                           out_w=int(p.out_w))


def site_map(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return (y & 1) * 2 + (x & 1)


def colour_map(c, H, W):
    return np.array(c.cfa, dtype=np.int64)[site_map(H, W)]


def _count(stats, key, mask):
    if stats is not None:
        stats[key] = stats.get(key, 0) + int(np.count_nonzero(mask))


def scale(mosaic, c, stats=None):
    """A: int64 (H, W) in [0, 65535]."""
    H, W = mosaic.shape
    k = site_map(H, W)
    t = mosaic.astype(np.int64) - c.black[k]
    f = t.astype(np.float32) * c.mul[k]  # one fp32 multiply
    v = np.trunc(f).astype(np.int64)
    _count(stats, "a_negative", t < 0)
    _count(stats, "a_clip_65535", v > 65535)
    return np.clip(v, 0, 65535)


def _ring(H, W, width):
    y, x = np.mgrid[0:H, 0:W]
    return (y < width) | (y >= H - width) | (x < width) | (x >= W - width)


def _shifter(H, W, pad=4):
    def sh(a, dy, dx, fill=0):
        p = np.full((H + 2 * pad, W + 2 * pad), fill, dtype=a.dtype)
        p[pad:pad + H, pad:pad + W] = a
        return p[pad + dy:pad + dy + H, pad + dx:pad + dx + W]
    return sh


def planes(S, c, stats=None):
    """B, vectorised: the (3, H, W) int64 planes of the scaled mosaic S."""
    H, W = S.shape
    col = colour_map(c, H, W)
    sh = _shifter(H, W)
    ring3, ring1 = _ring(H, W, 3), _ring(H, W, 1)
    # B0 everywhere (used in the ring only)
    b0 = []
    for cc in range(3):
        own = (col == cc).astype(np.int64)
        s = sum(sh(S * own, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
        n = sum(sh(own, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
        b0.append(np.where(n > 0, s // np.maximum(n, 1), 0))
    # B1
    guess, diff, lo, hi = [], [], [], []
    for dy, dx in ((0, 1), (1, 0)):
        m1, p1, m2, p2, m3, p3 = (sh(S, k * dy, k * dx) for k in (-1, 1, -2, 2, -3, 3))
        guess.append(2 * (m1 + S + p1) - m2 - p2)
        diff.append(3 * (np.abs(m2 - S) + np.abs(p2 - S) + np.abs(m1 - p1)) + 2 * (np.abs(p3 - p1) + np.abs(m3 - m1)))
        lo.append(np.minimum(m1, p1))
        hi.append(np.maximum(m1, p1))
    v = diff[0] > diff[1]
    gq = np.where(v, guess[1], guess[0]) >> 2
    glo, ghi = np.where(v, lo[1], lo[0]), np.where(v, hi[1], hi[0])
    b1_sites = (col != G) & ~ring3
    _count(stats, "b1_vertical", b1_sites & v)
    _count(stats, "b1_horizontal", b1_sites & ~v)
    _count(stats, "b1_tie", b1_sites & (diff[0] == diff[1]))
    _count(stats, "b1_clamp_low", b1_sites & (gq < glo))
    _count(stats, "b1_clamp_high", b1_sites & (gq > ghi))
    green = np.where(col == G, S, np.where(ring3, b0[G], np.clip(gq, glo, ghi)))
    out = [np.where(col == R, S, b0[R]), green, np.where(col == B, S, b0[B])]

    def clip(v_, where):
        _count(stats, "b23_clip_0", where & (v_ < 0))
        _count(stats, "b23_clip_65535", where & (v_ > 65535))
        return np.clip(v_, 0, 65535)

    # B2
    b2_sites = (col == G) & ~ring1
    for dy, dx in ((0, 1), (1, 0)):
        val = clip((sh(S, -dy, -dx) + sh(S, dy, dx) + 2 * S - sh(green, -dy, -dx) - sh(green, dy, dx)) >> 1, b2_sites)
        ncol = sh(col, dy, dx, -1)
        for cc in (R, B):
            out[cc] = np.where(b2_sites & (ncol == cc), val, out[cc])
    # B3
    b3_sites = (col != G) & ~ring1
    gs, ds = [], []
    for dx in (1, -1):
        sm, sp, gm, gp = sh(S, -1, -dx), sh(S, 1, dx), sh(green, -1, -dx), sh(green, 1, dx)
        ds.append(np.abs(sm - sp) + np.abs(gm - green) + np.abs(gp - green))
        gs.append(sm + sp + 2 * green - gm - gp)
    tie = ds[0] == ds[1]
    _count(stats, "b3_tie", b3_sites & tie)
    val = clip(np.where(tie, (gs[0] + gs[1]) >> 2, np.where(ds[0] > ds[1], gs[1], gs[0]) >> 1), b3_sites)
    out[R] = np.where(b3_sites & (col == B), val, out[R])
    out[B] = np.where(b3_sites & (col == R), val, out[B])
    return np.stack(out)


def planes_sequential(S, c):
    """B, literally: one image of three planes filled in place, pass after pass, pixel after pixel in reading order."""
    H, W = S.shape
    col = colour_map(c, H, W)
    img = [[[0, 0, 0] for _ in range(W)] for _ in range(H)]
    for y in range(H):
        for x in range(W):
            img[y][x][col[y, x]] = int(S[y, x])
    clip = lambda v: min(max(v, 0), 65535)  # noqa: E731
    for y in range(H):  # B0
        for x in range(W):
            if not (y < 3 or y >= H - 3 or x < 3 or x >= W - 3):
                continue
            for cc in range(3):
                if cc == col[y, x]:
                    continue
                s = n = 0
                for yy in range(max(y - 1, 0), min(y + 2, H)):
                    for xx in range(max(x - 1, 0), min(x + 2, W)):
                        if col[yy, xx] == cc:
                            s, n = s + img[yy][xx][cc], n + 1
                img[y][x][cc] = s // n if n else 0
    for y in range(3, H - 3):  # B1
        for x in range(3, W - 3):
            f = col[y, x]
            if f == G:
                continue
            guess, diff = [], []
            for dy, dx in ((0, 1), (1, 0)):
                px = lambda k, cc: img[y + k * dy][x + k * dx][cc]  # noqa: E731
                guess.append(2 * (px(-1, G) + px(0, f) + px(1, G)) - px(-2, f) - px(2, f))
                diff.append(3 * (abs(px(-2, f) - px(0, f)) + abs(px(2, f) - px(0, f)) + abs(px(-1, G) - px(1, G)))
                            + 2 * (abs(px(3, G) - px(1, G)) + abs(px(-3, G) - px(-1, G))))
            d = 1 if diff[0] > diff[1] else 0
            dy, dx = ((0, 1), (1, 0))[d]
            a, b = img[y - dy][x - dx][G], img[y + dy][x + dx][G]
            img[y][x][G] = min(max(guess[d] >> 2, min(a, b)), max(a, b))
    for y in range(1, H - 1):  # B2
        for x in range(1, W - 1):
            if col[y, x] != G:
                continue
            for dy, dx in ((0, 1), (1, 0)):
                cc = col[y + dy, x + dx]
                img[y][x][cc] = clip((img[y - dy][x - dx][cc] + img[y + dy][x + dx][cc] + 2 * img[y][x][G]
                                      - img[y - dy][x - dx][G] - img[y + dy][x + dx][G]) >> 1)
    for y in range(1, H - 1):  # B3
        for x in range(1, W - 1):
            if col[y, x] == G:
                continue
            cc = 2 - col[y, x]
            guess, diff = [], []
            for dx in (1, -1):
                m, p = img[y - 1][x - dx], img[y + 1][x + dx]
                diff.append(abs(m[cc] - p[cc]) + abs(m[G] - img[y][x][G]) + abs(p[G] - img[y][x][G]))
                guess.append(m[cc] + p[cc] + 2 * img[y][x][G] - m[G] - p[G])
            img[y][x][cc] = clip(guess[1 if diff[0] > diff[1] else 0] >> 1) if diff[0] != diff[1] else clip((guess[0] + guess[1]) >> 2)
    return np.array(img, dtype=np.int64).transpose(2, 0, 1)


def half_planes(S, c):
    """B': (3, H / 2, W / 2)."""
    quad = [S[(k >> 1)::2, (k & 1)::2] for k in range(4)]
    out = [None, 0, None]
    for k in range(4):
        if c.cfa[k] == G:
            out[G] = out[G] + quad[k]
        else:
            out[c.cfa[k]] = quad[k]
    out[G] = out[G] >> 1
    return np.stack(out)


def colour(p, c, stats=None):
    """C: (3, h, w) planes -> uint16 (h, w, 3)."""
    r, g, b = (p[i].astype(np.float32) for i in range(3))
    out = np.empty(p.shape[1:] + (3,), dtype=np.uint16)
    for k in range(3):
        acc = r * c.M[k, 0]
        acc = acc + g * c.M[k, 1]
        acc = acc + b * c.M[k, 2]
        assert acc.dtype == np.float32
        v = np.trunc(acc).astype(np.int64)
        _count(stats, "c_clip_0", v < 0)
        _count(stats, "c_clip_65535", v > 65535)
        out[..., k] = np.clip(v, 0, 65535)
    return out


def demosaic(mosaic, profile_or_constants, half_size=False, stats=None, sequential=False):
    """The whole definition: uint16 (H, W) -> uint16 (H_out, W_out, 3)."""
    H, W = mosaic.shape
    c = profile_or_constants if isinstance(profile_or_constants, SimpleNamespace) else constants(profile_or_constants, H, W, half_size)
    S = scale(np.asarray(mosaic), c, stats)
    if c.half_size:
        p = half_planes(S, c)
    else:
        p = planes_sequential(S, c) if sequential else planes(S, c, stats)
    return colour(p, c, stats)


# ---- fixtures
CAMERA = ((1.62, -0.41, -0.19), (-0.28, 1.52, -0.22), (0.04, -0.52, 1.49))
KINDS = ("random", "flat", "checker", "black", "negative-row")


def fixture(kind, pattern, H, W):
    """(mosaic, RawProfile) of one fixture kind, the same bytes for the same arguments."""
    rng = np.random.default_rng(zlib.crc32(f"{kind}/{pattern}/{H}x{W}".encode()))
    y, x = np.mgrid[0:H, 0:W]
    if kind == "random":  # full range; black above some samples, multipliers that push others past 65535, a camera-like matrix
        return (rng.integers(0, 65536, (H, W), dtype=np.uint16),
                RawProfile(pattern, black=(64, 60, 66, 64), multipliers=(2.1, 1.0, 1.6), matrix=CAMERA))
    if kind == "flat":  # near-flat: ties in B1 and B3
        return (rng.integers(30000, 30008, (H, W)).astype(np.uint16), RawProfile(pattern))
    if kind == "checker":  # 0 / 65535 in cells of 2 x 3 samples: every difference at full swing, clips in B2 and B3
        return ((((y // 2 + x // 3) & 1) * 65535).astype(np.uint16), RawProfile(pattern))
    if kind == "black":  # a black level above the samples
        return (rng.integers(0, 2000, (H, W)).astype(np.uint16),
                RawProfile(pattern, black=(2048, 1990, 1000, 2048), multipliers=(1.9, 1.0, 1.4), matrix=CAMERA))
    if kind == "negative-row":
        return (rng.integers(0, 65536, (H, W), dtype=np.uint16),
                RawProfile(pattern, black=16, multipliers=(1.0, 1.0, 1.0, 1.0), matrix=((-0.5, -0.2, -0.1), (0.3, 0.9, 0.2), (2.5, 1.5, 3.0))))
    raise KeyError(kind)
