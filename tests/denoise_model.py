"""The wavelet denoise of a Bayer mosaic as include/r2f.h defines it (r2f_mosaic_denoise), restated in NumPy: every plane's five
levels are float32 arrays, and every stated rounding is one float32 operation (NumPy's float32 arithmetic and sqrt are correctly
rounded, and an operation on two float32 arrays stays in float32; `astype` marks the places where a conversion rounds).  Nothing here
reads the library."""

import numpy as np

NOISE = np.array([0.8002, 0.2735, 0.1202, 0.0585, 0.0291], dtype=np.float32)
F32 = np.float32


def shift_of(maximum: int) -> int:
    """Step 1: the largest s >= 0 with (maximum << s) < 65536."""
    assert 1 <= maximum <= 65535
    s = 0
    while (maximum << (s + 1)) < 65536:
        s += 1
    return s


def taps(n: int, c: int):
    """(m, p) of hat() for every i of a line of n samples at distance c."""
    i = np.arange(n)
    m = np.where(i >= c, i - c, c - i)
    p = np.where(i + c < n, i + c, 2 * n - 2 - (i + c))
    assert m.min() >= 0 and m.max() < n and p.min() >= 0 and p.max() < n, (n, c)
    return m, p


def quarter_hat(b, c, axis):
    """0.25 * hat along `axis` of a float32 array: fl(fl(2 b[i] + b[m]) + b[p]), quartered (both products are exact)."""
    m, p = taps(b.shape[axis], c)
    acc = F32(2) * b
    acc = acc + np.take(b, m, axis=axis)
    acc = acc + np.take(b, p, axis=axis)
    assert acc.dtype == np.float32
    return F32(0.25) * acc


def denoise_plane(t, shift: int, threshold) -> np.ndarray:
    """Steps 2 to 4 of one plane: t = the black-subtracted, clamped integers (n_r, n_c) -> the uint16 samples that leave."""
    T = F32(threshold)
    F = F32(256) * np.sqrt((t.astype(np.int64) << shift).astype(np.float32))  # (exact conversions: at most 16 significant bits)
    assert F.dtype == np.float32
    low, D = F, None
    for lev in range(5):
        c = 1 << lev
        inp = low
        low = quarter_hat(quarter_hat(inp, c, axis=1), c, axis=0)  # rows first, then columns
        theta = T * NOISE[lev]
        assert isinstance(theta, np.float32)
        d = inp - low
        dd = np.where(d < -theta, d + theta, np.where(d > theta, d - theta, F32(0))).astype(np.float32)
        D = dd if D is None else D + dd
        assert D.dtype == np.float32 and low.dtype == np.float32
    s = D + low
    q = (s * s) / F32(65536)
    assert q.dtype == np.float32
    return np.clip(np.trunc(q), 0, 65535).astype(np.uint16)


def denoise(mosaic, black, maximum: int, threshold) -> np.ndarray:
    """The definition on a uint16 (H, W) mosaic; black: 4 levels per site k = (y & 1) * 2 + (x & 1) -> the uint16 mosaic that leaves,
    black-free and in units of t << shift_of(maximum)."""
    mosaic = np.asarray(mosaic)
    H, W = mosaic.shape
    assert mosaic.dtype == np.uint16 and H % 2 == 0 and W % 2 == 0 and H >= 64 and W >= 64
    assert 0 < float(threshold) <= 1e6 and F32(threshold) > 0
    s = shift_of(int(maximum))
    out = np.empty_like(mosaic)
    for k in range(4):
        yy, xx = k >> 1, k & 1
        t = np.maximum(mosaic[yy::2, xx::2].astype(np.int64) - int(black[k]), 0)
        out[yy::2, xx::2] = denoise_plane(t, s, threshold)
    return out
