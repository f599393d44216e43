"""Float64 model of the auto exposure the device measures (exposure="device"): calc_exposure (color_processing.py:71-99) with
every step after the first in double precision and the mean summed exactly.

    u over frame[::2, ::2, 1] of the whole decoded uint16 frame
    g      = float32(u) / float32(65535)      one correctly rounded fp32 division (raw_conversion.py:50), widened to double
    m      = fsum(g ** (1 / root)) / n         math.fsum: the correctly rounded sum
    stops  = log2(0.18 / m ** root)
    factor = float32(2 ** stops)

A plain module (no fixtures).  The device's reduction differs from this by the rounding of its fp64 pow and of its tree sum only:
about 4e-15 relative, times root <= 256, over ln 2 -- under 2e-12 stops (tests/test_gpu_auto_exposure.py asserts 1e-9).
"""

from __future__ import annotations

import math

import numpy as np

from raw2film_amd import decode

STOPS_TOL = 1e-9


def model_stops(frame_u16: np.ndarray, metadata: dict | None = None, ref_exposure: float = 0.18) -> float:
    """The stops of exposure compensation for a uint16 (H, W, 3+) frame, in float64; +inf when every sampled green is zero."""
    root = float(decode.exposure_root(metadata))
    green = frame_u16[::2, ::2, 1]
    assert green.dtype == np.uint16 and green.size > 0
    g = (green.astype(np.float32) / decode.U16_DIVISOR).astype(np.float64).ravel()
    inv = 1.0 / root
    # one pow per distinct sample value (at most 65536 of them), weighted by its count: exactly the fsum of the expanded list
    values, counts = np.unique(g, return_counts=True)
    total = _fsum_weighted([math.pow(float(v), inv) for v in values], counts)
    m = total / green.size
    average = math.pow(m, root)
    if average == 0.0:
        return math.inf
    return math.log2(ref_exposure / average)


def _fsum_weighted(powers, counts) -> float:
    """fsum over a list in which powers[i] appears counts[i] times, without building it: c * p is split into exactly representable
    parts (p times each set bit of c is a power-of-two multiple of p, hence exact)."""
    parts = []
    for p, c in zip(powers, counts):
        c, bit = int(c), 0
        while c:
            if c & 1:
                parts.append(math.ldexp(p, bit))
            c >>= 1
            bit += 1
    return math.fsum(parts)


def model_factor(stops: float) -> np.float32:
    """The float32 nearest to 2 ** stops (what decode.exposure_factor gives for the same stops)."""
    return decode.exposure_factor(stops)


def factor_agrees(factor, stops: float, tol: float = STOPS_TOL) -> bool:
    """Is `factor` the float32 of 2 ** s for some s within `tol` of `stops`?  2 ** s is monotone, so the candidates are the
    float32 values between the images of the interval's ends."""
    if math.isinf(stops):
        return bool(np.isinf(np.float32(factor))) and (float(factor) > 0) == (stops > 0)
    lo, hi = np.float32(2.0 ** (stops - tol)), np.float32(2.0 ** (stops + tol))
    return bool(lo <= np.float32(factor) <= hi)
