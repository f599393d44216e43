"""The NumPy statement of include/r2f.h's "scale of a mosaic from the sensor's levels": the data maximum (r2f_mosaic_maximum) and
the Scale steps (r2f_raw_scale_plan).  The fp32 multiply and comparison of the threshold are done in np.float32, everything else in
Python's ints and doubles.  What the planner, the kernel and the pipeline are compared with."""

import numpy as np


def black_plane(black, period, H, W, gy0=0):
    """black[(y % P) * P + x % P] for frame rows [gy0, gy0 + H) and columns [0, W), int64."""
    table = np.asarray(black, dtype=np.int64).reshape(period, period)
    ys, xs = (np.arange(gy0, gy0 + H) % period)[:, None], (np.arange(W) % period)[None, :]
    return table[ys, xs]


def data_maximum(mosaic, black, period, rows=None, gy0=0):
    """d over mosaic rows `rows` = (y0, y1) of the frame (default: all the array holds); the array's row 0 is frame row gy0.
    int16 arrays are read as the same bits.  0 for no rows."""
    m = np.asarray(mosaic)
    m = m.view(np.uint16) if m.dtype == np.int16 else m
    assert m.dtype == np.uint16 and m.ndim == 2 and len(black) == period * period
    y0, y1 = (gy0, gy0 + m.shape[0]) if rows is None else rows
    if y0 >= y1:
        return 0
    part = m[y0 - gy0:y1 - gy0].astype(np.int64)
    assert part.shape[0] == y1 - y0
    return int(np.maximum(part - black_plane(black, period, y1 - y0, m.shape[1], y0), 0).max())


def threshold(thr):
    """LibRaw's rule: None for no adjustment, else the threshold as a double."""
    if thr < 0.00001:
        return None
    return 0.75 if thr > 0.99999 else thr


def scale(white_balance, white_level, thr, black, d):
    """(mul[3] as doubles, maximum_used, adjusted), or None for what the Scale steps refuse (m < 1)."""
    m = int(white_level) - int(min(black))
    if m < 1:
        return None
    t = threshold(float(thr))
    adjusted = False
    if t is not None:
        product = np.float32(m) * np.float32(t)  # one fp32 multiply
        adjusted = bool(0 < d < m and np.float32(d) > product)
    m_eff = int(d) if adjusted else m
    wb = [float(v) for v in white_balance]
    lo = min(wb)
    return tuple(v / lo * 65535.0 / m_eff for v in wb), m_eff, adjusted
