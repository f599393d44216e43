"""The shapes, inputs and parameters the denoise tests share (tests/test_denoise_host.py, tests/test_gpu_denoise*.py), and the model's
result for each, computed once.  The shapes follow the kernel's tile (include/r2f.h: R2F_DENOISE_TILE_W x R2F_DENOISE_TILE_H plane
samples): the smallest mosaic (every tap of level 4 reflects), one that is no multiple of anything, one tile plus one plane sample each
way, two tiles plus an odd remainder each way."""

import functools

import numpy as np

import denoise_model as model
from raw2film_amd import _lib

TW, TH = _lib.DENOISE_TILE_W, _lib.DENOISE_TILE_H
SHAPES = ((64, 64), (66, 70), (2 * (TH + 1), 2 * (TW + 1)), (2 * (2 * TH + 5), 2 * (2 * TW + 7)))
THRESHOLDS = (1.0, 100.0, 400.0, 1e5)
MAXIMA = (1, 255, 16383 - 512, 32767, 32768)  # the header's maxima below 65535; their shifts:
SHIFTS = (15, 8, 2, 1, 0)
BLACK = (512, 515, 509, 700)  # per site; 700 lies above the dark side of the step edge at some samples
INPUTS = ("edge", "zeros", "full", "impulses")


@functools.lru_cache(maxsize=None)
def mosaic(shape, name) -> np.ndarray:
    """A test input, read-only.  edge: a seeded Gaussian field (sd 237) on a step from 640 to 12 000 that crosses the frame obliquely;
    zeros / full: all 0 / all 65535; impulses: a flat 600 with one sample of 60 000 per plane at each corner of the plane and at
    (c, c) for every level's c."""
    H, W = shape
    if name == "zeros":
        m = np.zeros(shape, np.uint16)
    elif name == "full":
        m = np.full(shape, 65535, np.uint16)
    elif name == "edge":
        rng = np.random.default_rng(2028 + 131 * H + W)
        y, x = np.mgrid[0:H, 0:W]
        base = np.where(3 * x + 2 * y < 2 * W + H, 640.0, 12000.0)
        m = np.clip(np.rint(base + rng.normal(0.0, 237.0, shape)), 0, 65535).astype(np.uint16)
    elif name == "impulses":
        m = np.full(shape, 600, np.uint16)
        nr, nc = H // 2, W // 2
        spots = [(0, 0), (0, nc - 1), (nr - 1, 0), (nr - 1, nc - 1)] + [(c, c) for c in (1, 2, 4, 8, 16)]
        for k in range(4):
            for (py, px) in spots:
                m[2 * py + (k >> 1), 2 * px + (k & 1)] = 60000
    else:
        raise KeyError(name)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def expected(shape, name, threshold, maximum) -> np.ndarray:
    """tests/denoise_model.py's bytes for that input with BLACK, read-only."""
    out = model.denoise(mosaic(shape, name), BLACK, maximum, threshold)
    out.setflags(write=False)
    return out
