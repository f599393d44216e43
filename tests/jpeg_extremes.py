"""Frames that drive the JPEG coder's coefficients to the ends of their ranges, which the frames of test_jpeg_host.contents()
never reach (their AC size categories stop at 9, their DC difference categories at 10): the longest thing the coder emits is a
16-bit AC code with 10 value bits, the widest difference a category-11 DC.  Shared by the host and the GPU tests."""

from __future__ import annotations

import numpy as np

import jpeg_model as jm

SIZES = ((16, 16), (33, 47), (64, 96))
QUALITIES = (100, 95, 50, 1, 0)

BLACK, WHITE = (0, 0, 0), (255, 255, 255)
BLUE, YELLOW = (0, 0, 255), (255, 255, 0)
RED, CYAN = (255, 0, 0), (0, 255, 255)


def _two(mask, a, b):
    return np.where(mask[..., None], np.array(a, np.uint8), np.array(b, np.uint8)).astype(np.uint8)


def frames(H, W):
    """block_checker: luma DC swings by the whole range from block to block.  pixel_checker, lines: all the energy in the
    highest AC coefficients (lines: one-pixel columns in even block rows, one-pixel rows in odd ones).  blue_yellow, red_cyan16:
    16 x 16 blocks, one chroma block each after 4:2:0, Cb resp. Cr DC swinging by the whole range.  red_cyan: 8 x 8 blocks, which
    4:2:0 averages away and 4:4:4 keeps."""
    yy, xx = np.mgrid[0:H, 0:W]
    return {
        "block_checker": _two((yy // 8 + xx // 8) % 2 == 0, BLACK, WHITE),
        "pixel_checker": _two((yy + xx) % 2 == 0, BLACK, WHITE),
        "lines": _two(np.where((yy // 8) % 2 == 0, xx, yy) % 2 == 0, BLACK, WHITE),
        "blue_yellow": _two((yy // 16 + xx // 16) % 2 == 0, BLUE, YELLOW),
        "red_cyan": _two((yy // 8 + xx // 8) % 2 == 0, RED, CYAN),
        "red_cyan16": _two((yy // 16 + xx // 16) % 2 == 0, RED, CYAN),
    }


def categories(img, quality=100):
    """Largest size category (bit length of the magnitude) the 4:2:0 baseline scan of `img` codes: DC differences of Y, Cb, Cr
    in scan order, and AC coefficients of any component."""
    c = jm.coefficients(img, quality)

    def bits(v):
        return int(np.abs(v).max()).bit_length()

    out = {}
    for name, dc in (("y_dc", c[:, :, :4, 0].reshape(-1)), ("cb_dc", c[:, :, 4, 0].reshape(-1)), ("cr_dc", c[:, :, 5, 0].reshape(-1))):
        out[name] = bits(np.diff(dc, prepend=0))
    out["ac"] = bits(c[..., 1:])
    return out
