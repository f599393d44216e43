"""The options of a JPEG export (HipProcessor.encode_jpeg, process_jpeg, process_preloaded_jpeg), checked before any work starts:
Pillow's quality, subsampling, optimize, exif, progressive, icc_profile, xmp, comment, dpi, restart_marker_blocks and
restart_marker_rows.  Pure host code: where Pillow wraps, ignores or fails late, these raise ValueError naming the option."""

from __future__ import annotations

import operator
import sys
from typing import NamedTuple

import numpy as np

from .jpeg_stream import ICC_OVERHEAD, MARKER_MAX, XMP_NAMESPACE, metadata_segments


def _jpeg_quality(quality) -> int:
    """The reference's quality slider: an int 0 .. 100 (0 writes what 1 writes, as in Pillow)."""
    if isinstance(quality, (bool, np.bool_)) or not isinstance(quality, (int, np.integer)):
        raise ValueError(f"JPEG quality must be an int in 0 .. 100, got {quality!r}")
    if not 0 <= int(quality) <= 100:
        raise ValueError(f"JPEG quality must be in 0 .. 100, got {int(quality)}")
    return int(quality)


_SUBSAMPLINGS = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}
_EXIF_MAX = MARKER_MAX  # a marker segment's payload (Pillow's MAX_BYTES_IN_MARKER)
_OPTIMIZE_REJECTED = "optimize=True: its Huffman tables need the whole frame's statistics before the first scan byte"
_PROGRESSIVE_REJECTED = "progressive=True: every one of its scans spans the whole frame"


def _jpeg_subsampling(subsampling) -> int:
    """Pillow's subsampling option -> 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0): -1 (libjpeg's default, 4:2:0), 0 / "4:4:4",
    1 / "4:2:2", 2 / "4:2:0".  "keep" (it needs a JPEG source), "4:1:1" (which Pillow maps with a warning) and anything else raise
    ValueError."""
    if isinstance(subsampling, str):
        if subsampling in _SUBSAMPLINGS:
            return _SUBSAMPLINGS[subsampling]
    elif not isinstance(subsampling, (bool, np.bool_)) and isinstance(subsampling, (int, np.integer)) and -1 <= int(subsampling) <= 2:
        return 2 if int(subsampling) == -1 else int(subsampling)
    raise ValueError(f"JPEG subsampling must be -1, 0 / '4:4:4', 1 / '4:2:2' or 2 / '4:2:0', got {subsampling!r}")


def _jpeg_exif(exif) -> bytes:
    """Pillow's exif option -> the APP1 payload: bytes-like, or a PIL.Image.Exif (its .tobytes()); b"" for none."""
    if isinstance(exif, (bytes, bytearray, memoryview)):
        data = bytes(exif)
    else:
        Exif = getattr(sys.modules.get("PIL.Image"), "Exif", None)  # (an Exif instance means Pillow is imported already)
        if Exif is None or not isinstance(exif, Exif):
            raise ValueError(f"JPEG exif must be bytes or a PIL.Image.Exif, got {type(exif).__name__}")
        data = exif.tobytes()
    if len(data) > _EXIF_MAX:
        raise ValueError(f"EXIF data is too long: {len(data)} bytes (a JPEG marker holds at most {_EXIF_MAX})")
    return data


def _jpeg_options(subsampling, optimize, exif):
    """(sampling 0 / 1 / 2, optimize, exif bytes) of an export's options, checked before any work starts."""
    return _jpeg_subsampling(subsampling), bool(optimize), _jpeg_exif(exif)


class _JpegExtras(NamedTuple):
    """The checked options of an export that need no table or kernel of their own (_jpeg_extras)."""
    icc_profile: bytes = b""
    xmp: bytes = b""
    comment: bytes = b""
    density: tuple = (0, 0)  # APP0's (x, y) in dots per inch; (0, 0): no units
    blocks: int = 0          # restart_marker_blocks
    rows: int = 0            # restart_marker_rows

    def restart(self, W: int, sampling: int) -> int:
        """MCUs per restart interval for a frame W pixels wide (0: none): `rows` MCU rows, clamped to 65535 as libjpeg does,
        else `blocks`."""
        if self.rows > 0:
            return min(self.rows * -(-W // (8 if sampling == 0 else 16)), 65535)
        return self.blocks

    def segments(self, exif: bytes) -> bytes:
        return metadata_segments(exif, self.xmp, self.icc_profile, self.comment)


_NO_EXTRAS = _JpegExtras()


def _jpeg_bytes(name, value, limit, what) -> bytes:
    if not isinstance(value, (bytes, bytearray, memoryview)):
        raise ValueError(f"JPEG {name} must be bytes, got {type(value).__name__}")
    data = bytes(value)
    if len(data) > limit:
        raise ValueError(f"JPEG {name} is too long: {len(data)} bytes ({what} at most {limit})")
    return data


def _jpeg_restart(name, value, limit) -> int:
    try:
        n = operator.index(value)
    except TypeError:
        raise ValueError(f"JPEG {name} must be an integer, got {value!r}") from None
    if n < 0 or (limit is not None and n > limit):
        raise ValueError(f"JPEG {name} must be {'in 0 .. ' + str(limit) if limit is not None else 'at least 0'}, got {n}")
    return n


def _jpeg_extras(icc_profile, xmp, comment, dpi, restart_marker_blocks, restart_marker_rows, progressive=False) -> _JpegExtras:
    """Pillow's icc_profile, xmp, comment, dpi, restart_marker_blocks and restart_marker_rows options, checked before any work
    starts.  Where Pillow wraps (blocks modulo 65536, a density modulo 65536), ignores (negative rows or dpi) or fails late (a
    segment too long for its marker), this raises ValueError naming the option."""
    icc = _jpeg_bytes("icc_profile", icc_profile, 255 * (MARKER_MAX - ICC_OVERHEAD), "255 APP2 chunks hold")
    x = _jpeg_bytes("xmp", xmp, MARKER_MAX - len(XMP_NAMESPACE), "its APP1 segment holds")
    if isinstance(comment, str):
        comment = comment.encode("utf-8")  # (as Pillow writes a str)
    elif not isinstance(comment, bytes):
        raise ValueError(f"JPEG comment must be bytes or str, got {type(comment).__name__}")
    if len(comment) > MARKER_MAX:
        raise ValueError(f"JPEG comment is too long: {len(comment)} bytes (a JPEG marker holds at most {MARKER_MAX})")
    try:
        density = tuple(int(round(v)) for v in dpi)
        ok = len(density) == 2 and all(0 <= v <= 65535 for v in density)
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"JPEG dpi must be two numbers that round to 0 .. 65535, got {dpi!r}")
    if not all(density):
        density = (0, 0)  # (Pillow sets the units only when both are positive)
    blocks = _jpeg_restart("restart_marker_blocks", restart_marker_blocks, 65535)
    rows = _jpeg_restart("restart_marker_rows", restart_marker_rows, None)
    if progressive and (blocks or rows):
        raise ValueError("JPEG progressive=True with restart_marker_blocks / restart_marker_rows is not supported: restart "
                         "intervals are written in baseline files only")
    return _JpegExtras(icc, x, comment, density, blocks, rows)


def _jpeg_progressive(progressive) -> bool:
    """Pillow's progressive option: True / False, or 0 / 1 (NumPy's included); anything else raises ValueError."""
    if isinstance(progressive, (bool, np.bool_)):
        return bool(progressive)
    if isinstance(progressive, (int, np.integer)) and int(progressive) in (0, 1):
        return bool(int(progressive))
    raise ValueError(f"JPEG progressive must be True / False (or 0 / 1), got {progressive!r}")


def _check_jpeg_image(is_uint8, shape, dtype):
    if not is_uint8:
        raise ValueError(f"encode_jpeg: the image must be uint8, got {dtype}")
    if len(shape) != 3 or shape[2] != 3:
        raise ValueError(f"encode_jpeg: the image must be (H, W, 3) RGB, got shape {tuple(shape)}")
    if not (1 <= shape[0] <= 65535 and 1 <= shape[1] <= 65535):
        raise ValueError(f"encode_jpeg: a JPEG holds 1 .. 65535 pixels per side, got {shape[0]} x {shape[1]}")


class JpegOptions(NamedTuple):
    """The checked options of one export (checked_options).  early: why an export with them takes the one-piece path whatever
    its frame (None where a reason does not apply) -- the export's own share of `stream_rejected`, ahead of the frame's."""
    quality: int
    subsampling: int  # 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0)
    optimize: bool
    exif: bytes
    progressive: bool
    extras: _JpegExtras
    early: tuple


def checked_options(quality, subsampling, optimize, exif, progressive, icc_profile, xmp, comment, dpi, restart_marker_blocks,
                    restart_marker_rows) -> JpegOptions:
    """Every JPEG keyword of an export, checked in the order that decides which of two bad options is named."""
    q = _jpeg_quality(quality)
    opts = _jpeg_options(subsampling, optimize, exif)
    prog = _jpeg_progressive(progressive)
    extras = _jpeg_extras(icc_profile, xmp, comment, dpi, restart_marker_blocks, restart_marker_rows, prog)
    return JpegOptions(q, *opts, prog, extras, (_PROGRESSIVE_REJECTED if prog else None, _OPTIMIZE_REJECTED if opts[1] else None))
