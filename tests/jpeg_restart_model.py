"""The NumPy JPEG model (tests/jpeg_options_model.py) extended with Pillow's restart_marker_blocks / restart_marker_rows, dpi,
icc_profile, xmp and comment options.

- restart intervals (libjpeg-turbo jchuff.c emit_restart, jcmarker.c write_scan_header): the DRI segment between the last DHT
  and SOS; every `interval` MCUs the partial byte is padded with 1-bits (and stuffed like any data byte if that makes it 0xFF),
  RSTn (n cycling 0 .. 7, not stuffed) is written and the DC predictors return to 0 -- in the gather pass of optimize too;
- the segments Pillow writes between APP0 and the first DQT, in its order: APP1 Exif, APP1 XMP, the APP2 ICC chunks, COM;
- dpi: APP0's units byte and densities.
Like the models it builds on, a slow reference: its bytes are compared with Pillow's on the host and the device encoder's on the
GPU.
"""

from __future__ import annotations

import numpy as np

import jpeg_model as jm
import jpeg_options_model as om

MARKER_MAX = 65533
XMP_NAMESPACE = b"http://ns.adobe.com/xap/1.0/\x00"


def restart_interval(W: int, s: int, blocks: int = 0, rows: int = 0) -> int:
    """MCUs per restart interval: `rows` MCU rows (clamped to 65535, jcmaster.c) when positive, else `blocks`."""
    if rows > 0:
        return min(rows * -(-W // om.LAYOUT[s][0]), 65535)
    return blocks


def intervals(coefs: np.ndarray, interval: int):
    n = len(coefs)
    step = interval if interval else max(n, 1)
    return [coefs[i:i + step] for i in range(0, n, step)]


def gather(coefs: np.ndarray, s: int, interval: int) -> np.ndarray:
    """om.gather with the DC predictors restarting at every interval."""
    return sum(om.gather(part, s) for part in intervals(coefs, interval))


def entropy_code(coefs: np.ndarray, s: int, tables, interval: int) -> bytes:
    """om.entropy_code per interval (each starts from predictors of 0 and ends padded and stuffed), RSTn between them."""
    parts = intervals(coefs, interval)
    out = bytearray()
    for i, part in enumerate(parts):
        out += om.entropy_code(part, s, tables)
        if i + 1 < len(parts):
            out += bytes([0xFF, 0xD0 + i % 8])
    return bytes(out)


def header(quality: int, H: int, W: int, s: int = 2, tables=None, interval: int = 0, dpi=(0, 0)) -> bytes:
    """om.header with APP0's density (Pillow: both of round(dpi) positive -> units 1) and the DRI segment in front of SOS."""
    h = bytearray(om.header(quality, H, W, s, tables))
    x, y = (round(v) for v in dpi)
    if x > 0 and y > 0:
        h[13:18] = bytes([1]) + x.to_bytes(2, "big") + y.to_bytes(2, "big")
    if interval:
        assert h[-14:-12] == b"\xff\xda"
        h[-14:-14] = b"\xff\xdd\x00\x04" + interval.to_bytes(2, "big")
    return bytes(h)


def _segment(marker: int, payload: bytes) -> bytes:
    assert len(payload) <= MARKER_MAX
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def segments(exif: bytes = b"", xmp: bytes = b"", icc_profile: bytes = b"", comment=b"") -> bytes:
    out = _segment(0xE1, bytes(exif)) if exif else b""
    if xmp:
        out += _segment(0xE1, XMP_NAMESPACE + bytes(xmp))
    step = MARKER_MAX - 14
    chunks = [icc_profile[i:i + step] for i in range(0, len(icc_profile), step)]
    for i, c in enumerate(chunks):
        out += _segment(0xE2, b"ICC_PROFILE\0" + bytes([i + 1, len(chunks)]) + bytes(c))
    if isinstance(comment, str):
        comment = comment.encode("utf-8")
    if comment:
        out += _segment(0xFE, bytes(comment))
    return out


def splice(data: bytes, segs: bytes) -> bytes:
    return data[:20] + segs + data[20:]


def encode(img: np.ndarray, quality: int = 100, subsampling: int = 2, optimize: bool = False, exif: bytes = b"", *,
           icc_profile: bytes = b"", xmp: bytes = b"", comment=b"", dpi=(0, 0), restart_marker_blocks: int = 0,
           restart_marker_rows: int = 0) -> bytes:
    """The bytes of Pillow's Image.fromarray(img).save(buf, "JPEG", ...) with these options."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    s = 2 if subsampling == -1 else subsampling
    interval = restart_interval(W, s, restart_marker_blocks, restart_marker_rows)
    coefs = om.coefficients(img, quality, s)
    tables = om.optimal_tables(gather(coefs, s, interval)) if optimize else om.std_tables()
    data = header(quality, H, W, s, tables, interval, dpi) + entropy_code(coefs, s, tables, interval) + bytes([0xFF, 0xD9])
    return splice(data, segments(exif, xmp, icc_profile, comment))


def bound_bytes(H: int, W: int, s: int, interval: int) -> int:
    """om.bound_bytes plus, with a restart interval, the DRI segment and per interval the marker, the byte the padding completes
    and that byte's stuffing."""
    k = -(-om.mcus(H, W, s) // interval) if interval else 0
    return om.bound_bytes(H, W, s) + (6 + 4 * k if k else 0)
