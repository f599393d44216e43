"""Expected values of the 16-bit output side (output_bits=16): what the tests of test_output16_host.py and test_gpu_output16.py
compare with.  This module only CALLS the oracle (oracle/stages.py, oracle/post.py); it restates nothing of the pipeline.

  to_uint16       cpu_processor.py:407's `(image * 255).astype(uint8)` with 2 ** 16 - 1, on the float frame oracle.stages.render
                  returns before its own cast
  lanczos4_u16    cv.resize(uint16, INTER_LANCZOS4): the oracle's float LANCZOS4 restatement, then saturate_cast<ushort>
  area_u16        cv.resize(uint16, INTER_AREA) after oracle/post.py's uint8 structure, with the wider clamp
  canvas_u16      effects.add_canvas on a uint16 frame: the layout geometry.canvas_layout pins against the reference
                  (tests/golden/geometry.npz), the colour c * 257 (255 -> 65535), the frame pasted at the layout's offset
  read_tiff       a baseline TIFF reader (struct + numpy): the full-depth array and the tag dictionary
"""

from __future__ import annotations

import struct

import numpy as np

from oracle import post

F32 = np.float32


def to_uint16(x) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        v = np.clip(np.asarray(x, dtype=F32) * F32(65535), F32(0), F32(65535))
    return np.nan_to_num(v, nan=0.0).astype(np.uint16)


def sat_u16(v) -> np.ndarray:
    """saturate_cast<ushort>(float): round half to even, clamp to [0, 65535]."""
    return np.clip(np.rint(np.asarray(v, dtype=F32)), 0, 65535).astype(np.uint16)


def lanczos4_u16(image, out_h: int, out_w: int) -> np.ndarray:
    return sat_u16(post.resize_lanczos4_f32(np.asarray(image, dtype=np.uint16).astype(F32), out_h, out_w))


def area_u16(image, out_h: int, out_w: int) -> np.ndarray:
    """oracle.post.resize_area_u8's structure on uint16: integer factors: 2 x 2 -> (s + 2) >> 2 in integers, else OpenCV's
    float32 block sum times 1 / area, other ratios take the float32 area tables, x first then the rows."""
    image = np.asarray(image, dtype=np.uint16)
    H, W = image.shape[:2]
    sx, sy = W / out_w, H / out_h
    if float(int(sx)) == sx and float(int(sy)) == sy:
        isx, isy = int(sx), int(sy)
        blocks = image[: out_h * isy, : out_w * isx].astype(np.int64).reshape(out_h, isy, out_w, isx, 3)
        if isx == 2 and isy == 2:
            return ((blocks.sum(axis=(1, 3)) + 2) >> 2).astype(np.uint16)
        # resizeAreaFast_<ushort, float>: the block's samples in row order, four at a time summed as integers, each group -- then each
        # sample left over -- added to a float32 sum (which rounds once it passes 2 ** 24: more than 256 bright samples)
        flat = blocks.transpose(0, 2, 4, 1, 3).reshape(out_h, out_w, 3, isy * isx)
        area4 = isy * isx // 4 * 4
        total = np.zeros((out_h, out_w, 3), F32)
        for k in range(0, area4, 4):
            total = (total + flat[..., k:k + 4].sum(axis=-1).astype(F32)).astype(F32)
        for k in range(area4, isy * isx):
            total = (total + flat[..., k].astype(F32)).astype(F32)
        return sat_u16((total * (F32(1.0) / F32(isx * isy))).astype(F32))
    xtab, ytab = post._area_tab(W, out_w), post._area_tab(H, out_h)
    src = image.astype(F32)
    buf = np.zeros((H, out_w, 3), F32)
    for dx, ent in enumerate(xtab):
        acc = np.zeros((H, 3), F32)
        for s, a in ent:
            acc = (acc + (src[:, s, :] * a).astype(F32)).astype(F32)
        buf[:, dx, :] = acc
    out = np.empty((out_h, out_w, 3), np.uint16)
    for dy, ent in enumerate(ytab):
        total = None
        for s, b in ent:
            term = (b * buf[s]).astype(F32)
            total = term if total is None else (total + term).astype(F32)
        out[dy] = sat_u16(total)
    return out


def canvas_u16(image, canvas_mode: str, canvas_scale: float = 1.0, canvas_ratio: float = 1.0) -> np.ndarray:
    from raw2film_amd import geometry

    image = np.asarray(image, dtype=np.uint16)
    (rows, cols), color, (oy, ox) = geometry.canvas_layout(image.shape, canvas_mode, canvas_scale, canvas_ratio)
    out = np.empty((rows, cols, 3), np.uint16)
    for c in range(3):
        out[:, :, c] = color[c] * 257
    out[oy:oy + image.shape[0], ox:ox + image.shape[1]] = image
    return out


_TYPES = {1: "B", 2: "c", 3: "H", 4: "I", 7: "B"}


def read_tiff(data: bytes):
    """(array (H, W, 3) at the file's depth, {tag: value or tuple of values}, {tag: offset of an out-of-line value}) of a
    little-endian baseline RGB TIFF; strips are read through StripOffsets / StripByteCounts, not assumed contiguous."""
    assert data[:4] == b"II*\0", "little-endian classic TIFF"
    (ifd,) = struct.unpack_from("<I", data, 4)
    (n,) = struct.unpack_from("<H", data, ifd)
    tags, where = {}, {}
    for i in range(n):
        tag, typ, count, raw = struct.unpack_from("<HHI4s", data, ifd + 2 + 12 * i)
        fmt = "<" + str(count) + _TYPES[typ]
        size = struct.calcsize(fmt)
        if size <= 4:
            vals = struct.unpack_from(fmt, raw)
        else:
            (off,) = struct.unpack("<I", raw)
            where[tag] = off
            vals = struct.unpack_from(fmt, data, off)
        tags[tag] = bytes(vals) if typ == 7 else (vals[0] if count == 1 else vals)
    assert struct.unpack_from("<I", data, ifd + 2 + 12 * n)[0] == 0 and sorted(tags) == list(tags), "one IFD, tags ascending"
    W, H, bps = tags[256], tags[257], tags[258]
    assert tags[259] == 1 and tags[262] == 2 and tags[277] == 3 and tags[284] == 1 and tags[274] == 1 and bps in ((8, 8, 8), (16, 16, 16))
    offs = tags[273] if isinstance(tags[273], tuple) else (tags[273],)
    cnts = tags[279] if isinstance(tags[279], tuple) else (tags[279],)
    body = b"".join(data[o:o + c] for o, c in zip(offs, cnts))
    arr = np.frombuffer(body, dtype="<u2" if bps[0] == 16 else np.uint8).reshape(H, W, 3)
    return arr, tags, where
