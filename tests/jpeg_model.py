"""A NumPy model of the baseline JPEG encoder that HipProcessor.encode_jpeg implements on the device.

It restates what Pillow's default JPEG save (libjpeg-turbo's C code: jcparam.c, jcmarker.c, jccolor.c, jcsample.c, jfdctint.c,
jcdctmgr.c, jccoefct.c, jchuff.c) does to a uint8 (H, W, 3) array, integer for integer, so that its bytes can be compared with
Pillow's on a host without a GPU and the device encoder's with both.  Slow on purpose: it is a reference, not a product path.
"""

from __future__ import annotations

import numpy as np

# Annex K.1 tables in natural order (jcparam.c std_luminance_quant_tbl / std_chrominance_quant_tbl)
STD_LUMA_Q = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
    103, 99], dtype=np.int64)
STD_CHROMA_Q = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
    + [99] * 32, dtype=np.int64)

# zigzag position -> natural index (jutils.c jpeg_natural_order)
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49,
    56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63], dtype=np.int64)

# Annex K.3 Huffman tables: (code counts per length 1..16, symbols)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])


def quant_tables(quality: int) -> tuple[np.ndarray, np.ndarray]:
    """jpeg_set_quality(quality, force_baseline=TRUE): the (luma, chroma) tables, natural order."""
    q = min(max(int(quality), 1), 100)  # jpeg_quality_scaling
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((t * scale + 50) // 100, 1, 255) for t in (STD_LUMA_Q, STD_CHROMA_Q))


def huff_codes(table) -> dict[int, tuple[int, int]]:
    """symbol -> (code, length) of a (counts, symbols) table (jchuff.c jpeg_make_c_derived_tbl)."""
    counts, symbols = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[symbols[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def header(quality: int, H: int, W: int) -> bytes:
    """SOI .. SOS of the file (jcmarker.c write_file_header / write_frame_header / write_scan_header)."""
    ql, qc = quant_tables(quality)

    def seg(marker, payload):
        return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)

    out = bytes([0xFF, 0xD8])
    out += seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i, t in enumerate((ql, qc)):
        out += seg(0xDB, bytes([i]) + bytes(int(v) for v in t[ZIGZAG]))
    out += seg(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for cls_idx, table in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += seg(0xC4, bytes([cls_idx]) + bytes(table[0]) + bytes(table[1]))
    out += seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def ycbcr(img: np.ndarray) -> np.ndarray:
    """jccolor.c rgb_ycc_convert (SCALEBITS 16) -> int64 (H, W, 3)."""
    fix = lambda x: int(x * 65536 + 0.5)  # noqa: E731
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    half, off = 1 << 15, 128 << 16
    y = (fix(0.299) * r + fix(0.587) * g + fix(0.114) * b + half) >> 16
    cb = (-fix(0.16874) * r - fix(0.33126) * g + fix(0.5) * b + off + half - 1) >> 16
    cr = (fix(0.5) * r - fix(0.41869) * g - fix(0.08131) * b + off + half - 1) >> 16
    return np.stack([y, cb, cr], -1)


def fdct_islow(blocks: np.ndarray) -> np.ndarray:
    """jfdctint.c jpeg_fdct_islow on (..., 8, 8) int64 samples (already level-shifted); outputs scaled by 8."""
    c = dict(c0298=2446, c0390=3196, c0541=4433, c0765=6270, c0899=7373, c1175=9633, c1501=12299, c1847=15137, c1961=16069,
             c2053=16819, c2562=20995, c3072=25172)
    CB, P1 = 13, 2

    def desc(x, n):
        return (x + (1 << (n - 1))) >> n

    def one_pass(d, first):
        d = np.moveaxis(d, -1, 0)  # transform along the last axis
        t0, t7 = d[0] + d[7], d[0] - d[7]
        t1, t6 = d[1] + d[6], d[1] - d[6]
        t2, t5 = d[2] + d[5], d[2] - d[5]
        t3, t4 = d[3] + d[4], d[3] - d[4]
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        o = [None] * 8
        sh = CB - P1 if first else CB + P1
        if first:
            o[0], o[4] = (t10 + t11) << P1, (t10 - t11) << P1
        else:
            o[0], o[4] = desc(t10 + t11, P1), desc(t10 - t11, P1)
        z1 = (t12 + t13) * c["c0541"]
        o[2] = desc(z1 + t13 * c["c0765"], sh)
        o[6] = desc(z1 - t12 * c["c1847"], sh)
        z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
        z5 = (z3 + z4) * c["c1175"]
        t4, t5, t6, t7 = t4 * c["c0298"], t5 * c["c2053"], t6 * c["c3072"], t7 * c["c1501"]
        z1, z2, z3, z4 = -z1 * c["c0899"], -z2 * c["c2562"], -z3 * c["c1961"] + z5, -z4 * c["c0390"] + z5
        o[7], o[5] = desc(t4 + z1 + z3, sh), desc(t5 + z2 + z4, sh)
        o[3], o[1] = desc(t6 + z2 + z3, sh), desc(t7 + z1 + z4, sh)
        return np.moveaxis(np.stack(o), 0, -1)

    rows = one_pass(blocks, True)
    return np.swapaxes(one_pass(np.swapaxes(rows, -1, -2), False), -1, -2)


def quantize(coef: np.ndarray, table: np.ndarray) -> np.ndarray:
    """jcdctmgr.c quantize with divisor 8 q: |x| rounded half up, sign kept."""
    d = (table.reshape(8, 8) * 8).astype(np.int64)
    return np.sign(coef) * ((np.abs(coef) + (d >> 1)) // d)


def coefficients(img: np.ndarray, quality: int) -> np.ndarray:
    """Quantised coefficients in scan order: (MCU rows, MCU cols, 6, 64) int64, zigzag within each block, dummy blocks included."""
    H, W = img.shape[:2]
    ql, qc = quant_tables(quality)
    my, mx = -(-H // 16), -(-W // 16)
    ycc = ycbcr(img)
    # luma: edges replicated to whole blocks (jcsample.c expand_right_edge, jcprepct.c expand_bottom_edge)
    ywb, yhb = -(-W // 8), -(-H // 8)
    yy = np.pad(ycc[..., 0], ((0, yhb * 8 - H), (0, ywb * 8 - W)), mode="edge")
    # chroma: rows padded to even, columns to whole MCUs, h2v2 with bias 1, 2, 1, 2 ..., then chroma rows padded to whole MCUs
    cpad = np.pad(ycc[..., 1:], ((0, H % 2), (0, mx * 16 - W), (0, 0)), mode="edge")
    s = cpad[0::2, 0::2] + cpad[0::2, 1::2] + cpad[1::2, 0::2] + cpad[1::2, 1::2]
    bias = np.where(np.arange(s.shape[1]) % 2 == 0, 1, 2)[None, :, None]
    ch = (s + bias) >> 2
    ch = np.pad(ch, ((0, my * 8 - ch.shape[0]), (0, 0), (0, 0)), mode="edge")

    def blocks_of(plane, table):
        h, w = plane.shape
        b = (plane - 128).reshape(h // 8, 8, w // 8, 8).swapaxes(1, 2)
        q = quantize(fdct_islow(b), table).reshape(h // 8, w // 8, 64)
        return q[..., ZIGZAG]

    yb = blocks_of(yy, ql)  # (yhb, ywb, 64)
    cb, cr = blocks_of(ch[..., 0], qc), blocks_of(ch[..., 1], qc)
    out = np.zeros((my, mx, 6, 64), dtype=np.int64)
    for r in range(my):
        for c in range(mx):
            for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                by, bx = 2 * r + dy, 2 * c + dx
                if by >= yhb:  # jccoefct.c: a row of dummy blocks at the bottom takes the DC of the block before the row
                    out[r, c, k, 0] = out[r, c, 1, 0]
                elif bx >= ywb:  # ... a dummy block at the right edge the DC of the block to its left
                    out[r, c, k, 0] = out[r, c, k - 1, 0]
                else:
                    out[r, c, k] = yb[by, bx]
            out[r, c, 4], out[r, c, 5] = cb[r, c], cr[r, c]
    return out


def _nbits(v: int) -> int:
    return int(abs(v)).bit_length()


def entropy_code(coefs: np.ndarray) -> bytes:
    """jchuff.c encode_one_block over the MCUs in raster order, one DC predictor per component, no restarts, flush_bits' 1-padding,
    0xFF stuffing."""
    dcl, dcc, acl, acc = (huff_codes(t) for t in (DC_LUMA, DC_CHROMA, AC_LUMA, AC_CHROMA))
    acc_bits, nacc = 0, 0  # bit accumulator: value, bit count
    out = bytearray()

    def put(code, length):
        nonlocal acc_bits, nacc
        acc_bits = (acc_bits << length) | (code & ((1 << length) - 1))
        nacc += length
        while nacc >= 8:
            nacc -= 8
            b = (acc_bits >> nacc) & 0xFF
            out.append(b)
            if b == 0xFF:
                out.append(0)
        acc_bits &= (1 << nacc) - 1

    pred = [0, 0, 0]
    flat = coefs.reshape(-1, 6, 64)
    for mcu in flat:
        for k in range(6):
            comp = 0 if k < 4 else k - 3
            dc_t, ac_t = (dcl, acl) if comp == 0 else (dcc, acc)
            blk = [int(v) for v in mcu[k]]
            diff = blk[0] - pred[comp]
            pred[comp] = blk[0]
            n = _nbits(diff)
            put(*dc_t[n])
            if n:
                put(diff if diff > 0 else diff - 1, n)
            run = 0
            for v in blk[1:]:
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    put(*ac_t[0xF0])
                    run -= 16
                n = _nbits(v)
                put(*ac_t[(run << 4) | n])
                put(v if v > 0 else v - 1, n)
                run = 0
            if run:
                put(*ac_t[0x00])
    if nacc:
        put(0x7F, 8 - nacc)  # flush_bits: fill the last byte with 1s
    return bytes(out)


def encode(img: np.ndarray, quality: int = 100) -> bytes:
    """The bytes Pillow's Image.fromarray(img).save(buf, "JPEG", quality=quality) writes."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    H, W = img.shape[:2]
    return header(quality, H, W) + entropy_code(coefficients(img, quality)) + bytes([0xFF, 0xD9])


def block_bound_bits() -> int:
    """Most bits one block can take: the longer DC code with an 11-bit difference, then 63 positions of at most a 16-bit code and
    10 value bits each (a ZRL or the EOB is charged to the zero positions it stands for)."""
    dc = max(huff_codes(t)[11][1] for t in (DC_LUMA, DC_CHROMA)) + 11
    ac = max(ln + (sym & 15) for t in (AC_LUMA, AC_CHROMA) for sym, (_, ln) in huff_codes(t).items())
    return dc + 63 * ac


def mcus(H: int, W: int) -> int:
    return -(-H // 16) * -(-W // 16)


def bound_bytes(H: int, W: int) -> int:
    """Largest file encode() can produce for an H x W frame at any quality."""
    scan = -(-mcus(H, W) * 6 * block_bound_bits() // 8)
    return len(header(100, H, W)) + 2 * scan + 2
