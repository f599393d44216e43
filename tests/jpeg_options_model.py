"""The NumPy JPEG model (tests/jpeg_model.py) extended with Pillow's subsampling, optimize and exif options.

- subsampling 0 (4:4:4, h1v1: 8 x 8 MCUs of Y Cb Cr) and 1 (4:2:2, h2v1: 16 x 8 MCUs of Y0 Y1 Cb Cr) next to jpeg_model's 2 (4:2:0);
- optimize: libjpeg-turbo's gather pass (jchuff.c htest_one_block) and jpeg_gen_optimal_table, restated step for step;
- exif: the APP1 segment Pillow writes right after SOI + APP0.
Like jpeg_model, a slow reference: its bytes are compared with Pillow's on the host and with the device encoder's on the GPU.
"""

from __future__ import annotations

import numpy as np

import jpeg_model as jm

# per sampling: (MCU width, MCU height, luma blocks per MCU, SOF0 sampling byte of Y)
LAYOUT = {0: (8, 8, 1, 0x11), 1: (16, 8, 2, 0x21), 2: (16, 16, 4, 0x22)}


def blocks_per_mcu(s: int) -> int:
    return LAYOUT[s][2] + 2


def block_components(s: int) -> list[int]:
    """component (0 Y, 1 Cb, 2 Cr) of each block of an MCU"""
    return [0] * LAYOUT[s][2] + [1, 2]


def mcus(H: int, W: int, s: int) -> int:
    mw, mh = LAYOUT[s][:2]
    return -(-H // mh) * -(-W // mw)


def _blocks_of(plane, table):
    h, w = plane.shape
    b = (plane - 128).reshape(h // 8, 8, w // 8, 8).swapaxes(1, 2)
    q = jm.quantize(jm.fdct_islow(b), table).reshape(h // 8, w // 8, 64)
    return q[..., jm.ZIGZAG]


def coefficients(img: np.ndarray, quality: int, s: int) -> np.ndarray:
    """Quantised coefficients in scan order: (MCUs, blocks per MCU, 64) int64, zigzag within each block, dummy blocks included."""
    if s == 2:
        return jm.coefficients(img, quality).reshape(-1, 6, 64)
    H, W = img.shape[:2]
    ql, qc = jm.quant_tables(quality)
    mw, mh = LAYOUT[s][:2]
    my, mx = -(-H // mh), -(-W // mw)
    ycc = jm.ycbcr(img)
    ywb = -(-W // 8)
    # luma: edges replicated to whole blocks (rows: to whole MCUs, which are one block high here)
    yy = np.pad(ycc[..., 0], ((0, my * 8 - H), (0, ywb * 8 - W)), mode="edge")
    yb = _blocks_of(yy, ql)  # (my, ywb, 64)
    if s == 0:  # fullsize_downsample: chroma as it is, edges replicated like luma's
        ch = np.pad(ycc[..., 1:], ((0, my * 8 - H), (0, mx * 8 - W), (0, 0)), mode="edge")
    else:  # h2v1_downsample: columns replicated to whole MCUs, pairs averaged with bias 0, 1, 0, 1 ...; rows replicated
        cpad = np.pad(ycc[..., 1:], ((0, my * 8 - H), (0, mx * 16 - W), (0, 0)), mode="edge")
        bias = np.where(np.arange(mx * 8) % 2 == 0, 0, 1)[None, :, None]
        ch = (cpad[:, 0::2] + cpad[:, 1::2] + bias) >> 1
    cb, cr = _blocks_of(ch[..., 0], qc), _blocks_of(ch[..., 1], qc)
    nb = blocks_per_mcu(s)
    out = np.zeros((my, mx, nb, 64), dtype=np.int64)
    if s == 0:
        out[:, :, 0] = yb
    else:
        out[:, :, 0] = yb[:, 0::2]
        right = yb[:, 1::2]  # (ceil(ywb / 2) columns less one when ywb is odd: that MCU's Y1 is a dummy)
        out[:, : right.shape[1], 1] = right
        if ywb % 2:  # jccoefct.c: the dummy block copies the DC of the block to its left, its AC coefficients are zero
            out[:, -1, 1, 0] = out[:, -1, 0, 0]
    out[:, :, nb - 2], out[:, :, nb - 1] = cb, cr
    return out.reshape(-1, nb, 64)


# ---------------------------------------------------------------------------------------------------------------- entropy coding
def gather(coefs: np.ndarray, s: int) -> np.ndarray:
    """jchuff.c htest_one_block over every block: (4, 257) int64 counts, rows DC0, AC0, DC1, AC1 (luma 0, Cb + Cr 1)."""
    freq = np.zeros((4, 257), dtype=np.int64)
    comps = block_components(s)
    pred = [0, 0, 0]
    for mcu in coefs:
        for k, comp in enumerate(comps):
            t = 0 if comp == 0 else 1
            blk = [int(v) for v in mcu[k]]
            diff = blk[0] - pred[comp]
            pred[comp] = blk[0]
            freq[2 * t, jm._nbits(diff)] += 1
            run = 0
            for v in blk[1:]:
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    freq[2 * t + 1, 0xF0] += 1
                    run -= 16
                freq[2 * t + 1, (run << 4) | jm._nbits(v)] += 1
                run = 0
            if run:
                freq[2 * t + 1, 0] += 1
    return freq


MAX_CLEN = 32


def optimal_table(freq, stats: dict | None = None):
    """jchuff.c jpeg_gen_optimal_table: 256 (or 257) counts -> (bits[17], huffval list), or None for a table libjpeg would
    refuse (counts past its 10^9 sentinel).  stats["adjusted"]: whether a code length over 16 had to be folded back (Annex K.3)."""
    freq_orig = [int(v) for v in list(freq)[:256]]
    freq = freq_orig + [1]  # the reserved symbol 256, count 1: no real symbol gets the all-ones code
    bits = [0] * (MAX_CLEN + 1)
    codesize = [0] * 257
    others = [-1] * 257
    while True:
        c1, v = -1, 1000000000
        for i in range(257):  # the smallest non-zero count, ties to the larger symbol
            if freq[i] and freq[i] <= v:
                v, c1 = freq[i], i
        c2, v = -1, 1000000000
        for i in range(257):
            if freq[i] and freq[i] <= v and i != c1:
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    for i in range(257):
        if codesize[i]:
            assert codesize[i] <= MAX_CLEN
            bits[codesize[i]] += 1
    adjusted = False
    i = MAX_CLEN
    while i > 16:
        while bits[i] > 0:
            adjusted = True
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
        i -= 1
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    # counts past the sentinel leave a counted symbol without a code, or more codes than the lengths allow: libjpeg refuses those
    code = 0
    for k in range(1, 17):
        code += bits[k]
        if code > (1 << k) - (k == 16):
            return None
        code <<= 1
    if any(f and not codesize[j] for j, f in enumerate(list(freq_orig)[:256])):
        return None
    huffval = [j for ln in range(1, MAX_CLEN + 1) for j in range(256) if codesize[j] == ln]
    if stats is not None:
        stats["adjusted"] = adjusted
    return bits[:17], huffval


def std_tables():
    """(DC0, AC0, DC1, AC1) as (counts[16], symbols)"""
    return (jm.DC_LUMA, jm.AC_LUMA, jm.DC_CHROMA, jm.AC_CHROMA)


def optimal_tables(freq, stats: dict | None = None):
    out, adjusted = [], False
    for t in range(4):
        st = {}
        bits, huffval = optimal_table(freq[t], st)
        adjusted |= st["adjusted"]
        out.append((bits[1:17], huffval))
    if stats is not None:
        stats["adjusted"] = adjusted
    return tuple(out)


def entropy_code(coefs: np.ndarray, s: int, tables) -> bytes:
    """jchuff.c encode_one_block over the MCUs in raster order with (DC0, AC0, DC1, AC1) tables."""
    dc0, ac0, dc1, ac1 = (jm.huff_codes(t) for t in tables)
    acc_bits, nacc = 0, 0
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
    comps = block_components(s)
    for mcu in coefs:
        for k, comp in enumerate(comps):
            dc_t, ac_t = (dc0, ac0) if comp == 0 else (dc1, ac1)
            blk = [int(v) for v in mcu[k]]
            diff = blk[0] - pred[comp]
            pred[comp] = blk[0]
            n = jm._nbits(diff)
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
                n = jm._nbits(v)
                put(*ac_t[(run << 4) | n])
                put(v if v > 0 else v - 1, n)
                run = 0
            if run:
                put(*ac_t[0x00])
    if nacc:
        put(0x7F, 8 - nacc)
    return bytes(out)


def header(quality: int, H: int, W: int, s: int = 2, tables=None) -> bytes:
    """SOI .. SOS with the sampling's SOF0 bytes and the given (DC0, AC0, DC1, AC1) tables (None: Annex K's)."""
    tables = std_tables() if tables is None else tables
    ql, qc = jm.quant_tables(quality)

    def seg(marker, payload):
        return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)

    out = bytes([0xFF, 0xD8])
    out += seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i, t in enumerate((ql, qc)):
        out += seg(0xDB, bytes([i]) + bytes(int(v) for v in t[jm.ZIGZAG]))
    out += seg(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, LAYOUT[s][3], 0, 2, 0x11, 1, 3, 0x11, 1]))
    for cls_idx, table in zip((0x00, 0x10, 0x01, 0x11), tables):
        out += seg(0xC4, bytes([cls_idx]) + bytes(table[0]) + bytes(table[1]))
    out += seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def splice_exif(data: bytes, exif: bytes) -> bytes:
    """Pillow's APP1: FF E1, length + 2 (big-endian), the bytes, right after SOI + APP0 (the first 20 bytes)."""
    if not exif:
        return data
    return data[:20] + bytes([0xFF, 0xE1]) + (len(exif) + 2).to_bytes(2, "big") + bytes(exif) + data[20:]


def encode(img: np.ndarray, quality: int = 100, subsampling: int = 2, optimize: bool = False, exif: bytes = b"",
           stats: dict | None = None) -> bytes:
    """The bytes of Pillow's Image.fromarray(img).save(buf, "JPEG", quality=, subsampling=, optimize=, exif=)."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    H, W = img.shape[:2]
    s = 2 if subsampling == -1 else subsampling
    coefs = coefficients(img, quality, s)
    tables = optimal_tables(gather(coefs, s), stats) if optimize else std_tables()
    data = header(quality, H, W, s, tables) + entropy_code(coefs, s, tables) + bytes([0xFF, 0xD9])
    return splice_exif(data, exif)


def bound_bytes(H: int, W: int, s: int) -> int:
    """Largest file encode() can produce for an H x W frame in sampling s at any quality, without exif."""
    scan = -(-mcus(H, W, s) * blocks_per_mcu(s) * jm.block_bound_bits() // 8)
    return len(jm.header(100, H, W)) + 2 * scan + 2
