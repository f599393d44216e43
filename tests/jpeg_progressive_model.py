"""The NumPy JPEG model extended with Pillow's progressive=True: libjpeg-turbo's progressive Huffman encoder (jcphuff.c) over
jpeg_simple_progression's ten scans, restated step for step on top of jpeg_options_model's coefficients and optimal tables.

Pillow's progressive save forces optimize_coding, so every scan carries its own optimized tables; `optimize` changes nothing.
Like the other models, a slow reference: its bytes are compared with Pillow's on the host and with the device encoder's on the GPU.
"""

from __future__ import annotations

import numpy as np

import jpeg_model as jm
import jpeg_options_model as om

# jpeg_simple_progression for 3-component YCbCr: (components, Ss, Se, Ah, Al); components 0 = Y, 1 = Cb, 2 = Cr
SCRIPT = (
    ((0, 1, 2), 0, 0, 0, 1),
    ((0,), 1, 5, 0, 2),
    ((2,), 1, 63, 0, 1),
    ((1,), 1, 63, 0, 1),
    ((0,), 6, 63, 0, 2),
    ((0,), 1, 63, 2, 1),
    ((0, 1, 2), 0, 0, 1, 0),
    ((2,), 1, 63, 1, 0),
    ((1,), 1, 63, 1, 0),
    ((0,), 1, 63, 1, 0),
)
MAX_CORR_BITS = 1000  # jcphuff.c: a refinement run is flushed once its buffered correction bits pass MAX_CORR_BITS - 64 + 1
EOBRUN_MAX = 0x7FFF


def component_blocks(coefs: np.ndarray, H: int, W: int, s: int, comp: int) -> np.ndarray:
    """The component's own blocks, ceil(comp_w / 8) x ceil(comp_h / 8) in row-major order, dummies left out: (n, 64)."""
    mw, mh, ny, _ = om.LAYOUT[s]
    my, mx = -(-H // mh), -(-W // mw)
    c = coefs.reshape(my, mx, ny + 2, 64)
    if comp:
        return c[:, :, ny + comp - 1].reshape(-1, 64)
    hy, vy = mw // 8, mh // 8
    grid = c[:, :, :ny].reshape(my, mx, vy, hy, 64).transpose(0, 2, 1, 3, 4).reshape(my * vy, mx * hy, 64)
    return grid[: -(-H // 8), : -(-W // 8)].reshape(-1, 64)


class Events:
    """A scan's symbols (table slot, symbol) and raw bits, in order."""

    def __init__(self):
        self.ev = []

    def sym(self, slot, symbol):
        self.ev.append((0, slot, symbol))

    def bits(self, value, n):
        if n:
            self.ev.append((1, value & ((1 << n) - 1), n))

    def counts(self, slots):
        freq = np.zeros((slots, 257), dtype=np.int64)
        for kind, a, b in self.ev:
            if kind == 0:
                freq[a, b] += 1
        return freq


def dc_first(coefs, s, Al, ev):
    comps = om.block_components(s)
    last = [0, 0, 0]
    for mcu in coefs:
        for k, comp in enumerate(comps):
            v = int(mcu[k, 0]) >> Al
            diff = v - last[comp]
            last[comp] = v
            n = jm._nbits(diff)
            ev.sym(0 if comp == 0 else 1, n)
            ev.bits(diff - 1 if diff < 0 else diff, n)


def dc_refine(coefs, Al, ev):
    for mcu in coefs:
        for blk in mcu:
            ev.bits((int(blk[0]) >> Al) & 1, 1)


def _emit_eobrun(st, ev, stats, reason):
    if st["run"] > 0:
        n = st["run"].bit_length() - 1
        ev.sym(0, n << 4)
        ev.bits(st["run"], n)
        for b in st["be"]:
            ev.bits(b, 1)
        st["run"], st["be"] = 0, []
        if stats is not None:
            stats[reason] = stats.get(reason, 0) + 1


def ac_first(blocks, Ss, Se, Al, ev, stats):
    """jcphuff.c encode_mcu_AC_first over the blocks, then finish_pass's flush."""
    st = {"run": 0, "be": []}
    for blk in blocks:
        r = 0
        if not np.any(np.abs(blk[Ss : Se + 1]) >> Al):  # (a block with nothing to code: the whole band is one zero run)
            r = Se - Ss + 1
        for k in range(Ss, Se + 1) if r == 0 else ():
            v = int(blk[k])
            t = (-v if v < 0 else v) >> Al
            if t == 0:
                r += 1
                continue
            _emit_eobrun(st, ev, stats, "coded")
            while r > 15:
                ev.sym(0, 0xF0)
                r -= 16
            n = t.bit_length()
            ev.sym(0, (r << 4) + n)
            ev.bits(~t if v < 0 else t, n)
            r = 0
        if r > 0:
            st["run"] += 1
            if st["run"] == EOBRUN_MAX:
                _emit_eobrun(st, ev, stats, "eobrun_cap")
    _emit_eobrun(st, ev, stats, "end")


def ac_refine(blocks, Ss, Se, Al, ev, stats):
    """jcphuff.c encode_mcu_AC_refine over the blocks, then finish_pass's flush."""
    st = {"run": 0, "be": []}
    for blk in blocks:
        if not np.any(np.abs(blk[Ss : Se + 1]) >> Al):
            st["run"] += 1
            if st["run"] == EOBRUN_MAX:
                _emit_eobrun(st, ev, stats, "eobrun_cap")
            continue
        absv = {k: abs(int(blk[k])) >> Al for k in range(Ss, Se + 1)}
        eob = max([k for k in absv if absv[k] == 1], default=0)
        r, br = 0, []
        for k in range(Ss, Se + 1):
            t = absv[k]
            if t == 0:
                r += 1
                continue
            while r > 15 and k <= eob:
                _emit_eobrun(st, ev, stats, "coded")
                ev.sym(0, 0xF0)
                r -= 16
                for b in br:
                    ev.bits(b, 1)
                br = []
            if t > 1:
                br.append(t & 1)
                continue
            _emit_eobrun(st, ev, stats, "coded")
            ev.sym(0, (r << 4) + 1)
            ev.bits(0 if blk[k] < 0 else 1, 1)
            for b in br:
                ev.bits(b, 1)
            br, r = [], 0
        if r > 0 or br:
            st["run"] += 1
            st["be"] += br
            if st["run"] == EOBRUN_MAX:
                _emit_eobrun(st, ev, stats, "eobrun_cap")
            elif len(st["be"]) > MAX_CORR_BITS - 64 + 1:
                _emit_eobrun(st, ev, stats, "be_cap")
    _emit_eobrun(st, ev, stats, "end")


def scan_events(coefs, H, W, s, scan, stats=None) -> Events:
    comps, Ss, Se, Ah, Al = scan
    ev = Events()
    if Ss == 0:
        (dc_first(coefs, s, Al, ev) if Ah == 0 else dc_refine(coefs, Al, ev))
    else:
        blocks = component_blocks(coefs, H, W, s, comps[0])
        (ac_first if Ah == 0 else ac_refine)(blocks, Ss, Se, Al, ev, stats)
    return ev


def pack(ev: Events, codes) -> bytes:
    """The scan's entropy-coded bytes: codes[slot][symbol] = (code, length); 1-bit padding, 0xFF stuffing (jcphuff.c)."""
    acc, nacc = 0, 0
    out = bytearray()

    def put(value, n):
        nonlocal acc, nacc
        acc = (acc << n) | (value & ((1 << n) - 1))
        nacc += n
        while nacc >= 8:
            nacc -= 8
            b = (acc >> nacc) & 0xFF
            out.append(b)
            if b == 0xFF:
                out.append(0)
        acc &= (1 << nacc) - 1

    for kind, a, b in ev.ev:
        if kind == 0:
            put(*codes[a][b])
        else:
            put(a, b)
    if nacc:
        put(0x7F, 8 - nacc)
    return bytes(out)


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def frame_header(quality: int, H: int, W: int, s: int) -> bytes:
    """SOI, APP0, the two DQT and SOF2 (jcmarker.c write_file_header / write_frame_header)."""
    ql, qc = jm.quant_tables(quality)
    out = bytes([0xFF, 0xD8]) + _seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i, t in enumerate((ql, qc)):
        out += _seg(0xDB, bytes([i]) + bytes(int(v) for v in t[jm.ZIGZAG]))
    return out + _seg(0xC2, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big")
                      + bytes([3, 1, om.LAYOUT[s][3], 0, 2, 0x11, 1, 3, 0x11, 1]))


def scan_header(scan, tables) -> bytes:
    """The scan's DHT segments (tables: one (bits[16], huffval) per table slot) and its SOS (jcmarker.c write_scan_header)."""
    comps, Ss, Se, Ah, Al = scan
    out = b""
    if Ss == 0 and Ah == 0:  # DC0 for Y, then DC1 once for Cb and Cr
        for slot, (bits, hv) in enumerate(tables):
            out += _seg(0xC4, bytes([slot]) + bytes(bits) + bytes(hv))
    elif Ss:
        bits, hv = tables[0]
        out += _seg(0xC4, bytes([0x10 | (1 if comps[0] else 0)]) + bytes(bits) + bytes(hv))
    sel = []
    for c in comps:
        td = (1 if c else 0) if Ss == 0 and Ah == 0 else 0
        ta = (1 if c else 0) if Se else 0
        sel += [c + 1, (td << 4) | ta]
    return out + _seg(0xDA, bytes([len(comps)] + sel + [Ss, Se, (Ah << 4) | Al]))


def encode(img: np.ndarray, quality: int = 75, subsampling: int = 2, exif: bytes = b"", stats: dict | None = None) -> bytes:
    """The bytes of Pillow's Image.fromarray(img).save(buf, "JPEG", quality=, subsampling=, progressive=True, exif=).
    stats (optional) counts the EOB-run flushes by reason: "coded", "eobrun_cap", "be_cap", "end"."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    H, W = img.shape[:2]
    s = 2 if subsampling == -1 else subsampling
    coefs = om.coefficients(img, quality, s)
    out = frame_header(quality, H, W, s)
    for scan in SCRIPT:
        ev = scan_events(coefs, H, W, s, scan, stats)
        if scan[1] == 0 and scan[3]:
            tables, codes = (), ()
        else:
            freq = ev.counts(2 if scan[1] == 0 else 1)
            tables = []
            for f in freq:
                bits, hv = om.optimal_table(f)
                tables.append((bits[1:17], hv))
            codes = [jm.huff_codes(t) for t in tables]
        out += scan_header(scan, tables) + pack(ev, codes)
    return om.splice_exif(out + bytes([0xFF, 0xD9]), exif)
