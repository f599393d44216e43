// r2f_jpeg_plan.cpp -- host side of the JPEG encoder (see r2f_jpeg_plan.h).  No HIP in this file: it is compiled by hipcc into the
// library and by g++ -fsanitize=address,undefined into the harness of tests/test_jpeg_host.py.
#include "r2f_jpeg_plan.h"

#include "../../include/r2f.h"

#include <algorithm>
#include <cstring>

namespace r2f {
namespace jpeg {

namespace {

// Annex K.1, natural order (libjpeg jcparam.c std_luminance_quant_tbl / std_chrominance_quant_tbl)
const uint8_t kStdQuant[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
     103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// zigzag position -> natural index
const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Annex K.3 tables: code counts per length 1..16, then the symbols
struct HuffSpec {
    uint8_t counts[16];
    const uint8_t* symbols;
    int n;
};
const uint8_t kDcSymbols[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcLumaSymbols[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const uint8_t kAcChromaSymbols[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
// in DHT order: DC luma (class 0, id 0), AC luma (1, 0), DC chroma (0, 1), AC chroma (1, 1) -- jcmarker.c write_scan_header
const HuffSpec kHuff[4] = {
    {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, kDcSymbols, 12},
    {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, kAcLumaSymbols, 162},
    {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, kDcSymbols, 12},
    {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}, kAcChromaSymbols, 162},
};
const uint8_t kHuffId[4] = {0x00, 0x10, 0x01, 0x11};

// Canonical codes of a table (jchuff.c jpeg_make_c_derived_tbl): out[symbol] = (code << 8) | length.
void derive(const HuffSpec& h, const uint8_t* counts, uint32_t* out, int n_out) {
    std::fill(out, out + n_out, 0u);
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < counts[len - 1] && k < h.n; ++i, ++k, ++code)
            if (h.symbols[k] < n_out) out[h.symbols[k]] = (code << 8) | (uint32_t)len;
        code <<= 1;
    }
}

struct Writer {
    uint8_t* p;
    size_t n = 0;
    void u8(int v) { p[n++] = (uint8_t)v; }
    void u16(int v) { u8(v >> 8), u8(v & 0xFF); }
    void marker(int m, int payload) { u8(0xFF), u8(m), u16(payload + 2); }
};

}  // namespace

void quant_tables(int quality, uint8_t out[2][64]) {
    const int q = std::min(std::max(quality, 1), 100);  // jpeg_quality_scaling
    const long scale = q < 50 ? 5000 / q : 200 - 2 * q;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i)  // jpeg_add_quant_table(..., force_baseline = TRUE)
            out[t][i] = (uint8_t)std::min(std::max((kStdQuant[t][i] * scale + 50) / 100, 1L), 255L);
}

void std_huffman(Huffman* h) {
    std::memset(h, 0, sizeof *h);
    for (int t = 0; t < 4; ++t) {
        std::memcpy(h->bits[t], kHuff[t].counts, 16);
        std::memcpy(h->huffval[t], kHuff[t].symbols, (size_t)kHuff[t].n);
        h->n[t] = kHuff[t].n;
    }
}

int optimal_table(const uint64_t freq_in[256], uint8_t bits_out[17], uint8_t huffval[256], bool* adjusted) {
    constexpr int kMaxClen = 32;
    uint64_t freq[257];
    int bits[kMaxClen + 1] = {}, codesize[257] = {}, others[257];
    for (int i = 0; i < 256; ++i) freq[i] = freq_in[i];
    freq[256] = 1;  // the reserved symbol: no real symbol gets the all-ones code
    for (int i = 0; i < 257; ++i) others[i] = -1;
    for (;;) {
        int c1 = -1, c2 = -1;
        uint64_t v = 1000000000ULL;
        for (int i = 0; i <= 256; ++i)  // the smallest non-zero count, ties to the larger symbol
            if (freq[i] && freq[i] <= v) v = freq[i], c1 = i;
        v = 1000000000ULL;
        for (int i = 0; i <= 256; ++i)
            if (freq[i] && freq[i] <= v && i != c1) v = freq[i], c2 = i;
        if (c2 < 0) break;
        freq[c1] += freq[c2];
        freq[c2] = 0;
        ++codesize[c1];
        while (others[c1] >= 0) ++codesize[c1 = others[c1]];
        others[c1] = c2;
        ++codesize[c2];
        while (others[c2] >= 0) ++codesize[c2 = others[c2]];
    }
    for (int i = 0; i <= 256; ++i)
        if (codesize[i]) {
            if (codesize[i] > kMaxClen) return -1;  // (libjpeg: JERR_HUFF_CLEN_OVERFLOW; 257 symbols cannot get there)
            ++bits[codesize[i]];
        }
    if (adjusted) *adjusted = false;
    int i = kMaxClen;
    for (; i > 16; --i)
        while (bits[i] > 0) {  // Annex K.3: fold a pair of the longest codes into the next length that is in use
            int j = i - 2;
            while (bits[j] == 0) --j;
            bits[i] -= 2, ++bits[i - 1], bits[j + 1] += 2, --bits[j];
            if (adjusted) *adjusted = true;
        }
    while (i > 0 && bits[i] == 0) --i;
    if (i == 0) return -1;  // (only the reserved symbol: every count was zero)
    --bits[i];
    int n = 0;
    bits_out[0] = 0;
    for (int k = 1; k <= 16; ++k) bits_out[k] = (uint8_t)bits[k], n += bits[k];
    // Counts past the sentinel stop the merging early and leave symbols without a code or lengths no prefix code can have; libjpeg
    // then fails (jpeg_make_c_derived_tbl: JERR_BAD_HUFF_TABLE, or a missing code when the symbol is encoded).  Only frames with
    // more than 10^9 symbols of one table can get there.
    uint64_t code = 0;
    for (int k = 1; k <= 16; ++k) {
        code += bits[k];
        if (code > (1ULL << k) - (k == 16 ? 1 : 0)) return -1;
        code <<= 1;
    }
    for (int j = 0; j < 256; ++j)
        if (freq_in[j] && !codesize[j]) return -1;
    int p = 0;
    for (int len = 1; len <= kMaxClen; ++len)
        for (int j = 0; j <= 255; ++j)
            if (codesize[j] == len) huffval[p++] = (uint8_t)j;
    return n;
}

void make_tables(int quality, const Huffman& h, Tables* t) {
    std::memset(t, 0, sizeof *t);
    uint8_t q[2][64];
    quant_tables(quality, q);
    for (int c = 0; c < 2; ++c) {
        derive(HuffSpec{{}, h.huffval[2 * c], h.n[2 * c]}, h.bits[2 * c], t->dc[c], 16);
        derive(HuffSpec{{}, h.huffval[2 * c + 1], h.n[2 * c + 1]}, h.bits[2 * c + 1], t->ac[c], 256);
        for (int i = 0; i < 64; ++i) t->qdiv[c][i] = (uint16_t)(q[c][i] * 8);
    }
}

void make_tables(int quality, Tables* t) {
    Huffman h;
    std_huffman(&h);
    make_tables(quality, h, t);
}

namespace {
// APP0: JFIF 1.01, no thumbnail; no units and density 1 : 1, or dots per inch when both densities are given (Pillow's dpi)
void app0(Writer& w, int xd, int yd) {
    const bool dpi = xd > 0 && yd > 0;
    w.marker(0xE0, 14);
    for (int c : {0x4A, 0x46, 0x49, 0x46, 0, 1, 1}) w.u8(c);  // "JFIF\0", version
    w.u8(dpi ? 1 : 0), w.u16(dpi ? xd : 1), w.u16(dpi ? yd : 1), w.u8(0), w.u8(0);
}
bool valid_density(int xd, int yd) { return xd >= 0 && yd >= 0 && xd <= kMaxDensity && yd <= kMaxDensity; }
}  // namespace

int header(int quality, int sampling, const Huffman& h, int H, int W, uint8_t* buf, size_t cap) {
    return header(quality, sampling, h, H, W, HeaderExtras{}, buf, cap);
}

int header(int quality, int sampling, const Huffman& h, int H, int W, const HeaderExtras& x, uint8_t* buf, size_t cap) {
    if (!buf || !valid_sampling(sampling) || quality < 0 || quality > 100 || H < 1 || W < 1 || H > kMaxDim || W > kMaxDim) return -1;
    if (!valid_restart(x.restart) || !valid_density(x.x_density, x.y_density)) return -1;
    int len = 275 + (x.restart ? kDriBytes : 0);  // everything but the DHT symbols
    for (int t = 0; t < 4; ++t) {
        int n = 0;
        for (int i = 0; i < 16; ++i) n += h.bits[t][i];
        if (n != h.n[t] || n < 1 || n > (t % 2 ? 162 : 12)) return -1;
        len += n;
    }
    if (cap < (size_t)len) return -1;
    uint8_t q[2][64];
    quant_tables(quality, q);
    Writer w{buf};
    w.u8(0xFF), w.u8(0xD8);  // SOI
    app0(w, x.x_density, x.y_density);
    for (int t = 0; t < 2; ++t) {  // one DQT per table, 8-bit entries in zigzag order
        w.marker(0xDB, 65);
        w.u8(t);
        for (int i = 0; i < 64; ++i) w.u8(q[t][kZigzag[i]]);
    }
    w.marker(0xC0, 15);  // SOF0: 8 bits, 3 components, Y 1x1 / 2x1 / 2x2 (table 0), Cb and Cr 1x1 (table 1)
    w.u8(8), w.u16(H), w.u16(W), w.u8(3);
    for (int c : {1, layout(sampling).y_factor, 0, 2, 0x11, 1, 3, 0x11, 1}) w.u8(c);
    for (int t = 0; t < 4; ++t) {
        w.marker(0xC4, 17 + h.n[t]);
        w.u8(kHuffId[t]);
        for (int i = 0; i < 16; ++i) w.u8(h.bits[t][i]);
        for (int i = 0; i < h.n[t]; ++i) w.u8(h.huffval[t][i]);
    }
    if (x.restart) w.marker(0xDD, 2), w.u16(x.restart);  // DRI: MCUs per restart interval (jcmarker.c write_scan_header)
    w.marker(0xDA, 10);  // SOS: 3 components (DC / AC tables 0/0, 1/1, 1/1), Ss 0, Se 63, Ah Al 0
    for (int c : {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0}) w.u8(c);
    return (int)w.n;
}

int header(int quality, int H, int W, uint8_t* buf, size_t cap) {
    if (cap < (size_t)kHeaderBytes) return -1;
    Huffman h;
    std_huffman(&h);
    return header(quality, 2, h, H, W, buf, cap);
}

uint64_t scan_bits(const uint64_t freq[4][256], const Huffman& h) {
    uint64_t total = 0;
    for (int t = 0; t < 4; ++t) {
        uint32_t codes[256];
        derive(HuffSpec{{}, h.huffval[t], h.n[t]}, h.bits[t], codes, 256);
        for (int s = 0; s < 256; ++s) {
            if (!freq[t][s]) continue;
            if (!codes[s]) return UINT64_MAX;
            total += freq[t][s] * (uint64_t)((codes[s] & 0xFF) + (t % 2 ? (s & 15) : s));
        }
    }
    return total;
}

uint64_t scan_partials(uint64_t n) {
    if (n <= (uint64_t)kScanBlock) return 0;
    const uint64_t nb = (n + kScanBlock - 1) / kScanBlock;
    return nb + 1 + scan_partials(nb);
}

Scratch scratch_layout(int H, int W) { return scratch_layout(H, W, 2); }

Scratch scratch_layout(int H, int W, int sampling, int restart) {
    Scratch s{};
    s.n_mcus = mcus(H, W, sampling);
    const uint64_t scan_bytes = (scan_bound_bits(H, W, sampling, restart) + 7) / 8;
    s.stuff_chunks = (scan_bytes + kStuffChunk - 1) / kStuffChunk;
    s.scan_words = s.stuff_chunks * (kStuffChunk / 4);  // (the 0xFF passes read whole chunks)
    s.partial_elems = std::max(scan_partials(s.n_mcus), scan_partials(s.stuff_chunks));  // (the intervals: no more than the MCUs)
    auto align = [](size_t v) { return (v + 15) & ~(size_t)15; };
    size_t at = 0;
    s.coefs = at, at = align(at + s.n_mcus * layout(sampling).nb * 64 * sizeof(int16_t));
    s.offsets = at, at = align(at + (s.n_mcus + 1) * sizeof(uint64_t));
    s.words = at, at = align(at + s.scan_words * sizeof(uint32_t));
    s.chunks = at, at = align(at + (s.stuff_chunks + 1) * sizeof(uint64_t));
    s.partial = at, at = align(at + s.partial_elems * sizeof(uint64_t));
    s.tables = at, at = align(at + sizeof(Tables));
    s.intervals = at;
    if (restart > 0) at = align(at + (restart_intervals(s.n_mcus, restart) + 2) * sizeof(uint64_t));
    s.total = at;
    return s;
}

bool rows_grid(int H, int W, int y0, int y1, RowsGrid* g) { return rows_grid(H, W, 2, y0, y1, g); }

bool rows_grid(int H, int W, int sampling, int y0, int y1, RowsGrid* g, int restart) {
    *g = RowsGrid{};
    if (!valid_sampling(sampling) || !valid_restart(restart)) return false;
    const Layout l = layout(sampling);
    if (H < 1 || W < 1 || H > kMaxDim || W > kMaxDim || y0 < 0 || y0 % l.mh || y1 <= y0 || y1 > H || (y1 % l.mh && y1 != H))
        return false;
    const uint64_t mx = (uint64_t)((W + l.mw - 1) / l.mw);
    g->m0 = (uint64_t)(y0 / l.mh) * mx;
    g->m1 = (uint64_t)((y1 + l.mh - 1) / l.mh) * mx;
    uint64_t bits = (g->m1 - g->m0) * l.nb * kBlockBoundBits;
    // (intervals that end in [m0, m1): one per `restart` MCUs, one more that began in a call before, and the frame's last)
    if (restart > 0) bits += 23 * ((g->m1 - g->m0) / restart + 2);
    const uint64_t bytes = (bits + 7) / 8 + 1;  // [floor(before / 8), ceil(after / 8)): the carried partial byte, then the new ones
    g->stuff_chunks = std::min((bytes + kStuffChunk - 1) / kStuffChunk, scratch_layout(H, W, sampling, restart).stuff_chunks);
    g->zero_words = (bits + 31) / 32;  // [ceil(before / 32), ceil(after / 32))
    return true;
}


// ---- progressive
namespace {
const ProgScan kProgScript[kProgScans] = {
    {3, 0, 0, 0, 0, 1}, {1, 0, 1, 5, 0, 2},  {1, 2, 1, 63, 0, 1}, {1, 1, 1, 63, 0, 1}, {1, 0, 6, 63, 0, 2},
    {1, 0, 1, 63, 2, 1}, {3, 0, 0, 0, 1, 0}, {1, 2, 1, 63, 1, 0}, {1, 1, 1, 63, 1, 0}, {1, 0, 1, 63, 1, 0},
};
}  // namespace

const ProgScan& prog_scan(int i) { return kProgScript[i]; }

ProgGeom prog_geom(int H, int W, int sampling, int scan) {
    const Layout l = layout(sampling);
    const ProgScan& s = kProgScript[scan];
    const int mx = (W + l.mw - 1) / l.mw, my = (H + l.mh - 1) / l.mh;
    if (s.Ss == 0) return ProgGeom{mcus(H, W, sampling) * (uint64_t)l.nb, l.nb, 0};
    const int bw = s.comp ? mx : (W + 7) / 8, bh = s.comp ? my : (H + 7) / 8;
    return ProgGeom{(uint64_t)bw * (uint64_t)bh, bw, bh};
}

int prog_frame_header(int quality, int sampling, int H, int W, uint8_t* buf, size_t cap, int x_density, int y_density) {
    if (!buf || !valid_sampling(sampling) || quality < 0 || quality > 100 || H < 1 || W < 1 || H > kMaxDim || W > kMaxDim ||
        cap < (size_t)kProgFrameHeaderBytes || !valid_density(x_density, y_density))
        return -1;
    uint8_t q[2][64];
    quant_tables(quality, q);
    Writer w{buf};
    w.u8(0xFF), w.u8(0xD8);
    app0(w, x_density, y_density);
    for (int t = 0; t < 2; ++t) {
        w.marker(0xDB, 65);
        w.u8(t);
        for (int i = 0; i < 64; ++i) w.u8(q[t][kZigzag[i]]);
    }
    w.marker(0xC2, 15);  // SOF2: as SOF0
    w.u8(8), w.u16(H), w.u16(W), w.u8(3);
    for (int c : {1, layout(sampling).y_factor, 0, 2, 0x11, 1, 3, 0x11, 1}) w.u8(c);
    return (int)w.n;
}

int prog_scan_header(int scan, const ProgTables& t, uint8_t* buf, size_t cap) {
    if (!buf || scan < 0 || scan >= kProgScans) return -1;
    const ProgScan& s = kProgScript[scan];
    const int slots = prog_slots(s);
    size_t len = 2 + 2 + 1 + 2 * (size_t)s.ncomp + 3;
    for (int k = 0; k < slots; ++k) {
        int n = 0;
        for (int i = 0; i < 16; ++i) n += t.bits[k][i];
        if (n != t.n[k] || n < 1 || n > (s.Ss ? kProgAcSymbols : 12)) return -1;
        len += 2 + 2 + 1 + 16 + (size_t)n;
    }
    if (cap < len) return -1;
    Writer w{buf};
    for (int k = 0; k < slots; ++k) {  // jcmarker.c emit_dht: DC0 then DC1 (once for Cb and Cr), or the AC scan's one table
        w.marker(0xC4, 17 + t.n[k]);
        w.u8(s.Ss ? 0x10 | (s.comp ? 1 : 0) : k);
        for (int i = 0; i < 16; ++i) w.u8(t.bits[k][i]);
        for (int i = 0; i < t.n[k]; ++i) w.u8(t.huffval[k][i]);
    }
    w.marker(0xDA, 2 * s.ncomp + 4);
    w.u8(s.ncomp);
    for (int c = 0; c < s.ncomp; ++c) {
        const int comp = s.ncomp == 3 ? c : s.comp;
        const int td = s.Ss == 0 && s.Ah == 0 ? (comp ? 1 : 0) : 0, ta = s.Se ? (comp ? 1 : 0) : 0;
        w.u8(comp + 1), w.u8((td << 4) | ta);
    }
    w.u8(s.Ss), w.u8(s.Se), w.u8((s.Ah << 4) | s.Al);
    return (int)w.n;
}

uint64_t prog_scan_bits(int scan, const uint64_t freq[2][256], const ProgTables& t, uint64_t extra) {
    const ProgScan& s = kProgScript[scan];
    uint64_t total = extra;
    for (int k = 0; k < prog_slots(s); ++k) {
        uint32_t codes[256];
        derive(HuffSpec{{}, t.huffval[k], t.n[k]}, t.bits[k], codes, 256);
        for (int v = 0; v < 256; ++v) {
            if (!freq[k][v]) continue;
            if (!codes[v]) return UINT64_MAX;
            // DC: the category's bits; AC: the size's bits, an EOB run's extra bits (ZRL: none)
            const int raw = s.Ss == 0 ? v : (v & 15) ? (v & 15) : (v == 0xF0 ? 0 : v >> 4);
            total += freq[k][v] * (uint64_t)((codes[v] & 0xFF) + raw);
        }
    }
    return total;
}

int prog_levels(uint64_t n, bool refine) {
    const uint64_t links = n / (refine ? 15 : kProgEobrunMax) + 2;
    int l = 1;
    while ((1ull << l) <= links) ++l;
    return l;
}

ProgScratch prog_scratch_layout(int H, int W, int sampling) {
    ProgScratch p{};
    const Scratch b = scratch_layout(H, W, sampling);
    for (int i = 0; i < kProgScans; ++i) {
        const ProgGeom g = prog_geom(H, W, sampling, i);
        p.n_max = std::max(p.n_max, g.n);
        if (kProgScript[i].Ss) p.run_at[i] = p.run_elems, p.run_elems += g.n;
    }
    p.levels = prog_levels(p.n_max, true);
    const uint64_t n1 = p.n_max + 1;
    const uint64_t scan_bytes = (p.n_max * kProgScanBlockBits + 7) / 8;
    p.stuff_chunks = (scan_bytes + kStuffChunk - 1) / kStuffChunk;
    p.scan_words = p.stuff_chunks * (kStuffChunk / 4);
    p.partial_elems = std::max(scan_partials(p.n_max), scan_partials(p.stuff_chunks));
    auto align = [](size_t v) { return (v + 15) & ~(size_t)15; };
    size_t at = b.total;
    p.coefs = b.coefs, p.tables = b.tables;
    p.runs = at, at = align(at + p.run_elems * sizeof(uint32_t));
    p.ecount = at, at = align(at + n1 * sizeof(uint64_t));
    p.bcount = at, at = align(at + n1 * sizeof(uint64_t));
    p.ccount = at, at = align(at + n1 * sizeof(uint64_t));
    p.jump = at, at = align(at + (size_t)p.levels * n1 * sizeof(uint32_t));
    p.mark = at, at = align(at + n1 * sizeof(uint32_t));
    p.offsets = at, at = align(at + n1 * sizeof(uint64_t));
    p.words = at, at = align(at + p.scan_words * sizeof(uint32_t));
    p.chunks = at, at = align(at + (p.stuff_chunks + 1) * sizeof(uint64_t));
    p.partial = at, at = align(at + p.partial_elems * sizeof(uint64_t));
    p.freq = at, at = align(at + kProgFreqWords * sizeof(uint64_t));
    p.total = at;
    return p;
}

}  // namespace jpeg
}  // namespace r2f

extern "C" {

int r2f_jpeg_header(int quality, int H, int W, uint8_t* buf, size_t cap, size_t* len) {
    if (!len) return R2F_EINVAL;
    const int n = r2f::jpeg::header(quality, H, W, buf, cap);
    if (n < 0) return R2F_EINVAL;
    *len = (size_t)n;
    return R2F_OK;
}

uint64_t r2f_jpeg_bound_bytes(int H, int W) {
    if (H < 1 || W < 1 || H > r2f::jpeg::kMaxDim || W > r2f::jpeg::kMaxDim) return 0;
    return r2f::jpeg::bound_bytes(H, W);
}

uint64_t r2f_jpeg_bound_bytes_ex(int H, int W, int sampling) {
    if (H < 1 || W < 1 || H > r2f::jpeg::kMaxDim || W > r2f::jpeg::kMaxDim || !r2f::jpeg::valid_sampling(sampling)) return 0;
    return r2f::jpeg::bound_bytes(H, W, sampling);
}

int r2f_jpeg_header_ex(const r2f_jpeg_opts* o, int H, int W, uint8_t* buf, size_t cap, size_t* len) {
    if (!o || !len || o->optimize || o->progressive) return R2F_EINVAL;  // (an optimized header needs the frame's statistics: r2f_jpeg_encode_ex)
    r2f::jpeg::Huffman h;
    r2f::jpeg::std_huffman(&h);
    const r2f::jpeg::HeaderExtras x{o->restart_interval, o->x_density, o->y_density};  // (header checks their ranges)
    const int n = r2f::jpeg::header(o->quality, o->sampling, h, H, W, x, buf, cap);
    if (n < 0) return R2F_EINVAL;
    *len = (size_t)n;
    return R2F_OK;
}

uint64_t r2f_jpeg_bound_bytes_opts(const r2f_jpeg_opts* o, int H, int W) {
    if (!o || (o->progressive != 0 && o->progressive != 1) || !r2f::jpeg::valid_restart(o->restart_interval)) return 0;
    if (o->progressive && o->restart_interval) return 0;  // (refused: r2f_jpeg_encode_ex)
    if (!o->progressive && !o->restart_interval) return r2f_jpeg_bound_bytes_ex(H, W, o->sampling);
    if (H < 1 || W < 1 || H > r2f::jpeg::kMaxDim || W > r2f::jpeg::kMaxDim || !r2f::jpeg::valid_sampling(o->sampling)) return 0;
    if (o->restart_interval) return r2f::jpeg::bound_bytes(H, W, o->sampling, o->restart_interval);
    return r2f::jpeg::prog_bound_bytes(H, W, o->sampling);
}

int r2f_jpeg_optimal_table(const uint64_t freq[256], uint8_t bits[17], uint8_t huffval[256], int* n) {
    if (!freq || !bits || !huffval || !n) return R2F_EINVAL;
    const int k = r2f::jpeg::optimal_table(freq, bits, huffval);
    if (k < 0) return R2F_EINVAL;
    *n = k;
    return R2F_OK;
}

}  // extern "C"
