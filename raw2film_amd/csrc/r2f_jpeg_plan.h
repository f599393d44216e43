// r2f_jpeg_plan.h -- host side of the baseline JPEG encoder (r2f_jpeg.hip), free of HIP: quantisation tables for a quality,
// Huffman code tables, the file's header bytes, the worst-case output size and the layout of the device scratch.  The output is
// the file Pillow's Image.save(..., "JPEG", quality=q) writes with its defaults (libjpeg-turbo: JFIF 1.01, 4:2:0, ISLOW DCT, the
// Annex K Huffman tables, one interleaved scan, no restart markers).  Plain C++, like r2f_plan.h, so that it also builds under
// `g++ -fsanitize=address,undefined` (tests/test_jpeg_host.py).
#pragma once

#include <cstddef>
#include <cstdint>

namespace r2f {
namespace jpeg {

constexpr int kMaxDim = 65535;         // SOF0 stores H and W in 16 bits
constexpr int kHeaderBytes = 623;      // SOI + APP0 + 2 DQT + SOF0 + 4 DHT + SOS: the same for every quality and size
constexpr int kDriBytes = 6;           // the DRI segment a restart interval puts between the last DHT and SOS (FF DD 00 04 hi lo)
constexpr int kMaxRestart = 65535;     // DRI stores the interval, in MCUs, in 16 bits
constexpr int kMaxDensity = 65535;     // APP0 stores each density in 16 bits
constexpr int kBlockBoundBits = 1660;  // most bits one block can take (DC: 11-bit code + 11 bits; 63 positions of <= 16 + 10 bits)
constexpr int kStuffChunk = 4096;      // bytes of the packed scan per workgroup of the 0xFF count / scatter passes
constexpr int kScanBlock = 1024;       // elements per workgroup of the device-side exclusive scan

// What the device kernels read: (code << 8) | length per symbol (0 = no such symbol), divisors 8 q in natural order.
// [0] = luminance, [1] = chrominance.
struct Tables {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
    uint16_t qdiv[2][64];
};

// jpeg_set_quality(quality, force_baseline = TRUE): quality 0..100 (0 acts as 1) -> tables in natural order.
void quant_tables(int quality, uint8_t out[2][64]);
// The device tables of a quality.
void make_tables(int quality, Tables* t);
// The header bytes (SOI .. SOS) of an H x W frame; returns their count (kHeaderBytes), or -1 for bad arguments or cap < kHeaderBytes.
int header(int quality, int H, int W, uint8_t* buf, size_t cap);

// MCUs of an H x W frame (16 x 16 pixels each: 4 luminance, 1 Cb, 1 Cr block).
inline uint64_t mcus(int H, int W) { return (uint64_t)((H + 15) / 16) * (uint64_t)((W + 15) / 16); }
// Most bits the scan can take before padding and byte stuffing (64-bit: a 100 MP frame's bound exceeds 2^32).
inline uint64_t scan_bound_bits(int H, int W) { return mcus(H, W) * 6 * kBlockBoundBits; }
// Largest file for H x W at any quality: header, every scan byte stuffed, EOI.
inline uint64_t bound_bytes(int H, int W) { return kHeaderBytes + 2 * ((scan_bound_bits(H, W) + 7) / 8) + 2; }

// ---- Pillow's subsampling and optimize options.  sampling: 0 = 4:4:4 (h1v1), 1 = 4:2:2 (h2v1), 2 = 4:2:0 (h2v2, the default);
// every overload below returns the function above's result for sampling 2.
struct Layout {
    int mw, mh;    // MCU width and height in pixels
    int ny, nb;    // luminance blocks and all blocks per MCU (Y.. Cb Cr)
    int y_factor;  // SOF0 sampling byte of Y
};
inline bool valid_sampling(int s) { return s >= 0 && s <= 2; }
inline Layout layout(int sampling) {
    return sampling == 0 ? Layout{8, 8, 1, 3, 0x11} : sampling == 1 ? Layout{16, 8, 2, 4, 0x21} : Layout{16, 16, 4, 6, 0x22};
}
inline uint64_t mcus(int H, int W, int sampling) {
    const Layout l = layout(sampling);
    return (uint64_t)((H + l.mh - 1) / l.mh) * (uint64_t)((W + l.mw - 1) / l.mw);
}
inline uint64_t scan_bound_bits(int H, int W, int sampling) { return mcus(H, W, sampling) * layout(sampling).nb * kBlockBoundBits; }
inline uint64_t bound_bytes(int H, int W, int sampling) { return kHeaderBytes + 2 * ((scan_bound_bits(H, W, sampling) + 7) / 8) + 2; }

// ---- Pillow's restart_marker_blocks / restart_marker_rows, resolved to `restart` MCUs per interval (0: none, the functions
// above).  Every interval starts with the DC predictors at 0 and ends on a byte boundary: its last byte is padded with 1-bits,
// and every interval but the last is followed by RSTn (FF D0 + n, n = the interval's index mod 8), which is not stuffed.
inline bool valid_restart(int restart) { return restart >= 0 && restart <= kMaxRestart; }
inline uint64_t restart_intervals(uint64_t n_mcus, int restart) { return restart > 0 ? (n_mcus + restart - 1) / restart : 0; }
// Most bits of the scan with its padding and markers in place, before byte stuffing: per interval at most 7 padding bits, and
// 16 marker bits behind all but the last.
inline uint64_t scan_bound_bits(int H, int W, int sampling, int restart) {
    const uint64_t k = restart_intervals(mcus(H, W, sampling), restart);
    return scan_bound_bits(H, W, sampling) + (k ? 23 * k - 16 : 0);
}
// Largest file: the DRI segment, and per interval 4 bytes more than the scan's own bytes -- the marker (2), the byte its padding
// completes (1) and the 0x00 stuffed behind that byte when it comes out as 0xFF (1).  With B = scan_bound_bits without restarts
// and k intervals: the data bytes number at most (B + 7 k) / 8, each may be stuffed, and 2 (k - 1) marker bytes are not, so the
// scan takes at most 2 (B + 7 k) / 8 + 2 (k - 1) <= 2 ceil(B / 8) + 4 k bytes.
inline uint64_t bound_bytes(int H, int W, int sampling, int restart) {
    const uint64_t k = restart_intervals(mcus(H, W, sampling), restart);
    return bound_bytes(H, W, sampling) + (k ? kDriBytes + 4 * k : 0);
}

// Huffman tables as DHT holds them, in DHT order DC0, AC0, DC1, AC1: code counts per length 1..16, then n symbols.
struct Huffman {
    uint8_t bits[4][16];
    uint8_t huffval[4][256];
    int n[4];
};
// Annex K.3's tables (what make_tables and header above use).
void std_huffman(Huffman* h);
// jchuff.c jpeg_gen_optimal_table, step for step: the reserved symbol 256 with count 1, the merge of the two smallest non-zero
// counts (ties to the larger symbol, counts above the 1000000000 sentinel never taken), the codesize / others chains, Annex K.3's
// folding of lengths over 16, the reserved code taken from the longest length, huffval sorted by code length, then symbol.
// bits[0] = 0, bits[1..16]; returns the symbol count, or -1 when every count is zero or the result is no table libjpeg would take
// (a counted symbol left without a code, or more codes than lengths allow: counts past the sentinel).  *adjusted (optional):
// lengths were folded.
int optimal_table(const uint64_t freq[256], uint8_t bits[17], uint8_t huffval[256], bool* adjusted = nullptr);
// The device tables of a quality with the given Huffman tables.
void make_tables(int quality, const Huffman& h, Tables* t);
// The header with the sampling's SOF0 and DHT from `h`; returns its length (<= kHeaderBytes: an optimized table holds at most
// 12 DC or 162 AC symbols), or -1 for bad arguments or a cap below the length.
int header(int quality, int sampling, const Huffman& h, int H, int W, uint8_t* buf, size_t cap);
// The same with a restart interval (> 0: the DRI segment, kDriBytes more) and the JFIF density (both > 0: units 1, dots per
// inch; else no units, 1 : 1 as above).
struct HeaderExtras {
    int restart = 0;
    int x_density = 0, y_density = 0;
};
int header(int quality, int sampling, const Huffman& h, int H, int W, const HeaderExtras& x, uint8_t* buf, size_t cap);
// The scan's exact bit count (before padding) for symbol counts freq[DC0, AC0, DC1, AC1][256] coded with `h`; UINT64_MAX when a
// counted symbol has no code.
uint64_t scan_bits(const uint64_t freq[4][256], const Huffman& h);

// Byte offsets of the encoder's device scratch (all 16-byte aligned), sized for an H x W frame.
struct Scratch {
    size_t coefs;    // int16 [mcus][6][64], zigzag order
    size_t offsets;  // uint64 [mcus + 1]: bits per MCU, then their exclusive scan (+ the total)
    size_t words;    // uint32 [scan_words]: the packed scan, big-endian within each word
    size_t chunks;   // uint64 [stuff_chunks + 1]: 0xFF bytes per kStuffChunk, then their exclusive scan
    size_t partial;  // uint64 [scan block sums of both scans]
    size_t tables;   // Tables
    size_t intervals;  // uint64 [restart intervals + 2]: each interval's bits, padding and marker included, then their scan (restart > 0)
    size_t total;
    uint64_t n_mcus, scan_words, stuff_chunks, partial_elems;
};
Scratch scratch_layout(int H, int W);
// (coefs: int16 [mcus][nb][64]; restart > 0: the scan's words and chunks are sized for its padding and markers too, and
// `intervals` follows the other regions; restart = 0 gives the layout it always gave)
Scratch scratch_layout(int H, int W, int sampling, int restart = 0);
// Workgroup sums the scan of n elements needs (recursively, every level).
uint64_t scan_partials(uint64_t n);

// One call of a row-wise encode (r2f_jpeg_rows): the MCUs of rows [y0, y1) of an H x W frame and the launch grids of its passes,
// fixed without the bit counts.  A call's scan bits are at most (m1 - m0) * 6 * kBlockBoundBits; the words it clears start at the
// first one the call before did not touch, and its stuffing passes cover the bytes that become complete, the partial byte carried
// in included: stuff_chunks chunks (never more than the frame's, which hold every byte of its scan), zero_words words.
struct RowsGrid {
    uint64_t m0, m1;  // MCUs [m0, m1): whole MCU rows, row-major
    uint64_t stuff_chunks, zero_words;
};
// y0 a multiple of 16, y0 < y1 <= H, y1 a multiple of 16 or H; returns false (grid zeroed) otherwise.
bool rows_grid(int H, int W, int y0, int y1, RowsGrid* g);
// The same for a sampling: y0 a multiple of the MCU height (16 or 8), y1 one too or H.
// restart > 0: the padding and markers of the intervals that end in the call counted in.
bool rows_grid(int H, int W, int sampling, int y0, int y1, RowsGrid* g, int restart = 0);

// ---- Pillow's progressive=True (libjpeg-turbo jcphuff.c over jpeg_simple_progression's ten scans; optimize_coding forced, so
// every scan but the DC refinement carries its own optimized tables).  The DC scans walk the MCU grid's blocks, dummies included;
// each AC scan walks its one component's ceil(comp_w / 8) x ceil(comp_h / 8) blocks row-major, dummies left out.
constexpr int kProgScans = 10;
constexpr int kProgEobrunMax = 0x7FFF;      // jcphuff.c: an EOB run is flushed when it reaches this many blocks
constexpr int kProgMaxBE = 1000 - 64 + 1;   // ... or when its buffered correction bits pass MAX_CORR_BITS - DCTSIZE2 + 1
// Most bits one block can add to all ten scans together: DC 16 + 11 and 1; per AC position the code and value bits of the scan
// that first makes it non-zero (16 + 10) and one correction bit per later refinement (Y 2, chroma 1); per AC scan at most three
// ZRLs (16 bits each) and one EOB run symbol with its extra bits (16 + 14).  Y: 28 + 63 * 28 + 9 * 16 + 4 * 30 = 2056;
// chroma: 28 + 63 * 27 + 6 * 16 + 2 * 30 = 1885.
constexpr int kProgBlockBoundBits = 2056;
// Most bits one block can take in one scan (its own symbols, a run's EOB symbol and its correction bits): 63 * (16 + 10 + 1) +
// 3 * 16 + 30 (the DC scans: 27 and 1).
constexpr int kProgScanBlockBits = 63 * 27 + 3 * 16 + 30;
constexpr int kProgFrameHeaderBytes = 177;  // SOI, APP0, 2 DQT, SOF2
// AC symbols of a progressive scan: run / size 160, ZRL, EOB0 .. EOB14 (176 at most, the baseline's 162 less EOB plus 15 runs)
constexpr int kProgAcSymbols = 176;
constexpr int kProgScanHeaderMax = 2 + 2 + 1 + 16 + kProgAcSymbols + 10;  // the largest scan header: an AC DHT and its SOS (DC: <= 80)
struct ProgScan {
    int ncomp, comp;  // components in the scan: 3 (Y Cb Cr, the DC scans) or 1 (`comp`: 0 Y, 1 Cb, 2 Cr)
    int Ss, Se, Ah, Al;
};
const ProgScan& prog_scan(int i);
// Table slots of a scan: 2 for the DC first scan (DC0 of Y, DC1 of Cb and Cr), 0 for the DC refinement, 1 for an AC scan.
inline int prog_slots(const ProgScan& s) { return s.Ss == 0 ? (s.Ah == 0 ? 2 : 0) : 1; }
// The blocks a scan walks, and their grid for an AC scan (bw x bh; the DC scans: mcus x blocks per MCU, bw = blocks per MCU).
struct ProgGeom {
    uint64_t n;
    int bw, bh;
};
ProgGeom prog_geom(int H, int W, int sampling, int scan);
// Worst-case bits of the whole entropy-coded data, and the file: headers, every scan byte stuffed, the padding bytes, EOI.
inline uint64_t prog_bound_bits(int H, int W, int sampling) { return mcus(H, W, sampling) * layout(sampling).nb * kProgBlockBoundBits; }
inline uint64_t prog_bound_bytes(int H, int W, int sampling) {
    return kProgFrameHeaderBytes + 2 * (uint64_t)kProgScans * (kProgScanHeaderMax + 1) + 2 * ((prog_bound_bits(H, W, sampling) + 7) / 8) + 2;
}
// One scan's optimized tables: bits[slot][16] (lengths 1..16) and huffval[slot][n[slot]].
struct ProgTables {
    uint8_t bits[2][16];
    uint8_t huffval[2][256];
    int n[2];
};
// SOI .. SOF2 (densities as in HeaderExtras); returns its length (kProgFrameHeaderBytes) or -1 for bad arguments or a cap below it.
int prog_frame_header(int quality, int sampling, int H, int W, uint8_t* buf, size_t cap, int x_density = 0, int y_density = 0);
// The scan's DHT segments (none for the DC refinement) and SOS; returns the length or -1.
int prog_scan_header(int scan, const ProgTables& t, uint8_t* buf, size_t cap);
// The scan's exact bits before padding: freq[slot][256] coded with `t`, plus the raw bits no symbol implies (`extra`: the
// correction bits of a refinement, the one bit per block of the DC refinement).  UINT64_MAX when a counted symbol has no code.
uint64_t prog_scan_bits(int scan, const uint64_t freq[2][256], const ProgTables& t, uint64_t extra);
// Pointer-doubling levels the run resolution of an n-block scan needs: consecutive flushes of one stretch lie at least 15 blocks
// apart in a refinement scan (a flush needs 938 correction bits, at most 63 per block) and 0x7FFF apart in a first scan, so a
// chain has at most n / 15 + 2 (n / 0x7FFF + 2) links; 2^levels exceeds that.
int prog_levels(uint64_t n, bool refine);

// Byte offsets of the progressive encoder's device scratch (16-byte aligned): the baseline scratch (whose coefficients, tables
// and transform pass it shares), then the per-scan state.
struct ProgScratch {
    size_t coefs, tables;  // as Scratch
    size_t runs;           // uint32 per block of each AC scan: the EOB run a block starts (0: none), scans back to back
    size_t ecount, bcount, ccount;  // uint64 [n_max + 1]: joining blocks, correction bits, coded blocks -> exclusive prefix sums
    size_t jump;           // uint32 [levels][n_max + 1]: the run chain's pointer-doubling levels
    size_t mark;           // uint32 [n_max + 1]: run starts
    size_t offsets;        // uint64 [n_max + 1]: bits per block, then their exclusive scan
    size_t words;          // uint32 [scan_words]: one packed scan
    size_t chunks;         // uint64 [stuff_chunks + 1]
    size_t partial;        // uint64 [partial_elems]
    size_t freq;           // uint64 [kProgScans][2][256] symbol counts, then [kProgScans] extra bits, then 2 words: file position, overflow
    size_t total;
    uint64_t n_max, run_elems, scan_words, stuff_chunks, partial_elems;
    uint64_t run_at[kProgScans];  // element offset of each AC scan's runs
    int levels;
};
ProgScratch prog_scratch_layout(int H, int W, int sampling);
constexpr size_t kProgFreqWords = (size_t)kProgScans * 2 * 256 + kProgScans + 2;

}  // namespace jpeg
}  // namespace r2f
