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
    size_t total;
    uint64_t n_mcus, scan_words, stuff_chunks, partial_elems;
};
Scratch scratch_layout(int H, int W);
Scratch scratch_layout(int H, int W, int sampling);  // (coefs: int16 [mcus][nb][64])
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
bool rows_grid(int H, int W, int sampling, int y0, int y1, RowsGrid* g);

}  // namespace jpeg
}  // namespace r2f
