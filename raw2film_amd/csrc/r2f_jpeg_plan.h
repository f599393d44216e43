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

}  // namespace jpeg
}  // namespace r2f
