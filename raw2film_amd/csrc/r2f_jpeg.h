// r2f_jpeg.h -- the launcher of the JPEG encoder (r2f_jpeg.hip), called by r2f_jpeg_encode in r2f_jpeg_api.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "r2f_jpeg_plan.h"

namespace r2f {
// r2f_jpeg.hip: the whole encoder on `s` (tables, header and scratch laid out by r2f_jpeg_plan.cpp)
struct JpegEncodeArgs {
    const uint8_t* image;  // uint8 (H, W, 3), rows row_stride bytes apart
    long long row_stride;
    int H, W;
    void* scratch;  // jpeg::scratch_layout(H, W, sampling).total bytes
    jpeg::Tables tables;
    const uint8_t* header;  // header_len <= jpeg::kHeaderBytes + jpeg::kDriBytes bytes (host memory: copied into a launch argument)
    uint8_t* out;           // >= jpeg::bound_bytes(H, W, sampling, restart)
    unsigned long long* out_len;
    void* carry = nullptr;  // row-wise: 2 device words, the scan's bits and 0xFF bytes so far
    int sampling = 2;       // 0 4:4:4, 1 4:2:2, 2 4:2:0
    int header_len = jpeg::kHeaderBytes;
    int restart = 0;        // MCUs per restart interval (0: none); the scratch is then jpeg::scratch_layout(H, W, sampling, restart)
    bool recount = false;   // encode: the coefficients are in the scratch already (launch_jpeg_stats); count bits with `tables`
};
hipError_t launch_jpeg_encode(const JpegEncodeArgs& a, hipStream_t s);
// optimize, first half: the standard tables (for their quantisation), the transform, and the symbol counts of the frame into the
// device words freq[DC0, AC0, DC1, AC1][256]; then launch_jpeg_encode with the optimized tables and recount = true.
hipError_t launch_jpeg_stats(const JpegEncodeArgs& a, unsigned long long* freq, hipStream_t s);
// Row-wise: begin copies the tables into the scratch and writes the header, an empty carry and *out_len; each rows launch encodes
// the MCUs of grid `g` against the carry (`last`: they end the frame) and leaves in *out_len the bytes of the file that are final.
hipError_t launch_jpeg_rows_begin(const JpegEncodeArgs& a, hipStream_t s);
hipError_t launch_jpeg_rows(const JpegEncodeArgs& a, const jpeg::RowsGrid& g, bool last, hipStream_t s);
// The tables copied into the scratch and the transform pass alone: the frame's coefficients in the scratch (progressive).
hipError_t launch_jpeg_transform(const JpegEncodeArgs& a, hipStream_t s);
// The exclusive 64-bit scan of r2f_jpeg.hip: data[0, n) in place, the total to data[n]; partial: jpeg::scan_partials(n) words.
void jpeg_scan_u64(unsigned long long* data, long long n, unsigned long long* partial, hipStream_t s);

// r2f_jpeg_prog.hip: progressive=True.  prog_stats: the transform, then per scan the blocks' symbols and the EOB runs resolved,
// into the scratch's counts (jpeg::ProgScratch::freq); the host reads them back and builds every scan's tables and header.
// prog_pack: the frame header, then per scan its bits, packing, stuffing and header into `out` (at most out_cap bytes), and the
// file's length (0 when it does not fit) into *out_len.
struct ProgScanPlan {
    uint32_t codes[2][256];  // (code << 8) | length per symbol of the scan's table slots
    uint8_t header[jpeg::kProgScanHeaderMax];
    int header_len;
};
hipError_t launch_jpeg_prog_stats(const JpegEncodeArgs& a, hipStream_t s);
hipError_t launch_jpeg_prog_pack(const JpegEncodeArgs& a, const uint8_t* frame_header, const ProgScanPlan* plans, uint64_t out_cap,
                                 hipStream_t s);

}  // namespace r2f
