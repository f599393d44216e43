// r2f_jpeg.h -- the launcher of the JPEG encoder (r2f_jpeg.hip), called by r2f_jpeg_encode in r2f_api.hip.
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
    const uint8_t* header;  // header_len <= jpeg::kHeaderBytes bytes (host memory: copied into a launch argument)
    uint8_t* out;           // >= jpeg::bound_bytes(H, W, sampling)
    unsigned long long* out_len;
    void* carry = nullptr;  // row-wise: 2 device words, the scan's bits and 0xFF bytes so far
    int sampling = 2;       // 0 4:4:4, 1 4:2:2, 2 4:2:0
    int header_len = jpeg::kHeaderBytes;
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

}  // namespace r2f
