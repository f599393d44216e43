// r2f_xtrans.hip -- the X-Trans demosaic ahead of the uint16 hand-off (include/r2f.h: r2f_demosaic_xtrans_u16), its two kernels
// next to their entry point, beside the Bayer path (r2f_demosaic.hip) and not inside it.  The arithmetic is r2f_xtrans_math.h's (the
// text tests/xtrans_check.cpp compiles for the CPU); this file adds the staging: which samples a block holds in LDS, how they are
// loaded and how the finished pixels leave.
//   xtrans_full_kernel     one launch: the planner's tables, the scaled tile + 3-sample apron and the colour-difference plane S - G
//                          of the tile + 1-sample apron in LDS, then B2 / C per output pixel
//   xtrans_reduced_kernel  one lane per output pixel of the reduced (third-size) form
// Neither runs inside r2f_render or a timed step.  The kernels have static LDS and one instantiation each, like the Bayer ones: they
// need no dynamic-LDS attribute and so no row in r2f_kernels.hip's instantiation tables.
#include <cstdint>
#include <cstring>

#include "r2f_ctx.h"
#include "r2f_xtrans_math.h"

using namespace r2f;

namespace r2f {
namespace {

constexpr int kTW = R2F_XTRANS_TILE_W, kTH = R2F_XTRANS_TILE_H;  // lanes along x: a wave is one row of the tile
constexpr int kReach = 3;                                        // B1 reaches 2 samples, B2 one more
constexpr int kApronX = 4;                                       // staged columns each side: kReach rounded up to a pair
constexpr int kSW = kTW + 2 * kApronX, kSH = kTH + 2 * kReach;   // the scaled samples: 72 x 38
constexpr int kDW = kTW + 2, kDH = kTH + 2;                      // the colour-difference plane: 66 x 34
constexpr int kRowsPerLane = kTH / 4;
constexpr int kParamWords = (int)(sizeof(r2f_xtrans_params) / 4);
static_assert(kTW == 64 && kTH % 4 == 0 && kSW % 2 == 0 && kApronX >= kReach && kApronX % 2 == 0,
              "a wave per tile row, workgroups of (64, 4), the samples loaded in pairs at even columns");
static_assert(sizeof(r2f_xtrans_params) % 4 == 0 && alignof(r2f_xtrans_params) == 4, "copied to LDS in 32-bit words");
// LDS per block: 900 (tables) + 5472 (samples) + 8976 (differences, int32: 17 bits) + 1536 (row buffers) = 16.9 KB: nine blocks fit a
// CU's 160 KB, more than its wave slots take at 256 threads

struct XTransArgs {
    const uint16_t* src;  // row src_gy0 of the mosaic
    int src_gy0;
    long long pitch;  // samples
    int H, W;
    r2f_xtrans_params p;
    uint16_t* dst;  // row 0 of the demosaiced frame
    int y0, y1;     // the rows of it this call writes
    int wide;       // 1: src is 4-byte aligned and the pitch even -> a pair of samples at an even x is one 32-bit load
};

// The planner's tables from the kernel's arguments into LDS, where a lane indexes them by its phase.
__device__ __forceinline__ void stage_params(const XTransArgs& a, r2f_xtrans_params& s_p, int tid) {
    const uint32_t* from = reinterpret_cast<const uint32_t*>(&a.p);
    uint32_t* to = reinterpret_cast<uint32_t*>(&s_p);
    for (int i = tid; i < kParamWords; i += 256) to[i] = from[i];
}

// The samples (y, x) and (y, x + 1), x even, scaled (step A); 0 for one outside the frame.  One 32-bit load where that is allowed
// and both are inside, else one 16-bit load each: the same samples either way.  y is inside the frame.
__device__ __forceinline__ void load_pair(const XTransArgs& a, const r2f_xtrans_params& p, int y, int x, int& s0, int& s1) {
    const bool in0 = x >= 0 && x < a.W, in1 = x + 1 >= 0 && x + 1 < a.W;
    unsigned r0 = 0, r1 = 0;
    if (in0 || in1) {
        const uint16_t* row = a.src + (long long)(y - a.src_gy0) * a.pitch;
        if (in0 && in1 && a.wide) {
            const uint32_t v = *reinterpret_cast<const uint32_t*>(row + x);
            r0 = v & 0xFFFFu, r1 = v >> 16;
        } else {
            if (in0) r0 = row[x];
            if (in1) r1 = row[x + 1];
        }
    }
    const int px = in0 ? x % 6 : 0, row_ph = (y % 6) * 6;
    const int v0 = xtrans::scale_sample(p, (int)r0, row_ph + px), v1 = xtrans::scale_sample(p, (int)r1, row_ph + xtrans::wrap6(px + 1));
    s0 = in0 ? v0 : 0, s1 = in1 ? v1 : 0;
}

struct TileS {  // the scaled samples of a block, at frame coordinates
    const uint16_t* s;
    int y_org, x_org;  // frame coordinates of s[0]
    __device__ __forceinline__ int operator()(int y, int x) const { return s[(y - y_org) * kSW + (x - x_org)]; }
};
struct TileD {  // its colour-difference plane
    const int* d;
    int y_org, x_org;
    __device__ __forceinline__ int operator()(int y, int x) const { return d[(y - y_org) * kDW + (x - x_org)]; }
};

// n contiguous uint16 from LDS to `seg`, by the wave's 64 lanes: 32-bit words where the segment starts on one.
__device__ __forceinline__ void store_segment(uint16_t* seg, const uint16_t* s, int n, int tx) {
    if ((reinterpret_cast<uintptr_t>(seg) & 3u) == 0) {
        uint32_t* seg32 = reinterpret_cast<uint32_t*>(seg);
        const uint32_t* out32 = reinterpret_cast<const uint32_t*>(s);
        for (int j = tx; j < n / 2; j += 64) seg32[j] = out32[j];
        if ((n & 1) && tx == 0) seg[n - 1] = s[n - 1];
    } else {
        for (int j = tx; j < n; j += 64) seg[j] = s[j];
    }
}

// The tile grid is anchored to the frame's column 0 (tile origins at multiples of 64: load_pair's x stays even) and to the call's
// first row.  Every phase is taken from frame coordinates: 64 and 32 are no multiples of 6.
__global__ __launch_bounds__(256) void xtrans_full_kernel(const XTransArgs a) {
    __shared__ r2f_xtrans_params s_p;
    __shared__ __align__(16) uint16_t s_s[kSH * kSW];
    __shared__ __align__(16) int s_d[kDH * kDW];
    __shared__ __align__(16) uint16_t s_out[4][3 * kTW];
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * 64 + tx;
    const int tx0 = (int)blockIdx.x * kTW, ty0 = a.y0 + blockIdx.y * kTH;
    stage_params(a, s_p, tid);
    __syncthreads();
    // the rows this call may read (the entry point has checked that the source window holds them)
    const int ry0 = a.y0 - kReach > 0 ? a.y0 - kReach : 0, ry1 = a.y1 + kReach < a.H ? a.y1 + kReach : a.H;

    for (int i = tid; i < kSH * (kSW / 2); i += 256) {
        const int r = i / (kSW / 2), c = 2 * (i % (kSW / 2));
        const int y = ty0 - kReach + r, x = tx0 - kApronX + c;  // (x is even: the tile origin is a multiple of 64)
        int s0 = 0, s1 = 0;
        if (y >= ry0 && y < ry1) load_pair(a, s_p, y, x, s0, s1);
        s_s[r * kSW + c] = (uint16_t)s0, s_s[r * kSW + c + 1] = (uint16_t)s1;
    }
    __syncthreads();

    const TileS S{s_s, ty0 - kReach, tx0 - kApronX};
    // S - G where B2 of this call's rows reads it: rows [y0 - 1, y1 + 1) of the frame, inside B1's range
    const int dy0 = a.y0 - 1 > 2 ? a.y0 - 1 : 2, dy1 = a.y1 + 1 < a.H - 2 ? a.y1 + 1 : a.H - 2;
    for (int i = tid; i < kDH * kDW; i += 256) {
        const int r = i / kDW, c = i % kDW;
        const int y = ty0 - 1 + r, x = tx0 - 1 + c;
        int d = 0;
        if (y >= dy0 && y < dy1 && x >= 2 && x < a.W - 2) d = xtrans::diff_at(s_p, S, y, x);
        s_d[i] = d;
    }
    __syncthreads();

    const TileD D{s_d, ty0 - 1, tx0 - 1};
    const int x = tx0 + tx;
    const int xb = tx0 + kTW < a.W ? tx0 + kTW : a.W, n = 3 * (xb - tx0);  // this tile's share of a row: columns [tx0, xb)
    for (int q = 0; q < kRowsPerLane; ++q) {
        const int y = ty0 + ty + 4 * q;  // (the same for all 64 lanes of a wave)
        if (y < a.y1 && x < xb) {
            int rgb[3];
            uint16_t out[3];
            xtrans::pixel_rgb(s_p, S, D, a.H, a.W, y, x, rgb);
            xtrans::colour(s_p, rgb, out);
            uint16_t* o = s_out[ty] + 3 * tx;
            o[0] = out[0], o[1] = out[1], o[2] = out[2];
        }
        __syncthreads();
        // the wave's row segment: n contiguous elements of dst
        if (y < a.y1) store_segment(a.dst + ((long long)y * a.W + tx0) * 3, s_out[ty], n, tx);
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void xtrans_reduced_kernel(const XTransArgs a) {
    __shared__ r2f_xtrans_params s_p;
    stage_params(a, s_p, threadIdx.y * 64 + threadIdx.x);
    __syncthreads();
    const int x = blockIdx.x * 64 + threadIdx.x, y = a.y0 + blockIdx.y * 4 + threadIdx.y;
    if (x >= s_p.out_w || y >= a.y1) return;
    const int cy = y & 1, cx = x & 1;  // the cell's phase is (3 cy, 3 cx)
    int q[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const uint16_t* row = a.src + (long long)(3 * y + j - a.src_gy0) * a.pitch + 3 * x;
#pragma unroll
        for (int i = 0; i < 3; ++i) q[3 * j + i] = xtrans::scale_sample(s_p, (int)row[i], (3 * cy + j) * 6 + 3 * cx + i);
    }
    int rgb[3];
    uint16_t out[3];
    xtrans::reduced_rgb(s_p, q, y, x, rgb);
    xtrans::colour(s_p, rgb, out);
    uint16_t* d = a.dst + ((long long)y * s_p.out_w + x) * 3;
    d[0] = out[0], d[1] = out[1], d[2] = out[2];
}

}  // namespace
}  // namespace r2f

// =============================================================================== C ABI
extern "C" {

int r2f_demosaic_xtrans_u16(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W,
                            const r2f_xtrans_params* params, uint16_t* dst_u16_hwc3, int y0, int y1, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    const char* what = "demosaic_xtrans_u16";
    constexpr int kMaxSide = 1 << 17;  // (the reduced grid has a block per four rows; indices go through long long)
    if (!src_rows || !params || !dst_u16_hwc3 || H < 6 || W < 6 || H > kMaxSide || W > kMaxSide || src_pitch < W || src_gy0 < 0 ||
        src_nrows < 0)
        return fail(ctx, R2F_EINVAL, "%s: a mosaic of at least 6 x 6 samples, a pitch of at least W and a source window are required", what);
    const r2f_xtrans_params& p = *params;
    const bool reduced = p.reduced != 0;
    r2f_xtrans_params check;  // the tables index LDS: they must be the planner's
    memcpy(&check, &p, sizeof check);
    if (!xtrans_tables(p.cfa, reduced, &check) || memcmp(&check, &p, sizeof check) != 0)
        return fail(ctx, R2F_EINVAL, "%s: the params' tables are not those of an admissible pattern (r2f_xtrans_plan makes them)", what);
    if (p.out_h != (reduced ? H / 3 : H) || p.out_w != (reduced ? W / 3 : W))
        return fail(ctx, R2F_EINVAL, "%s: the params are those of another frame size (r2f_xtrans_plan)", what);
    if (y0 < 0 || y1 > p.out_h || y0 > y1)
        return fail(ctx, R2F_EINVAL, "%s: rows [%d, %d) not inside the output's [0, %d)", what, y0, y1, p.out_h);
    if (y0 == y1) return R2F_OK;
    const int lo = reduced ? 3 * y0 : (y0 - kReach > 0 ? y0 - kReach : 0), hi = reduced ? 3 * y1 : (y1 + kReach < H ? y1 + kReach : H);
    if (lo < src_gy0 || (long long)hi > (long long)src_gy0 + src_nrows)
        return fail(ctx, R2F_EINVAL, "%s: rows [%d, %d) read mosaic rows [%d, %d), the source window holds [%d, %lld)", what, y0, y1, lo, hi,
                    src_gy0, (long long)src_gy0 + src_nrows);
    const int wide = ((reinterpret_cast<uintptr_t>(src_rows) & 3u) == 0 && src_pitch % 2 == 0) ? 1 : 0;
    const XTransArgs a{src_rows, src_gy0, (long long)src_pitch, H, W, p, dst_u16_hwc3, y0, y1, wide};
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (reduced)
        launch_k(xtrans_reduced_kernel, dim3((p.out_w + 63) / 64, (y1 - y0 + 3) / 4), dim3(64, 4), 0, s, a);
    else
        launch_k(xtrans_full_kernel, dim3((W + kTW - 1) / kTW, (y1 - y0 + kTH - 1) / kTH), dim3(64, 4), 0, s, a);
    R2F_HIP(ctx, take_launch_status());
    return R2F_OK;
}

}  // extern "C"
