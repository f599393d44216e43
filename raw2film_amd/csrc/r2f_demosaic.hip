// r2f_demosaic.hip -- the Bayer demosaic ahead of the uint16 hand-off (include/r2f.h: r2f_demosaic_u16), its two kernels next to
// their entry point.  The arithmetic is r2f_demosaic_math.h's (the text tests/demosaic_check.cpp compiles for the CPU); this file
// adds the staging: which samples a block holds in LDS, how they are loaded and how the finished pixels leave.
//   demosaic_full_kernel   one launch: scaled tile + 4-sample apron in LDS, green plane + 1-sample apron in LDS, then B2 / B3 / C
//   demosaic_half_kernel   one lane per output pixel of the half-size form
// Neither runs inside r2f_render or a timed step.
#include <cstdint>

#include "r2f_ctx.h"
#include "r2f_demosaic_math.h"

using namespace r2f;

namespace r2f {
namespace {

constexpr int kTW = R2F_DEMOSAIC_TILE_W, kTH = R2F_DEMOSAIC_TILE_H;  // lanes along x: a wave is one row of the tile
constexpr int kApron = 4;                                            // B1 reaches 3 samples, B2 / B3 one more
constexpr int kSW = kTW + 2 * kApron, kSH = kTH + 2 * kApron;        // the scaled samples: 72 x 40
constexpr int kGW = kTW + 2, kGH = kTH + 2;                          // the green plane: 66 x 34
constexpr int kRowsPerLane = kTH / 4;
static_assert(kTW == 64 && kTH % 4 == 0 && kSW % 2 == 0, "a wave per tile row, workgroups of (64, 4), the samples loaded in pairs");
// 5760 + 4488 + 1536 bytes of LDS per block: a dozen blocks fit a CU's 160 KB, so the wave slots are the limit, not LDS

struct DemosaicArgs {
    const uint16_t* src;  // row src_gy0 of the mosaic
    int src_gy0;
    long long pitch;  // samples
    int H, W;
    r2f_demosaic_params p;
    uint16_t* dst;
    int y0, y1;
    int wide;  // 1: src is 4-byte aligned and the pitch even -> a pair of samples at an even x is one 32-bit load
};

// The samples (y, x) and (y, x + 1), x even, scaled (step A); 0 for one outside the frame.  One 32-bit load where that is allowed
// and both are inside, else one 16-bit load each: the same samples either way.
__device__ __forceinline__ void load_pair(const DemosaicArgs& a, int y, int x, int& s0, int& s1) {
    const bool in0 = x >= 0 && x < a.W, in1 = in0 && x + 1 < a.W;
    unsigned r0 = 0, r1 = 0;
    if (in0) {
        const uint16_t* row = a.src + (long long)(y - a.src_gy0) * a.pitch;
        if (in1 && a.wide) {
            const uint32_t v = *reinterpret_cast<const uint32_t*>(row + x);
            r0 = v & 0xFFFFu, r1 = v >> 16;
        } else {
            r0 = row[x];
            if (in1) r1 = row[x + 1];
        }
    }
    const int k = (y & 1) * 2;
    const int v0 = demosaic::scale_sample(a.p, (int)r0, k), v1 = demosaic::scale_sample(a.p, (int)r1, k + 1);
    s0 = in0 ? v0 : 0, s1 = in1 ? v1 : 0;
}

struct TileS {  // the scaled samples of a block, at frame coordinates
    const uint16_t* s;
    int y_org, x_org;  // frame coordinates of s[0]
    __device__ __forceinline__ int operator()(int y, int x) const { return s[(y - y_org) * kSW + (x - x_org)]; }
};
struct TileG {  // its green plane
    const uint16_t* g;
    int y_org, x_org;
    __device__ __forceinline__ int operator()(int y, int x) const { return g[(y - y_org) * kGW + (x - x_org)]; }
};

__global__ __launch_bounds__(256) void demosaic_full_kernel(const DemosaicArgs a) {
    __shared__ __align__(16) uint16_t s_s[kSH * kSW];
    __shared__ __align__(16) uint16_t s_g[kGH * kGW];
    __shared__ __align__(16) uint16_t s_out[4][3 * kTW];
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * 64 + tx;
    const int tx0 = blockIdx.x * kTW, ty0 = a.y0 + blockIdx.y * kTH;
    // the rows this call may read (the entry point has checked that the source window holds them)
    const int ry0 = a.y0 - kApron > 0 ? a.y0 - kApron : 0, ry1 = a.y1 + kApron < a.H ? a.y1 + kApron : a.H;

    for (int i = tid; i < kSH * (kSW / 2); i += 256) {
        const int r = i / (kSW / 2), c = 2 * (i % (kSW / 2));
        const int y = ty0 - kApron + r, x = tx0 - kApron + c;  // (x is even: the tile origin is a multiple of 64)
        int s0 = 0, s1 = 0;
        if (y >= ry0 && y < ry1) load_pair(a, y, x, s0, s1);
        s_s[r * kSW + c] = (uint16_t)s0, s_s[r * kSW + c + 1] = (uint16_t)s1;
    }
    __syncthreads();

    const TileS S{s_s, ty0 - kApron, tx0 - kApron};
    // green where B2 / B3 of this call's rows read it: rows [y0 - 1, y1 + 1) of the frame
    const int gy0 = a.y0 - 1 > 0 ? a.y0 - 1 : 0, gy1 = a.y1 + 1 < a.H ? a.y1 + 1 : a.H;
    for (int i = tid; i < kGH * kGW; i += 256) {
        const int r = i / kGW, c = i % kGW;
        const int y = ty0 - 1 + r, x = tx0 - 1 + c;
        int g = 0;
        if (y >= gy0 && y < gy1 && x >= 0 && x < a.W) g = demosaic::green_at(a.p, S, a.H, a.W, y, x);
        s_g[i] = (uint16_t)g;
    }
    __syncthreads();

    const TileG G{s_g, ty0 - 1, tx0 - 1};
    const int x = tx0 + tx;
    const int cols = a.W - tx0 < kTW ? a.W - tx0 : kTW, n = 3 * cols;  // uint16 elements of this tile's share of a row
    for (int q = 0; q < kRowsPerLane; ++q) {
        const int y = ty0 + ty + 4 * q;  // (the same for all 64 lanes of a wave)
        if (y < a.y1 && x < a.W) {
            int rgb[3];
            uint16_t out[3];
            demosaic::pixel_rgb(a.p, S, G, a.H, a.W, y, x, rgb);
            demosaic::colour(a.p, rgb, out);
            s_out[ty][3 * tx] = out[0], s_out[ty][3 * tx + 1] = out[1], s_out[ty][3 * tx + 2] = out[2];
        }
        __syncthreads();
        if (y < a.y1) {
            // the wave's row segment: n contiguous uint16 of dst, as 32-bit words where the segment starts on one
            uint16_t* seg = a.dst + ((long long)y * a.p.out_w + tx0) * 3;
            if ((reinterpret_cast<uintptr_t>(seg) & 3u) == 0) {
                uint32_t* seg32 = reinterpret_cast<uint32_t*>(seg);
                const uint32_t* out32 = reinterpret_cast<const uint32_t*>(s_out[ty]);
                for (int j = tx; j < n / 2; j += 64) seg32[j] = out32[j];
                if ((n & 1) && tx == 0) seg[n - 1] = s_out[ty][n - 1];
            } else {
                for (int j = tx; j < n; j += 64) seg[j] = s_out[ty][j];
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void demosaic_half_kernel(const DemosaicArgs a) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = a.y0 + blockIdx.y * 4 + threadIdx.y;
    if (x >= a.p.out_w || y >= a.y1) return;
    int q[4];
    load_pair(a, 2 * y, 2 * x, q[0], q[1]);  // (W is even: both samples of a pair are inside)
    load_pair(a, 2 * y + 1, 2 * x, q[2], q[3]);
    int rgb[3];
    uint16_t out[3];
    demosaic::half_rgb(a.p, q, rgb);
    demosaic::colour(a.p, rgb, out);
    uint16_t* d = a.dst + ((long long)y * a.p.out_w + x) * 3;
    d[0] = out[0], d[1] = out[1], d[2] = out[2];
}

}  // namespace
}  // namespace r2f

// =============================================================================== C ABI
extern "C" {

int r2f_demosaic_u16(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W,
                     const r2f_demosaic_params* params, uint16_t* dst_u16_hwc3, int y0, int y1, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    constexpr int kMaxSide = 1 << 17;  // (the half-size grid has a block per four rows; indices go through long long)
    if (!src_rows || !params || !dst_u16_hwc3 || H < 2 || W < 2 || H > kMaxSide || W > kMaxSide || src_pitch < W || src_gy0 < 0 ||
        src_nrows < 0)
        return fail(ctx, R2F_EINVAL, "demosaic_u16: a mosaic of at least 2 x 2 samples, a pitch of at least W and a source window are required");
    const r2f_demosaic_params& p = *params;
    int count[3] = {0, 0, 0};
    for (int k = 0; k < 4; ++k) {
        if (p.cfa[k] < 0 || p.cfa[k] > 2) return fail(ctx, R2F_EINVAL, "demosaic_u16: colour id %d at site %d", p.cfa[k], k);
        ++count[p.cfa[k]];
    }
    const bool diagonal = (p.cfa[0] == 1 && p.cfa[3] == 1) || (p.cfa[1] == 1 && p.cfa[2] == 1);  // the greens of a quad
    if (count[0] != 1 || count[1] != 2 || count[2] != 1 || !diagonal)
        return fail(ctx, R2F_EINVAL, "demosaic_u16: not a Bayer pattern (r2f_demosaic_plan makes one)");
    const bool half = p.half_size != 0;
    if (half && ((H | W) & 1)) return fail(ctx, R2F_EINVAL, "demosaic_u16: the half-size form needs an even frame, got %d x %d", H, W);
    if (p.out_h != (half ? H / 2 : H) || p.out_w != (half ? W / 2 : W))
        return fail(ctx, R2F_EINVAL, "demosaic_u16: the params are those of another frame size (r2f_demosaic_plan)");
    if (y0 < 0 || y1 > p.out_h || y0 > y1)
        return fail(ctx, R2F_EINVAL, "demosaic_u16: rows [%d, %d) not inside the output's [0, %d)", y0, y1, p.out_h);
    if (y0 == y1) return R2F_OK;
    const int lo = half ? 2 * y0 : (y0 - 4 > 0 ? y0 - 4 : 0), hi = half ? 2 * y1 : (y1 + 4 < H ? y1 + 4 : H);
    if (lo < src_gy0 || (long long)hi > (long long)src_gy0 + src_nrows)
        return fail(ctx, R2F_EINVAL, "demosaic_u16: rows [%d, %d) read mosaic rows [%d, %d), the source window holds [%d, %lld)", y0, y1, lo,
                    hi, src_gy0, (long long)src_gy0 + src_nrows);
    const int wide = ((reinterpret_cast<uintptr_t>(src_rows) & 3u) == 0 && src_pitch % 2 == 0) ? 1 : 0;
    const DemosaicArgs a{src_rows, src_gy0, (long long)src_pitch, H, W, p, dst_u16_hwc3, y0, y1, wide};
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (half)
        launch_k(demosaic_half_kernel, dim3((p.out_w + 63) / 64, (y1 - y0 + 3) / 4), dim3(64, 4), 0, s, a);
    else
        launch_k(demosaic_full_kernel, dim3((W + kTW - 1) / kTW, (y1 - y0 + kTH - 1) / kTH), dim3(64, 4), 0, s, a);
    R2F_HIP(ctx, take_launch_status());
    return R2F_OK;
}

}  // extern "C"
