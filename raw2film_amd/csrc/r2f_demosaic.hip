// r2f_demosaic.hip -- the Bayer demosaic ahead of the uint16 hand-off (include/r2f.h: r2f_demosaic_u16, r2f_demosaic_f32), its two
// kernels next to their entry points.  The arithmetic is r2f_demosaic_math.h's (the text tests/demosaic_check.cpp compiles for the
// CPU); this file adds the staging: which samples a block holds in LDS, how they are loaded and how the finished pixels leave.
//   demosaic_full_kernel   one launch: scaled tile + 4-sample apron in LDS, green plane + 1-sample apron in LDS, then B2 / B3 / C
//   demosaic_half_kernel   one lane per output pixel of the half-size form
// Each is a template over its epilogue: the uint16 frame (r2f_demosaic_u16), or a window of it decoded to the float frame the front
// stage reads (r2f_demosaic_f32: decode_sample of r2f_device.h on each finished sample) -- the staging is the same text.
// Neither runs inside r2f_render or a timed step.
#include <cstdint>
#include <type_traits>

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
// 5760 + 4488 bytes of LDS per block for the samples and the green plane, and the row buffer of the epilogue: 1536 (uint16) or
// 3072 (float) -- 11.5 or 13 KB: a dozen blocks fit a CU's 160 KB either way, so the wave slots are the limit, not LDS

struct DemosaicArgs {
    const uint16_t* src;  // row src_gy0 of the mosaic
    int src_gy0;
    long long pitch;  // samples
    int H, W;
    r2f_demosaic_params p;
    void* dst;   // row dst_y0, column x0 of the demosaiced frame D: rows of x1 - x0 pixels, uint16 or float
    int y0, y1;  // the rows of D this call writes
    int wide;    // 1: src is 4-byte aligned and the pitch even -> a pair of samples at an even x is one 32-bit load
    int dst_y0, x0, x1;     // the window of D that dst holds (r2f_demosaic_u16: all of it)
    float divisor, factor;  // the float epilogue's
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

// What leaves: the finished uint16 sample, or its decode to the float frame.
template <bool F32>
using OutT = std::conditional_t<F32, float, uint16_t>;
template <bool F32>
__device__ __forceinline__ OutT<F32> finish_sample(const DemosaicArgs& a, uint16_t v) {
    if constexpr (F32)
        return decode_sample(v, a.divisor, a.factor);
    else
        return v;
}

// n contiguous elements from LDS to `seg`, by the wave's 64 lanes, in stores as wide as seg's alignment allows: uint16 as 32-bit
// words where the segment starts on one; float as 16-byte stores behind the up to three floats that lead to a 16-byte boundary.
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
__device__ __forceinline__ void store_segment(float* seg, const float* s, int n, int tx) {
    int head = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(seg) & 15u)) & 15u) >> 2;  // (seg is 4-byte aligned)
    head = head < n ? head : n;
    const int quads = (n - head) / 4;
    if (tx < head) seg[tx] = s[tx];
    float4* seg4 = reinterpret_cast<float4*>(seg + head);
    for (int j = tx; j < quads; j += 64) {
        const float* q = s + head + 4 * j;
        seg4[j] = make_float4(q[0], q[1], q[2], q[3]);
    }
    for (int j = head + 4 * quads + tx; j < n; j += 64) seg[j] = s[j];
}

// The tile grid is anchored to the frame's columns (tile origins at multiples of 64, so that load_pair's x stays even whatever the
// window's col0) and to the call's first row; lanes outside the window's columns compute nothing and store nothing.
template <bool F32>
__global__ __launch_bounds__(256) void demosaic_full_kernel(const DemosaicArgs a) {
    __shared__ __align__(16) uint16_t s_s[kSH * kSW];
    __shared__ __align__(16) uint16_t s_g[kGH * kGW];
    __shared__ __align__(16) OutT<F32> s_out[4][3 * kTW];
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * 64 + tx;
    const int tx0 = (a.x0 / kTW + (int)blockIdx.x) * kTW, ty0 = a.y0 + blockIdx.y * kTH;
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
    // this tile's share of a row of the window: columns [xa, xb), n elements
    const int xa = tx0 > a.x0 ? tx0 : a.x0, xb = tx0 + kTW < a.x1 ? tx0 + kTW : a.x1, n = 3 * (xb - xa);
    for (int q = 0; q < kRowsPerLane; ++q) {
        const int y = ty0 + ty + 4 * q;  // (the same for all 64 lanes of a wave)
        if (y < a.y1 && x >= xa && x < xb) {
            int rgb[3];
            uint16_t out[3];
            demosaic::pixel_rgb(a.p, S, G, a.H, a.W, y, x, rgb);
            demosaic::colour(a.p, rgb, out);
            OutT<F32>* o = s_out[ty] + 3 * (x - xa);
            o[0] = finish_sample<F32>(a, out[0]), o[1] = finish_sample<F32>(a, out[1]), o[2] = finish_sample<F32>(a, out[2]);
        }
        __syncthreads();
        // the wave's row segment: n contiguous elements of dst
        if (y < a.y1)
            store_segment(static_cast<OutT<F32>*>(a.dst) + ((long long)(y - a.dst_y0) * (a.x1 - a.x0) + (xa - a.x0)) * 3, s_out[ty], n, tx);
        __syncthreads();
    }
}

template <bool F32>
__global__ __launch_bounds__(256) void demosaic_half_kernel(const DemosaicArgs a) {
    const int x = a.x0 + blockIdx.x * 64 + threadIdx.x, y = a.y0 + blockIdx.y * 4 + threadIdx.y;
    if (x >= a.x1 || y >= a.y1) return;
    int q[4];
    load_pair(a, 2 * y, 2 * x, q[0], q[1]);  // (W is even: both samples of a pair are inside)
    load_pair(a, 2 * y + 1, 2 * x, q[2], q[3]);
    int rgb[3];
    uint16_t out[3];
    demosaic::half_rgb(a.p, q, rgb);
    demosaic::colour(a.p, rgb, out);
    OutT<F32>* d = static_cast<OutT<F32>*>(a.dst) + ((long long)(y - a.dst_y0) * (a.x1 - a.x0) + (x - a.x0)) * 3;
    d[0] = finish_sample<F32>(a, out[0]), d[1] = finish_sample<F32>(a, out[1]), d[2] = finish_sample<F32>(a, out[2]);
}

// Both entry points: the checks, then one launch.  The window (row0, col0, rows, cols) of the demosaiced frame is what dst holds;
// [y0, y1) are rows of the window.  `what` names the entry point in messages.
template <bool F32>
int demosaic_rows(r2f_ctx* ctx, const char* what, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W,
                  const r2f_demosaic_params* params, const int* window, float divisor, float factor, void* dst, int y0, int y1,
                  void* stream) {
    constexpr int kMaxSide = 1 << 17;  // (the half-size grid has a block per four rows; indices go through long long)
    if (!src_rows || !params || !dst || H < 2 || W < 2 || H > kMaxSide || W > kMaxSide || src_pitch < W || src_gy0 < 0 || src_nrows < 0)
        return fail(ctx, R2F_EINVAL, "%s: a mosaic of at least 2 x 2 samples, a pitch of at least W and a source window are required", what);
    const r2f_demosaic_params& p = *params;
    int count[3] = {0, 0, 0};
    for (int k = 0; k < 4; ++k) {
        if (p.cfa[k] < 0 || p.cfa[k] > 2) return fail(ctx, R2F_EINVAL, "%s: colour id %d at site %d", what, p.cfa[k], k);
        ++count[p.cfa[k]];
    }
    const bool diagonal = (p.cfa[0] == 1 && p.cfa[3] == 1) || (p.cfa[1] == 1 && p.cfa[2] == 1);  // the greens of a quad
    if (count[0] != 1 || count[1] != 2 || count[2] != 1 || !diagonal)
        return fail(ctx, R2F_EINVAL, "%s: not a Bayer pattern (r2f_demosaic_plan makes one)", what);
    const bool half = p.half_size != 0;
    if (half && ((H | W) & 1)) return fail(ctx, R2F_EINVAL, "%s: the half-size form needs an even frame, got %d x %d", what, H, W);
    if (p.out_h != (half ? H / 2 : H) || p.out_w != (half ? W / 2 : W))
        return fail(ctx, R2F_EINVAL, "%s: the params are those of another frame size (r2f_demosaic_plan)", what);
    const int row0 = window ? window[0] : 0, col0 = window ? window[1] : 0, rows = window ? window[2] : p.out_h,
              cols = window ? window[3] : p.out_w;
    if (row0 < 0 || col0 < 0 || rows <= 0 || cols <= 0 || rows > p.out_h - row0 || cols > p.out_w - col0)
        return fail(ctx, R2F_EINVAL, "%s: the window (%d, %d, %d, %d) is empty or not inside the %d x %d frame", what, row0, col0, rows, cols,
                    p.out_h, p.out_w);
    if (y0 < 0 || y1 > rows || y0 > y1) return fail(ctx, R2F_EINVAL, "%s: rows [%d, %d) not inside the output's [0, %d)", what, y0, y1, rows);
    if (F32 && (!(divisor > 0.f) || (reinterpret_cast<uintptr_t>(dst) & 3u)))
        return fail(ctx, R2F_EINVAL, "%s: a positive divisor and a 4-byte aligned destination are required", what);
    if (y0 == y1) return R2F_OK;
    const int fy0 = row0 + y0, fy1 = row0 + y1;  // the rows of the demosaiced frame
    const int lo = half ? 2 * fy0 : (fy0 - 4 > 0 ? fy0 - 4 : 0), hi = half ? 2 * fy1 : (fy1 + 4 < H ? fy1 + 4 : H);
    if (lo < src_gy0 || (long long)hi > (long long)src_gy0 + src_nrows)
        return fail(ctx, R2F_EINVAL, "%s: rows [%d, %d) read mosaic rows [%d, %d), the source window holds [%d, %lld)", what, y0, y1, lo, hi,
                    src_gy0, (long long)src_gy0 + src_nrows);
    const int wide = ((reinterpret_cast<uintptr_t>(src_rows) & 3u) == 0 && src_pitch % 2 == 0) ? 1 : 0;
    const DemosaicArgs a{src_rows, src_gy0, (long long)src_pitch, H, W, p, dst, fy0, fy1, wide, row0, col0, col0 + cols, divisor, factor};
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (half) {
        launch_k(demosaic_half_kernel<F32>, dim3((cols + 63) / 64, (y1 - y0 + 3) / 4), dim3(64, 4), 0, s, a);
    } else {
        const int tiles_x = (col0 + cols - 1) / kTW - col0 / kTW + 1;  // (the whole frame: ceil(W / 64), tiles from column 0)
        launch_k(demosaic_full_kernel<F32>, dim3(tiles_x, (y1 - y0 + kTH - 1) / kTH), dim3(64, 4), 0, s, a);
    }
    R2F_HIP(ctx, take_launch_status());
    return R2F_OK;
}

}  // namespace
}  // namespace r2f

// =============================================================================== C ABI
extern "C" {

int r2f_demosaic_u16(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W,
                     const r2f_demosaic_params* params, uint16_t* dst_u16_hwc3, int y0, int y1, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    return demosaic_rows<false>(ctx, "demosaic_u16", src_rows, src_gy0, src_nrows, src_pitch, H, W, params, nullptr, 1.f, 1.f, dst_u16_hwc3,
                                y0, y1, stream);
}

int r2f_demosaic_f32(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W,
                     const r2f_demosaic_params* params, int row0, int col0, int rows, int cols, float divisor, float factor,
                     float* dst_f32_hwc3, int y0, int y1, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    const int window[4] = {row0, col0, rows, cols};
    return demosaic_rows<true>(ctx, "demosaic_f32", src_rows, src_gy0, src_nrows, src_pitch, H, W, params, window, divisor, factor,
                               dst_f32_hwc3, y0, y1, stream);
}

}  // extern "C"
