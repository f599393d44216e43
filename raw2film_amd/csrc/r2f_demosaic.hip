// r2f_demosaic.hip -- the Bayer demosaic ahead of the uint16 hand-off (include/r2f.h: r2f_demosaic_u16, r2f_demosaic_f32): what the
// Bayer pattern supplies to the staging of r2f_mosaic_stage.h (kernels, LDS tiles, loads, stores and the entry points' checks), and
// its seven entry points, each of which names what it passes in a MosaicCall and hands it to mosaic_rows.  The arithmetic is r2f_demosaic_math.h's (the text tests/demosaic_check.cpp compiles for the CPU).  Seven
// kernels: the full and the half size, each with the uint16 and with the float epilogue; and for r2f_demosaic_oriented_u16 the
// mirrored and the turned full size and the oriented half size (uint16).  Seven more with Blend for r2f_demosaic_blend_u16 /
// r2f_demosaic_blend_f32: the same staging and LDS, mosaic::blend_pixel ahead of the matrix (2 more VGPRs at full size).  And seven
// median kernels for r2f_demosaic_median_u16 / r2f_demosaic_median_f32 (step M; r2f_mosaic_stage.h has them and their LDS).
// LDS per block of the full size: 5760 (72 x 40 samples) + 4488 (the green plane, 66 x 34) and the row buffer of the epilogue, 1536
// (uint16, upright or mirrored) or 3072 (float) -- 11.5 or 13 KB: a dozen blocks fit a CU's 160 KB either way, so the wave slots are
// the limit, not LDS.  The turned class holds the whole tile in O's layout instead, 64 rows of 196 bytes = 12544: 22.3 KB, seven
// blocks a CU -- 28 waves of its 32 (the upright kernels keep their 11.5 KB: the class is a template parameter)
#include "r2f_mosaic_stage.h"  // (first: the HIP runtime, whose qualifiers the math headers use)

#include "r2f_demosaic_math.h"

using namespace r2f;

namespace r2f {
namespace {

struct BayerPattern {
    using Params = r2f_demosaic_params;
    using Aux = uint16_t;  // the finished green plane
    static constexpr int kMinSide = 2, kReduction = 2;
    // B1 reaches 3 samples, B2 / B3 one more.  raw2film_amd/payload.py states the same 4 as DEMOSAIC_REACH: what the bands of a
    // streamed mosaic overlap by.
    static constexpr int kReachY = 4, kApronX = 4;
    static constexpr int kAuxRing = 0;  // green has the whole frame for its domain
    static constexpr bool kParamsInLds = false;  // pick4's selects from the kernel's arguments: no lane indexes a table
    static constexpr const char* kPlanner = "r2f_demosaic_plan";

    static bool reduced(const Params& p) { return p.half_size != 0; }

    static int check_params(r2f_ctx* ctx, const char* what, const Params& p, int H, int W) {
        int count[3] = {0, 0, 0};
        for (int k = 0; k < 4; ++k) {
            if (p.cfa[k] < 0 || p.cfa[k] > 2) return fail(ctx, R2F_EINVAL, "%s: colour id %d at site %d", what, p.cfa[k], k);
            ++count[p.cfa[k]];
        }
        const bool diagonal = (p.cfa[0] == 1 && p.cfa[3] == 1) || (p.cfa[1] == 1 && p.cfa[2] == 1);  // the greens of a quad
        if (count[0] != 1 || count[1] != 2 || count[2] != 1 || !diagonal)
            return fail(ctx, R2F_EINVAL, "%s: not a Bayer pattern (r2f_demosaic_plan makes one)", what);
        if (reduced(p) && ((H | W) & 1)) return fail(ctx, R2F_EINVAL, "%s: the half-size form needs an even frame, got %d x %d", what, H, W);
        return R2F_OK;
    }

    // the site of a sample is k = (y & 1) * 2 + (x & 1), and x is even
    static __device__ __forceinline__ void scale_pair(const Params& p, int y, int, int r0, int r1, int& v0, int& v1) {
        const int k = (y & 1) * 2;
        v0 = demosaic::scale_sample(p, r0, k), v1 = demosaic::scale_sample(p, r1, k + 1);
    }
    template <typename SFn>
    static __device__ __forceinline__ int aux_at(const Params& p, const SFn& S, int H, int W, int y, int x) {
        return demosaic::green_at(p, S, H, W, y, x);
    }
    template <typename SFn, typename GFn>
    static __device__ __forceinline__ void pixel_rgb(const Params& p, const SFn& S, const GFn& G, int H, int W, int y, int x, int (&rgb)[3]) {
        demosaic::pixel_rgb(p, S, G, H, W, y, x, rgb);
    }
    // B': the quad at (2 y, 2 x), two pairs
    static __device__ __forceinline__ void reduced_rgb(const MosaicArgs<Params>& a, const Params& p, int y, int x, int (&rgb)[3]) {
        int q[4];
        load_pair<BayerPattern>(a, p, 2 * y, 2 * x, q[0], q[1]);  // (W is even: both samples of a pair are inside)
        load_pair<BayerPattern>(a, p, 2 * y + 1, 2 * x, q[2], q[3]);
        demosaic::half_rgb(p, q, rgb);
    }
};

}  // namespace
}  // namespace r2f

// =============================================================================== C ABI
// Each entry point fills a MosaicCall: the head and the tail all share, then what it alone takes, by name.
extern "C" {

int r2f_demosaic_u16(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W,
                     const r2f_demosaic_params* params, uint16_t* dst_u16_hwc3, int y0, int y1, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    return mosaic_rows<BayerPattern, false>(ctx, params,
                                            {"demosaic_u16", src_rows, src_gy0, src_nrows, src_pitch, H, W, dst_u16_hwc3, y0, y1, stream});
}

int r2f_demosaic_oriented_u16(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W,
                              const r2f_demosaic_params* params, int orientation, uint16_t* dst_u16_hwc3, int y0, int y1, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    MosaicCall c{"demosaic_oriented_u16", src_rows, src_gy0, src_nrows, src_pitch, H, W, dst_u16_hwc3, y0, y1, stream};
    c.orientation = orientation;
    return mosaic_rows<BayerPattern, false>(ctx, params, c);
}

int r2f_demosaic_f32(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W,
                     const r2f_demosaic_params* params, int row0, int col0, int rows, int cols, float divisor, float factor,
                     float* dst_f32_hwc3, int y0, int y1, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    const int window[4] = {row0, col0, rows, cols};
    MosaicCall c{"demosaic_f32", src_rows, src_gy0, src_nrows, src_pitch, H, W, dst_f32_hwc3, y0, y1, stream};
    c.window = window, c.divisor = divisor, c.factor = factor;
    return mosaic_rows<BayerPattern, true>(ctx, params, c);
}

// The same kernels with Blend between the interpolation and step C (seven more: every epilogue and class above)
int r2f_demosaic_blend_u16(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W,
                           const r2f_demosaic_params* params, int orientation, int clip, uint16_t* dst_u16_hwc3, int y0, int y1,
                           void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    MosaicCall c{"demosaic_blend_u16", src_rows, src_gy0, src_nrows, src_pitch, H, W, dst_u16_hwc3, y0, y1, stream};
    c.form = MosaicForm::kBlend, c.orientation = orientation, c.clip = clip;
    return mosaic_rows<BayerPattern, false>(ctx, params, c);
}

int r2f_demosaic_blend_f32(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W,
                           const r2f_demosaic_params* params, int clip, int row0, int col0, int rows, int cols, float divisor, float factor,
                           float* dst_f32_hwc3, int y0, int y1, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    const int window[4] = {row0, col0, rows, cols};
    MosaicCall c{"demosaic_blend_f32", src_rows, src_gy0, src_nrows, src_pitch, H, W, dst_f32_hwc3, y0, y1, stream};
    c.form = MosaicForm::kBlend, c.clip = clip, c.window = window, c.divisor = divisor, c.factor = factor;
    return mosaic_rows<BayerPattern, true>(ctx, params, c);
}

// Step M between the interpolation and Blend (clip 0: no Blend): the median kernels of r2f_mosaic_stage.h
int r2f_demosaic_median_u16(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W,
                            const r2f_demosaic_params* params, int orientation, int clip, int passes, uint16_t* dst_u16_hwc3, int y0, int y1,
                            void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    MosaicCall c{"demosaic_median_u16", src_rows, src_gy0, src_nrows, src_pitch, H, W, dst_u16_hwc3, y0, y1, stream};
    c.form = MosaicForm::kMedian, c.orientation = orientation, c.clip = clip, c.passes = passes;
    return mosaic_rows<BayerPattern, false>(ctx, params, c);
}

int r2f_demosaic_median_f32(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W,
                            const r2f_demosaic_params* params, int clip, int passes, int row0, int col0, int rows, int cols, float divisor,
                            float factor, float* dst_f32_hwc3, int y0, int y1, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    const int window[4] = {row0, col0, rows, cols};
    MosaicCall c{"demosaic_median_f32", src_rows, src_gy0, src_nrows, src_pitch, H, W, dst_f32_hwc3, y0, y1, stream};
    c.form = MosaicForm::kMedian, c.clip = clip, c.passes = passes, c.window = window, c.divisor = divisor, c.factor = factor;
    return mosaic_rows<BayerPattern, true>(ctx, params, c);
}

}  // extern "C"
