// r2f_xtrans.hip -- the X-Trans demosaic ahead of the uint16 hand-off (include/r2f.h: r2f_demosaic_xtrans_u16): what the X-Trans
// pattern supplies to the staging of r2f_mosaic_stage.h (kernels, LDS tiles, loads, stores and the entry point's checks), and its
// four entry points, each of which names what it passes in a MosaicCall and hands it to mosaic_rows.  The arithmetic is
// r2f_xtrans_math.h's (the text tests/xtrans_check.cpp compiles for the CPU).  Five kernels: the
// full and the reduced (third) size with the uint16 epilogue, and for r2f_demosaic_xtrans_oriented_u16 the mirrored and the turned
// full size and the oriented reduced size; the float epilogue and the window exist in the staging and are not instantiated for this
// pattern.  Five more with Blend for r2f_demosaic_xtrans_blend_u16: the same staging and LDS.  And five median kernels for
// r2f_demosaic_xtrans_median_u16 (step M; r2f_mosaic_stage.h has them and their LDS).
// LDS per block of the full size: 900 (tables) + 5472 (72 x 38 samples) + 8976 (differences, 66 x 34 int32: 17 bits) + 1536 (row
// buffers, upright or mirrored) = 16.9 KB: nine blocks fit a CU's 160 KB, more than its wave slots take at 256 threads.  The turned
// class holds the whole tile in O's layout in place of the row buffers, 64 rows of 196 bytes = 12544: 27.9 KB, five blocks a CU --
// 20 waves of its 32
#include <cstring>

#include "r2f_mosaic_stage.h"  // (first: the HIP runtime, whose qualifiers the math headers use)

#include "r2f_xtrans_math.h"

using namespace r2f;

namespace r2f {
namespace {

struct XTransPattern {
    using Params = r2f_xtrans_params;
    using Aux = int;  // the colour difference S - G
    static constexpr int kMinSide = 6, kReduction = 3;
    static constexpr int kReachY = 3;  // B1 reaches 2 samples, B2 one more
    static constexpr int kApronX = 4;  // kReachY rounded up to a pair
    static constexpr int kAuxRing = 2;  // B1's range; B2 reads S - G nowhere else
    static constexpr bool kParamsInLds = true;  // a lane indexes the planner's tables by its phase
    static constexpr const char* kPlanner = "r2f_xtrans_plan";

    static bool reduced(const Params& p) { return p.reduced != 0; }

    static int check_params(r2f_ctx* ctx, const char* what, const Params& p, int, int) {
        Params check;  // the tables index LDS: they must be the planner's
        memcpy(&check, &p, sizeof check);
        if (!xtrans_tables(p.cfa, reduced(p), &check) || memcmp(&check, &p, sizeof check) != 0)
            return fail(ctx, R2F_EINVAL, "%s: the params' tables are not those of an admissible pattern (r2f_xtrans_plan makes them)", what);
        return R2F_OK;
    }

    // the phase of a sample is (y % 6) * 6 + x % 6.  A pair left of the frame (x < 0) is discarded by the caller: it gets a phase that
    // indexes the tables all the same
    static __device__ __forceinline__ void scale_pair(const Params& p, int y, int x, int r0, int r1, int& v0, int& v1) {
        const int px = x >= 0 ? x % 6 : 0, row_ph = (y % 6) * 6;
        v0 = xtrans::scale_sample(p, r0, row_ph + px), v1 = xtrans::scale_sample(p, r1, row_ph + xtrans::wrap6(px + 1));
    }
    template <typename SFn>
    static __device__ __forceinline__ int aux_at(const Params& p, const SFn& S, int, int, int y, int x) {
        return xtrans::diff_at(p, S, y, x);
    }
    template <typename SFn, typename DFn>
    static __device__ __forceinline__ void pixel_rgb(const Params& p, const SFn& S, const DFn& D, int H, int W, int y, int x, int (&rgb)[3]) {
        xtrans::pixel_rgb(p, S, D, H, W, y, x, rgb);
    }
    // B': the cell at (3 y, 3 x), whose phase is (3 cy, 3 cx); its rows start at odd columns too, so no pair loads
    static __device__ __forceinline__ void reduced_rgb(const MosaicArgs<Params>& a, const Params& p, int y, int x, int (&rgb)[3]) {
        const int cy = y & 1, cx = x & 1;
        int q[9];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const uint16_t* row = a.src + (long long)(3 * y + j - a.src_gy0) * a.pitch + 3 * x;
#pragma unroll
            for (int i = 0; i < 3; ++i) q[3 * j + i] = xtrans::scale_sample(p, (int)row[i], (3 * cy + j) * 6 + 3 * cx + i);
        }
        xtrans::reduced_rgb(p, q, y, x, rgb);
    }
};

}  // namespace
}  // namespace r2f

// =============================================================================== C ABI
// Each entry point fills a MosaicCall: the head and the tail all share, then what it alone takes, by name.
extern "C" {

int r2f_demosaic_xtrans_u16(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W,
                            const r2f_xtrans_params* params, uint16_t* dst_u16_hwc3, int y0, int y1, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    return mosaic_rows<XTransPattern, false>(ctx, params,
                                             {"demosaic_xtrans_u16", src_rows, src_gy0, src_nrows, src_pitch, H, W, dst_u16_hwc3, y0, y1, stream});
}

int r2f_demosaic_xtrans_oriented_u16(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W,
                                     const r2f_xtrans_params* params, int orientation, uint16_t* dst_u16_hwc3, int y0, int y1,
                                     void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    MosaicCall c{"demosaic_xtrans_oriented_u16", src_rows, src_gy0, src_nrows, src_pitch, H, W, dst_u16_hwc3, y0, y1, stream};
    c.orientation = orientation;
    return mosaic_rows<XTransPattern, false>(ctx, params, c);
}

// The same kernels with Blend between the interpolation and step C (five more)
int r2f_demosaic_xtrans_blend_u16(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W,
                                  const r2f_xtrans_params* params, int orientation, int clip, uint16_t* dst_u16_hwc3, int y0, int y1,
                                  void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    MosaicCall c{"demosaic_xtrans_blend_u16", src_rows, src_gy0, src_nrows, src_pitch, H, W, dst_u16_hwc3, y0, y1, stream};
    c.form = MosaicForm::kBlend, c.orientation = orientation, c.clip = clip;
    return mosaic_rows<XTransPattern, false>(ctx, params, c);
}

// Step M between the interpolation and Blend (clip 0: no Blend): the median kernels of r2f_mosaic_stage.h
int r2f_demosaic_xtrans_median_u16(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W,
                                   const r2f_xtrans_params* params, int orientation, int clip, int passes, uint16_t* dst_u16_hwc3, int y0,
                                   int y1, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    MosaicCall c{"demosaic_xtrans_median_u16", src_rows, src_gy0, src_nrows, src_pitch, H, W, dst_u16_hwc3, y0, y1, stream};
    c.form = MosaicForm::kMedian, c.orientation = orientation, c.clip = clip, c.passes = passes;
    return mosaic_rows<XTransPattern, false>(ctx, params, c);
}

}  // extern "C"
