// r2f_mosaic_denoise.hip -- the wavelet denoise of a Bayer mosaic (include/r2f.h: r2f_mosaic_denoise; the arithmetic is
// r2f_denoise_math.h's).  Off the render path: one kernel template, its arguments and its entry points (the chain,
// and one level alone for tools/denoise_probe.py).
//   One launch per level (c = 1 << level).  A block of 256 lanes owns a kTW x kTH tile of a plane.  It stages the tile of In with an
//   apron of c samples on all four sides in LDS (s_in), runs the row pass over every staged row into s_row (tile columns only), then
//   the column pass, the threshold and the accumulation per output sample.  The box a block stages is [x0 - c, x0 + kTW + c) x
//   [y0 - c, y0 + kTH + c) clipped to the plane; both taps of every sample it needs reflect in PLANE coordinates and land inside
//   that box (r2f_denoise_math.h: n >= 32 > c), so a position of the box outside the plane is never loaded and never read (it holds 0).
//   The global loads of a block's staging and its D samples are issued together, into registers, ahead of the first LDS store: with
//   a few waves a CU (the LDS of the wide aprons) a load per loop round would pay its latency every round.
//   Level 0 (grid z = 1): the block reads the mosaic rows of its box as pairs of neighbouring samples -- one 32-bit load a lane where
//   the source's alignment and pitch allow, else two 16-bit ones --, lifts both (step 2) into the LDS tiles of their two planes, and
//   then walks its four planes; it writes D and L.
//   Levels 1 .. 3 (grid z = 4 planes): In is the L buffer of the level before, the other L buffer is written, D updated in place by the
//   lane that owns the sample.
//   Level 4 (grid z = 1): the block walks its four planes, finishes step 4 into an LDS image of its 2 kTH mosaic rows and writes them
//   as pairs (32-bit stores where dst allows).
//   LDS: level 0 4 x 34 x 66 + 34 x 64 floats (43.6 KiB); level 4 64 x 96 + 64 x 64 floats and 64 x 64 words (56 KiB).
#include "r2f_ctx.h"
#include "r2f_denoise_math.h"

using namespace r2f;

namespace r2f {
namespace {

constexpr int kTW = 64, kTH = 32, kLanes = 256, kRowsPerLane = kTH / (kLanes / kTW);
static_assert(R2F_DENOISE_TILE_W == kTW && R2F_DENOISE_TILE_H == kTH, "include/r2f.h states the tile");
static_assert(kLanes % kTW == 0 && kTH % (kLanes / kTW) == 0, "a lane keeps its column and walks rows kLanes / kTW apart");

struct DenoiseArgs {
    const uint16_t* src;  // level 0
    long long src_pitch;  // samples
    uint16_t* dst;        // level 4
    long long dst_pitch;
    const float* lin;  // levels 1 .. 4: L of the level before, 4 planes of nr x nc
    float* lout;       // levels 0 .. 3
    float* det;        // D
    int nr, nc;        // a plane's rows and columns
    int black[4];
    int shift;
    float theta;
    int src_pairs, dst_pairs;  // 32-bit accesses of neighbouring samples are aligned
};

template <int LEV>
__global__ __launch_bounds__(kLanes) void denoise_level_kernel(const DenoiseArgs a) {
    constexpr int C = 1 << LEV, IW = kTW + 2 * C, IH = kTH + 2 * C;
    constexpr bool kFirst = LEV == 0, kLast = LEV == denoise::kLevels - 1, kWalk = kFirst || kLast;
    __shared__ float s_in[kFirst ? 4 : 1][IH][IW];
    __shared__ float s_row[IH][kTW];
    __shared__ uint32_t s_out[kLast ? 2 * kTH : 1][kLast ? kTW : 1];  // the block's mosaic rows as pairs (xx = 0 in the low half)
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    const int bx0 = x0 - C, by0 = y0 - C;  // the box's origin in plane coordinates
    const int nr = a.nr, nc = a.nc;
    const size_t plane = (size_t)nr * (size_t)nc;

    if (kFirst) {
        // (every load of the box is issued before the first value is used: two loops over a register array)
        constexpr int kN = (2 * IH * IW + kLanes - 1) / kLanes;
        uint32_t word[kN];
        R2F_UNROLL
        for (int n = 0; n < kN; ++n) {
            const int i = tid + n * kLanes, j = i % IW, rr = i / IW, gy = by0 + (rr >> 1), gx = bx0 + j;
            word[n] = 0;
            if (i < 2 * IH * IW && gy >= 0 && gy < nr && gx >= 0 && gx < nc) {
                const uint16_t* p = a.src + (long long)(2 * gy + (rr & 1)) * a.src_pitch + 2 * gx;
                word[n] = a.src_pairs ? *reinterpret_cast<const uint32_t*>(p) : (uint32_t)p[0] | (uint32_t)p[1] << 16;
            }
        }
        R2F_UNROLL
        for (int n = 0; n < kN; ++n) {
            const int i = tid + n * kLanes, j = i % IW, rr = i / IW, r = rr >> 1, yy = rr & 1;
            if (i >= 2 * IH * IW) break;
            s_in[2 * yy][r][j] = denoise::lift((int)(word[n] & 0xffffu), a.black[2 * yy], a.shift);
            s_in[2 * yy + 1][r][j] = denoise::lift((int)(word[n] >> 16), a.black[2 * yy + 1], a.shift);
        }
    }
    for (int w = 0; w < (kWalk ? 4 : 1); ++w) {
        const int k = kWalk ? w : (int)blockIdx.z;
        const float(*in)[IW] = s_in[kFirst ? k : 0];
        const int x = tid % kTW, gx = x0 + x;
        float prev[kRowsPerLane];  // D of the lane's samples, asked for ahead of the passes
        if (!kFirst) {
            const float* lin = a.lin + (size_t)k * plane;
            constexpr int kN = (IH * IW + kLanes - 1) / kLanes;
            float v[kN];
            R2F_UNROLL
            for (int n = 0; n < kN; ++n) {
                const int i = tid + n * kLanes, j = i % IW, r = i / IW, gy = by0 + r, bx = bx0 + j;
                v[n] = i < IH * IW && gy >= 0 && gy < nr && bx >= 0 && bx < nc ? lin[(size_t)gy * nc + bx] : 0.f;
            }
            R2F_UNROLL
            for (int q = 0; q < kRowsPerLane; ++q) {
                const int gy = y0 + tid / kTW + q * (kLanes / kTW);
                prev[q] = gx < nc && gy < nr ? a.det[(size_t)k * plane + (size_t)gy * nc + gx] : 0.f;
            }
            R2F_UNROLL
            for (int n = 0; n < kN; ++n) {
                const int i = tid + n * kLanes;
                if (i < IH * IW) s_in[0][i / IW][i % IW] = v[n];
            }
        }
        __syncthreads();
        if (gx < nc) {
            const int xm = denoise::reflect_m(gx, C) - bx0, xp = denoise::reflect_p(gx, C, nc) - bx0;
            for (int r = tid / kTW; r < IH; r += kLanes / kTW) {
                const int gy = by0 + r;
                if (gy < 0 || gy >= nr) continue;
                s_row[r][x] = denoise::quarter_hat(in[r][x + C], in[r][xm], in[r][xp]);
            }
        }
        __syncthreads();
        if (gx < nc) {
            R2F_UNROLL
            for (int q = 0; q < kRowsPerLane; ++q) {
                const int y = tid / kTW + q * (kLanes / kTW), gy = y0 + y;
                if (gy >= nr) break;
                const int ym = denoise::reflect_m(gy, C) - by0, yp = denoise::reflect_p(gy, C, nr) - by0;
                const float low = denoise::quarter_hat(s_row[y + C][x], s_row[ym][x], s_row[yp][x]);
                const float dd = denoise::shrink(in[y + C][x + C], low, a.theta);
                const size_t idx = (size_t)k * plane + (size_t)gy * nc + gx;
                float D = dd;
                if (!kFirst) {
                    R2F_NO_CONTRACT
                    D = prev[q] + dd;
                }
                if (kLast) {
                    reinterpret_cast<uint16_t*>(&s_out[2 * y + (k >> 1)][x])[k & 1] = (uint16_t)denoise::finish(D, low);
                } else {
                    a.det[idx] = D;
                    a.lout[idx] = low;
                }
            }
        }
        __syncthreads();  // (the next plane's staging and row pass write what this one's passes read)
    }
    if (kLast) {
        for (int i = tid; i < 2 * kTH * kTW; i += kLanes) {
            const int j = i % kTW, rr = i / kTW;
            const int my = 2 * y0 + rr, gx = x0 + j;
            if (my >= 2 * nr || gx >= nc) continue;
            const uint32_t w = s_out[rr][j];
            uint16_t* p = a.dst + (long long)my * a.dst_pitch + 2 * gx;
            if (a.dst_pairs)
                *reinterpret_cast<uint32_t*>(p) = w;
            else
                p[0] = (uint16_t)(w & 0xffffu), p[1] = (uint16_t)(w >> 16);
        }
    }
}

template <int LEV>
void launch_level(const DenoiseArgs& a, hipStream_t s) {
    const bool walk = LEV == 0 || LEV == denoise::kLevels - 1;
    launch_k(denoise_level_kernel<LEV>, dim3((a.nc + kTW - 1) / kTW, (a.nr + kTH - 1) / kTH, walk ? 1 : 4), dim3(kLanes), 0, s, a);
}

bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + nb && b0 < a0 + na;
}

// The entry points' checks and the launches of levels [lev0, lev1): every level finds its buffers where the whole chain keeps them.
int denoise_levels(r2f_ctx* ctx, const char* what, const uint16_t* src, int64_t src_pitch, int H, int W, const r2f_denoise_params* params,
                   uint16_t* dst, int64_t dst_pitch, void* workspace, size_t workspace_bytes, void* stream, int lev0, int lev1) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (!src || !dst || !params || !workspace) return fail(ctx, R2F_EINVAL, "%s: the source, the destination, the params and the workspace are required", what);
    if (!denoise::side_ok(H) || !denoise::side_ok(W)) return fail(ctx, R2F_EINVAL, "%s: a mosaic of %d x %d samples; both sides must be even and at least %d", what, H, W, denoise::kMinSide);
    if (src_pitch < W || dst_pitch < W) return fail(ctx, R2F_EINVAL, "%s: pitches of at least W = %d samples are required", what, W);
    if (!denoise::params_ok(params->black, params->shift, params->threshold))
        return fail(ctx, R2F_EINVAL, "%s: params the planner does not produce (black levels in [0, 65535], a shift in [0, 15], a threshold in (0, 1e6])", what);
    const size_t need = r2f_mosaic_denoise_workspace_bytes(H, W);
    if (workspace_bytes < need) return fail(ctx, R2F_EINVAL, "%s: a workspace of %zu bytes, %zu are needed", what, workspace_bytes, need);
    if (!aligned16(workspace)) return fail(ctx, R2F_EINVAL, "%s: the workspace must be 16-byte aligned", what);
    const size_t src_span = ((size_t)(H - 1) * (size_t)src_pitch + W) * 2, dst_span = ((size_t)(H - 1) * (size_t)dst_pitch + W) * 2;
    if (ranges_overlap(workspace, need, src, src_span) || ranges_overlap(workspace, need, dst, dst_span))
        return fail(ctx, R2F_EINVAL, "%s: the workspace overlaps the source or the destination", what);
    DenoiseArgs a{};
    a.src = src, a.src_pitch = (long long)src_pitch, a.dst = dst, a.dst_pitch = (long long)dst_pitch;
    a.nr = H / 2, a.nc = W / 2;
    for (int k = 0; k < 4; ++k) a.black[k] = params->black[k];
    a.shift = params->shift;
    a.src_pairs = (reinterpret_cast<uintptr_t>(src) & 3u) == 0 && src_pitch % 2 == 0;
    a.dst_pairs = (reinterpret_cast<uintptr_t>(dst) & 3u) == 0 && dst_pitch % 2 == 0;
    const size_t samples = (size_t)H * (size_t)W;  // floats of one buffer: four planes
    float* const D = static_cast<float*>(workspace);
    float* const La = D + samples;
    float* const Lb = La + samples;
    a.det = D;
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int lev = lev0; lev < lev1; ++lev) {  // L alternates between the two buffers: level 0 writes La, level 4 reads Lb
        a.theta = denoise::theta_of(params->threshold, lev);
        a.lin = lev == 0 ? nullptr : (lev % 2 ? La : Lb);
        a.lout = lev == denoise::kLevels - 1 ? nullptr : (lev % 2 ? Lb : La);
        switch (lev) {
            case 0: launch_level<0>(a, s); break;
            case 1: launch_level<1>(a, s); break;
            case 2: launch_level<2>(a, s); break;
            case 3: launch_level<3>(a, s); break;
            default: launch_level<4>(a, s); break;
        }
    }
    R2F_HIP(ctx, take_launch_status());
    return R2F_OK;
}

}  // namespace
}  // namespace r2f

// =============================================================================== C ABI
extern "C" {

int r2f_mosaic_denoise(r2f_ctx* ctx, const uint16_t* src, int64_t src_pitch, int H, int W, const r2f_denoise_params* params, uint16_t* dst,
                       int64_t dst_pitch, void* workspace, size_t workspace_bytes, void* stream) {
    return denoise_levels(ctx, "mosaic_denoise", src, src_pitch, H, W, params, dst, dst_pitch, workspace, workspace_bytes, stream, 0, denoise::kLevels);
}

int r2f_mosaic_denoise_level(r2f_ctx* ctx, int level, const uint16_t* src, int64_t src_pitch, int H, int W, const r2f_denoise_params* params,
                             uint16_t* dst, int64_t dst_pitch, void* workspace, size_t workspace_bytes, void* stream) {
    if (!ctx) return R2F_EINVAL;
    if (level < 0 || level >= denoise::kLevels) return fail(ctx, R2F_EINVAL, "mosaic_denoise_level: level %d outside 0 .. 4", level);
    return denoise_levels(ctx, "mosaic_denoise_level", src, src_pitch, H, W, params, dst, dst_pitch, workspace, workspace_bytes, stream, level,
                          level + 1);
}

}  // extern "C"
