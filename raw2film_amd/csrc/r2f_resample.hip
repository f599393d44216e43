// r2f_resample.hip -- every resampler on either side of the render path, with its entry point (include/r2f.h) next to its kernel:
//   resize_area            pre-path INTER_AREA down-scale of the float frame to the preview resolution
//   resize_area_u8 / _u16  cpu_processor.py:411-412 -> utils.resolution_scaling -> cv.resize(canvas, INTER_AREA): the final shrink of
//                          the rendered (and canvas-framed) uint8 / uint16 frame to the requested resolution
//   warp_affine            pre-path free rotation (cv.warpAffine, INTER_LINEAR, zero border)
//   lens_correct           pre-path lens correction: radial map, cv2.remap(INTER_LANCZOS4, zero border), clamp, vignetting gain
//   lanczos4_u8            post-path up-scale of the uint8 result (cv.resize INTER_LANCZOS4): the way back from max_scale
//   lanczos4_f32 / _u16    the float-weight LANCZOS4: the float frame before the path, the uint16 result after it
// None of this runs inside r2f_render or a timed step; the kernels are one lane per output pixel (launch_64x4).
#include <climits>
#include <cstring>
#include <vector>

#include "r2f_ctx.h"
#include "r2f_lens_math.h"

using namespace r2f;

namespace r2f {

// ------------------------------------------------------------------------------ INTER_AREA
// Two forms, different on purpose.  The float one (the frame before the path) takes its weights in double from area_cell() and
// accumulates with fmaf: it is held to the oracle's tolerance.  The integer one (the finished uint8 / uint16 frame) restates
// OpenCV's own float tables and its separate roundings with contraction off: it is bit exact.  Their arithmetic is not shared.
struct ResizeArgs {
    const void* in;
    int in_layout, H, W;
    DevPlanes dst;
    int out_h, out_w;
};

// One lane per destination pixel: weighted mean over its source footprint with the INTER_AREA weights of
// area_cell(), all three channels at once.  Pre-path and run once per preview; no tuning beyond coalesced x.
__global__ __launch_bounds__(256) void resize_area_kernel(const ResizeArgs a) {
    const int dx = blockIdx.x * 64 + threadIdx.x, dy = blockIdx.y * 4 + threadIdx.y;
    if (dx >= a.out_w || dy >= a.out_h) return;
    int ry0, ry1, rs1, rs2, cx0, cx1, cs1, cs2;
    double wyf, wy, wyl, wxf, wx, wxl;
    area_cell(dy, (double)a.H / a.out_h, a.H, ry0, ry1, rs1, rs2, wyf, wy, wyl);
    area_cell(dx, (double)a.W / a.out_w, a.W, cx0, cx1, cs1, cs2, wxf, wx, wxl);
    float accX = 0.f, accY = 0.f, accZ = 0.f;
    for (int y = ry0; y <= ry1; ++y) {
        const float wv = area_weight(y, rs1, rs2, wyf, wy, wyl);
        if (wv == 0.f) continue;
        float rX = 0.f, rY = 0.f, rZ = 0.f;
        for (int x = cx0; x <= cx1; ++x) {
            const float wh = area_weight(x, cs1, cs2, wxf, wx, wxl);
            float X, Y, Z;
            load_input1(a.in, a.in_layout, 0, a.H, a.W, y, x, X, Y, Z);
            rX = fmaf(wh, X, rX);
            rY = fmaf(wh, Y, rY);
            rZ = fmaf(wh, Z, rZ);
        }
        accX = fmaf(wv, rX, accX);
        accY = fmaf(wv, rY, accY);
        accZ = fmaf(wv, rZ, accZ);
    }
    float* p0 = a.dst.data + (long long)(dy - a.dst.gy0) * a.out_w + dx;
    p0[0] = accX;
    p0[a.dst.plane_stride] = accY;
    p0[2 * a.dst.plane_stride] = accZ;
}

namespace {

// cv::resize(CV_8UC3, INTER_AREA), shrinking (imgproc/src/resize.cpp).  Integer scale factors take resizeAreaFast_: the
// integer sum of the scale_y x scale_x block, 2 x 2 as (s + 2) >> 2 (the SIMD form), anything else as
// saturate_cast<uchar>(sum * (1.f / area)).  Other factors take resizeArea_ with the DecimateAlpha tables of
// computeResizeAreaTab (float weights from double arithmetic): per source row a float buffer buf[dx] = sum_k S[sx_k] * alpha_k
// (k ascending, starting from 0), rows combined as sum = beta_0 * buf_0, sum += beta_j * buf_j, saturate_cast<uchar>(sum).
// Multiplications and additions are separate roundings (the generic C++ path has no FMA contraction).
__device__ __forceinline__ void area_tab(int d, double scale, int ssize, int& s_first, int& n, float& w_first, float& w_full, float& w_last,
                                         int& has_first, int& n_full, int& has_last) {
#pragma clang fp contract(off)
    // (separate roundings, like the host code this restates: a contracted d * scale + scale can land on the other side of an
    // integer.  HIP's __fmul_rn / __dadd_rn are plain operators the compiler is free to fuse; the pragma is what forbids it)
    // (plain operators: HIP's __dmul_rn / __fadd_rn wrappers are compiled with contraction allowed and fuse after inlining)
    const double f1 = (double)d * scale, f2 = f1 + scale;
    const double cell = fmin(scale, (double)ssize - f1);
    int s1 = (int)ceil(f1), s2 = (int)floor(f2);
    s2 = min(s2, ssize - 1);
    s1 = min(s1, s2);
    has_first = ((double)s1 - f1 > 1e-3) ? 1 : 0;
    w_first = (float)(((double)s1 - f1) / cell);
    n_full = s2 - s1;
    w_full = (float)(1.0 / cell);
    has_last = (f2 - (double)s2 > 1e-3) ? 1 : 0;
    w_last = (float)(fmin(fmin(f2 - (double)s2, 1.0), cell) / cell);
    s_first = has_first ? s1 - 1 : s1;
    n = has_first + n_full + has_last;
}

__device__ __forceinline__ float area_w(int k, int has_first, int n_full, float w_first, float w_full, float w_last) {
    if (has_first && k == 0) return w_first;
    if (k - has_first < n_full) return w_full;
    return w_last;
}

__device__ __forceinline__ uint8_t sat_u8(float v) {  // saturate_cast<uchar>(float): cvRound (nearest even), then clamp
    const int r = __float2int_rn(v);
    return (uint8_t)min(max(r, 0), 255);
}

__device__ __forceinline__ uint16_t sat_u16(float v) {  // saturate_cast<ushort>(float): the same rounding, the wider clamp
    const int r = __float2int_rn(v);
    return (uint16_t)min(max(r, 0), 65535);
}
template <typename T>
__device__ __forceinline__ T sat_as(float v) {
    if constexpr (sizeof(T) == 1)
        return sat_u8(v);
    else
        return sat_u16(v);
}

// T = uint8_t, or uint16_t for the 16-bit output (cv.resize(uint16, INTER_AREA): the same structure with saturate_cast<ushort>;
// the block sums of the integer factors are float sums there, as OpenCV's are -- a uint8 block sum is exact either way)
template <typename T>
struct AreaArgs {
    const T* src;
    T* dst;
    int H, W, out_h, out_w;
};

template <typename T>
__global__ __launch_bounds__(256) void resize_area_int_kernel(const AreaArgs<T> a) {
#pragma clang fp contract(off)
    const int dx = blockIdx.x * 64 + threadIdx.x, dy = blockIdx.y * 4 + threadIdx.y;
    if (dx >= a.out_w || dy >= a.out_h) return;
    const double sx = (double)a.W / a.out_w, sy = (double)a.H / a.out_h;
    const int isx = (int)sx, isy = (int)sy;
    T* o = a.dst + ((long long)dy * a.out_w + dx) * 3;
    if ((double)isx == sx && (double)isy == sy) {  // resizeAreaFast_
        int sum[3] = {0, 0, 0};
        if constexpr (sizeof(T) == 2) {
            if (isx != 2 || isy != 2) {
                // resizeAreaFast_<ushort, float>: the block's samples in row order, four at a time added as integers and each group
                // (then each sample that is left) added to a FLOAT sum -- past 256 bright samples that sum rounds, and so must this
                const int area = isx * isy, area4 = area & ~3;
                float fsum[3] = {0.f, 0.f, 0.f};
                int k = 0;
                for (int y = 0; y < isy; ++y) {
                    const T* row = a.src + ((long long)(dy * isy + y) * a.W + (long long)dx * isx) * 3;
                    for (int x = 0; x < isx; ++x) {
                        for (int c = 0; c < 3; ++c) sum[c] += row[3 * x + c];
                        ++k;
                        if (k > area4 || (k & 3) == 0)
                            for (int c = 0; c < 3; ++c) fsum[c] = fsum[c] + (float)sum[c], sum[c] = 0;
                    }
                }
                const float scale = 1.f / (float)area;
                for (int c = 0; c < 3; ++c) o[c] = sat_as<T>(fsum[c] * scale);
                return;
            }
        }
        for (int y = 0; y < isy; ++y) {
            const T* row = a.src + ((long long)(dy * isy + y) * a.W + (long long)dx * isx) * 3;
            for (int x = 0; x < isx; ++x)
                for (int c = 0; c < 3; ++c) sum[c] += row[3 * x + c];
        }
        if (isx == 2 && isy == 2) {
            for (int c = 0; c < 3; ++c) o[c] = (T)((sum[c] + 2) >> 2);
        } else {
            const float scale = 1.f / (float)(isx * isy);
            for (int c = 0; c < 3; ++c) o[c] = sat_as<T>((float)sum[c] * scale);
        }
        return;
    }
    int x0, nx, hfx, nfx, hlx, y0, ny, hfy, nfy, hly;
    float wfx, wx, wlx, wfy, wy, wly;
    area_tab(dx, sx, a.W, x0, nx, wfx, wx, wlx, hfx, nfx, hlx);
    area_tab(dy, sy, a.H, y0, ny, wfy, wy, wly, hfy, nfy, hly);
    float sum[3] = {0.f, 0.f, 0.f};
    for (int j = 0; j < ny; ++j) {
        const T* row = a.src + ((long long)(y0 + j) * a.W + x0) * 3;
        float buf[3] = {0.f, 0.f, 0.f};
        for (int k = 0; k < nx; ++k) {
            const float alpha = area_w(k, hfx, nfx, wfx, wx, wlx);
            for (int c = 0; c < 3; ++c) {
                const float prod = (float)row[3 * k + c] * alpha;
                buf[c] = buf[c] + prod;
            }
        }
        const float beta = area_w(j, hfy, nfy, wfy, wy, wly);
        for (int c = 0; c < 3; ++c) {
            const float term = beta * buf[c];
            sum[c] = j == 0 ? term : sum[c] + term;
        }
    }
    for (int c = 0; c < 3; ++c) o[c] = sat_as<T>(sum[c]);
}

}  // namespace

// ------------------------------------------------------------------------------ free rotation (pre-path)
// dst(y, x) = bilinear sample of `in` at M * (x + ox, y + oy, 1), zero outside (cv.warpAffine, INTER_LINEAR, BORDER_CONSTANT); only
// the window the rotate() crop keeps is produced.
struct WarpArgs {
    const void* in;
    int in_layout, H, W;
    DevPlanes dst;
    int out_h, out_w, oy, ox;
    float m[6];  // dst -> src, row-major 2 x 3, rounded from double like OpenCV's float kernels
};

// effects.rotate (effects.py:46-75): cv.warpAffine(rgb, getRotationMatrix2D(centre, -degrees, 1), same size, INTER_LINEAR)
// followed by a centred crop; the kernel produces the cropped window only.  One lane per destination pixel, lanes along x.
// Source coordinates and the two-step lerp are float32, like OpenCV's linear warp kernels (>= 4.11); taps that fall
// outside the frame read the constant border 0.  HBM/L2-bound gather: neighbouring lanes read neighbouring texels for
// the small angles a horizon correction uses.
__global__ __launch_bounds__(256) void warp_affine_kernel(const WarpArgs a) {
    const int dx = blockIdx.x * 64 + threadIdx.x, dy = blockIdx.y * 4 + threadIdx.y;
    if (dx >= a.out_w || dy >= a.out_h) return;
    const float xf = (float)(dx + a.ox), yf = (float)(dy + a.oy);
    float sx, sy;
    {
        // every product and sum its own rounding, like the float32 array arithmetic this restates: plain operators with
        // contraction off (the pragma is what keeps them apart, see area_tab)
#pragma clang fp contract(off)
        sx = (xf * a.m[0] + yf * a.m[1]) + a.m[2];
        sy = (xf * a.m[3] + yf * a.m[4]) + a.m[5];
    }
    const float fx0 = floorf(sx), fy0 = floorf(sy);
    const float ax = sx - fx0, ay = sy - fy0;
    float v[3] = {0.f, 0.f, 0.f};
    // int conversion only for coordinates that can touch the frame (also keeps huge values out of the cast)
    if (fx0 >= -1.f && fy0 >= -1.f && fx0 < (float)a.W && fy0 < (float)a.H) {
        const int x0 = (int)fx0, y0 = (int)fy0;
        float t[2][2][3];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int xx = x0 + i, yy = y0 + j;
                if (xx >= 0 && xx < a.W && yy >= 0 && yy < a.H)
                    load_input1(a.in, a.in_layout, 0, a.H, a.W, yy, xx, t[j][i][0], t[j][i][1], t[j][i][2]);
                else
                    t[j][i][0] = t[j][i][1] = t[j][i][2] = 0.f;
            }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            // the two-step lerp: difference, product and sum each rounded on its own (contraction off, as above)
#pragma clang fp contract(off)
            const float top = t[0][0][c] + ax * (t[0][1][c] - t[0][0][c]);
            const float bot = t[1][0][c] + ax * (t[1][1][c] - t[1][0][c]);
            v[c] = top + ay * (bot - top);
        }
    }
    float* p0 = a.dst.data + (long long)(dy - a.dst.gy0) * a.out_w + dx;
    p0[0] = v[0];
    p0[a.dst.plane_stride] = v[1];
    p0[2 * a.dst.plane_stride] = v[2];
}

// ------------------------------------------------------------------------------ lens correction (pre-path)
// effects.lens_correction (effects.py:22-43) from caller-supplied numbers; the definition is in include/r2f.h and its arithmetic in
// r2f_lens_math.h (the text tests/lens_check.cpp compiles for the CPU).  Lanes along x, four output rows per lane; the 32 x 8 phase
// table sits in LDS (1 KiB, one float per thread to fill).
struct LensArgs {
    const void* in;
    int in_layout, H, W;
    DevPlanes dst;
    int out_h, out_w, oy, ox;
    r2f_lens_params p;
    const float* table;  // 32 x 8, device
};

struct LensFetch {
    const float* src;
    int in_layout, H, W;
    __device__ __forceinline__ void operator()(int y, int x, float (&v)[3]) const {
        if (in_layout == R2F_LAYOUT_CHW) {
            const long long plane = (long long)H * W, o = (long long)y * W + x;
            v[0] = src[o], v[1] = src[plane + o], v[2] = src[2 * plane + o];
        } else {
            const float* px = src + ((long long)y * W + x) * (in_layout == R2F_LAYOUT_HWC4 ? 4 : 3);
            v[0] = px[0], v[1] = px[1], v[2] = px[2];
        }
    }
};

// A block of 256 threads makes a 64 x 16 tile (four rows per lane), finds the box of source texels its taps touch,
// and -- when the box fits kLensBoxTexels -- copies it into LDS once (a texel outside the frame as 0, which is what such a tap
// reads), so that a texel crosses the memory system once per block instead of once per tap.  The sums are sample64's over another
// fetch functor: the same samples in the same order, so the result does not depend on whether a block staged.  A block whose box
// does not fit (a strong magnification: scale well below 1) gathers its taps from global memory.  Against one lane per pixel
// gathering every tap from global memory: 5.0 instead of 7.7 ms at 100 MP; two or eight rows per lane and an interleaved float4
// box were slower (profiles/r15_lens_correct.txt).
constexpr int kLensRows = 4;            // rows per lane
constexpr int kLensBoxTexels = 3072;    // 36 KiB of LDS for three planes: 71 x 23 texels for an undistorted tile

struct LensLdsFetch {
    const float* box;  // [3][kLensBoxTexels], rows bw apart
    int x0, y0, bw;
    __device__ __forceinline__ void operator()(int y, int x, float (&v)[3]) const {
        const int o = (y - y0) * bw + (x - x0);
        v[0] = box[o], v[1] = box[kLensBoxTexels + o], v[2] = box[2 * kLensBoxTexels + o];
    }
};

__global__ __launch_bounds__(256) void lens_correct_kernel(const LensArgs a) {
    __shared__ float table[lens::kPhases * lens::kTaps];
    __shared__ float box[3 * kLensBoxTexels];
    __shared__ int ext[4];  // min ix, max ix, min iy, max iy over the block's inside pixels
    const int tid = threadIdx.y * 64 + threadIdx.x;
    table[tid] = a.table[tid];
    if (tid < 4) ext[tid] = (tid & 1) ? INT_MIN : INT_MAX;
    __syncthreads();
    const int dx = blockIdx.x * 64 + threadIdx.x, dy0 = blockIdx.y * (4 * kLensRows) + threadIdx.y;
    const LensFetch global{static_cast<const float*>(a.in), a.in_layout, a.H, a.W};
    int ix[kLensRows], iy[kLensRows], ph[kLensRows];  // ph: fx | fy << 8, or -1 for a pixel that samples nothing
    float ddx[kLensRows], ddy[kLensRows];
    int lo_x = INT_MAX, hi_x = INT_MIN, lo_y = INT_MAX, hi_y = INT_MIN;
#pragma unroll
    for (int r = 0; r < kLensRows; ++r) {
        const int dy = dy0 + 4 * r;
        ph[r] = -1;
        ix[r] = iy[r] = 0;
        ddx[r] = ddy[r] = 0.f;
        if (dx >= a.out_w || dy >= a.out_h) continue;
        float sx, sy;
        lens::source_coord(a.p, dx + a.ox, dy + a.oy, sx, sy, ddx[r], ddy[r]);
        int fx, fy;
        if (!lens::split_phase(sx, a.W, ix[r], fx) || !lens::split_phase(sy, a.H, iy[r], fy)) continue;
        ph[r] = fx | (fy << 8);
        lo_x = min(lo_x, ix[r]), hi_x = max(hi_x, ix[r]), lo_y = min(lo_y, iy[r]), hi_y = max(hi_y, iy[r]);
    }
    if (lo_x <= hi_x) {
        atomicMin(&ext[0], lo_x), atomicMax(&ext[1], hi_x);
        atomicMin(&ext[2], lo_y), atomicMax(&ext[3], hi_y);
    }
    __syncthreads();
    // (block-uniform from here: every thread reads the same four words)
    const int x0 = ext[0] - 3, y0 = ext[2] - 3;
    const bool any = ext[0] <= ext[1];
    // ix, iy lie in [-4, n + 2] (split_phase), so the extents are small ints and their products cannot overflow
    const int bw = any ? ext[1] + 4 - x0 + 1 : 0, bh = any ? ext[3] + 4 - y0 + 1 : 0;
    const bool staged = any && (long long)bw * bh <= kLensBoxTexels;
    if (staged) {
        for (int i = tid; i < bw * bh; i += 256) {
            const int y = y0 + i / bw, x = x0 + i % bw;
            float v[3] = {0.f, 0.f, 0.f};
            if (y >= 0 && y < a.H && x >= 0 && x < a.W) global(y, x, v);
            box[i] = v[0], box[kLensBoxTexels + i] = v[1], box[2 * kLensBoxTexels + i] = v[2];
        }
    }
    __syncthreads();
    const LensLdsFetch lds{box, x0, y0, bw};
#pragma unroll
    for (int r = 0; r < kLensRows; ++r) {
        const int dy = dy0 + 4 * r;
        if (dx >= a.out_w || dy >= a.out_h) continue;
        float v[3] = {0.f, 0.f, 0.f};
        if (ph[r] >= 0) {
            float acc[3];
            const float *wx = table + (ph[r] & 31) * lens::kTaps, *wy = table + (ph[r] >> 8) * lens::kTaps;
            if (staged)
                lens::sample64(lds, a.H, a.W, ix[r], iy[r], wx, wy, acc);
            else
                lens::sample64(global, a.H, a.W, ix[r], iy[r], wx, wy, acc);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = lens::finish(a.p, acc[c], ddx[r], ddy[r]);
        }
        float* p0 = a.dst.data + (long long)(dy - a.dst.gy0) * a.out_w + dx;
        p0[0] = v[0];
        p0[a.dst.plane_stride] = v[1];
        p0[2 * a.dst.plane_stride] = v[2];
    }
}

// ------------------------------------------------------------------------------ lens correction with TCA (pre-path)
// r2f_lens_correct_tca: red and blue sample at coordinates of their own (lens::channel_coord).  The shape is lens_correct_kernel's
// -- a 64 x 16 tile, four rows per lane, the phase table and one planar box of kLensBoxTexels in LDS -- with these differences:
//   - the box is the union of the three channels' tap extents (a texel is staged once for all of its channels, so an interleaved
//     source is still read in whole pixels), and the staged / unstaged decision is made on that union;
//   - a lane keeps nothing per row between the extent pass and the sampling pass: it evaluates the map again (some 40 operations
//     beside 3 x 64 taps), so that beyond the map's result only one channel's indices, phases and accumulator are live at a time;
//   - rows and channels are loops, not unrolled copies: one staged and one unstaged 64-tap body in the program.
// The sums are lens::sample64_channel's over either fetch functor: results do not depend on whether a block staged.
// The compiler reports (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage) 145 VGPRs, no VGPR spills, no scratch, 21 SGPRs
// spilled into VGPR lanes, 37,904 B of LDS and 3 waves per SIMD, against lens_correct_kernel's 253 VGPRs and 2 waves.  Beside that
// kernel in one process: 1.08 x its time with factors of 1, 1.15 x / 1.23 x at 24 / 100 MP with a poly3 record that parts red and
// blue by up to 12 px at 100 MP, where a tenth of the blocks' unions no longer fit the box (profiles/r25_lens_tca_probe.txt).
struct LensTcaArgs {
    LensArgs lens;
    r2f_lens_tca_params tca;
};

struct LensChannelFetch {
    const float* src;
    int in_layout, H, W;
    __device__ __forceinline__ float operator()(int ch, int y, int x) const {
        if (in_layout == R2F_LAYOUT_CHW) return src[(long long)ch * H * W + (long long)y * W + x];
        return src[((long long)y * W + x) * (in_layout == R2F_LAYOUT_HWC4 ? 4 : 3) + ch];
    }
};

struct LensLdsChannelFetch {
    const float* box;  // [3][kLensBoxTexels], rows bw apart
    int x0, y0, bw;
    __device__ __forceinline__ float operator()(int ch, int y, int x) const { return box[ch * kLensBoxTexels + (y - y0) * bw + (x - x0)]; }
};

__global__ __launch_bounds__(256) void lens_correct_tca_kernel(const LensTcaArgs t) {
    const LensArgs& a = t.lens;
    __shared__ float table[lens::kPhases * lens::kTaps];
    __shared__ float box[3 * kLensBoxTexels];
    __shared__ int ext[4];  // min ix, max ix, min iy, max iy over the block's inside pixels, all channels
    const int tid = threadIdx.y * 64 + threadIdx.x;
    table[tid] = a.table[tid];
    if (tid < 4) ext[tid] = (tid & 1) ? INT_MIN : INT_MAX;
    __syncthreads();
    const int dx = blockIdx.x * 64 + threadIdx.x, dy0 = blockIdx.y * (4 * kLensRows) + threadIdx.y;
    int lo_x = INT_MAX, hi_x = INT_MIN, lo_y = INT_MAX, hi_y = INT_MIN;
    if (dx < a.out_w) {
#pragma unroll 1
        for (int dy = dy0; dy < min(a.out_h, dy0 + 4 * kLensRows); dy += 4) {
            float ox, oy, ddx, ddy;
            lens::source_offset(a.p, dx + a.ox, dy + a.oy, ox, oy, ddx, ddy);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                float sx, sy;
                lens::channel_coord(a.p, t.tca, ch, ox, oy, sx, sy);
                int ix, iy, fx, fy;
                if (!lens::split_phase(sx, a.W, ix, fx) || !lens::split_phase(sy, a.H, iy, fy)) continue;
                lo_x = min(lo_x, ix), hi_x = max(hi_x, ix), lo_y = min(lo_y, iy), hi_y = max(hi_y, iy);
            }
        }
    }
    if (lo_x <= hi_x) {
        atomicMin(&ext[0], lo_x), atomicMax(&ext[1], hi_x);
        atomicMin(&ext[2], lo_y), atomicMax(&ext[3], hi_y);
    }
    __syncthreads();
    // (block-uniform from here: every thread reads the same four words)
    const int x0 = ext[0] - 3, y0 = ext[2] - 3;
    const bool any = ext[0] <= ext[1];
    // ix, iy lie in [-4, n + 2] (split_phase), so the extents are small ints and their products cannot overflow
    const int bw = any ? ext[1] + 4 - x0 + 1 : 0, bh = any ? ext[3] + 4 - y0 + 1 : 0;
    const bool staged = any && (long long)bw * bh <= kLensBoxTexels;
    if (staged) {
        const LensFetch global{static_cast<const float*>(a.in), a.in_layout, a.H, a.W};
        for (int i = tid; i < bw * bh; i += 256) {
            const int y = y0 + i / bw, x = x0 + i % bw;
            float v[3] = {0.f, 0.f, 0.f};
            if (y >= 0 && y < a.H && x >= 0 && x < a.W) global(y, x, v);
            box[i] = v[0], box[kLensBoxTexels + i] = v[1], box[2 * kLensBoxTexels + i] = v[2];
        }
    }
    __syncthreads();
    if (dx >= a.out_w) return;  // (no barrier below)
    const LensLdsChannelFetch lds{box, x0, y0, bw};
    const LensChannelFetch global{static_cast<const float*>(a.in), a.in_layout, a.H, a.W};
#pragma unroll 1
    for (int dy = dy0; dy < min(a.out_h, dy0 + 4 * kLensRows); dy += 4) {
        float ox, oy, ddx, ddy;
        lens::source_offset(a.p, dx + a.ox, dy + a.oy, ox, oy, ddx, ddy);
        float* p0 = a.dst.data + (long long)(dy - a.dst.gy0) * a.out_w + dx;
#pragma unroll 1
        for (int ch = 0; ch < 3; ++ch) {
            float sx, sy;
            lens::channel_coord(a.p, t.tca, ch, ox, oy, sx, sy);
            int ix, iy, fx, fy;
            float v = 0.f;
            if (lens::split_phase(sx, a.W, ix, fx) && lens::split_phase(sy, a.H, iy, fy)) {
                const float *wx = table + fx * lens::kTaps, *wy = table + fy * lens::kTaps;
                const float acc = staged ? lens::sample64_channel(lds, ch, a.H, a.W, ix, iy, wx, wy)
                                         : lens::sample64_channel(global, ch, a.H, a.W, ix, iy, wx, wy);
                v = lens::finish(a.p, acc, ddx, ddy);
            }
            p0[ch * a.dst.plane_stride] = v;
        }
    }
}

// ------------------------------------------------------------------------------ lens correction of a projected lens (pre-path)
// r2f_lens_correct_projected: the fisheye-to-rectilinear step in front of the distortion model (lens::source_offset with the
// projection params), without a TCA record (kTca false: one coordinate, lens::sample64 over three channels) or with one (kTca true:
// lens::channel_coord and lens::sample64_channel per channel).  The shape is lens_correct_tca_kernel's -- a 64 x 16 tile, four rows
// per lane, the map evaluated again in the sampling pass so that nothing per row stays live -- with another staging rule.  A fisheye
// frame at its auto scale is magnified in the middle (scale 0.70 for a 180-degree diagonal on 3:2: a centre tile's taps span some
// 99 x 31 texels and more with a TCA record, at or past the 3072 a box holds) and shrunk towards the corners, so the tiles that cover
// most of the picture would be the ones to lose their box.  Three routes, decided per block from the tap extents of its two halves
// (tile rows 0 .. 7 and 8 .. 15):
//   whole   the union of the halves' extents fits the box: one staging, one sampling pass over all four rows per lane;
//   halves  it does not: each half is a pass of its own with its own box (some 99 x 20 texels at scale 0.70), staged when it fits;
//   gather  a half whose box does not fit either takes its taps from global memory.
// The sums are lens::sample64's / sample64_channel's over either fetch functor in the same order: the result does not depend on the
// route.  The compiler reports (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage) for <false> / <true>: 253 / 153 VGPRs,
// 2 / 3 waves per SIMD, no VGPR spills, no scratch, 0 / 7 SGPRs spilled into VGPR lanes, 37,920 B of LDS; lens_correct_kernel and
// lens_correct_tca_kernel keep their 253 VGPRs / 2 waves and 145 VGPRs / 3 waves / 37,904 B.
// Measured beside the unprojected kernels in one process (profiles/r26_lens_projection_probe.txt), 24 / 100 MP:
//   - identity record (P exactly 1, the same texels, bit-identical output): <false> 1.39 x / 1.40 x lens_correct_kernel -- the price
//     of evaluating the map twice and of rows as a loop where that kernel keeps four unrolled rows' indices in registers; a form
//     of <false> with lens_correct_kernel's unrolled rows inside the pass loop spilled (9.5 KB of scratch per lane) and was
//     dropped; <true> 1.20 x / 1.18 x lens_correct_tca_kernel;
//   - fisheye record (focal 2/pi) at its auto scale (0.76 on these 2:3 frames): every block whole without a record; with the poly3
//     record 5 % / 26 % of the blocks work in halves and 0 / 5 % gather.  <false> 1.97 x / 2.05 x lens_correct_kernel at the same
//     scale, <true> 1.20 x / 1.00 x lens_correct_tca_kernel;
//   - equisolid record (0.55) at its auto scale (0.60): 12 % of the blocks in halves without a record; with it 18 % / 15 % in halves
//     and 5 % / 22 % gathering.  <false> 2.34 x / 2.34 x, <true> 1.71 x / 1.96 x their unprojected kernels at the same scale.
// The unprojected kernels get FASTER as the scale falls (lens_correct_kernel 1.24 -> 0.82 ms at 24 MP from scale 1.02 to 0.60, its
// gathering blocks included: a magnified frame reads fewer texels and its gathers hit in cache), while the projected ones stay at
// 19 - 21 x the copy: at these scales the two-halves route saves less than the estimate that motivated it, and the projected
// kernels are bound by their per-pixel arithmetic (the map twice, one division and a 19-operation polynomial or two square roots
// and up to three divisions for P), not by staging.
struct LensProjectedArgs {
    LensArgs lens;
    r2f_lens_projection_params proj;
    r2f_lens_tca_params tca;  // read by the kernel with a TCA record only
};

template <bool kTca>
__global__ __launch_bounds__(256) void lens_correct_projected_kernel(const LensProjectedArgs t) {
    const LensArgs& a = t.lens;
    __shared__ float table[lens::kPhases * lens::kTaps];
    __shared__ float box[3 * kLensBoxTexels];
    __shared__ int ext[2][4];  // per half: min ix, max ix, min iy, max iy over its inside pixels, all channels
    const int tid = threadIdx.y * 64 + threadIdx.x;
    table[tid] = a.table[tid];
    if (tid < 8) ext[tid >> 2][tid & 3] = (tid & 1) ? INT_MIN : INT_MAX;
    __syncthreads();
    const int dx = blockIdx.x * 64 + threadIdx.x, dy0 = blockIdx.y * (4 * kLensRows) + threadIdx.y;
    const bool col_in = dx < a.out_w;
    constexpr int kHalfRows = kLensRows / 2;  // rows per lane in a half
    if (col_in) {
#pragma unroll 1
        for (int half = 0; half < 2; ++half) {
            int lo_x = INT_MAX, hi_x = INT_MIN, lo_y = INT_MAX, hi_y = INT_MIN;
#pragma unroll 1
            for (int r = half * kHalfRows; r < (half + 1) * kHalfRows; ++r) {
                const int dy = dy0 + 4 * r;
                if (dy >= a.out_h) break;
                float ox, oy, ddx, ddy;
                lens::source_offset(a.p, t.proj, dx + a.ox, dy + a.oy, ox, oy, ddx, ddy);
#pragma unroll
                for (int ch = kTca ? 0 : 1; ch < (kTca ? 3 : 2); ++ch) {  // (without a record every channel is green's)
                    float sx, sy;
                    if constexpr (kTca)
                        lens::channel_coord(a.p, t.tca, ch, ox, oy, sx, sy);
                    else
                        lens::centre_coord(a.p, ox, oy, sx, sy);
                    int ix, iy, fx, fy;
                    if (!lens::split_phase(sx, a.W, ix, fx) || !lens::split_phase(sy, a.H, iy, fy)) continue;
                    lo_x = min(lo_x, ix), hi_x = max(hi_x, ix), lo_y = min(lo_y, iy), hi_y = max(hi_y, iy);
                }
            }
            if (lo_x <= hi_x) {
                atomicMin(&ext[half][0], lo_x), atomicMax(&ext[half][1], hi_x);
                atomicMin(&ext[half][2], lo_y), atomicMax(&ext[half][3], hi_y);
            }
        }
    }
    __syncthreads();
    // (block-uniform from here: every thread reads the same eight words; ix, iy lie in [-4, n + 2] (split_phase), so the extents
    // are small ints and their products cannot overflow)
    const int un_lo_x = min(ext[0][0], ext[1][0]), un_hi_x = max(ext[0][1], ext[1][1]);
    const int un_lo_y = min(ext[0][2], ext[1][2]), un_hi_y = max(ext[0][3], ext[1][3]);
    const bool whole = un_lo_x > un_hi_x || (long long)(un_hi_x - un_lo_x + 8) * (un_hi_y - un_lo_y + 8) <= kLensBoxTexels;
    const LensFetch global3{static_cast<const float*>(a.in), a.in_layout, a.H, a.W};
    const LensChannelFetch global1{static_cast<const float*>(a.in), a.in_layout, a.H, a.W};
#pragma unroll 1
    for (int pass = 0; pass < (whole ? 1 : 2); ++pass) {
        const int lo_x = whole ? un_lo_x : ext[pass][0], hi_x = whole ? un_hi_x : ext[pass][1];
        const int lo_y = whole ? un_lo_y : ext[pass][2], hi_y = whole ? un_hi_y : ext[pass][3];
        const int r_begin = whole ? 0 : pass * kHalfRows, r_end = whole ? kLensRows : (pass + 1) * kHalfRows;
        const bool any = lo_x <= hi_x;
        const int x0 = lo_x - 3, y0 = lo_y - 3;
        const int bw = any ? hi_x + 4 - x0 + 1 : 0, bh = any ? hi_y + 4 - y0 + 1 : 0;
        const bool staged = any && (long long)bw * bh <= kLensBoxTexels;
        if (pass) __syncthreads();  // (the first half's lanes are done with the box)
        if (staged) {
            for (int i = tid; i < bw * bh; i += 256) {
                const int y = y0 + i / bw, x = x0 + i % bw;
                float v[3] = {0.f, 0.f, 0.f};
                if (y >= 0 && y < a.H && x >= 0 && x < a.W) global3(y, x, v);
                box[i] = v[0], box[kLensBoxTexels + i] = v[1], box[2 * kLensBoxTexels + i] = v[2];
            }
        }
        __syncthreads();
        if (!col_in) continue;  // (block-uniform trip count: such a lane still meets every barrier)
        const LensLdsFetch lds3{box, x0, y0, bw};
        const LensLdsChannelFetch lds1{box, x0, y0, bw};
#pragma unroll 1
        for (int r = r_begin; r < r_end; ++r) {
            const int dy = dy0 + 4 * r;
            if (dy >= a.out_h) break;
            float ox, oy, ddx, ddy;
            lens::source_offset(a.p, t.proj, dx + a.ox, dy + a.oy, ox, oy, ddx, ddy);
            float* p0 = a.dst.data + (long long)(dy - a.dst.gy0) * a.out_w + dx;
            if constexpr (kTca) {
#pragma unroll 1
                for (int ch = 0; ch < 3; ++ch) {
                    float sx, sy;
                    lens::channel_coord(a.p, t.tca, ch, ox, oy, sx, sy);
                    int ix, iy, fx, fy;
                    float v = 0.f;
                    if (lens::split_phase(sx, a.W, ix, fx) && lens::split_phase(sy, a.H, iy, fy)) {
                        const float *wx = table + fx * lens::kTaps, *wy = table + fy * lens::kTaps;
                        const float acc = staged ? lens::sample64_channel(lds1, ch, a.H, a.W, ix, iy, wx, wy)
                                                 : lens::sample64_channel(global1, ch, a.H, a.W, ix, iy, wx, wy);
                        v = lens::finish(a.p, acc, ddx, ddy);
                    }
                    p0[ch * a.dst.plane_stride] = v;
                }
            } else {
                float sx, sy;
                lens::centre_coord(a.p, ox, oy, sx, sy);
                int ix, iy, fx, fy;
                float v[3] = {0.f, 0.f, 0.f};
                if (lens::split_phase(sx, a.W, ix, fx) && lens::split_phase(sy, a.H, iy, fy)) {
                    const float *wx = table + fx * lens::kTaps, *wy = table + fy * lens::kTaps;
                    float acc[3];
                    if (staged)
                        lens::sample64(lds3, a.H, a.W, ix, iy, wx, wy, acc);
                    else
                        lens::sample64(global3, a.H, a.W, ix, iy, wx, wy, acc);
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[c] = lens::finish(a.p, acc[c], ddx, ddy);
                }
                p0[0] = v[0];
                p0[a.dst.plane_stride] = v[1];
                p0[2 * a.dst.plane_stride] = v[2];
            }
        }
    }
}

// ------------------------------------------------------------------------------ LANCZOS4, uint8 (post-path)
struct LanczosArgs {
    const uint8_t* src;  // (H, W, 3)
    uint8_t* dst;        // (out_h, out_w, 3)
    int H, W, out_h, out_w;
    const int* xofs;     // out_w: source column of tap 3
    const short* xcoef;  // out_w x 8
    const int* yofs;     // out_h
    const short* ycoef;  // out_h x 8
};

// utils.resolution_scaling -> cv.resize(uint8, INTER_LANCZOS4) (utils.py:237-242): 8 x 8 taps per output pixel with the
// 11-bit fixed-point weights OpenCV derives per destination column / row (built on the host, r2f_api.hip), exact int32
// accumulation, one rounding (+2^21 >> 22), replicated border.  One lane per output pixel, all three channels.
__global__ __launch_bounds__(256) void lanczos4_u8_kernel(const LanczosArgs a) {
    const int dx = blockIdx.x * 64 + threadIdx.x, dy = blockIdx.y * 4 + threadIdx.y;
    if (dx >= a.out_w || dy >= a.out_h) return;
    const int sx = a.xofs[dx] - 3, sy = a.yofs[dy] - 3;
    int wx[8], wy[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) wx[k] = a.xcoef[dx * 8 + k], wy[k] = a.ycoef[dy * 8 + k];
    int acc[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint8_t* row = a.src + (long long)clampi(sy + k, 0, a.H - 1) * a.W * 3;
        int h[3] = {0, 0, 0};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint8_t* p = row + clampi(sx + j, 0, a.W - 1) * 3;
            h[0] += (int)p[0] * wx[j];
            h[1] += (int)p[1] * wx[j];
            h[2] += (int)p[2] * wx[j];
        }
        acc[0] += h[0] * wy[k];
        acc[1] += h[1] * wy[k];
        acc[2] += h[2] * wy[k];
    }
    uint8_t* o = a.dst + ((long long)dy * a.out_w + dx) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (uint8_t)clampi((acc[c] + (1 << 21)) >> 22, 0, 255);
}

// ------------------------------------------------------------------------------ LANCZOS4, float weights
// cv::resize's generic path for CV_32F and CV_16U: float weights from interpolateLanczos4 (host tables, below), HResizeLanczos4 = the
// 8 products of a row summed left to right, then VResizeLanczos4 = the 8 rows times beta summed top to bottom; indices outside the
// frame repeat the edge sample.  One kernel over the frame type that fetches a source pixel and stores a result:
//   PlanesFrame  cv.resize(float32 frame, INTER_LANCZOS4): utils.resolution_scaling's other branch (utils.py:237-242), taken BEFORE
//                the path when the preview is larger than the frame (cpu_processor.py:134); any input layout -> planes
//   U16Frame     cv.resize(uint16 frame, INTER_LANCZOS4): the way back from max_scale for a 16-bit result; ends in
//                saturate_cast<ushort>: round half to even, clamp to [0, 65535]
namespace {

struct PlanesFrame {
    const void* in;
    int in_layout, H, W;
    DevPlanes dst;
    int out_w;
    // (load_input1's job, spelt out: written this way the compiler fetches an interleaved pixel as 8 + 4 bytes, through load_input1
    // as three 4-byte loads -- 3.12 against 4.49 ms on a 24 MP frame, profiles/r14_kernel_files_headline_ab.txt)
    __device__ __forceinline__ void load(int y, int x, float (&v)[3]) const {
        const float* src = static_cast<const float*>(in);
        if (in_layout == R2F_LAYOUT_CHW) {
            const long long plane = (long long)H * W, o = (long long)y * W + x;
            v[0] = src[o], v[1] = src[plane + o], v[2] = src[2 * plane + o];
        } else {
            const float* p = src + ((long long)y * W + x) * (in_layout == R2F_LAYOUT_HWC4 ? 4 : 3);
            v[0] = p[0], v[1] = p[1], v[2] = p[2];
        }
    }
    __device__ __forceinline__ void store(int dy, int dx, const float (&acc)[3]) const {
        float* p0 = dst.data + (long long)(dy - dst.gy0) * out_w + dx;
        p0[0] = acc[0];
        p0[dst.plane_stride] = acc[1];
        p0[2 * dst.plane_stride] = acc[2];
    }
};

struct U16Frame {
    const uint16_t* src;  // (H, W, 3)
    uint16_t* dst;        // (out_h, out_w, 3)
    int W, out_w;
    __device__ __forceinline__ void load(int y, int x, float (&v)[3]) const {
        const uint16_t* px = src + (long long)y * W * 3 + (long long)x * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (float)px[c];
    }
    __device__ __forceinline__ void store(int dy, int dx, const float (&acc)[3]) const {
        uint16_t* o = dst + ((long long)dy * out_w + dx) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = sat_u16(acc[c]);
    }
};

template <typename Frame>
struct LanczosFloatArgs {
    Frame f;
    int H, W, out_h, out_w;
    const int* xofs;     // out_w: source column of tap 3
    const float* xcoef;  // out_w x 8
    const int* yofs;
    const float* ycoef;
};

template <typename Frame>
__global__ __launch_bounds__(256) void lanczos4_float_kernel(const LanczosFloatArgs<Frame> a) {
#pragma clang fp contract(off)
    const int dx = blockIdx.x * 64 + threadIdx.x, dy = blockIdx.y * 4 + threadIdx.y;
    if (dx >= a.out_w || dy >= a.out_h) return;
    const int sx = a.xofs[dx] - 3, sy = a.yofs[dy] - 3;
    float wx[8], wy[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) wx[k] = a.xcoef[dx * 8 + k], wy[k] = a.ycoef[dy * 8 + k];
    float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int yy = clampi(sy + k, 0, a.H - 1);
        float h[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v[3];
            a.f.load(yy, clampi(sx + j, 0, a.W - 1), v);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float prod = v[c] * wx[j];
                h[c] = j == 0 ? prod : h[c] + prod;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float prod = h[c] * wy[k];
            acc[c] = k == 0 ? prod : acc[c] + prod;
        }
    }
    a.f.store(dy, dx, acc);
}

}  // namespace

// ------------------------------------------------------------------------------ LANCZOS4 tables
static void lanczos4_table(int n, int out_n, int* ofs, short* coef) { r2f_lanczos4_table(n, out_n, ofs, coef); }
static void lanczos4_table(int n, int out_n, int* ofs, float* coef) { r2f_lanczos4_table_f32(n, out_n, ofs, coef); }

template <typename Coef>
int LanczosTables::tables(r2f_ctx* ctx, int H, int W, int out_h, int out_w, const int** xofs, const int** yofs, const Coef** xcoef,
                          const Coef** ycoef) {
    const size_t n_ofs = (size_t)out_w + out_h, coef_off = (n_ofs * sizeof(int) + 15) / 16 * 16;
    const int want[4] = {H, W, out_h, out_w};
    if (memcmp(want, key, sizeof key) != 0 || !buf.p) {
        std::vector<unsigned char> host(coef_off + 8 * n_ofs * sizeof(Coef));
        int* ofs = reinterpret_cast<int*>(host.data());
        Coef* coef = reinterpret_cast<Coef*>(host.data() + coef_off);
        lanczos4_table(W, out_w, ofs, coef);
        lanczos4_table(H, out_h, ofs + out_w, coef + 8 * (size_t)out_w);
        int rc = upload(ctx, buf, host.data(), host.size());  // (waits for renders in flight, like every table upload)
        if (rc) return rc;
        memcpy(key, want, sizeof key);
    }
    const unsigned char* base = static_cast<const unsigned char*>(buf.p);
    *xofs = reinterpret_cast<const int*>(base);
    *yofs = *xofs + out_w;
    *xcoef = reinterpret_cast<const Coef*>(base + coef_off);
    *ycoef = *xcoef + 8 * (size_t)out_w;
    return R2F_OK;
}

}  // namespace r2f

// =============================================================================== C ABI
extern "C" {

int r2f_resize_area(r2f_ctx* ctx, const void* in, int in_layout, int H, int W, const r2f_planes* dst, int out_h, int out_w,
                    void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (!in || in_layout < 0 || in_layout > 2 || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0 || out_h > H || out_w > W)
        return fail(ctx, R2F_EINVAL, "resize_area: the target must be a non-empty frame no larger than the source");
    int rc = check_rows(ctx, "resize dst", dst, 0, out_h);
    if (rc) return rc;
    const ResizeArgs a{in, in_layout, H, W, to_dev(dst), out_h, out_w};
    R2F_HIP(ctx, launch_64x4(resize_area_kernel, out_w, out_h, static_cast<hipStream_t>(stream), a));
    return R2F_OK;
}

int r2f_warp_affine(r2f_ctx* ctx, const void* in, int in_layout, int H, int W, const double* m_dst_to_src, const r2f_planes* dst,
                    int out_h, int out_w, int oy, int ox, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (!in || !m_dst_to_src || in_layout < 0 || in_layout > 2 || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0)
        return fail(ctx, R2F_EINVAL, "warp_affine: bad arguments");
    int rc = check_rows(ctx, "warp dst", dst, 0, out_h);
    if (rc) return rc;
    WarpArgs a{in, in_layout, H, W, to_dev(dst), out_h, out_w, oy, ox, {}};
    for (int i = 0; i < 6; ++i) a.m[i] = (float)m_dst_to_src[i];
    R2F_HIP(ctx, launch_64x4(warp_affine_kernel, out_w, out_h, static_cast<hipStream_t>(stream), a));
    return R2F_OK;
}

// What both lens entry points check and set up: the arguments, the rows of `dst`, the phase table on the device -> the kernel's args.
static int lens_args(r2f_ctx* ctx, const char* what, const void* in, int in_layout, int H, int W, const r2f_lens_params* params,
                     const r2f_planes* dst, int out_h, int out_w, int oy, int ox, LensArgs* a) {
    // (the phase split adds 3 to a frame side and multiplies by 32 in float; the window's coordinates go through int sums)
    constexpr int kMaxSide = 1 << 24;
    if (!in || !params || in_layout < 0 || in_layout > 2 || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0 || H > kMaxSide || W > kMaxSide ||
        out_h > kMaxSide || out_w > kMaxSide || oy < -kMaxSide || oy > kMaxSide || ox < -kMaxSide || ox > kMaxSide)
        return fail(ctx, R2F_EINVAL, "%s: bad arguments", what);
    if (params->model < R2F_LENS_NONE || params->model > R2F_LENS_PTLENS)
        return fail(ctx, R2F_EINVAL, "%s: unknown distortion model %d", what, params->model);
    int rc = check_rows(ctx, "lens dst", dst, 0, out_h);
    if (rc) return rc;
    if (!ctx->lens_table.p) {
        float host[lens::kPhases * lens::kTaps];
        r2f_lens_phase_table(host);
        rc = upload(ctx, ctx->lens_table, host, sizeof host);  // (once per context)
        if (rc) return rc;
    }
    *a = LensArgs{in, in_layout, H, W, to_dev(dst), out_h, out_w, oy, ox, *params, static_cast<const float*>(ctx->lens_table.p)};
    return R2F_OK;
}

static dim3 lens_grid(int out_h, int out_w) { return dim3((out_w + 63) / 64, (out_h + 4 * kLensRows - 1) / (4 * kLensRows)); }

int r2f_lens_correct(r2f_ctx* ctx, const void* in, int in_layout, int H, int W, const r2f_lens_params* params, const r2f_planes* dst,
                     int out_h, int out_w, int oy, int ox, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    LensArgs a;
    const int rc = lens_args(ctx, "lens_correct", in, in_layout, H, W, params, dst, out_h, out_w, oy, ox, &a);
    if (rc) return rc;
    launch_k(lens_correct_kernel, lens_grid(out_h, out_w), dim3(64, 4), 0, static_cast<hipStream_t>(stream), a);
    R2F_HIP(ctx, take_launch_status());
    return R2F_OK;
}

int r2f_lens_correct_tca(r2f_ctx* ctx, const void* in, int in_layout, int H, int W, const r2f_lens_params* params,
                         const r2f_lens_tca_params* tca_params, const r2f_planes* dst, int out_h, int out_w, int oy, int ox, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (!tca_params) return fail(ctx, R2F_EINVAL, "lens_correct_tca: bad arguments");
    if (tca_params->model != R2F_TCA_LINEAR && tca_params->model != R2F_TCA_POLY3)
        return fail(ctx, R2F_EINVAL, "lens_correct_tca: TCA model %d (without TCA the call is r2f_lens_correct)", tca_params->model);
    LensTcaArgs a;
    const int rc = lens_args(ctx, "lens_correct_tca", in, in_layout, H, W, params, dst, out_h, out_w, oy, ox, &a.lens);
    if (rc) return rc;
    a.tca = *tca_params;
    launch_k(lens_correct_tca_kernel, lens_grid(out_h, out_w), dim3(64, 4), 0, static_cast<hipStream_t>(stream), a);
    R2F_HIP(ctx, take_launch_status());
    return R2F_OK;
}

int r2f_lens_correct_projected(r2f_ctx* ctx, const void* in, int in_layout, int H, int W, const r2f_lens_params* params,
                               const r2f_lens_projection_params* projection_params, const r2f_lens_tca_params* tca_params,
                               const r2f_planes* dst, int out_h, int out_w, int oy, int ox, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (!projection_params) return fail(ctx, R2F_EINVAL, "lens_correct_projected: bad arguments");
    if (projection_params->type < R2F_PROJ_FISHEYE || projection_params->type > R2F_PROJ_ORTHOGRAPHIC)
        return fail(ctx, R2F_EINVAL, "lens_correct_projected: projection type %d (without a projection the call is r2f_lens_correct or r2f_lens_correct_tca)",
                    projection_params->type);
    if (tca_params && tca_params->model != R2F_TCA_LINEAR && tca_params->model != R2F_TCA_POLY3)
        return fail(ctx, R2F_EINVAL, "lens_correct_projected: TCA model %d (without TCA pass no record)", tca_params->model);
    LensProjectedArgs a{};
    const int rc = lens_args(ctx, "lens_correct_projected", in, in_layout, H, W, params, dst, out_h, out_w, oy, ox, &a.lens);
    if (rc) return rc;
    a.proj = *projection_params;
    if (tca_params) a.tca = *tca_params;
    // the two forms of the projected kernel, by whether there is a TCA record
    static constexpr void (*kProjected[2])(LensProjectedArgs) = {lens_correct_projected_kernel<false>, lens_correct_projected_kernel<true>};
    launch_k(kProjected[tca_params ? 1 : 0], lens_grid(out_h, out_w), dim3(64, 4), 0, static_cast<hipStream_t>(stream), a);
    R2F_HIP(ctx, take_launch_status());
    return R2F_OK;
}

int r2f_resize_lanczos4_f32(r2f_ctx* ctx, const void* in, int in_layout, int H, int W, const r2f_planes* dst, int out_h, int out_w,
                            void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (!in || in_layout < 0 || in_layout > 2 || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0)
        return fail(ctx, R2F_EINVAL, "resize_lanczos4_f32: bad arguments");
    int rc = check_rows(ctx, "lanczos dst", dst, 0, out_h);
    if (rc) return rc;
    const int *xofs, *yofs;
    const float *xcoef, *ycoef;
    rc = ctx->lanczos_f32.tables(ctx, H, W, out_h, out_w, &xofs, &yofs, &xcoef, &ycoef);
    if (rc) return rc;
    const LanczosFloatArgs<PlanesFrame> a{{in, in_layout, H, W, to_dev(dst), out_w}, H, W, out_h, out_w, xofs, xcoef, yofs, ycoef};
    R2F_HIP(ctx, launch_64x4(lanczos4_float_kernel<PlanesFrame>, out_w, out_h, static_cast<hipStream_t>(stream), a));
    return R2F_OK;
}

int r2f_resize_lanczos4_u8(r2f_ctx* ctx, const uint8_t* src_hwc, int H, int W, uint8_t* dst_hwc, int out_h, int out_w, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (!src_hwc || !dst_hwc || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0)
        return fail(ctx, R2F_EINVAL, "resize_lanczos4: bad arguments");
    LanczosArgs a;
    a.src = src_hwc;
    a.dst = dst_hwc;
    a.H = H, a.W = W, a.out_h = out_h, a.out_w = out_w;
    int rc = ctx->lanczos_u8.tables(ctx, H, W, out_h, out_w, &a.xofs, &a.yofs, &a.xcoef, &a.ycoef);
    if (rc) return rc;
    R2F_HIP(ctx, launch_64x4(lanczos4_u8_kernel, out_w, out_h, static_cast<hipStream_t>(stream), a));
    return R2F_OK;
}

int r2f_resize_lanczos4_u16(r2f_ctx* ctx, const uint16_t* src_hwc, int H, int W, uint16_t* dst_hwc, int out_h, int out_w, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (!src_hwc || !dst_hwc || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0)
        return fail(ctx, R2F_EINVAL, "resize_lanczos4_u16: bad arguments");
    if ((reinterpret_cast<uintptr_t>(src_hwc) | reinterpret_cast<uintptr_t>(dst_hwc)) & 1u)
        return fail(ctx, R2F_EINVAL, "resize_lanczos4_u16: source and destination must be 2-byte aligned");
    const int *xofs, *yofs;
    const float *xcoef, *ycoef;
    int rc = ctx->lanczos_u16.tables(ctx, H, W, out_h, out_w, &xofs, &yofs, &xcoef, &ycoef);
    if (rc) return rc;
    const LanczosFloatArgs<U16Frame> a{{src_hwc, dst_hwc, W, out_w}, H, W, out_h, out_w, xofs, xcoef, yofs, ycoef};
    R2F_HIP(ctx, launch_64x4(lanczos4_float_kernel<U16Frame>, out_w, out_h, static_cast<hipStream_t>(stream), a));
    return R2F_OK;
}

int r2f_resize_area_u16(r2f_ctx* ctx, const uint16_t* src_hwc, int H, int W, uint16_t* dst_hwc, int out_h, int out_w, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (!src_hwc || !dst_hwc || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0 || out_h > H || out_w > W)
        return fail(ctx, R2F_EINVAL, "resize_area_u16: the target must be a non-empty frame no larger than the source");
    if ((reinterpret_cast<uintptr_t>(src_hwc) | reinterpret_cast<uintptr_t>(dst_hwc)) & 1u)
        return fail(ctx, R2F_EINVAL, "resize_area_u16: source and destination must be 2-byte aligned");
    const AreaArgs<uint16_t> a{src_hwc, dst_hwc, H, W, out_h, out_w};
    R2F_HIP(ctx, launch_64x4(resize_area_int_kernel<uint16_t>, out_w, out_h, static_cast<hipStream_t>(stream), a));
    return R2F_OK;
}

int r2f_resize_area_u8(r2f_ctx* ctx, const uint8_t* src_hwc, int H, int W, uint8_t* dst_hwc, int out_h, int out_w, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (!src_hwc || !dst_hwc || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0 || out_h > H || out_w > W)
        return fail(ctx, R2F_EINVAL, "resize_area_u8: the target must be a non-empty frame no larger than the source");
    const AreaArgs<uint8_t> a{src_hwc, dst_hwc, H, W, out_h, out_w};
    R2F_HIP(ctx, launch_64x4(resize_area_int_kernel<uint8_t>, out_w, out_h, static_cast<hipStream_t>(stream), a));
    return R2F_OK;
}

}  // extern "C"
