// r2f_resample.hip -- every resampler on either side of the render path, with its entry point (include/r2f.h) next to its kernel:
//   resize_area            pre-path INTER_AREA down-scale of the float frame to the preview resolution
//   resize_area_u8 / _u16  cpu_processor.py:411-412 -> utils.resolution_scaling -> cv.resize(canvas, INTER_AREA): the final shrink of
//                          the rendered (and canvas-framed) uint8 / uint16 frame to the requested resolution
//   warp_affine            pre-path free rotation (cv.warpAffine, INTER_LINEAR, zero border)
//   lanczos4_u8            post-path up-scale of the uint8 result (cv.resize INTER_LANCZOS4): the way back from max_scale
//   lanczos4_f32 / _u16    the float-weight LANCZOS4: the float frame before the path, the uint16 result after it
// None of this runs inside r2f_render or a timed step; the kernels are one lane per output pixel (launch_64x4).  The lens step, a
// resampler with a staging scheme of its own, is r2f_lens.hip.
#include <cstring>
#include <vector>

#include "r2f_ctx.h"

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
