// r2f_post.hip -- what sits after the path on the caller's side, kept on the device:
//   resize_area_u16 / lanczos4_u16: the same two steps on a 16-bit result (output_bits = 16)
//   resize_area_u8     cpu_processor.py:411-412 -> utils.resolution_scaling -> cv.resize(uint8 canvas, INTER_AREA): the CPU
//                      processor's final shrink of the rendered (and canvas-framed) uint8 frame to the requested resolution
//   blit_rgba8         shaders/copy_to_int.wgsl (bound by gpu_processor.py:1416-1539): the display-referred float frame
//                      letterboxed into the preview widget's RGBA8 texture -- bilinear sample, canvas colour inside the canvas
//                      bounds, transparent outside
//   histogram_render   shaders/histogram.wgsl pass2_process + pass3_render and shaders/scale_texture.wgsl: the 3 x 256 counts
//                      (r2f_histogram_u8 = pass 1) -> log1p, 3-bin smoothing, bar heights -> the 256 x height RGBA bar image ->
//                      nearest-neighbour copy into the histogram widget's texture
// None of this is on the timed hot path; the kernels are one lane per output pixel.
#include "r2f_launch.h"

#include "../../include/r2f.h"

namespace r2f {

namespace {

// ---------------------------------------------------------------------------------------------------- INTER_AREA, uint8
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

// ---------------------------------------------------------------------------------------------------- LANCZOS4, float32
// cv.resize(float32 frame, INTER_LANCZOS4): utils.resolution_scaling's other branch (utils.py:237-242), taken BEFORE the path
// when the preview is larger than the frame (cpu_processor.py:134).  cv::resize's generic path for CV_32F: float weights from
// interpolateLanczos4 (host tables, r2f_api.hip), HResizeLanczos4 = the 8 products of a row summed left to right, then
// VResizeLanczos4 = the 8 rows times beta summed top to bottom; indices outside the frame repeat the edge sample.
struct LanczosF32Args {
    const void* in;
    int in_layout, H, W;
    DevPlanes dst;
    int out_h, out_w;
    const int* xofs;    // out_w: source column of tap 3
    const float* xcoef;  // out_w x 8
    const int* yofs;
    const float* ycoef;
};

__device__ __forceinline__ void load_px(const void* in_, int layout, int H, int W, int y, int x, float (&v)[3]) {
    const float* in = static_cast<const float*>(in_);
    if (layout == R2F_LAYOUT_CHW) {
        const long long plane = (long long)H * W, o = (long long)y * W + x;
        v[0] = in[o], v[1] = in[plane + o], v[2] = in[2 * plane + o];
    } else {
        const float* p = in + ((long long)y * W + x) * (layout == R2F_LAYOUT_HWC4 ? 4 : 3);
        v[0] = p[0], v[1] = p[1], v[2] = p[2];
    }
}

__global__ __launch_bounds__(256) void lanczos4_f32_kernel(const LanczosF32Args a) {
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
            load_px(a.in, a.in_layout, a.H, a.W, yy, clampi(sx + j, 0, a.W - 1), v);
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
    float* p0 = a.dst.data + (long long)(dy - a.dst.gy0) * a.out_w + dx;
    p0[0] = acc[0];
    p0[a.dst.plane_stride] = acc[1];
    p0[2 * a.dst.plane_stride] = acc[2];
}

// ---------------------------------------------------------------------------------------------------- LANCZOS4, uint16
// cv.resize(uint16 frame, INTER_LANCZOS4): the way back from max_scale for a 16-bit result.  CV_16U takes the float-weight path of
// the float frame above (the same tables), HResizeLanczos4 then VResizeLanczos4 in float, and ends in saturate_cast<ushort>:
// round half to even, clamp to [0, 65535].  One lane per output pixel.
struct LanczosU16Args {
    const uint16_t* src;  // (H, W, 3)
    uint16_t* dst;        // (out_h, out_w, 3)
    int H, W, out_h, out_w;
    const int* xofs;
    const float* xcoef;
    const int* yofs;
    const float* ycoef;
};

__global__ __launch_bounds__(256) void lanczos4_u16_kernel(const LanczosU16Args a) {
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
        const uint16_t* row = a.src + (long long)clampi(sy + k, 0, a.H - 1) * a.W * 3;
        float h[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint16_t* px = row + (long long)clampi(sx + j, 0, a.W - 1) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float prod = (float)px[c] * wx[j];
                h[c] = j == 0 ? prod : h[c] + prod;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float prod = h[c] * wy[k];
            acc[c] = k == 0 ? prod : acc[c] + prod;
        }
    }
    uint16_t* o = a.dst + ((long long)dy * a.out_w + dx) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = sat_u16(acc[c]);
}

// ---------------------------------------------------------------------------------------------------- preview blit
struct BlitArgs {
    const float* src;  // (H, W, 3) display-referred float
    uint8_t* dst;      // (dst_h, dst_w, 4)
    int H, W, dst_h, dst_w;
    r2f_blit t;
};

__device__ __forceinline__ uint8_t unorm8(float v) { return (uint8_t)__float2int_rn(fminf(fmaxf(v, 0.f), 1.f) * 255.f); }

// textureSampleLevel(linear, clamp-to-edge) at normalised uv: texel centres at (i + 0.5) / size
__device__ __forceinline__ void sample_bilinear(const float* src, int H, int W, float u, float v, float (&rgb)[3]) {
    const float fx = u * (float)W - 0.5f, fy = v * (float)H - 0.5f;
    const float x0f = floorf(fx), y0f = floorf(fy);
    const float tx = fx - x0f, ty = fy - y0f;
    const int x0 = clampi((int)x0f, 0, W - 1), x1 = clampi((int)x0f + 1, 0, W - 1);
    const int y0 = clampi((int)y0f, 0, H - 1), y1 = clampi((int)y0f + 1, 0, H - 1);
    const float* p00 = src + ((long long)y0 * W + x0) * 3;
    const float* p01 = src + ((long long)y0 * W + x1) * 3;
    const float* p10 = src + ((long long)y1 * W + x0) * 3;
    const float* p11 = src + ((long long)y1 * W + x1) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float top = p00[c] + tx * (p01[c] - p00[c]), bot = p10[c] + tx * (p11[c] - p10[c]);
        rgb[c] = top + ty * (bot - top);
    }
}

__global__ __launch_bounds__(256) void blit_rgba8_kernel(const BlitArgs a) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= a.dst_w || y >= a.dst_h) return;
    const float cx = (float)x + 0.5f, cy = (float)y + 0.5f;
    const float u = (cx - a.t.offset_x) * a.t.scale_x, v = (cy - a.t.offset_y) * a.t.scale_y;
    uchar4 out = make_uchar4(0, 0, 0, 0);  // outside everything: transparent
    if (u >= 0.f && u <= 1.f && v >= 0.f && v <= 1.f) {
        float rgb[3];
        sample_bilinear(a.src, a.H, a.W, u, v, rgb);
        out = make_uchar4(unorm8(rgb[0]), unorm8(rgb[1]), unorm8(rgb[2]), 255);
    } else if (cx >= a.t.canvas_min_x && cx <= a.t.canvas_max_x && cy >= a.t.canvas_min_y && cy <= a.t.canvas_max_y) {
        out = make_uchar4(unorm8(a.t.canvas_color[0]), unorm8(a.t.canvas_color[1]), unorm8(a.t.canvas_color[2]), 255);
    }
    reinterpret_cast<uchar4*>(a.dst)[(long long)y * a.dst_w + x] = out;
}

// ---------------------------------------------------------------------------------------------------- histogram image
struct HistArgs {
    const uint32_t* counts;  // [3][256]
    uint8_t* image;          // (height, 256, 4)
    uint8_t* target;         // (th, tw, 4) or null
    int height, th, tw;
    uint32_t mix[8];         // the 2 x 2 x 2 colour table, RGBA packed little-endian, index is_r * 4 + is_g * 2 + is_b
};

// One workgroup of 256 lanes: histogram.wgsl pass2_process (float32 throughout, like the shader), then pass3_render for the
// whole 256 x height image, then scale_texture.wgsl into the widget texture.
__global__ __launch_bounds__(256) void histogram_render_kernel(const HistArgs a) {
    __shared__ float sh[3][256];
    __shared__ float red[256];
    __shared__ uint32_t heights[3][256];
    const int i = threadIdx.x;
    float v[3];
    for (int c = 0; c < 3; ++c) v[c] = (float)a.counts[c * 256 + i];
    auto block_max = [&](float mine) {
        red[i] = mine;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (i < s) red[i] = fmaxf(red[i], red[i + s]);
            __syncthreads();
        }
        const float m = red[0];
        __syncthreads();
        return m;
    };
    float m = block_max(fmaxf(v[0], fmaxf(v[1], v[2])));
    if (!(m > 0.f)) m = 1.f;
    for (int c = 0; c < 3; ++c) sh[c][i] = logf(1.0f + v[c] / m);
    __syncthreads();
    const int l = i == 0 ? i : i - 1, r = i == 255 ? i : i + 1;
    float s3[3];
    for (int c = 0; c < 3; ++c) s3[c] = (sh[c][l] + sh[c][i] + sh[c][r]) / 3.0f;
    float fm = block_max(fmaxf(s3[0], fmaxf(s3[1], s3[2])));
    if (fm == 0.f) fm = 1.f;
    for (int c = 0; c < 3; ++c) heights[c][i] = (uint32_t)((s3[c] * (float)a.height) / fm);
    __syncthreads();
    uint32_t* img = reinterpret_cast<uint32_t*>(a.image);
    const uint32_t hr = heights[0][i], hg = heights[1][i], hb = heights[2][i];
    for (int y = 0; y < a.height; ++y) {  // lane i = bin column i
        const uint32_t is_r = (uint32_t)y >= (uint32_t)a.height - hr, is_g = (uint32_t)y >= (uint32_t)a.height - hg,
                       is_b = (uint32_t)y >= (uint32_t)a.height - hb;
        img[y * 256 + i] = a.mix[is_r * 4 + is_g * 2 + is_b];
    }
    if (!a.target) return;
    __threadfence_block();
    __syncthreads();
    uint32_t* tgt = reinterpret_cast<uint32_t*>(a.target);
    for (long long p = i; p < (long long)a.th * a.tw; p += 256) {  // scale_texture.wgsl: nearest, uv = id / target size
        const int ty = (int)(p / a.tw), tx = (int)(p - (long long)ty * a.tw);
        const int sx = (int)(((float)tx / (float)a.tw) * 256.0f), sy = (int)(((float)ty / (float)a.th) * (float)a.height);
        tgt[p] = img[min(sy, a.height - 1) * 256 + min(sx, 255)];
    }
}

}  // namespace

namespace {

// The hand-off from RAW decoding, raw_to_linear's last two lines (raw_conversion.py:50-52) on LibRaw's 16-bit output:
// x = float(u) / 65535 (one correctly rounded fp32 division, like NumPy's), then x *= the float32 exposure factor, then the
// upload clamp of the GPU path (gpu_processor.py:275: min(x, 65504); the input cannot be negative).
// One lane = 4 pixels of an (n, ch) uint16 frame -> 12 floats of the (n, 3) float frame.
struct DecodeU16Args {
    const uint16_t* src;
    float* dst;
    long long n;  // pixels
    int ch;       // 3 or 4 (a fourth channel is dropped)
    float divisor, factor;
    int vec;      // 1: both buffers 16-byte aligned and ch == 3 -> 8-byte loads, 16-byte stores
};

#pragma clang fp contract(off)
__global__ __launch_bounds__(256) void decode_u16_kernel(const DecodeU16Args a) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;  // quad of pixels
    const long long p0 = q * 4;
    if (p0 >= a.n) return;
    if (a.vec && p0 + 4 <= a.n) {
        const uint2* s2 = reinterpret_cast<const uint2*>(a.src + p0 * 3);  // 24 bytes = 12 samples
        const uint2 w0 = s2[0], w1 = s2[1], w2 = s2[2];
        const unsigned w[6] = {w0.x, w0.y, w1.x, w1.y, w2.x, w2.y};
        float f[12];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            f[2 * i] = fminf((float)(w[i] & 0xffffu) / a.divisor * a.factor, 65504.0f);
            f[2 * i + 1] = fminf((float)(w[i] >> 16) / a.divisor * a.factor, 65504.0f);
        }
        float4* d4 = reinterpret_cast<float4*>(a.dst + p0 * 3);
        d4[0] = make_float4(f[0], f[1], f[2], f[3]);
        d4[1] = make_float4(f[4], f[5], f[6], f[7]);
        d4[2] = make_float4(f[8], f[9], f[10], f[11]);
        return;
    }
    for (long long p = p0; p < min(p0 + 4, a.n); ++p)
        for (int c = 0; c < 3; ++c) a.dst[p * 3 + c] = fminf((float)a.src[p * a.ch + c] / a.divisor * a.factor, 65504.0f);
}

// ---------------------------------------------------------------------------------------------------- auto exposure
// calc_exposure (color_processing.py:71-99) measured on the uploaded uint16 frame: over u = frame[::2, ::2, 1],
//   g = (float)u / 65535 (the fp32 division of raw_conversion.py:50), widened to double; m = mean(pow(g, 1 / root));
//   stops = log2(ref / pow(m, root)); factor = (float)(2 ** stops)
// -- upstream's formula in fp64 (upstream's own float32 evaluation is 2e-8 .. 5e-5 stops away from it).
//
// exposure_rows_kernel: one workgroup per sampled row (global row index even) -> that row's fp64 sum in sums[y / 2].  The shape of
// the sum is a function of W alone: the row is cut into chunks of 8 pixels (4 samples, 48 bytes of a 3-channel row), lane t adds
// the chunks t, t + 256, ... sample by sample into one accumulator, and the 256 accumulators meet in a fixed LDS tree.  Whether a
// chunk comes in as three 16-byte loads (3 channels, row base 16-byte aligned) or sample by sample changes no operand, so a
// row's sum depends only on its bytes, W, channels and root: the same bits however the rows are delivered.  No atomics.
struct ExposureRowsArgs {
    const uint16_t* src;  // row src_gy0 of the (H, W, ch) frame
    int src_gy0;
    int W, ch;
    int y_first, n_rows;  // first sampled row (even) and the number of sampled rows of this call
    double inv_root;
    double* sums;  // [ceil(H / 2)]
};

__device__ __forceinline__ double exposure_term(unsigned u, double inv_root) {
    const float g = (float)u / 65535.0f;  // correctly rounded, like NumPy's and decode_u16_kernel's
    return pow((double)g, inv_root);
}

// The sum of 256 lane accumulators in a fixed order (s = 128, 64, ... 1: red[i] += red[i + s]); every lane gets it.
__device__ __forceinline__ double block_sum_256(double mine, double* red) {
    const int i = threadIdx.x;
    red[i] = mine;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (i < s) red[i] = red[i] + red[i + s];
        __syncthreads();
    }
    const double total = red[0];
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(256) void exposure_rows_kernel(const ExposureRowsArgs a) {
    __shared__ double red[256];
    if ((int)blockIdx.x >= a.n_rows) return;
    const int y = a.y_first + 2 * (int)blockIdx.x;
    const uint16_t* row = a.src + (long long)(y - a.src_gy0) * a.W * a.ch;
    const bool vec = a.ch == 3 && (reinterpret_cast<uintptr_t>(row) & 15u) == 0;  // (uniform over the workgroup)
    const int chunks = (a.W + 7) / 8;
    double acc = 0.0;
    for (int c = threadIdx.x; c < chunks; c += 256) {
        const int x0 = 8 * c;
        if (vec && x0 + 8 <= a.W) {
            const uint4* s4 = reinterpret_cast<const uint4*>(row + (long long)x0 * 3);  // 24 samples; the greens are 1, 7, 13, 19
            const uint4 w0 = s4[0], w1 = s4[1], w2 = s4[2];
            acc = acc + exposure_term(w0.x >> 16, a.inv_root);
            acc = acc + exposure_term(w0.w >> 16, a.inv_root);
            acc = acc + exposure_term(w1.z >> 16, a.inv_root);
            acc = acc + exposure_term(w2.y >> 16, a.inv_root);
        } else {
            for (int x = x0; x < min(x0 + 8, a.W); x += 2)
                acc = acc + exposure_term(row[(long long)x * a.ch + 1], a.inv_root);
        }
    }
    const double total = block_sum_256(acc, red);
    if (threadIdx.x == 0) a.sums[y >> 1] = total;
}

// exposure_finish_kernel: ONE workgroup adds the ceil(H / 2) row sums (lane t takes t, t + 256, ... in order, then the same LDS
// tree) and writes stops and factor into the context's record.
struct ExposureFinishArgs {
    const double* sums;
    int n_rows;        // ceil(H / 2)
    double n_samples;  // ceil(H / 2) * ceil(W / 2)
    double root, ref;
    ExposureRecord* rec;
};

__global__ __launch_bounds__(256) void exposure_finish_kernel(const ExposureFinishArgs a) {
    __shared__ double red[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < a.n_rows; i += 256) acc = acc + a.sums[i];
    const double total = block_sum_256(acc, red);
    if (threadIdx.x != 0) return;
    const double m = total / a.n_samples;
    const double stops = log2(a.ref / pow(m, a.root));  // (an all-zero sample set: 0.18 / 0 = +inf stops, like the host's)
    a.rec->stops = stops;
    a.rec->factor = (float)exp2(stops);
    a.rec->pad = 0u;
}

// decode_u16_kernel with the factor read from the record and a pitched source: W pixels of each of H rows that lie src_pitch
// pixels apart (a crop of the uploaded frame is a pointer offset plus the pitch).  The same expression, contraction off: the same
// floats for the same factor.  One lane = 4 pixels of one row.
struct DecodeU16AutoArgs {
    const uint16_t* src;
    float* dst;
    long long W, src_pitch;  // pixels
    int H, ch;
    unsigned quad_blocks;    // workgroups per row
    float divisor;
    const ExposureRecord* rec;
    int vec;  // 1: ch == 3, every source row starts 8-byte and every destination row 16-byte aligned -> 8-byte loads, 16-byte stores
};

__global__ __launch_bounds__(256) void decode_u16_auto_kernel(const DecodeU16AutoArgs a) {
    const long long y = blockIdx.x / a.quad_blocks;
    const long long p0 = ((long long)(blockIdx.x % a.quad_blocks) * 256 + threadIdx.x) * 4;
    if (y >= a.H || p0 >= a.W) return;
    const float factor = a.rec->factor;
    const uint16_t* src = a.src + y * a.src_pitch * a.ch;
    float* dst = a.dst + y * a.W * 3;
    if (a.vec && p0 + 4 <= a.W) {
        const uint2* s2 = reinterpret_cast<const uint2*>(src + p0 * 3);
        const uint2 w0 = s2[0], w1 = s2[1], w2 = s2[2];
        const unsigned w[6] = {w0.x, w0.y, w1.x, w1.y, w2.x, w2.y};
        float f[12];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            f[2 * i] = fminf((float)(w[i] & 0xffffu) / a.divisor * factor, 65504.0f);
            f[2 * i + 1] = fminf((float)(w[i] >> 16) / a.divisor * factor, 65504.0f);
        }
        float4* d4 = reinterpret_cast<float4*>(dst + p0 * 3);
        d4[0] = make_float4(f[0], f[1], f[2], f[3]);
        d4[1] = make_float4(f[4], f[5], f[6], f[7]);
        d4[2] = make_float4(f[8], f[9], f[10], f[11]);
        return;
    }
    for (long long p = p0; p < min(p0 + 4, a.W); ++p)
        for (int c = 0; c < 3; ++c) dst[p * 3 + c] = fminf((float)src[p * a.ch + c] / a.divisor * factor, 65504.0f);
}

// Measurement aid (bench.py's `copy_ceiling`): a float4 streaming copy, 2 x `bytes` of HBM traffic -- what this chip moves when a
// kernel does nothing but load and store coalesced 16-byte lanes.  One float4 per lane, non-temporal both ways, one workgroup per
// 4 KB: the fastest of the shapes in tools/ubench/copy_rate.hip on MI355X (6.57 TB/s; plain loads / stores 6.23, four float4 per
// lane 5.84, a persistent grid-stride loop 4.6-4.8, hipMemcpyDtoD 5.10).
typedef float f4v __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void stream_copy_kernel(const f4v* __restrict__ src, f4v* __restrict__ dst, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
}

}  // namespace

hipError_t launch_stream_copy(const void* src, void* dst, long long bytes, hipStream_t s) {
    const long long n = bytes / 16;
    launch_k(stream_copy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, static_cast<const f4v*>(src),
                       static_cast<f4v*>(dst), n);
    return take_launch_status();
}

hipError_t launch_decode_u16(const uint16_t* src, long long n, int ch, float divisor, float factor, float* dst, hipStream_t s) {
    DecodeU16Args a{src, dst, n, ch, divisor, factor,
                    (ch == 3 && (reinterpret_cast<uintptr_t>(src) & 15u) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) ? 1 : 0};
    const long long quads = (n + 3) / 4;
    launch_k(decode_u16_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, s, a);
    return take_launch_status();
}

hipError_t launch_exposure_rows(const uint16_t* src, int src_gy0, int W, int ch, int y0, int y1, double root, double* sums, hipStream_t s) {
    const int y_first = y0 + (y0 & 1), n_rows = (y1 - y_first + 1) / 2;  // the even rows of [y0, y1)
    if (n_rows <= 0) return hipSuccess;
    ExposureRowsArgs a{src, src_gy0, W, ch, y_first, n_rows, 1.0 / root, sums};
    launch_k(exposure_rows_kernel, dim3((unsigned)n_rows), dim3(256), 0, s, a);
    return take_launch_status();
}

hipError_t launch_exposure_finish(const double* sums, int H, int W, double root, double ref, ExposureRecord* rec, hipStream_t s) {
    const int n_rows = (H + 1) / 2;
    ExposureFinishArgs a{sums, n_rows, (double)n_rows * (double)((W + 1) / 2), root, ref, rec};
    launch_k(exposure_finish_kernel, dim3(1), dim3(256), 0, s, a);
    return take_launch_status();
}

hipError_t launch_decode_u16_auto(const uint16_t* src, int H, int W, int ch, long long src_pitch, float divisor, const ExposureRecord* rec,
                                  float* dst, hipStream_t s) {
    DecodeU16AutoArgs a{src, dst, W, src_pitch, H, ch, 0u, divisor, rec, 0};
    if (src_pitch == W) a.W = a.src_pitch = (long long)H * W, a.H = 1;  // contiguous rows: one long row, like decode_u16_kernel
    const bool rows_ok = a.H == 1 || (a.W % 4 == 0 && a.src_pitch % 4 == 0);
    a.vec = (ch == 3 && rows_ok && (reinterpret_cast<uintptr_t>(src) & 7u) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) ? 1 : 0;
    const long long quads = (a.W + 3) / 4;
    a.quad_blocks = (unsigned)((quads + 255) / 256);
    launch_k(decode_u16_auto_kernel, dim3((unsigned)((long long)a.quad_blocks * a.H)), dim3(256), 0, s, a);
    return take_launch_status();
}

hipError_t launch_resize_area_u8(const uint8_t* src, int H, int W, uint8_t* dst, int out_h, int out_w, hipStream_t s) {
    AreaArgs<uint8_t> a{src, dst, H, W, out_h, out_w};
    launch_k(resize_area_int_kernel<uint8_t>, dim3((out_w + 63) / 64, (out_h + 3) / 4), dim3(64, 4), 0, s, a);
    return take_launch_status();
}

hipError_t launch_resize_area_u16(const uint16_t* src, int H, int W, uint16_t* dst, int out_h, int out_w, hipStream_t s) {
    AreaArgs<uint16_t> a{src, dst, H, W, out_h, out_w};
    launch_k(resize_area_int_kernel<uint16_t>, dim3((out_w + 63) / 64, (out_h + 3) / 4), dim3(64, 4), 0, s, a);
    return take_launch_status();
}

hipError_t launch_lanczos4_u16(const uint16_t* src, int H, int W, uint16_t* dst, int out_h, int out_w, const int* xofs, const float* xcoef,
                               const int* yofs, const float* ycoef, hipStream_t s) {
    LanczosU16Args a{src, dst, H, W, out_h, out_w, xofs, xcoef, yofs, ycoef};
    launch_k(lanczos4_u16_kernel, dim3((out_w + 63) / 64, (out_h + 3) / 4), dim3(64, 4), 0, s, a);
    return take_launch_status();
}

hipError_t launch_lanczos4_f32(const void* in, int in_layout, int H, int W, const DevPlanes& dst, int out_h, int out_w, const int* xofs,
                               const float* xcoef, const int* yofs, const float* ycoef, hipStream_t s) {
    LanczosF32Args a{in, in_layout, H, W, dst, out_h, out_w, xofs, xcoef, yofs, ycoef};
    launch_k(lanczos4_f32_kernel, dim3((out_w + 63) / 64, (out_h + 3) / 4), dim3(64, 4), 0, s, a);
    return take_launch_status();
}

hipError_t launch_blit_rgba8(const float* src, int H, int W, uint8_t* dst, int dst_h, int dst_w, const r2f_blit& t, hipStream_t s) {
    BlitArgs a{src, dst, H, W, dst_h, dst_w, t};
    launch_k(blit_rgba8_kernel, dim3((dst_w + 63) / 64, (dst_h + 3) / 4), dim3(64, 4), 0, s, a);
    return take_launch_status();
}

hipError_t launch_histogram_render(const uint32_t* counts, const uint8_t* mix_rgba, int height, uint8_t* image, uint8_t* target, int th,
                                   int tw, hipStream_t s) {
    HistArgs a;
    a.counts = counts, a.image = image, a.target = target, a.height = height, a.th = th, a.tw = tw;
    for (int k = 0; k < 8; ++k)
        a.mix[k] = (uint32_t)mix_rgba[4 * k] | ((uint32_t)mix_rgba[4 * k + 1] << 8) | ((uint32_t)mix_rgba[4 * k + 2] << 16) |
                   ((uint32_t)mix_rgba[4 * k + 3] << 24);
    launch_k(histogram_render_kernel, dim3(1), dim3(256), 0, s, a);
    return take_launch_status();
}

}  // namespace r2f
