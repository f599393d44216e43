// r2f_post.hip -- everything off the render path that is not a resampler (those: r2f_resample.hip) or the lens step (r2f_lens.hip), each stage's entry point
// (include/r2f.h) next to its kernel.  Before the path:
//   decode_u16 / exposure_rows, _finish / decode_u16_auto   the hand-off from RAW decoding: uint16 -> float frame, with the exposure
//                      factor given or measured on the device (calc_exposure)
//   chroma_h / _v      chroma NR: xyY + separable Gaussian on the chromaticity planes
// after it, on the caller's side:
//   blit_rgba8         shaders/copy_to_int.wgsl (bound by gpu_processor.py:1416-1539): the display-referred float frame
//                      letterboxed into the preview widget's RGBA8 texture -- bilinear sample, canvas colour inside the canvas
//                      bounds, transparent outside
//   histogram_u8       utils.generate_histogram / histogram.wgsl pass 1: RGB counts of the uint8 output
//   histogram_render   shaders/histogram.wgsl pass2_process + pass3_render and shaders/scale_texture.wgsl: the 3 x 256 counts
//                      -> log1p, 3-bin smoothing, bar heights -> the 256 x height RGBA bar image -> nearest-neighbour copy into
//                      the histogram widget's texture
// and a measurement aid: stream_copy (bench.py's copy ceiling).  None of this runs inside r2f_render.
#include <algorithm>
#include <cstring>

#include "r2f_ctx.h"

using namespace r2f;

namespace r2f {

// ---------------------------------------------------------------------------------------------------- chroma NR (pre-path)
constexpr int kChromaMaxTaps = 63;
struct ChromaArgs {
    const void* in;  // pass 1 input image
    int in_layout, in_gy0, in_rows;
    DevPlanes src;  // pass 2 input planes
    DevPlanes dst;
    int y0, y1, W, H_global;
    int radius;  // taps = 2*radius + 1
    int vec;
    float w[kChromaMaxTaps];
};

// effects.XYZ_to_xyY, effects.py:496-518
__device__ __forceinline__ void xyz_to_xy(float X, float Y, float Z, float& cx, float& cy) {
    const float denom = (X + Y) + Z;
    if (denom > 1e-8f) {
        cx = X / denom;
        cy = Y / denom;
    } else {
        cx = 0.f;
        cy = 0.f;
    }
}

// Pass 1: one workgroup = one row segment of 1024 pixels.  Chromaticities of the segment plus `radius` clamped
// neighbours on each side are staged in LDS (the one truly separable blur near this path), then every lane blurs its
// 4 pixels horizontally.  Output planes: x', y', Y.
constexpr int kChromaSeg = 1024;
__global__ __launch_bounds__(256) void chroma_h_kernel(const ChromaArgs a) {
    __shared__ float sx[kChromaSeg + 2 * 31], sy[kChromaSeg + 2 * 31];
    const int gy = a.y0 + blockIdx.y;
    const int seg0 = blockIdx.x * kChromaSeg;
    const int r = a.radius;
    const int n = kChromaSeg + 2 * r;
    float Yown[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < n; i += 256) {
        const int gx = clampi(seg0 - r + i, 0, a.W - 1);  // ix = min(max(x + i, 0), w - 1), effects.py:452
        float X, Y, Z;
        load_input1(a.in, a.in_layout, a.in_gy0, a.in_rows, a.W, gy, gx, X, Y, Z);
        xyz_to_xy(X, Y, Z, sx[i], sy[i]);
    }
    __syncthreads();
    const int x0 = seg0 + 4 * threadIdx.x;
    if (x0 >= a.W) return;
    const int nv = min(4, a.W - x0);
    float bx[4], by[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        float accx = 0.f, accy = 0.f;
        const int c = 4 * threadIdx.x + p;  // window [c, c + 2r] in LDS
        for (int t = 0; t <= 2 * r; ++t) {
            accx = fmaf(sx[c + t], a.w[t], accx);
            accy = fmaf(sy[c + t], a.w[t], accy);
        }
        bx[p] = accx;
        by[p] = accy;
        if (p < nv) {
            float X, Y, Z;
            load_input1(a.in, a.in_layout, a.in_gy0, a.in_rows, a.W, gy, x0 + p, X, Y, Z);
            Yown[p] = Y;
        }
    }
    store_planes4(a.dst, gy, x0, a.W, nv, a.vec != 0, bx, by, Yown);
}

// Pass 2: vertical blur of x', y' (rows clamped to the frame) and effects.xyY_to_XYZ (effects.py:521-544).
__global__ __launch_bounds__(256) void chroma_v_kernel(const ChromaArgs a) {
    const int x = (blockIdx.x * 64 + threadIdx.x) * 4;
    const int gy = a.y0 + blockIdx.y * 4 + threadIdx.y;
    if (x >= a.W || gy >= a.y1) return;
    const int nv = min(4, a.W - x);
    const bool vec = a.vec != 0;
    const int r = a.radius;
    float ax[4] = {0.f, 0.f, 0.f, 0.f}, ay[4] = {0.f, 0.f, 0.f, 0.f};
    float Yc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t <= 2 * r; ++t) {
        const int sy = clampi(gy - r + t, 0, a.H_global - 1);  // iy = min(max(y + i, 0), h - 1), effects.py:476
        float px[4], py[4], pY[4];
        load_planes4(a.src, sy, x, a.W, nv, vec, px, py, pY);
        const float w = a.w[t];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            ax[p] = fmaf(px[p], w, ax[p]);
            ay[p] = fmaf(py[p], w, ay[p]);
            if (t == r) Yc[p] = pY[p];
        }
    }
    float X[4], Z[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        if (ay[p] > 1e-8f) {
            const float inv = Yc[p] / ay[p];
            X[p] = ax[p] * inv;
            Z[p] = ((1.0f - ax[p]) - ay[p]) * inv;
        } else {
            X[p] = 0.f;
            Yc[p] = 0.f;
            Z[p] = 0.f;
        }
    }
    store_planes4(a.dst, gy, x, a.W, nv, vec, X, Yc, Z);
}

// ---------------------------------------------------------------------------------------------------- histogram counts
// utils.generate_histogram's counting loop (utils.py:160-165) / histogram.wgsl pass1_accumulate on the uint8 (H, W, 3)
// output: 3 x 256 counts.  HBM-bound (3 B/px); the byte stream is read 16 B per lane, channel = byte index mod 3.  Flat
// images put most pixels into a few bins, so every group of 8 lanes owns a private copy of the table in LDS (same-address
// LDS atomics serialise) and the copies are folded into global memory once per workgroup.
constexpr int kHistCopies = 8, kHistThreads = 256, kHistBytesPerLane = 16, kHistIters = 16;

__global__ __launch_bounds__(kHistThreads) void histogram_u8_kernel(const uint8_t* __restrict__ image, long long n_bytes,
                                                                    uint32_t* __restrict__ counts) {
    __shared__ uint32_t h[kHistCopies][768];
    for (int i = threadIdx.x; i < kHistCopies * 768; i += kHistThreads) (&h[0][0])[i] = 0;
    __syncthreads();
    uint32_t* mine = h[threadIdx.x & (kHistCopies - 1)];
    const long long chunk = (long long)kHistThreads * kHistBytesPerLane;
    long long base = (long long)blockIdx.x * chunk * kHistIters;
    for (int it = 0; it < kHistIters; ++it, base += chunk) {
        const long long o = base + (long long)threadIdx.x * kHistBytesPerLane;
        if (o >= n_bytes) break;
        int ch = (int)(o % 3);
        if (o + kHistBytesPerLane <= n_bytes) {
            const uint4 v = *reinterpret_cast<const uint4*>(image + o);  // hipMalloc'ed images are 16-byte aligned
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    atomicAdd(&mine[ch * 256 + ((w[k] >> (8 * b)) & 255u)], 1u);
                    ch = ch == 2 ? 0 : ch + 1;
                }
        } else {
            for (long long i = o; i < n_bytes; ++i) {
                atomicAdd(&mine[ch * 256 + image[i]], 1u);
                ch = ch == 2 ? 0 : ch + 1;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 768; i += kHistThreads) {
        uint32_t s = 0;
#pragma unroll
        for (int c = 0; c < kHistCopies; ++c) s += h[c][i];
        if (s) atomicAdd(&counts[i], s);
    }
}

namespace {

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

#pragma clang fp contract(off)  // (file scope: the division and the product of the hand-off round separately, here and below)
// Pixels p0 .. p0 + 3 of a row of n pixels (fewer at its end): the body of both decode kernels.
__device__ __forceinline__ void decode_quad(const uint16_t* src, float* dst, long long p0, long long n, int ch, int vec, float divisor,
                                            float factor) {
    if (vec && p0 + 4 <= n) {
        const uint2* s2 = reinterpret_cast<const uint2*>(src + p0 * 3);  // 24 bytes = 12 samples
        const uint2 w0 = s2[0], w1 = s2[1], w2 = s2[2];
        const unsigned w[6] = {w0.x, w0.y, w1.x, w1.y, w2.x, w2.y};
        float f[12];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            f[2 * i] = decode_sample(w[i] & 0xffffu, divisor, factor);
            f[2 * i + 1] = decode_sample(w[i] >> 16, divisor, factor);
        }
        float4* d4 = reinterpret_cast<float4*>(dst + p0 * 3);
        d4[0] = make_float4(f[0], f[1], f[2], f[3]);
        d4[1] = make_float4(f[4], f[5], f[6], f[7]);
        d4[2] = make_float4(f[8], f[9], f[10], f[11]);
        return;
    }
    for (long long p = p0; p < min(p0 + 4, n); ++p)
        for (int c = 0; c < 3; ++c) dst[p * 3 + c] = decode_sample(src[p * ch + c], divisor, factor);
}

__global__ __launch_bounds__(256) void decode_u16_kernel(const DecodeU16Args a) {
    const long long p0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;  // the lane's quad of pixels
    if (p0 >= a.n) return;
    decode_quad(a.src, a.dst, p0, a.n, a.ch, a.vec, a.divisor, a.factor);
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
// pixels apart (a crop of the uploaded frame is a pointer offset plus the pitch).  The same decode_quad: the same floats for the
// same factor.  One lane = 4 pixels of one row.
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
    decode_quad(a.src + y * a.src_pitch * a.ch, a.dst + y * a.W * 3, p0, a.W, a.ch, a.vec, a.divisor, a.rec->factor);
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

}  // namespace r2f

// =============================================================================== C ABI
extern "C" {

int r2f_decode_u16(r2f_ctx* ctx, const uint16_t* src_hwc, int H, int W, int channels, float divisor, float factor, float* dst_f32_hwc3,
                   void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (!src_hwc || !dst_f32_hwc3 || H <= 0 || W <= 0 || (channels != 3 && channels != 4) || !(divisor > 0.f))
        return fail(ctx, R2F_EINVAL, "decode_u16: a non-empty 3- or 4-channel frame and a positive divisor are required");
    const long long n = (long long)H * W;
    const DecodeU16Args a{src_hwc, dst_f32_hwc3, n, channels, divisor, factor, (channels == 3 && aligned16(src_hwc) && aligned16(dst_f32_hwc3)) ? 1 : 0};
    launch_k(decode_u16_kernel, dim3((unsigned)(((n + 3) / 4 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    R2F_HIP(ctx, take_launch_status());
    return R2F_OK;
}

// ------------------------------------------------------------------------------- auto exposure on the device
static bool exposure_root_ok(double root) { return root >= 1.0 && root <= 1.0e6; }  // (calc_exposure's is sqrt(...) + 1; NaN fails)

int r2f_exposure_rows(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int H, int W, int channels, int y0, int y1,
                      double root, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (!src_rows || H <= 0 || W <= 0 || (channels != 3 && channels != 4) || !exposure_root_ok(root))
        return fail(ctx, R2F_EINVAL, "exposure_rows: a non-empty 3- or 4-channel frame and a root in [1, 1e6] are required");
    if (y0 < 0 || y1 > H || y0 > y1 || src_gy0 < 0 || src_nrows < 0 || y0 < src_gy0 || (long long)y1 > (long long)src_gy0 + src_nrows)
        return fail(ctx, R2F_EINVAL, "exposure_rows: rows [%d, %d) not inside the frame's [0, %d) and the buffer's [%d, %lld)", y0, y1, H,
                    src_gy0, (long long)src_gy0 + src_nrows);
    const int n_rows = (H + 1) / 2;
    if (n_rows > ctx->exposure.rows_cap) {  // a taller frame: the sums of a shorter one are not kept (its finish has been queued)
        int rc = ctx->exposure.sums.reserve(ctx, (size_t)n_rows * sizeof(double), Grow::Sync);
        if (rc) return rc;
        ctx->exposure.rows_cap = n_rows;
    }
    const int y_first = y0 + (y0 & 1), sampled = (y1 - y_first + 1) / 2;  // the even rows of [y0, y1) -> sums[y / 2]
    if (sampled <= 0) return R2F_OK;
    const ExposureRowsArgs a{src_rows, src_gy0, W, channels, y_first, sampled, 1.0 / root, static_cast<double*>(ctx->exposure.sums.p)};
    launch_k(exposure_rows_kernel, dim3((unsigned)sampled), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    R2F_HIP(ctx, take_launch_status());
    return R2F_OK;
}

int r2f_exposure_finish(r2f_ctx* ctx, int H, int W, double root, double ref_exposure, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (H <= 0 || W <= 0 || !exposure_root_ok(root) || !(ref_exposure > 0.0))
        return fail(ctx, R2F_EINVAL, "exposure_finish: a non-empty frame, a root in [1, 1e6] and a positive reference are required");
    auto& ex = ctx->exposure;
    if ((H + 1) / 2 > ex.rows_cap) return fail(ctx, R2F_EINVAL, "exposure_finish: no row sums of a frame of %d rows (r2f_exposure_rows)", H);
    // (each under its own check: one that failed is tried again by the next call, and nothing is used before it exists)
    if (!ex.stream) R2F_HIP(ctx, hipStreamCreateWithFlags(&ex.stream, hipStreamNonBlocking));
    if (!ex.done) R2F_HIP(ctx, hipEventCreateWithFlags(&ex.done, hipEventDisableTiming));
    if (!ex.host) R2F_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&ex.host), sizeof(ExposureRecord), hipHostMallocDefault));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int n_rows = (H + 1) / 2;
    const ExposureFinishArgs a{static_cast<const double*>(ex.sums.p), n_rows, (double)n_rows * (double)((W + 1) / 2), root, ref_exposure,
                               static_cast<ExposureRecord*>(ex.rec.p)};
    launch_k(exposure_finish_kernel, dim3(1), dim3(256), 0, s, a);
    R2F_HIP(ctx, take_launch_status());
    R2F_HIP(ctx, hipEventRecord(ex.done, s));
    R2F_HIP(ctx, hipStreamWaitEvent(ex.stream, ex.done, 0));
    R2F_HIP(ctx, hipMemcpyAsync(ex.host, ex.rec.p, sizeof(ExposureRecord), hipMemcpyDeviceToHost, ex.stream));
    ex.measured = true;
    return R2F_OK;
}

int r2f_decode_u16_auto(r2f_ctx* ctx, const uint16_t* src_hwc, int H, int W, int channels, int64_t src_pitch, float divisor,
                        float* dst_f32_hwc3, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (!src_hwc || !dst_f32_hwc3 || H <= 0 || W <= 0 || (channels != 3 && channels != 4) || !(divisor > 0.f) || src_pitch < W)
        return fail(ctx, R2F_EINVAL, "decode_u16_auto: a non-empty 3- or 4-channel frame, a pitch of at least W pixels and a positive "
                                     "divisor are required");
    if (!ctx->exposure.measured) return fail(ctx, R2F_EINVAL, "decode_u16_auto: no exposure has been measured (r2f_exposure_finish)");
    DecodeU16AutoArgs a{src_hwc, dst_f32_hwc3, W, src_pitch, H, channels, 0u, divisor, static_cast<const ExposureRecord*>(ctx->exposure.rec.p), 0};
    if (src_pitch == W) a.W = a.src_pitch = (long long)H * W, a.H = 1;  // contiguous rows: one long row, like decode_u16_kernel
    const bool rows_ok = a.H == 1 || (a.W % 4 == 0 && a.src_pitch % 4 == 0);
    a.vec = (channels == 3 && rows_ok && (reinterpret_cast<uintptr_t>(src_hwc) & 7u) == 0 && aligned16(dst_f32_hwc3)) ? 1 : 0;
    a.quad_blocks = (unsigned)(((a.W + 3) / 4 + 255) / 256);
    launch_k(decode_u16_auto_kernel, dim3((unsigned)((long long)a.quad_blocks * a.H)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    R2F_HIP(ctx, take_launch_status());
    return R2F_OK;
}

int r2f_exposure_result(r2f_ctx* ctx, double* stops, float* factor) {
    if (!ctx || !stops || !factor) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (!ctx->exposure.measured) return fail(ctx, R2F_EINVAL, "exposure_result: no exposure has been measured (r2f_exposure_finish)");
    R2F_HIP(ctx, hipStreamSynchronize(ctx->exposure.stream));  // (behind the last finish kernel, not behind what was queued after it)
    *stops = ctx->exposure.host->stops;
    *factor = ctx->exposure.host->factor;
    return R2F_OK;
}

int r2f_stream_copy(r2f_ctx* ctx, const void* src, void* dst, size_t bytes, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (!src || !dst || bytes % 16 != 0 || !aligned16(src) || !aligned16(dst))
        return fail(ctx, R2F_EINVAL, "stream_copy: 16-byte aligned buffers and a multiple of 16 bytes are required");
    const long long n = (long long)bytes / 16;
    launch_k(stream_copy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const f4v*>(src),
             static_cast<f4v*>(dst), n);
    R2F_HIP(ctx, take_launch_status());
    return R2F_OK;
}

int r2f_blit_rgba8(r2f_ctx* ctx, const float* src_f32_hwc, int H, int W, uint8_t* dst_rgba, int dst_h, int dst_w, const r2f_blit* t,
                   void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (!src_f32_hwc || !dst_rgba || !t || H <= 0 || W <= 0 || dst_h <= 0 || dst_w <= 0)
        return fail(ctx, R2F_EINVAL, "blit: bad arguments");
    if (reinterpret_cast<uintptr_t>(dst_rgba) & 3u) return fail(ctx, R2F_EINVAL, "blit: the destination must be 4-byte aligned");
    const BlitArgs a{src_f32_hwc, dst_rgba, H, W, dst_h, dst_w, *t};
    R2F_HIP(ctx, launch_64x4(blit_rgba8_kernel, dst_w, dst_h, static_cast<hipStream_t>(stream), a));
    return R2F_OK;
}

int r2f_histogram_render(r2f_ctx* ctx, const uint32_t* counts, const uint8_t* mix_table_rgba, int height, uint8_t* image_rgba,
                         uint8_t* target_rgba, int target_h, int target_w, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (!counts || !mix_table_rgba || !image_rgba || height <= 0 || (target_rgba && (target_h <= 0 || target_w <= 0)))
        return fail(ctx, R2F_EINVAL, "histogram_render: bad arguments");
    if ((reinterpret_cast<uintptr_t>(image_rgba) & 3u) || (reinterpret_cast<uintptr_t>(target_rgba) & 3u))
        return fail(ctx, R2F_EINVAL, "histogram_render: images must be 4-byte aligned");
    HistArgs a;
    a.counts = counts, a.image = image_rgba, a.target = target_rgba, a.height = height, a.th = target_h, a.tw = target_w;
    for (int k = 0; k < 8; ++k) {
        const uint8_t* m = mix_table_rgba + 4 * k;
        a.mix[k] = (uint32_t)m[0] | ((uint32_t)m[1] << 8) | ((uint32_t)m[2] << 16) | ((uint32_t)m[3] << 24);
    }
    launch_k(histogram_render_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    R2F_HIP(ctx, take_launch_status());
    return R2F_OK;
}

static int chroma_weights(r2f_ctx* ctx, int size, ChromaArgs& a) {
    static_assert(kChromaMaxTaps == plan::kChromaMaxTaps, "one tap limit");
    if (!plan::chroma_weights(size, a.w)) return fail(ctx, R2F_EINVAL, "chroma_nr size must be in [1, %d]", (kChromaMaxTaps - 1) / 2);
    a.radius = size;
    return R2F_OK;
}

int r2f_stage_chroma_nr_h(r2f_ctx* ctx, const void* in, int in_layout, int in_gy0, int in_rows, const r2f_planes* dst, int size,
                          int y0, int y1, int W, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (y1 <= y0) return R2F_OK;
    if (!in || W <= 0 || y0 < in_gy0 || y1 > in_gy0 + in_rows || in_layout < 0 || in_layout > 2)
        return fail(ctx, R2F_EINVAL, "chroma_nr: bad input geometry");
    ChromaArgs a;
    memset(&a, 0, sizeof a);
    int rc = chroma_weights(ctx, size, a);
    if (rc) return rc;
    rc = check_rows(ctx, "chroma_nr dst", dst, y0, y1);
    if (rc) return rc;
    a.in = in;
    a.in_layout = in_layout;
    a.in_gy0 = in_gy0;
    a.in_rows = in_rows;
    a.dst = to_dev(dst);
    a.y0 = y0;
    a.y1 = y1;
    a.W = W;
    a.H_global = in_gy0 + in_rows;
    a.vec = planes_vec_ok(dst, W) ? 1 : 0;
    launch_k(chroma_h_kernel, dim3((W + kChromaSeg - 1) / kChromaSeg, y1 - y0), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    R2F_HIP(ctx, take_launch_status());
    return R2F_OK;
}

int r2f_stage_chroma_nr_v(r2f_ctx* ctx, const r2f_planes* src, const r2f_planes* dst, int size, int y0, int y1, int W,
                          int H_global, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (y1 <= y0) return R2F_OK;
    if (W <= 0 || y0 < 0 || y1 > H_global) return fail(ctx, R2F_EINVAL, "chroma_nr: bad geometry");
    ChromaArgs a;
    memset(&a, 0, sizeof a);
    int rc = chroma_weights(ctx, size, a);
    if (rc) return rc;
    rc = check_rows(ctx, "chroma_nr dst", dst, y0, y1);
    if (rc) return rc;
    rc = check_rows(ctx, "chroma_nr src", src, std::max(y0 - size, 0), std::min(y1 + size, H_global));
    if (rc) return rc;
    if (planes_overlap(src, dst, W)) return fail(ctx, R2F_EINVAL, "chroma_nr: source and destination planes overlap (out of place only)");
    a.src = to_dev(src);
    a.dst = to_dev(dst);
    a.y0 = y0;
    a.y1 = y1;
    a.W = W;
    a.H_global = H_global;
    a.vec = (planes_vec_ok(src, W) && planes_vec_ok(dst, W)) ? 1 : 0;
    R2F_HIP(ctx, launch_64x4(chroma_v_kernel, (W + 3) / 4, y1 - y0, static_cast<hipStream_t>(stream), a));
    return R2F_OK;
}

int r2f_histogram_u8(r2f_ctx* ctx, const uint8_t* image_hwc, int H, int W, uint32_t* counts, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (!counts || H < 0 || W < 0 || (!image_hwc && H > 0 && W > 0)) return fail(ctx, R2F_EINVAL, "histogram: bad arguments");
    if (!aligned16(image_hwc)) return fail(ctx, R2F_EINVAL, "histogram: image must be 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long n_bytes = (long long)H * W * 3, per_block = (long long)kHistThreads * kHistBytesPerLane * kHistIters;
    R2F_HIP(ctx, hipMemsetAsync(counts, 0, 768 * sizeof(uint32_t), s));  // counts[3][256] is zeroed first
    if (n_bytes <= 0) return R2F_OK;
    launch_k(histogram_u8_kernel, dim3((unsigned)((n_bytes + per_block - 1) / per_block)), dim3(kHistThreads), 0, s, image_hwc, n_bytes, counts);
    R2F_HIP(ctx, take_launch_status());
    return R2F_OK;
}

}  // extern "C"
