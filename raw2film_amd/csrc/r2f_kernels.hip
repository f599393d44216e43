// r2f_kernels.hip -- gfx950 kernels of the film-emulation render path and their launchers; nothing here runs off the path (the
// resamplers are in r2f_resample.hip, the lens step in r2f_lens.hip, the hand-off, chroma NR, blit and histograms in r2f_post.hip).
//
// Kernel inventory (pass graph mirrors gpu_processor.py:1763-1862, fused where it is free):
//   front_kernel      S0 3x3 + S1 2-D LUT [+ S3 log + S4 curve [+ S8 3-D LUT + S9 u8]]        HBM-bound
//   stencil_kernel    S2 halation (+S3+S4 epilogue) / S5 MTF: LDS-tiled direct stencil         fp32-VALU-bound
//   single_tap_kernel a stencil channel of one tap (the halation's identity plane)             HBM-bound
//   tail_kernel       S6 hash noise -> LDS, grain stencil, grain LUT, clip [, S8, S9]          VALU/LDS
//   lut3d_kernel      [S7 burn subtract +] S8 + S9 from density planes                         HBM-bound
//   burn_sums/_map    S7: INTER_AREA cell sums of the green density; clip + Gaussian on the map
//   noise_kernel      S6a test entry (hash + Gaussian field)
//   frame_params / exposure_range   the per-render frame block and the exposure-range record
#include <algorithm>
#include <array>
#include <utility>

#include "r2f_launch.h"

#include "../../include/r2f.h"

#ifndef R2F_CURVE_BATCH3
#define R2F_CURVE_BATCH3 1  // A/B switch: a pixel's three curve evaluations as one batch (see front_kernel)
#endif

namespace r2f {

constexpr StencilVariant kStencilVariants[kNumStencilVariants] = {  // (constexpr here: the generic stencil table below is built from it)
    {0, 32, 16, 4},  // 512 threads, tile 128 x 64, 4x4 outputs per lane
    {1, 16, 8, 4},   // 128 threads, tile 64 x 32: fallback for very wide stencils
    {2, 32, 8, 4},   // 256 threads, tile 128 x 32: never auto-selected first; occupancy experiments (2 waves per SIMD)
};

// ------------------------------------------------------------------------------ output
__device__ __forceinline__ uint32_t to_u8(float v) {
    // cpu_processor.py:407: (image * 255).astype(uint8) -- truncation
    float s = fminf(fmaxf(v * 255.0f, 0.0f), 255.0f);
    return (uint32_t)s;
}

__device__ __forceinline__ uint32_t to_u16(float v) {
    // cpu_processor.py:407 with 2 ** 16 - 1 in place of 255: (image * 65535).astype(uint16) -- truncation, from the same float
    float s = fminf(fmaxf(v * 65535.0f, 0.0f), 65535.0f);
    return (uint32_t)s;
}

// Four pixels (twelve samples, 24 bytes) of a uint16 row at `o`.  A pixel is 6 bytes and a row 6 W, so `o` is only 2-byte aligned
// when W is odd; a lane's segments lie 24 bytes apart, so (address & 7) is the same for every lane of a ROW.  A wave of the
// pointwise kernels (64 lanes along x) therefore takes ONE of the four shapes below.  A wave of tail_kernel spans four rows (16
// lanes each): when 6 W is no multiple of 8 (W no multiple of 4) its rows differ in phase and the wave runs through up to four
// shapes one after the other, each with a quarter of its lanes -- every shape covers the same 24 bytes, so only time is at stake
// (profiles/r11_output16_probe.txt, W against W - 2).  8-byte stores where the address allows them (the 16-byte phase alternates
// from lane to lane -- a 16-byte store would split every wave in two), a 4-byte and a 2-byte store at the ends.  Plain vector stores.
__device__ __forceinline__ void store_u16x12(uint16_t* o, const uint32_t (&h)[12]) {
    const uint32_t phase = (uint32_t)(reinterpret_cast<uintptr_t>(o) & 7u);
    if ((phase & 2u) == 0) {
        uint32_t w[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) w[i] = h[2 * i] | (h[2 * i + 1] << 16);
        uint32_t* d = reinterpret_cast<uint32_t*>(o);
        if (phase == 0) {
            *reinterpret_cast<uint2*>(d) = make_uint2(w[0], w[1]);
            *reinterpret_cast<uint2*>(d + 2) = make_uint2(w[2], w[3]);
            *reinterpret_cast<uint2*>(d + 4) = make_uint2(w[4], w[5]);
        } else {  // 4
            d[0] = w[0];
            *reinterpret_cast<uint2*>(d + 1) = make_uint2(w[1], w[2]);
            *reinterpret_cast<uint2*>(d + 3) = make_uint2(w[3], w[4]);
            d[5] = w[5];
        }
    } else {
        uint32_t w[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) w[i] = h[2 * i + 1] | (h[2 * i + 2] << 16);
        o[0] = (uint16_t)h[0];
        uint32_t* d = reinterpret_cast<uint32_t*>(o + 1);
        if (phase == 6) {  // o + 1 is 8-byte aligned
            *reinterpret_cast<uint2*>(d) = make_uint2(w[0], w[1]);
            *reinterpret_cast<uint2*>(d + 2) = make_uint2(w[2], w[3]);
            d[4] = w[4];
        } else {  // 2: o + 1 is 4-byte aligned, o + 3 8-byte
            d[0] = w[0];
            *reinterpret_cast<uint2*>(d + 1) = make_uint2(w[1], w[2]);
            *reinterpret_cast<uint2*>(d + 3) = make_uint2(w[3], w[4]);
        }
        o[11] = (uint16_t)h[11];
    }
}

// Write `nv` (1..4) consecutive pixels of global row `gy` starting at column x, interleaved HWC.
__device__ __forceinline__ void emit_hwc(const HwcOut& out, int gy, int x, int W, int nv, bool vec, const float (&r)[4],
                                         const float (&g)[4], const float (&b)[4]) {
    const long long base = ((long long)(gy - out.gy0) * W + x) * 3;
    if (out.u16) {  // (2-byte aligned is all it asks: the shape is chosen per row segment, whatever `vec` says about the others)
        uint16_t* o = out.u16 + base;
        if (nv == 4) {
            uint32_t h[12];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                h[3 * p + 0] = to_u16(r[p]);
                h[3 * p + 1] = to_u16(g[p]);
                h[3 * p + 2] = to_u16(b[p]);
            }
            store_u16x12(o, h);
        } else {  // the last one to three pixels of a row whose width is no multiple of 4
            for (int p = 0; p < nv; ++p) {
                o[3 * p + 0] = (uint16_t)to_u16(r[p]);
                o[3 * p + 1] = (uint16_t)to_u16(g[p]);
                o[3 * p + 2] = (uint16_t)to_u16(b[p]);
            }
        }
    }
    if (out.f32) {
        float* o = out.f32 + base;
        if (vec && nv == 4) {
            float4* o4 = reinterpret_cast<float4*>(o);
            o4[0] = make_float4(r[0], g[0], b[0], r[1]);
            o4[1] = make_float4(g[1], b[1], r[2], g[2]);
            o4[2] = make_float4(b[2], r[3], g[3], b[3]);
        } else {
            for (int p = 0; p < nv; ++p) {
                o[3 * p + 0] = r[p];
                o[3 * p + 1] = g[p];
                o[3 * p + 2] = b[p];
            }
        }
    }
    if (out.u8) {
        uint8_t* o = out.u8 + base;
        if (vec && nv == 4) {
            uint32_t q[12];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                q[3 * p + 0] = to_u8(r[p]);
                q[3 * p + 1] = to_u8(g[p]);
                q[3 * p + 2] = to_u8(b[p]);
            }
            uint32_t* o32 = reinterpret_cast<uint32_t*>(o);
            o32[0] = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
            o32[1] = q[4] | (q[5] << 8) | (q[6] << 16) | (q[7] << 24);
            o32[2] = q[8] | (q[9] << 8) | (q[10] << 16) | (q[11] << 24);
        } else {
            for (int p = 0; p < nv; ++p) {
                o[3 * p + 0] = (uint8_t)to_u8(r[p]);
                o[3 * p + 1] = (uint8_t)to_u8(g[p]);
                o[3 * p + 2] = (uint8_t)to_u8(b[p]);
            }
        }
    }
}

__device__ __forceinline__ void apply_lut3d(const DevLut3D& L, float scale, int mode, float& r, float& g, float& b) {
    if (mode == 0)
        apply_lut3d_tetra(L, scale * (float)(L.n - 1), r, g, b);
    else
        apply_lut3d_trilinear(L, scale, r, g, b);
}

// ------------------------------------------------------------------------------ front
// One lane = 4 consecutive pixels of one row.  Block (64, BYF); each block walks down the frame in
// steps of gridDim.y * BYF rows.  LDSC: the density curve (3 x (m-1) float4 cells, 48 KB at m = 1024)
// is copied to LDS once per block, so the three data-dependent curve look-ups per pixel are LDS reads
// instead of scattered 16-byte global gathers (which made the fused LUT-only pass gather-bound).
constexpr int kFrontBY = 8;

template <bool LDSC>
__global__ __launch_bounds__(64 * kFrontBY) void front_kernel(const FrontArgs a) {
    extern __shared__ __attribute__((aligned(16))) float4 cells_lds[];
    if (LDSC) {
        const int n = 3 * (a.curve.m - 1);
        for (int i = threadIdx.y * 64 + threadIdx.x; i < n; i += 64 * kFrontBY) cells_lds[i] = a.curve.cells[i];
        __syncthreads();
    }
    const int x = (blockIdx.x * 64 + threadIdx.x) * 4;
    if (x >= a.W) return;
    const int W = a.W;
    const int nv = min(4, W - x);
    const bool vec = a.vec != 0;
    const float* in = static_cast<const float*>(a.in);
    for (int gy = a.y0 + blockIdx.y * kFrontBY + threadIdx.y; gy < a.y1; gy += gridDim.y * kFrontBY) {
        const long long irow = gy - a.in_gy0;
        float r[4], g[4], b[4];
        if (a.in_layout == R2F_LAYOUT_CHW) {
            DevPlanes pl;
            pl.data = const_cast<float*>(in);
            pl.plane_stride = (long long)a.in_rows * W;
            pl.gy0 = a.in_gy0;
            pl.rows = a.in_rows;
            load_planes4(pl, gy, x, W, nv, vec, r, g, b);
        } else if (a.in_layout == R2F_LAYOUT_HWC3) {
            const float* p = in + (irow * W + x) * 3;
            if (vec && nv == 4) {
                const float4* p4 = reinterpret_cast<const float4*>(p);
                const float4 v0 = p4[0], v1 = p4[1], v2 = p4[2];
                r[0] = v0.x; g[0] = v0.y; b[0] = v0.z;
                r[1] = v0.w; g[1] = v1.x; b[1] = v1.y;
                r[2] = v1.z; g[2] = v1.w; b[2] = v2.x;
                r[3] = v2.y; g[3] = v2.z; b[3] = v2.w;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const bool ok = q < nv;
                    r[q] = ok ? p[3 * q + 0] : 0.f;
                    g[q] = ok ? p[3 * q + 1] : 0.f;
                    b[q] = ok ? p[3 * q + 2] : 0.f;
                }
            }
        } else {  // HWC4, alpha ignored (gpu_processor.py:765)
            const float4* p4 = reinterpret_cast<const float4*>(in + (irow * W + x) * 4);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (q < nv) {
                    const float4 v = p4[q];
                    r[q] = v.x; g[q] = v.y; b[q] = v.z;
                } else {
                    r[q] = g[q] = b[q] = 0.f;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (a.use_matrix) apply_matrix(a.mat, r[q], g[q], b[q]);
            apply_lut2d(a.lut2d, r[q], g[q], b[q]);
            if (a.upto >= R2F_UPTO_DENSITY) {
                if (R2F_CURVE_BATCH3) {
                    // the pixel's three evaluations together: three gathers in flight, and the corrective gathers only if some
                    // lane of the wave sits on a breakpoint (curve_eval_batch)
                    float v3[3] = {log10_fast(r[q], a.log_eps), log10_fast(g[q], a.log_eps), log10_fast(b[q], a.log_eps)};
                    if (LDSC)
                        curve_eval_batch<3, 3>((const float4*)cells_lds, a.curve, 0, v3);
                    else
                        curve_eval_batch<3, 3>(a.curve.cells, a.curve, 0, v3);
                    r[q] = v3[0], g[q] = v3[1], b[q] = v3[2];
                } else if (LDSC) {
                    r[q] = curve_eval_at(cells_lds, a.curve, 0, log10_fast(r[q], a.log_eps));
                    g[q] = curve_eval_at(cells_lds, a.curve, 1, log10_fast(g[q], a.log_eps));
                    b[q] = curve_eval_at(cells_lds, a.curve, 2, log10_fast(b[q], a.log_eps));
                } else {
                    r[q] = log_curve(a.curve, 0, r[q], a.log_eps);
                    g[q] = log_curve(a.curve, 1, g[q], a.log_eps);
                    b[q] = log_curve(a.curve, 2, b[q], a.log_eps);
                }
            }
            if (a.upto == R2F_UPTO_OUTPUT) apply_lut3d(a.lut3d, a.lut3d_scale, a.lut3d_mode, r[q], g[q], b[q]);
        }
        if (a.upto == R2F_UPTO_OUTPUT)
            emit_hwc(a.out, gy, x, W, nv, vec, r, g, b);
        else
            store_planes4(a.dst, gy, x, W, nv, vec, r, g, b);
    }
}

// ------------------------------------------------------------------------------ lut3d
struct Lut3dArgs {
    DevPlanes src;
    HwcOut out;
    int y0, y1, W;
    DevLut3D lut3d;
    float lut3d_scale;
    int lut3d_mode;
    int vec;
    BurnUp burn;
    DevPlanes gfield;  // has_gfield: the grain field K_g * noise computed ahead of time (tail_kernel, to_planes = 2)
    int has_gfield;
    DevCurve grain_lut;
};

// S7: the highlight map at pixel (gy, x): ndimage.zoom(map, cell, order=1) = linear interpolation at the
// coordinate o * (in - 1) / (out - 1), evaluated in double like SciPy does, then edge padding to the frame
// (effects.py:381-388).  SciPy's default mode="constant" returns 0 for a coordinate beyond the last sample,
// and o * ((in-1)/(out-1)) can exceed in-1 by one ulp at o = out-1 (e.g. 223 * (31/223) > 31): the reference's
// last zoomed column / row is then 0, and so is the edge padding copied from it.  Reproduced here on purpose.
__device__ __forceinline__ float burn_sample(const BurnUp& bu, int gy, int x) {
    const double cy = (double)min(gy, bu.h_up - 1) * bu.zy, cx = (double)min(x, bu.w_up - 1) * bu.zx;
    if (cy > (double)(bu.h_lo - 1) || cx > (double)(bu.w_lo - 1)) return 0.f;
    const int y0 = (int)cy, x0 = (int)cx;
    const int y1 = min(y0 + 1, bu.h_lo - 1), x1 = min(x0 + 1, bu.w_lo - 1);
    const float ty = (float)(cy - (double)y0), tx = (float)(cx - (double)x0);
    const float a = bu.map[y0 * bu.w_lo + x0], b = bu.map[y0 * bu.w_lo + x1];
    const float c = bu.map[y1 * bu.w_lo + x0], d = bu.map[y1 * bu.w_lo + x1];
    const float top = a + tx * (b - a), bot = c + tx * (d - c);
    return top + ty * (bot - top);
}

__global__ __launch_bounds__(256) void lut3d_kernel(const Lut3dArgs a) {
    const int x = (blockIdx.x * 64 + threadIdx.x) * 4;
    const int gy = a.y0 + blockIdx.y * 4 + threadIdx.y;
    if (x >= a.W || gy >= a.y1) return;
    const int nv = min(4, a.W - x);
    float r[4], g[4], b[4];
    load_planes4(a.src, gy, x, a.W, nv, a.vec != 0, r, g, b);
    if (a.has_gfield) {  // S6c grain.wgsl:78-89 + clip cpu_processor.py:397, with the field from the side stream
        float gr[4], gg[4], gb[4];
        load_planes4(a.gfield, gy, x, a.W, nv, a.vec != 0, gr, gg, gb);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float ar = curve_eval(a.grain_lut, 0, r[q]), ag = curve_eval(a.grain_lut, 1, g[q]), ab = curve_eval(a.grain_lut, 2, b[q]);
            {
                // product and sum rounded separately, like NumPy's image + grain * factor (and like the fused tail kernel): plain
                // operators with contraction off for this block alone (the pragma is lexical: curve_eval keeps its fmaf)
#pragma clang fp contract(off)
                r[q] = fmaxf(r[q] + gr[q] * ar, 0.f);
                g[q] = fmaxf(g[q] + gg[q] * ag, 0.f);
                b[q] = fmaxf(b[q] + gb[q] * ab, 0.f);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (a.burn.map) {  // S7: subtract the up-sampled highlight map from all three channels, clip at 0
            const float v = a.burn.strength * burn_sample(a.burn, gy, x + q);
            r[q] = fmaxf(r[q] - v, 0.f);
            g[q] = fmaxf(g[q] - v, 0.f);
            b[q] = fmaxf(b[q] - v, 0.f);
        }
        apply_lut3d(a.lut3d, a.lut3d_scale, a.lut3d_mode, r[q], g[q], b[q]);
    }
    emit_hwc(a.out, gy, x, a.W, nv, a.vec != 0, r, g, b);
}

// ------------------------------------------------------------------------------ stencil
// XCD-aware block order: consecutive linear ids are dealt round-robin to the 8 XCDs, so give
// each XCD a contiguous run of tiles (neighbouring tiles share halo columns/rows in that L2).
__device__ __forceinline__ int xcd_remap(int id, int nwg) {
    const int xcd = id & 7, q = nwg >> 3, r = nwg & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
}

// Fill rows x RS floats of an LDS tile from a source plane with BORDER_REFLECT_101 on the
// global frame.  Tile element (r, c) <-> global (ty0 + r, tx0 + c).  Columns >= cols_valid are
// zero (they only meet zero padding taps).  One wave per tile row, lanes along x (coalesced);
// each lane first issues all its loads for KR rows, then writes them to LDS, so several global
// round trips are in flight per wave instead of one.
template <int NT>
__device__ __forceinline__ void fill_tile_reflect(float* lds, int RS, int rows, int cols_valid, const float* src,
                                                  int src_gy0, int src_rows, int W, int H_global, int ty0, int tx0) {
    constexpr int NW = NT / 64, KR = 4, KC = 4;
    const int tid = fresh_tid();
    const int wave = tid >> 6, lane = tid & 63;
    for (int cb = 0; cb < RS; cb += 64 * KC) {  // column blocks of 256 (one pass for stencils up to 128 taps wide)
        int sx[KC];
#pragma unroll
        for (int k = 0; k < KC; ++k) sx[k] = reflect101(tx0 + cb + lane + 64 * k, W);
        for (int r0 = wave * KR; r0 < rows; r0 += NW * KR) {
            float v[KR][KC];
#pragma unroll
            for (int i = 0; i < KR; ++i) {
                int sy = reflect101(ty0 + r0 + i, H_global) - src_gy0;
                sy = clampi(sy, 0, src_rows - 1);  // only rows feeding discarded outputs can fall outside
                const float* srow = src + (long long)sy * W;
#pragma unroll
                for (int k = 0; k < KC; ++k) {
                    const int c = cb + lane + 64 * k;
                    v[i][k] = (c < cols_valid && r0 + i < rows) ? srow[sx[k]] : 0.f;
                }
            }
#pragma unroll
            for (int i = 0; i < KR; ++i) {
                if (r0 + i < rows) {
                    float* drow = lds + (r0 + i) * RS;
#pragma unroll
                    for (int k = 0; k < KC; ++k) {
                        const int c = cb + lane + 64 * k;
                        if (c < RS) drow[c] = v[i][k];
                    }
                }
            }
        }
    }
}

// amdgpu_waves_per_eu(4): two 512-thread workgroups per CU (4 waves per SIMD) is the operating point the LDS budget is
// built around, so the register allocator must stay within 128 VGPRs.
// FR > 0: every channel of the launch is a square mirror-symmetric (2 FR + 1)^2 stencil in one LDS phase: the fully unrolled
// stencil_fixed instead of the entry list.
template <int BX, int BY, int Q, int EPI, int FR = 0>
__global__ __launch_bounds__(BX* BY) __attribute__((amdgpu_waves_per_eu(4, 8))) void stencil_kernel(const StencilArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NT = BX * BY, TW = 4 * BX, TH = Q * BY;
    int bx = blockIdx.x, by = blockIdx.y;
    const int ch = a.chan[blockIdx.z];
    if (a.xcd_remap) {
        // remap inside the channel's own 2-D tile grid: channels differ wildly in cost (the blue
        // halation plane is the identity), so a remap across channels would unbalance the XCDs
        const int nwg = gridDim.x * gridDim.y, lin = bx + gridDim.x * by;
        const int id = a.xcd_remap == 2 ? a.order[lin] : xcd_remap(lin, nwg);
        bx = id % gridDim.x;
        by = id / gridDim.x;
    }
    const DevStencil st = a.st[ch];
    const int tile_x0 = bx * TW, tile_y0 = a.y0 + by * TH;
    const int RS = st.RS;
    const float* src = a.src.data + (long long)ch * a.src.plane_stride;
    const int tx = threadIdx.x % BX, ty = threadIdx.x / BX;
    const float* lds_lane = smem + ty * Q * RS + 4 * tx;
    float2v acc[Q / 2][4];
#pragma unroll
    for (int j = 0; j < Q / 2; ++j)
#pragma unroll
        for (int p = 0; p < 4; ++p) acc[j][p] = (float2v){0.f, 0.f};

    if (FR > 0) {
        constexpr int R = FR > 0 ? FR : 1;
        if (a.ablate != 1)
            fill_tile_reflect<NT>(smem, RS, TH + 2 * R, TW + st.kw - 1, src, a.src.gy0, a.src.rows, a.W, a.H_global, tile_y0 - st.ay,
                                  tile_x0 - st.ax);
        __syncthreads();
        if (a.ablate != 2)
            stencil_fixed<R, Q>(lds_lane, RS, (const float2v R2F_CONSTANT*)a.fixed_w + ch * (2 * R + Q) * (R + 1) * (Q / 2), acc);
    }
    const int R2F_CONSTANT* phases = (const int R2F_CONSTANT*)st.phases;
    for (int ph = 0; ph < (FR > 0 ? 0 : st.n_phases); ++ph) {
        const int m0 = phases[4 * ph], lds_rows = phases[4 * ph + 1];
        const int row_begin = phases[4 * ph + 2], e0 = phases[4 * ph + 3];
        const int row_end = phases[4 * ph + 6];
        if (ph > 0) __syncthreads();  // all lanes are done reading the previous phase's rows
        if (a.ablate != 1)
            fill_tile_reflect<NT>(smem, RS, lds_rows, TW + st.kw - 1, src, a.src.gy0, a.src.rows, a.W, a.H_global,
                                  tile_y0 - st.ay + m0, tile_x0 - st.ax);
        __syncthreads();
        if (a.ablate != 2) {
            if (st.sym)  // per channel, wave-uniform
                stencil_accumulate_sym<Q, true>(lds_lane, st, row_begin, row_end, e0, acc);
            else
                stencil_accumulate<Q>(lds_lane, st, row_begin, row_end, e0, acc);
        }
    }

    const int tid_out = fresh_tid();  // (the output coordinates are made here, not carried through the loops above)
    const int gx = tile_x0 + 4 * (tid_out % BX);
    if (gx >= a.W) return;
    const int nv = min(4, a.W - gx);
    float* dplane = a.dst.data + (long long)ch * a.dst.plane_stride;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int gy = tile_y0 + (tid_out / BX) * Q + q;
        if (gy >= a.y1) break;
        float v[4] = {acc[q / 2][0][q & 1], acc[q / 2][1][q & 1], acc[q / 2][2][q & 1], acc[q / 2][3][q & 1]};
        if (EPI == 1) {
#pragma unroll
            for (int p = 0; p < 4; ++p) v[p] = log10_fast(v[p], a.log_eps);
            curve_eval_batch<4, 1>(a.curve.cells, a.curve, ch, v);
        }
        float* d = dplane + (long long)(gy - a.dst.gy0) * a.W + gx;
        if (a.vec && nv == 4) {
            *reinterpret_cast<float4*>(d) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            for (int p = 0; p < nv; ++p) d[p] = v[p];
        }
    }
}

// ------------------------------------------------------------------------------ single-tap stencil channel
// The blue plane of the colour-stock halation is the identity (effects.py:248-263: f_b = 0): one tap of weight 1 at the
// anchor.  Pointwise, 4 B + 4 B per pixel, instead of the tiled kernel's LDS round trip.
__global__ __launch_bounds__(256) void single_tap_kernel(const TapArgs a) {
    const int gy = a.y0 + blockIdx.y;
    const int x = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (x >= a.W) return;
    const float* s = a.src.data + (long long)a.ch * a.src.plane_stride + (long long)(gy - a.src.gy0) * a.W + x;
    float* d = a.dst.data + (long long)a.ch * a.dst.plane_stride + (long long)(gy - a.dst.gy0) * a.W + x;
    const int nv = min(4, a.W - x);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.vec && nv == 4) {
        const float4 t = *reinterpret_cast<const float4*>(s);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
        for (int p = 0; p < nv; ++p) v[p] = s[p];
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) v[p] = a.w * v[p];
    if (a.epilogue == 1) {
#pragma unroll
        for (int p = 0; p < 4; ++p) v[p] = log10_fast(v[p], a.log_eps);
        curve_eval_batch<4, 1>(a.curve.cells, a.curve, a.ch, v);
    }
    if (a.vec && nv == 4) {
        *reinterpret_cast<float4*>(d) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int p = 0; p < nv; ++p) d[p] = v[p];
    }
}

// ------------------------------------------------------------------------------ tail (grain)
// FR > 0: the fully unrolled (2 FR + 1)^2 grain stencil (stencil_fixed: square mirror-symmetric kernels up to 19 x 19);
// FR = 0: the generic entry list, every tap column of every entry (run-time masks, i.e. branches, cost more than the
// padding columns they skip in a stencil of two entries per row step).
// SEP (with FR = R > 0): every channel's grain stencil is separable, K = u v^T to fp32 rounding (checked on the host; any
// Gaussian-like kernel is): the noise is filtered along x, then along y out of LDS -- 2 (2 R + 1) taps per pixel instead of
// (2 R + 1)^2.  The pass along x takes one of two forms, which sum the same taps in the same order and so give the same bits:
//   in registers (XREG; R <= kTailXRegMaxR): a lane hashes the four samples of one 4-column segment, takes the R samples on
//     either side from the lanes next to it (DPP wave shifts, no LDS) and stores the FILTERED segment: planes of TH + 2 R rows x TW
//     columns, one barrier;
//   in LDS, in place (R > kTailXRegMaxR, or the option grain_xpass_lds): every thread hashes single samples into planes of
//     pitch RS, barrier, reads the inputs of its row segments, barrier, stores, barrier.
static_assert(kTailXRegMaxR <= 4, "a segment's taps must reach no further than the segment on either side");

// neighbouring lanes' values inside a wave: lane l takes lane l - 1's (from_left) or lane l + 1's; lanes 0 / 63 get 0
__device__ __forceinline__ float wave_from_left(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, true));
}
__device__ __forceinline__ float wave_from_right(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x130 /* wave_shl:1 */, 0xf, 0xf, true));
}

template <int FR, bool SEP = false, bool XREG = false>
__global__ __launch_bounds__(kTailBX* kTailBY) void tail_kernel(const TailArgs a) {
    static_assert(!XREG || (SEP && FR >= 1 && FR <= kTailXRegMaxR), "the pass along x in registers: separable stencils of R <= 4");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NT = kTailBX * kTailBY, TW = 4 * kTailBX, TH = kTailQ * kTailBY, Q = kTailQ;
    const int tile_x0 = blockIdx.x * TW, tile_y0 = a.y0 + blockIdx.y * TH;
    const DevStencil g0 = a.gk[0];
    const int RS = XREG ? TW : g0.RS;  // (TW: a lane's two rows of the pass along y then start 2 x 64 banks apart, conflict free)
    const int rows = TH + g0.kh - 1;
    // + slack: the prefetch of the dummy entry reads past the last row (the register form holds output columns only, and no slack)
    const int plane_sz = XREG ? (TH + 2 * FR) * TW : rows * RS + 16;
    const int cols_valid = TW + g0.kw - 1;
    const bool mono = a.mono != 0;
    const uint32_t seed = a.frame->seed;  // wave-uniform: one scalar load
    // The lane's own density samples (2 rows x 4 pixels x 3 planes) are requested NOW: the kernel's only reads from HBM then
    // travel while the noise is hashed and filtered, instead of starting after it (by ablation the 0.44 ms of memory time
    // used to add to the 0.7 ms of compute; neither the compiler nor the hardware moves a load across the barriers below).
    const int ptx = threadIdx.x % kTailBX, pty = threadIdx.x / kTailBX;
    const int pgx = tile_x0 + 4 * ptx;
    float pre_r[Q][4], pre_g[Q][4], pre_b[Q][4];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int gy = tile_y0 + pty * Q + q;
#pragma unroll
        for (int p = 0; p < 4; ++p) pre_r[q][p] = pre_g[q][p] = pre_b[q][p] = 0.f;
        if (a.to_planes != 2 && pgx < a.W && gy < a.y1) load_planes4<true>(a.src, gy, pgx, a.W, min(4, a.W - pgx), a.vec != 0, pre_r[q], pre_g[q], pre_b[q]);
    }
#ifndef R2F_TAIL_LUT_BATCH
#define R2F_TAIL_LUT_BATCH 2  // pixels of a lane whose 3-D LUT gathers are in flight together (1, 2 or 4)
#endif
#ifndef R2F_TAIL_EXP
#define R2F_TAIL_EXP 0  // development switch (tools/ablate_stencil.py): bit 0 no noise generation, 1 no grain stencil, 2 no LUTs
#endif
    // S6a: hash noise for the tile + halo, straight into LDS.  Coordinates are clamped to the
    // frame like the shader's texture reads (grain.wgsl:63-75); the hash sees GLOBAL coordinates.
    // (row, column) of element idx advance with it: one division per thread, not one per element
    // Only the cols_valid columns that taps can reach are hashed (the padding columns up to RS are zeroed below): every lane
    // of a wave then does a hash, instead of the lanes that fall on padding idling through it.
    if constexpr (XREG) {
        // S6a + the pass along x in one.  The 4-column segments of the tile and its halo, s = -1 .. TW / 4 of rows 0 .. TH + 2 R - 1, are
        // numbered row by row; a wave step takes 64 consecutive ones, so that segment e's neighbours e -+ 1 sit in lanes -+ 1.  Lanes 0
        // and 63 have only one neighbour: they hash (for the lane beside them) and store nothing, and the next step starts on lane
        // 63's segment again -- 62 segments of a step are new, about 4 % more hashes than samples.  Every lane of a wave runs every
        // hash and every shift (a DPP read of an idle lane returns nothing): numbers past the ends are clamped, never branched on.
        constexpr int R = FR > 0 ? FR : 1, SEGS = TW / 4 + 2, TOTAL = (TH + 2 * R) * SEGS, OWN = 62;
        constexpr int STEPS = (TOTAL + OWN - 1) / OWN, NWAVES = NT / 64, MAXI = (STEPS + NWAVES - 1) / NWAVES;
        static_assert(NT % 64 == 0 && TW % 4 == 0, "whole waves, whole segments");
        const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
#pragma unroll
        for (int i = 0; i < ((R2F_TAIL_EXP & 1) ? 0 : MAXI); ++i) {
            const int k = wave + NWAVES * i;  // wave-uniform
            if (k >= STEPS) break;
            const int e_raw = OWN * k + lane - 1, e = clampi(e_raw, 0, TOTAL - 1);
            const int rr = e / SEGS, s = e - rr * SEGS - 1;
            const int sy = clampi(tile_y0 - g0.ay + rr, 0, a.H_global - 1);
            float n[3][4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int sx = clampi(tile_x0 + 4 * s + p, 0, a.W - 1);
                gaussian_noise((uint32_t)sx, (uint32_t)sy, seed, mono, n[0][p], n[1][p], n[2][p]);
            }
            const bool owner = lane >= 1 && lane <= OWN && e_raw < TOTAL && s >= 0 && s < TW / 4;
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                if (pl > 0 && mono) break;
                const float* wv = a.sep_v[pl];  // compile-time plane index: the taps stay in SGPRs
                float x[12];  // columns 4 s - 4 .. 4 s + 7; only 4 - R .. 7 + R are used
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    x[j] = j >= 4 - R ? wave_from_left(n[pl][j]) : 0.f;
                    x[4 + j] = n[pl][j];
                    x[8 + j] = j < R ? wave_from_right(n[pl][j]) : 0.f;
                }
                float o[4];
#pragma unroll
                for (int pp = 0; pp < 4; ++pp) {  // mirrored taps summed first (v is symmetric), outer taps to the centre
                    float acc = wv[0] * (x[4 - R + pp] + x[4 - R + pp + 2 * R]);
#pragma unroll
                    for (int j = 1; j < R; ++j) acc = fmaf(wv[j], x[4 - R + pp + j] + x[4 - R + pp + 2 * R - j], acc);
                    o[pp] = fmaf(wv[R], x[4 + pp], acc);
                }
                if (owner) *reinterpret_cast<float4v*>(smem + pl * plane_sz + rr * TW + 4 * s) = (float4v){o[0], o[1], o[2], o[3]};
            }
        }
    }
    const int step_r = NT / cols_valid, step_c = NT - step_r * cols_valid;
    int r = (int)threadIdx.x / cols_valid, c = (int)threadIdx.x - r * cols_valid;
    for (int idx = threadIdx.x; idx < ((XREG || (R2F_TAIL_EXP & 1)) ? 0 : rows * cols_valid); idx += NT, r += step_r, c += step_c) {
        if (c >= cols_valid) c -= cols_valid, ++r;
        float nr, ng, nb;
        const int sx = clampi(tile_x0 - g0.ax + c, 0, a.W - 1);
        const int sy = clampi(tile_y0 - g0.ay + r, 0, a.H_global - 1);
        gaussian_noise((uint32_t)sx, (uint32_t)sy, seed, mono, nr, ng, nb);
        const int at = r * RS + c;
        smem[at] = nr;
        if (!mono) {
            smem[plane_sz + at] = ng;
            smem[2 * plane_sz + at] = nb;
        }
    }
    if constexpr (!XREG) {  // (the register form stores every float of its planes, and nothing reads past them)
        const int padc = RS - cols_valid;  // < 16
        for (int idx = threadIdx.x; idx < rows * padc; idx += NT) {
            const int rr = idx / padc, at = rr * RS + cols_valid + (idx - rr * padc);
            smem[at] = 0.f;
            if (!mono) smem[plane_sz + at] = 0.f, smem[2 * plane_sz + at] = 0.f;
        }
        if (threadIdx.x < 16) {  // the slack past the last row (prefetch target of the generic entry list)
            smem[rows * RS + threadIdx.x] = 0.f;
            if (!mono) smem[plane_sz + rows * RS + threadIdx.x] = 0.f, smem[2 * plane_sz + rows * RS + threadIdx.x] = 0.f;
        }
    }
    // the grain LUT's cells next to the noise planes: 24 gathers per lane hit LDS instead of the vector L1
    const float4* gcells = a.grain_lut.cells;
    float4* cells_lds = reinterpret_cast<float4*>(smem + a.cells_off);
    if (a.cells_in_lds)
        for (int i = threadIdx.x; i < 3 * (a.grain_lut.m - 1); i += NT) cells_lds[i] = gcells[i];
    __syncthreads();

    const int tx = threadIdx.x % kTailBX, ty = threadIdx.x / kTailBX;
    float2v G[3][Q / 2][4];
    if (SEP && FR > 0) {
        // ---- pass along x, in place.  LDS column of image column tile_x0 + x is x + AX; segment s = 4 output columns
        // 4 s .. 4 s + 3 of one row of one plane; its result goes to columns 4 s .. of that row (16-byte aligned).
        constexpr int R = FR > 0 ? FR : 1, AX = fixed_stencil_ax(R), O = AX - R, NB = (O + 2 * R + 4 + 3) / 4;
        constexpr int SEGS = TW / 4, PER = (TH + 2 * R) * SEGS, MAXI = (PER + NT - 1) / NT;
        if constexpr (!XREG) {  // (the register form stored filtered rows)
            float4v held[3][MAXI];
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                if (pl > 0 && mono) break;
                const float* wv = a.sep_v[pl];  // compile-time plane index: the taps stay in SGPRs
#pragma unroll
                for (int i = 0; i < MAXI; ++i) {
                    const int rem = (int)threadIdx.x + NT * i;
                    held[pl][i] = (float4v){0.f, 0.f, 0.f, 0.f};
                    if (rem < PER) {
                        const int rr = rem / SEGS, sg = rem - rr * SEGS;
                        const float* src = smem + pl * plane_sz + rr * RS + 4 * sg;
                        float x[4 * NB];
#pragma unroll
                        for (int b = 0; b < NB; ++b) {
                            const float4v v = *reinterpret_cast<const float4v*>(src + 4 * b);
                            x[4 * b] = v.x, x[4 * b + 1] = v.y, x[4 * b + 2] = v.z, x[4 * b + 3] = v.w;
                        }
                        float o[4];
#pragma unroll
                        for (int pp = 0; pp < 4; ++pp) {  // mirrored taps summed first (v is symmetric), outer taps to the centre
                            float acc = wv[0] * (x[O + pp] + x[O + pp + 2 * R]);
#pragma unroll
                            for (int j = 1; j < R; ++j) acc = fmaf(wv[j], x[O + pp + j] + x[O + pp + 2 * R - j], acc);
                            o[pp] = fmaf(wv[R], x[O + pp + R], acc);
                        }
                        held[pl][i] = (float4v){o[0], o[1], o[2], o[3]};
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                if (pl > 0 && mono) break;
#pragma unroll
                for (int i = 0; i < MAXI; ++i) {
                    const int rem = (int)threadIdx.x + NT * i;
                    if (rem < PER) {
                        const int rr = rem / SEGS, sg = rem - rr * SEGS;
                        *reinterpret_cast<float4v*>(smem + pl * plane_sz + rr * RS + 4 * sg) = held[pl][i];
                    }
                }
            }
            __syncthreads();
        }
        // ---- pass along y: output row y of the tile reads rows y .. y + 2 R of the filtered plane
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c > 0 && mono && a.fixed_same) {
#pragma unroll
                for (int p = 0; p < 4; ++p) G[c][0][p] = G[0][0][p];
                continue;
            }
            const float* plane = smem + (mono ? 0 : c * plane_sz) + ty * Q * RS + 4 * tx;
            const float* wu = a.sep_u[c];
            static_assert(Q == 2, "the separable grain pass packs the lane's two output rows");
#pragma unroll
            for (int p = 0; p < 4; ++p) G[c][0][p] = (float2v){0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 2 * R + Q; ++i) {
                const float4v h = *reinterpret_cast<const float4v*>(plane + i * RS);
                const float2v w = {i <= 2 * R ? wu[i] : 0.f, i >= 1 ? wu[i - 1] : 0.f};  // (row 0's tap, row 1's tap)
                G[c][0][0] = __builtin_elementwise_fma(w, (float2v){h.x, h.x}, G[c][0][0]);
                G[c][0][1] = __builtin_elementwise_fma(w, (float2v){h.y, h.y}, G[c][0][1]);
                G[c][0][2] = __builtin_elementwise_fma(w, (float2v){h.z, h.z}, G[c][0][2]);
                G[c][0][3] = __builtin_elementwise_fma(w, (float2v){h.w, h.w}, G[c][0][3]);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < ((SEP && FR > 0) ? 0 : 3); ++c) {
#pragma unroll
        for (int j = 0; j < Q / 2; ++j)
#pragma unroll
            for (int p = 0; p < 4; ++p) G[c][j][p] = (float2v){0.f, 0.f};
        const float* plane = smem + (mono ? 0 : c * plane_sz);
        if (R2F_TAIL_EXP & 2) continue;
        if (FR > 0) {

            if (c > 0 && mono && a.fixed_same) {  // one noise plane, one set of taps: the field of channel 0
#pragma unroll
                for (int p = 0; p < 4; ++p) G[c][0][p] = G[0][0][p];
            } else {
                constexpr int R = FR > 0 ? FR : 1;
                stencil_fixed<R, Q>(plane + ty * Q * RS + 4 * tx, RS,
                                    (const float2v R2F_CONSTANT*)a.fixed_w + c * (2 * R + Q) * (R + 1) * (Q / 2), G[c]);
            }
            continue;
        }
        if (a.gk[c].sym)
            stencil_accumulate_sym<Q, false>(plane + ty * Q * RS + 4 * tx, a.gk[c], 0, a.gk[c].n_rowsteps, 0, G[c]);
        else
            stencil_accumulate<Q>(plane + ty * Q * RS + 4 * tx, a.gk[c], 0, a.gk[c].n_rowsteps, 0, G[c]);
    }

    const int gx = tile_x0 + 4 * tx;
    if (gx >= a.W) return;
    const int nv = min(4, a.W - gx);
    const bool vec = a.vec != 0;
    const bool tetra_nonneg = a.lut3d_mode == 0 && a.lut3d.n >= 2 && a.lut3d.n <= 512;
    const float s3 = a.lut3d_scale * (float)(a.lut3d.n - 1);
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int gy = tile_y0 + ty * Q + q;
        if (gy >= a.y1) break;
        float r[4], g[4], b[4];
        if (a.to_planes == 2) {  // the field itself: nothing of the image is read
#pragma unroll
            for (int p = 0; p < 4; ++p) r[p] = G[0][q / 2][p][q & 1], g[p] = G[1][q / 2][p][q & 1], b[p] = G[2][q / 2][p][q & 1];
            store_planes4(a.dst, gy, gx, a.W, nv, vec, r, g, b);
            continue;
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) r[p] = pre_r[q][p], g[p] = pre_g[q][p], b[p] = pre_b[q][p];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            // S6c grain.wgsl:78-89 + clip cpu_processor.py:397
            float ar, ag, ab;
            if (R2F_CURVE_BATCH3) {
                float v3[3] = {r[p], g[p], b[p]};
                if (a.cells_in_lds)
                    curve_eval_batch<3, 3>((const float4*)cells_lds, a.grain_lut, 0, v3);
                else
                    curve_eval_batch<3, 3>(gcells, a.grain_lut, 0, v3);
                ar = v3[0], ag = v3[1], ab = v3[2];
            } else if (a.cells_in_lds) {
                ar = curve_eval_at((const float4*)cells_lds, a.grain_lut, 0, r[p]);
                ag = curve_eval_at((const float4*)cells_lds, a.grain_lut, 1, g[p]);
                ab = curve_eval_at((const float4*)cells_lds, a.grain_lut, 2, b[p]);
            } else {
                ar = curve_eval(a.grain_lut, 0, r[p]);
                ag = curve_eval(a.grain_lut, 1, g[p]);
                ab = curve_eval(a.grain_lut, 2, b[p]);
            }
            {
                // product and sum rounded separately, like NumPy's image + grain * factor: plain operators with contraction off
                // for this block alone
#pragma clang fp contract(off)
                r[p] = fmaxf(r[p] + G[0][q / 2][p][q & 1] * ar, 0.f);
                g[p] = fmaxf(g[p] + G[1][q / 2][p][q & 1] * ag, 0.f);
                b[p] = fmaxf(b[p] + G[2][q / 2][p][q & 1] * ab, 0.f);
            }
            if (!a.to_planes && !(R2F_TAIL_EXP & 4)) {
                if (!tetra_nonneg)
                    apply_lut3d(a.lut3d, a.lut3d_scale, a.lut3d_mode, r[p], g[p], b[p]);
                else if (R2F_TAIL_LUT_BATCH == 1)  // the clip above made every input >= 0
                    apply_lut3d_tetra_nonneg(a.lut3d, s3, r[p], g[p], b[p]);
                else if ((p + 1) % R2F_TAIL_LUT_BATCH == 0) {
                    constexpr int NB = R2F_TAIL_LUT_BATCH;
                    float rn[NB], gn[NB], bn[NB];
#pragma unroll
                    for (int k = 0; k < NB; ++k) rn[k] = r[p + 1 - NB + k], gn[k] = g[p + 1 - NB + k], bn[k] = b[p + 1 - NB + k];
                    apply_lut3d_tetra_nonneg_batch<NB>(a.lut3d, s3, rn, gn, bn);
#pragma unroll
                    for (int k = 0; k < NB; ++k) r[p + 1 - NB + k] = rn[k], g[p + 1 - NB + k] = gn[k], b[p + 1 - NB + k] = bn[k];
                }
            }
        }
        if (a.to_planes)
            store_planes4(a.dst, gy, gx, a.W, nv, vec, r, g, b);
        else
            emit_hwc(a.out, gy, gx, a.W, nv, vec, r, g, b);
    }
}

// ------------------------------------------------------------------------------ S7 highlight burn
// One workgroup per low-res cell: area-weighted sum of the green density over the cell's source pixels that
// lie in rows [y0, y1) (a row shard contributes its part; shards' arrays add up to the full-frame value).
__global__ __launch_bounds__(256) void burn_sums_kernel(const BurnSumsArgs a) {
    const int j = blockIdx.x, i = blockIdx.y;
    int ry0, ry1, rs1, rs2, cx0, cx1, cs1, cs2;
    double wyf, wy, wyl, wxf, wx, wxl;
    area_cell(i, (double)a.H_global / a.h_lo, a.H_global, ry0, ry1, rs1, rs2, wyf, wy, wyl);
    area_cell(j, (double)a.W / a.w_lo, a.W, cx0, cx1, cs1, cs2, wxf, wx, wxl);
    const int ra = max(ry0, a.y0), rb = min(ry1, a.y1 - 1);
    const int ncols = cx1 - cx0 + 1;
    const float* green = a.src.data + a.src.plane_stride;
    // float32 weights (cv.resize's), the products and the sum in float64 with ONE rounding of the cell's sum: the burn map goes
    // through the 3-D LUT, whose slope turns every ulp lost here into output error (a float32 sum of up to ~10^3 terms loses
    // ~1e-6 relative: 4 of 1 620 fuzz cases with hostile tables sat 3-10 % over their bound, profiles/r04_parity_budget.txt);
    // the map is tiny, the extra width costs nothing
    double acc = 0.0;
    if (rb >= ra) {
        const int n = (rb - ra + 1) * ncols;
        for (int idx = threadIdx.x; idx < n; idx += 256) {
            const int rr = idx / ncols, cc = idx - rr * ncols;
            const int y = ra + rr, x = cx0 + cc;
            const float w = area_weight(y, rs1, rs2, wyf, wy, wyl) * area_weight(x, cs1, cs2, wxf, wx, wxl);
            acc += (double)w * (double)green[(long long)(y - a.src.gy0) * a.W + x];
        }
    }
    __shared__ double red[256];
    const double total = block_sum_256(acc, red);
    if (threadIdx.x == 0) a.cell_sums[i * a.w_lo + j] = (float)total;
}

// scipy.ndimage "reflect" boundary: d c b a | a b c d | d c b a
__device__ __forceinline__ int reflect_sym(int i, int n) {
    while (i < 0 || i >= n) i = i < 0 ? -i - 1 : 2 * n - 1 - i;
    return i;
}

// clip(x - d_ref, 0) then gaussian_filter(sigma=3, truncate=2): two 13-tap passes (axis 0, then axis 1), double
// accumulation and a float32 store after each pass, like scipy's correlate1d.  One workgroup; the map is tiny.
__global__ __launch_bounds__(256) void burn_map_kernel(const BurnMapArgs a) {
    const int n = a.h_lo * a.w_lo;
    float* t0 = a.scratch;
    float* t1 = a.scratch + n;
    for (int k = threadIdx.x; k < n; k += 256) t0[k] = fmaxf(a.cell_sums[k] - a.d_ref, 0.f);
    __syncthreads();
    for (int k = threadIdx.x; k < n; k += 256) {
        const int i = k / a.w_lo, j = k - i * a.w_lo;
        double acc = 0.0;
        for (int t = 0; t < 13; ++t) acc += a.w[t] * (double)t0[reflect_sym(i + t - 6, a.h_lo) * a.w_lo + j];
        t1[k] = (float)acc;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < n; k += 256) {
        const int i = k / a.w_lo, j = k - i * a.w_lo;
        double acc = 0.0;
        for (int t = 0; t < 13; ++t) acc += a.w[t] * (double)t1[i * a.w_lo + reflect_sym(j + t - 6, a.w_lo)];
        a.map[k] = (float)acc;
    }
}

// ------------------------------------------------------------------------------ noise (test)
__global__ __launch_bounds__(256) void noise_kernel(const NoiseArgs a) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int gy = a.y0 + blockIdx.y;
    if (x >= a.W) return;
    const long long rows = a.y1 - a.y0;
    const long long plane = rows * a.W;
    const long long o = (long long)(gy - a.y0) * a.W + x;
    const uint32_t seed = a.frame->seed;
    if (a.hash) {
        uint32_t vx = (uint32_t)x, vy = (uint32_t)gy, vz = seed;
        pcg3d(vx, vy, vz);
        a.hash[o] = vx;
        a.hash[plane + o] = vy;
        a.hash[2 * plane + o] = vz;
    }
    if (a.noise) {
        float nr, ng, nb;
        gaussian_noise((uint32_t)x, (uint32_t)gy, seed, a.mono != 0, nr, ng, nb);
        a.noise[o] = nr;
        a.noise[plane + o] = ng;
        a.noise[2 * plane + o] = nb;
    }
}

// ------------------------------------------------------------------------------ launchers
size_t stencil_lds_bytes(const StencilVariant& v, const DevStencil* st, int nchan) {
    size_t best = 0;
    for (int c = 0; c < nchan; ++c) {
        size_t b = ((size_t)st[c].RS * (size_t)st[c].max_lds_rows + 16) * sizeof(float);
        if (b > best) best = b;
    }
    return best;
}

// noise planes, then (when they fit next to them in half a CU's LDS) the grain LUT's cells
// (xreg_r = R: the separable form with the pass along x in registers, whose planes hold the tile's columns only and no slack)
size_t tail_plane_floats(const DevStencil* gk, int mono, int xreg_r) {
    const size_t plane = xreg_r ? (size_t)(kTailQ * kTailBY + 2 * xreg_r) * (size_t)(4 * kTailBX) : (size_t)gk[0].RS * (size_t)gk[0].max_lds_rows + 16;
    return (plane * (mono ? 1 : 3) + 3) / 4 * 4;
}
size_t tail_lds_bytes(const DevStencil* gk, int mono, int cells_in_lds, int grain_m, int xreg_r) {
    return tail_plane_floats(gk, mono, xreg_r) * sizeof(float) + (cells_in_lds ? (size_t)3 * (grain_m - 1) * sizeof(float4) : 0);
}

// Every instantiation of the two templated kernel families, listed ONCE: init_kernel_attributes raises the dynamic-LDS limit of every
// entry and the launchers index the same tables, so what can be launched is what had its attribute set.
using StencilFn = void (*)(StencilArgs);
using TailFn = void (*)(TailArgs);
constexpr int kStencilFixedN = 12, kTailFixedN = 10;  // R = 0 (the entry list) and the unrolled forms R = 1 .. 11 / 1 .. 9

template <int EPI, int... R>
constexpr std::array<StencilFn, sizeof...(R)> stencil_fixed_row(std::integer_sequence<int, R...>) {
    return {{stencil_kernel<32, 16, 4, EPI, R>...}};
}
template <int EPI, int... V>
constexpr std::array<StencilFn, sizeof...(V)> stencil_generic_row(std::integer_sequence<int, V...>) {
    return {{stencil_kernel<kStencilVariants[V].BX, kStencilVariants[V].BY, kStencilVariants[V].Q, EPI>...}};
}
template <bool SEP, int... R>
constexpr std::array<TailFn, sizeof...(R)> tail_row(std::integer_sequence<int, R...>) {
    return {{tail_kernel<R, SEP && (R > 0)>...}};  // (R = 0 has no separable form: the entry list either way)
}
template <int... R>
constexpr std::array<TailFn, sizeof...(R)> tail_xreg_row(std::integer_sequence<int, R...>) {
    return {{tail_kernel<R + 1, true, true>...}};  // R = 1 .. kTailXRegMaxR
}
template <int N>
using UpTo = std::make_integer_sequence<int, N>;
// [EPI][R]: variant 0's tile; R = 0 is its entry-list form
constexpr std::array<std::array<StencilFn, kStencilFixedN>, 2> kStencilFixed = {
    {stencil_fixed_row<0>(UpTo<kStencilFixedN>{}), stencil_fixed_row<1>(UpTo<kStencilFixedN>{})}};
// [EPI][variant]: the entry-list form on every tile of kStencilVariants
constexpr std::array<std::array<StencilFn, kNumStencilVariants>, 2> kStencilGeneric = {
    {stencil_generic_row<0>(UpTo<kNumStencilVariants>{}), stencil_generic_row<1>(UpTo<kNumStencilVariants>{})}};
// [SEP][R]
constexpr std::array<std::array<TailFn, kTailFixedN>, 2> kTail = {{tail_row<false>(UpTo<kTailFixedN>{}), tail_row<true>(UpTo<kTailFixedN>{})}};
// [R - 1]: the separable form of R <= kTailXRegMaxR with the pass along x in registers (kTail[1][R] has it in LDS)
constexpr std::array<std::array<TailFn, kTailXRegMaxR>, 1> kTailXReg = {{tail_xreg_row(UpTo<kTailXRegMaxR>{})}};

hipError_t init_kernel_attributes() {
    auto raise = [](const void* k) { return hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds); };
    auto raise_all = [&](const auto& table) {
        for (const auto& row : table)
            for (auto k : row) {
                const hipError_t e = raise(reinterpret_cast<const void*>(k));
                if (e != hipSuccess) return e;
            }
        return hipSuccess;
    };
    hipError_t e = raise_all(kStencilFixed);
    if (e == hipSuccess) e = raise_all(kStencilGeneric);
    if (e == hipSuccess) e = raise_all(kTail);
    if (e == hipSuccess) e = raise_all(kTailXReg);
    if (e == hipSuccess) e = raise(reinterpret_cast<const void*>(front_kernel<true>));
    return e;
}

hipError_t launch_front(const FrontArgs& a, hipStream_t s) {
    if (a.y1 <= a.y0 || a.W <= 0) return hipSuccess;
    if (a.fast && front_fast_eligible(a)) return launch_front_fast(a, s);
    const int quads = (a.W + 3) / 4;
    const int gx = (quads + 63) / 64;
    const int row_groups = (a.y1 - a.y0 + kFrontBY - 1) / kFrontBY;
    dim3 block(64, kFrontBY);
    const size_t cell_bytes = (size_t)3 * (a.curve.m > 1 ? a.curve.m - 1 : 0) * sizeof(float4);
    const bool ldsc = a.upto >= R2F_UPTO_DENSITY && cell_bytes > 0 && cell_bytes <= 64 * 1024;
    if (ldsc) {
        // persistent-ish grid: a few blocks per CU in total, so the table copy is amortised over many rows.  Three blocks
        // are resident per CU at 48 KB of cells each; 24 MP LUT-only frame: 0.51 / 0.35 / 0.26 / 0.25 ms at 1 / 2 / 3 / 6 per CU
        int gy = ((a.blocks_per_cu > 0 ? a.blocks_per_cu : 6) * 256 + gx - 1) / gx;
        if (gy > row_groups) gy = row_groups;
        if (gy < 1) gy = 1;
        launch_k(front_kernel<true>, dim3(gx, gy), block, cell_bytes, s, a);
    } else {
        launch_k(front_kernel<false>, dim3(gx, row_groups), block, 0, s, a);
    }
    return take_launch_status();
}

hipError_t launch_stencil(const StencilArgs& a, int variant, hipStream_t s) {
    if (a.y1 <= a.y0 || a.W <= 0) return hipSuccess;
    const StencilVariant& v = kStencilVariants[variant];
    const size_t lds = stencil_lds_bytes(v, a.st, 3);  // any subset of the channels may be in a.chan
    dim3 block(v.BX * v.BY), grid((a.W + v.TW() - 1) / v.TW(), (a.y1 - a.y0 + v.TH() - 1) / v.TH(), a.nchan);
    const int epi = a.epilogue == 1 ? 1 : 0;
    // small square mirror-symmetric stencils: the unrolled form (variant 0's tile only)
    const bool fixed = variant == 0 && a.fixed_r > 0 && a.fixed_r < kStencilFixedN;
    launch_k(fixed ? kStencilFixed[epi][a.fixed_r] : kStencilGeneric[epi][variant], grid, block, lds, s, a);
    return take_launch_status();
}

hipError_t launch_tail(const TailArgs& a, hipStream_t s) {
    if (a.y1 <= a.y0 || a.W <= 0) return hipSuccess;
    if (!a.grain) {
        Lut3dArgs l;
        l.src = a.src;
        l.out = a.out;
        l.y0 = a.y0;
        l.y1 = a.y1;
        l.W = a.W;
        l.lut3d = a.lut3d;
        l.lut3d_scale = a.lut3d_scale;
        l.lut3d_mode = a.lut3d_mode;
        l.vec = a.vec;
        l.burn = a.burn;
        l.gfield = a.gfield;
        l.has_gfield = a.has_gfield;
        l.grain_lut = a.grain_lut;
        return launch_64x4(lut3d_kernel, (a.W + 3) / 4, a.y1 - a.y0, s, l);
    }
    const int TW = 4 * kTailBX, TH = kTailQ * kTailBY;
    dim3 block(kTailBX * kTailBY), grid((a.W + TW - 1) / TW, (a.y1 - a.y0 + TH - 1) / TH);
    TailArgs b = a;
    // small square mirror-symmetric stencils take the unrolled form, separable ones two 1-D passes
    const int r = a.fixed_r > 0 && a.fixed_r < kTailFixedN ? a.fixed_r : 0;
    const bool x_in_reach = a.sep && r >= 1 && r <= kTailXRegMaxR;  // the pass along x can run in registers
    const int xreg_r = x_in_reach && !a.xpass_lds ? r : 0;
    b.cells_off = (int)tail_plane_floats(a.gk, a.mono, xreg_r);
    b.cells_in_lds = tail_lds_bytes(a.gk, a.mono, 1, a.grain_lut.m, xreg_r) <= 80 * 1024 ? 1 : 0;  // keep two workgroups per CU
    const size_t lds = tail_lds_bytes(a.gk, a.mono, b.cells_in_lds, a.grain_lut.m, xreg_r);
    launch_k(xreg_r ? kTailXReg[0][r - 1] : kTail[a.sep ? 1 : 0][r], grid, block, lds, s, b);
    return take_launch_status();
}

hipError_t launch_burn_sums(const BurnSumsArgs& a, hipStream_t s) {
    if (a.h_lo <= 0 || a.w_lo <= 0) return hipSuccess;
    launch_k(burn_sums_kernel, dim3(a.w_lo, a.h_lo), dim3(256), 0, s, a);
    return take_launch_status();
}

hipError_t launch_burn_map(const BurnMapArgs& a, hipStream_t s) {
    launch_k(burn_map_kernel, dim3(1), dim3(256), 0, s, a);
    return take_launch_status();
}

hipError_t launch_single_tap(const TapArgs& a, hipStream_t s) {
    if (a.y1 <= a.y0 || a.W <= 0) return hipSuccess;
    launch_k(single_tap_kernel, dim3((a.W + 1023) / 1024, a.y1 - a.y0), dim3(256), 0, s, a);
    return take_launch_status();
}

hipError_t launch_noise(const NoiseArgs& a, hipStream_t s) {
    if (a.y1 <= a.y0 || a.W <= 0) return hipSuccess;
    dim3 block(256), grid((a.W + 255) / 256, a.y1 - a.y0);
    launch_k(noise_kernel, grid, block, 0, s, a);
    return take_launch_status();
}

// mode 0: only the seed (a stage entry's own write in the middle of a frame keeps the exposure range the front kernel recorded);
// 1: the whole block (seed + range reset: the start of a frame); 2: only the range reset (a caller that keeps the seed resident);
// 3: the range is made unusable (max = +inf) -- a front kernel that was asked to record the range of what it writes and cannot (its
// rows' TILES stay unwritten, but they may share a tile with rows another call recorded: fft_decide_kernel reads the mark and keeps
// every pair of the call on complex128).
// Modes 1 and 2 also reset the record's tile grid ({+inf, 0} = unknown), one thread per tile.
__global__ __launch_bounds__(256) void frame_params_kernel(FrameParams* dst, const FrameParams v, const int mode, int2* tiles, const int n_tiles) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {
        if (mode == 1)
            *dst = v;
        else if (mode == 0)
            dst->seed = v.seed;
        else if (mode == 2)
            dst->e_min = v.e_min, dst->e_max = v.e_max;
        else
            dst->e_max = 0x7f800000u;
    }
    if ((mode == 1 || mode == 2) && i < n_tiles) tiles[i] = make_int2((int)kFrameMinReset, (int)kFrameMaxReset);
}

hipError_t launch_frame_params(const RangeRecord& rec, const FrameParams& v, int mode, hipStream_t s) {
    const int n_tiles = (rec.tiles && (mode == 1 || mode == 2)) ? rec.tyn * rec.txn : 0;
    launch_k(frame_params_kernel, dim3(n_tiles > 0 ? (n_tiles + 255) / 256 : 1), dim3(n_tiles > 0 ? 256 : 1), 0, s, rec.blk, v, mode, rec.tiles,
             n_tiles);
    return take_launch_status();
}

// min / max |.| of rows [y0, y1) and [y2, y3) of the planes in `mask`, merged into the record's tiles like the front kernel's own
// (r2f_stage_exposure_range: the halo rows a row shard received from its neighbours above and below, one launch for both bands).
// A wave takes 256 columns of one row -- one tile column, like a wave of the front kernel --, a workgroup 16 consecutive rows whose
// waves combine through LDS before one of them merges into the (one or two) tiles they touch: grid (ceil(W / 256), ceil(rows / 16)),
// block (64, 16).  NaNs drop out of fminf / fmaxf, like there.
constexpr int kRangeRowsPerBlock = 16;
__global__ __launch_bounds__(64 * kRangeRowsPerBlock) void exposure_range_kernel(const DevPlanes src, const int y0, const int y1, const int y2,
                                                                                  const int y3, const int W, const int mask,
                                                                                  const RangeRecord rec) {
    __shared__ int wg_ty[kRangeRowsPerBlock];
    __shared__ float wg_lo[kRangeRowsPerBlock], wg_hi[kRangeRowsPerBlock];
    const int n0 = y1 - y0, r = blockIdx.y * kRangeRowsPerBlock + threadIdx.y;
    const bool live = r < n0 + (y3 - y2);  // (wave-uniform)
    const int gy = r < n0 ? y0 + r : y2 + (r - n0);
    float lo = __builtin_inff(), hi = 0.f;
    if (live) {
        const int x0 = (blockIdx.x * 64 + threadIdx.x) * 4;
        for (int c = 0; c < 3; ++c) {
            if (!((mask >> c) & 1)) continue;
            const float* p = src.data + c * src.plane_stride + (long long)(gy - src.gy0) * W;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x0 + k < W) {
                    const float v = p[x0 + k];
                    lo = range_min(lo, v), hi = fmaxf(hi, fabsf(v));
                }
        }
    }
    lo = wave_extreme<false>(lo), hi = wave_extreme<true>(hi);
    if (threadIdx.x == 63) wg_ty[threadIdx.y] = live ? (gy >> kRangeTileRowsLog2) : -1, wg_lo[threadIdx.y] = lo, wg_hi[threadIdx.y] = hi;
    __syncthreads();
    if (threadIdx.y == 0 && threadIdx.x == 0) {
        for (int i = 0; i < kRangeRowsPerBlock; ++i) {
            const int ty = wg_ty[i];
            if (ty < 0) continue;
            float l2 = wg_lo[i], h2 = wg_hi[i];
            for (int j = i + 1; j < kRangeRowsPerBlock; ++j)
                if (wg_ty[j] == ty) l2 = fminf(l2, wg_lo[j]), h2 = fmaxf(h2, wg_hi[j]), wg_ty[j] = -1;
            merge_tile(rec, ty << kRangeTileRowsLog2, blockIdx.x, l2, h2);
        }
    }
}

hipError_t launch_exposure_range(const DevPlanes& src, int y0, int y1, int y2, int y3, int W, int mask, const RangeRecord& rec, hipStream_t s) {
    if (y1 < y0) y1 = y0;
    if (y3 < y2) y3 = y2;
    const int rows = (y1 - y0) + (y3 - y2);
    if (rows <= 0 || W <= 0 || !(mask & 7)) return hipSuccess;
    launch_k(exposure_range_kernel, dim3((W + kRangeTileCols - 1) / kRangeTileCols, (rows + kRangeRowsPerBlock - 1) / kRangeRowsPerBlock),
             dim3(64, kRangeRowsPerBlock), 0, s, src, y0, y1, y2, y3, W, mask, rec);
    return take_launch_status();
}

}  // namespace r2f
