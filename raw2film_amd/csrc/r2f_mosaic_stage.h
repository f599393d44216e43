// r2f_mosaic_stage.h -- the staging of the two demosaics (r2f_demosaic.hip the Bayer pattern's, r2f_xtrans.hip the X-Trans one's):
// which samples a block holds in LDS, how they are loaded and how the finished pixels leave; and the entry points' checks.  Device
// text, included by those two files.  The arithmetic is not here: it is the pattern's (r2f_demosaic_math.h, r2f_xtrans_math.h) and
// r2f_mosaic_math.h's.
//   mosaic_full_kernel     one launch: scaled tile + apron in LDS (step A once per sample), the pattern's auxiliary plane of the tile +
//                          1-sample apron in LDS, then the pattern's pixel_rgb and step C per output pixel; a wave's row leaves
//                          through an LDS transpose as one contiguous segment
//   mosaic_reduced_kernel  one lane per output pixel of the reduced form (a half or a third of the mosaic's sides)
//   mosaic_median_full_kernel, mosaic_median_reduced_kernel   the same two with step M (LibRaw's med_passes) behind the interpolation:
//                          the tile's three planes plus an n-pixel ring in LDS, n passes of the 3 x 3 median of R - G and B - G there
//                          (median_passes; the arithmetic is r2f_median_math.h's), then the epilogues above (leave_tile)
//   MosaicCall, mosaic_rows  what an entry point passes (its form -- plain, blend or median -- among it); the checks every entry point
//                          makes, then one launch: the choice among reduced, turned, mirrored and upright is written once for all forms
// Each is a template over a Pattern and over the epilogue: the uint16 frame, or a window of it decoded to the float frame the front
// stage reads (decode_sample of r2f_device.h on each finished sample); and, for the uint16 frame written the way round the sensor
// was held (the oriented entry points; the index map is r2f_mosaic_math.h's orient), over an OrientClass: mirrored rows leave from
// the row buffer, quarter turns through the whole tile transposed in LDS; and over a Blend flag (the blend entry points: LibRaw's
// highlight mode 2), which runs mosaic::blend_pixel on the pixel's three integers between pixel_rgb / reduced_rgb and step C -- in
// registers: it stages nothing, and a wave diverges on it only where its row crosses a blown area.  The instantiations without the
// flag are the kernels of before it.  A Pattern states what differs and nothing else:
//   Params, Aux                   its r2f_*_params and the auxiliary plane's element type (uint16_t green / int colour difference)
//   kMinSide, kReduction          the smallest mosaic side, what the reduced form divides the sides by
//   kReachY, kApronX              mosaic rows a full-size output row reads above and below it; staged columns each side of a tile
//   kParamsInLds                  whether lanes index the params' tables (then a block keeps them in LDS, else they stay arguments)
//   kPlanner                      the planner's name, for messages
//   reduced(p)                    whether p asks for the reduced form
//   check_params(ctx, what, p, H, W)     R2F_OK, or the refusal of params no planner made
//   scale_pair(p, y, x, r0, r1, v0, v1)  step A of the raw samples (y, x) and (y, x + 1), x even, with the pattern's phase rule
//   kAuxRing, aux_at(p, S, H, W, y, x)   the auxiliary plane at a frame site at least kAuxRing samples from every edge (0 is staged
//                                 outside: nothing reads it there)
//   pixel_rgb(p, S, A, H, W, y, x, rgb)  the three planes of an output pixel, before the matrix
//   reduced_rgb(a, p, y, x, rgb)  those of a pixel of the reduced form, from the cell it loads itself
// Nothing here runs inside r2f_render or a timed step.  The kernels have static LDS: they need no dynamic-LDS attribute and so no row
// in r2f_kernels.hip's instantiation tables.
#pragma once

#include <cstdint>
#include <type_traits>

#include "r2f_ctx.h"
#include "r2f_median_math.h"
#include "r2f_mosaic_math.h"

namespace r2f {
namespace {

constexpr int kTW = 64, kTH = 32;  // the tile; lanes along x: a wave is one row of it
constexpr int kRowsPerLane = kTH / 4;
static_assert(R2F_DEMOSAIC_TILE_W == kTW && R2F_DEMOSAIC_TILE_H == kTH && R2F_XTRANS_TILE_W == kTW && R2F_XTRANS_TILE_H == kTH,
              "include/r2f.h states the tile of either pattern");
static_assert(kTW == 64 && kTH % 4 == 0, "a wave per tile row, workgroups of (64, 4)");

template <typename Params>
struct MosaicArgs {
    const uint16_t* src;  // row src_gy0 of the mosaic
    int src_gy0;
    long long pitch;  // samples
    int H, W;
    Params p;
    void* dst;   // row dst_y0, column x0 of the demosaiced frame D: rows of x1 - x0 pixels, uint16 or float
    int y0, y1;  // the rows of D this call writes
    int wide;    // 1: src is 4-byte aligned and the pitch even -> a pair of samples at an even x is one 32-bit load
    int dst_y0, x0, x1;     // the window of D that dst holds (the uint16 entry points: all of it)
    float divisor, factor;  // the float epilogue's
    int orientation;        // the oriented entry points': dst is then row 0 of O, and [y0, y1) x [x0, x1) the rectangle of D it takes
    int clip;               // the blend entry points': mosaic::blend_pixel's level (read by the Blend instantiations only)
};

// How the finished pixels of the full size leave: as rows of D; as rows of O that are rows of D mirrored (bits 1 and 2 of the
// orientation); or as rows of O that are columns of D (bit 4).  A compile-time class: each has its own epilogue and LDS.
enum OrientClass { kUpright = 0, kMirrored = 1, kTurned = 2 };
// The turned class collects a tile's finished pixels in LDS in O's layout: kTW rows of O (a column of D each) of up to kTH pixels.
// A wave's 64 lanes hold one row of D: each writes its pixel into a different row of that buffer, at the same offset in it.  Every
// ds_write goes to bank (byte address / 4) % 32, lanes conflict within a 32-lane half; with a pitch of P dwords lane l's bank is
// (l * P + const) % 32, and for an odd P the 32 lanes of a half hit 32 different banks.  A row holds 3 * kTH uint16 = 48 dwords; 49
// is the next odd number: 98 uint16.  (A pitch of 48 would put lanes l and l + 2 on one bank: 16 ways.)
constexpr int kTurnPitch = 3 * kTH + 2;  // uint16
static_assert(kTurnPitch % 2 == 0 && (kTurnPitch / 2) % 2 == 1, "whole dwords per row (store_segment reads them), an odd number of them");

// The extents of what a block stages: the scaled samples, and the auxiliary plane with its 1-sample apron.
template <typename Pattern>
struct Staged {
    static constexpr int kSW = kTW + 2 * Pattern::kApronX, kSH = kTH + 2 * Pattern::kReachY;
    static constexpr int kAW = kTW + 2, kAH = kTH + 2;
    // The tile origin is a multiple of 64 and the apron even, so load_pair's x is even.  For an even x, x + 1 >= 0 exactly when
    // x >= 0: load_pair's `in1 = in0 && x + 1 < W` and the symmetric `x + 1 >= 0 && x + 1 < W` are the same predicate.
    static_assert(kTW % 2 == 0 && Pattern::kApronX % 2 == 0 && kSW % 2 == 0, "the samples are loaded in pairs at even columns");
    static_assert(Pattern::kApronX >= Pattern::kReachY, "the staged columns cover the reach");
};

// A pattern's params where its lanes read them: the kernel's arguments, or a block's copy of them in LDS.
template <typename Pattern>
__device__ __forceinline__ const typename Pattern::Params& params_of(const MosaicArgs<typename Pattern::Params>& a,
                                                                     const typename Pattern::Params& s_p) {
    if constexpr (Pattern::kParamsInLds)
        return s_p;
    else
        return a.p;
}
template <typename Params>
__device__ __forceinline__ void stage_params(const MosaicArgs<Params>& a, Params& s_p, int tid) {
    static_assert(sizeof(Params) % 4 == 0 && alignof(Params) == 4, "copied to LDS in 32-bit words");
    const uint32_t* from = reinterpret_cast<const uint32_t*>(&a.p);
    uint32_t* to = reinterpret_cast<uint32_t*>(&s_p);
    for (int i = tid; i < (int)(sizeof(Params) / 4); i += 256) to[i] = from[i];
}

// The samples (y, x) and (y, x + 1), x even, scaled (step A); 0 for one outside the frame's columns.  One 32-bit load where that is
// allowed and both are inside, else one 16-bit load each: the same samples either way.  y is inside the frame.
template <typename Pattern>
__device__ __forceinline__ void load_pair(const MosaicArgs<typename Pattern::Params>& a, const typename Pattern::Params& p, int y, int x,
                                          int& s0, int& s1) {
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
    int v0, v1;
    Pattern::scale_pair(p, y, x, (int)r0, (int)r1, v0, v1);
    s0 = in0 ? v0 : 0, s1 = in1 ? v1 : 0;
}

template <typename T, int Pitch>
struct Tile {  // a plane a block holds in LDS, at frame coordinates
    const T* s;
    int y_org, x_org;  // frame coordinates of s[0]
    __device__ __forceinline__ int operator()(int y, int x) const { return s[(y - y_org) * Pitch + (x - x_org)]; }
};

// What leaves: the finished uint16 sample, or its decode to the float frame.
template <bool F32>
using OutT = std::conditional_t<F32, float, uint16_t>;
template <bool F32, typename Params>
__device__ __forceinline__ OutT<F32> finish_sample(const MosaicArgs<Params>& a, uint16_t v) {
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
// window's col0) and to the call's first row; lanes outside the window's columns compute nothing and store nothing.  Every phase is
// taken from frame coordinates, never from the tile's.
template <typename Pattern, bool F32, int Cls = kUpright, bool Blend = false>
__global__ __launch_bounds__(256) void mosaic_full_kernel(const MosaicArgs<typename Pattern::Params> a) {
    static_assert(Cls == kUpright || !F32, "the float epilogue is upright");
    using St = Staged<Pattern>;
    using Aux = typename Pattern::Aux;
    constexpr int kReachY = Pattern::kReachY, kApronX = Pattern::kApronX, kSW = St::kSW, kSH = St::kSH, kAW = St::kAW, kAH = St::kAH;
    __shared__ typename Pattern::Params s_p;  // (no use of it, and so no LDS, unless the pattern keeps its params there)
    __shared__ __align__(16) uint16_t s_s[kSH * kSW];
    __shared__ __align__(16) Aux s_a[kAH * kAW];
    using OutBuffer = std::conditional_t<Cls == kTurned, uint16_t[kTW * kTurnPitch], OutT<F32>[4][3 * kTW]>;  // the tile, or a row per wave
    __shared__ __align__(16) OutBuffer s_out;
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * 64 + tx;
    const int tx0 = (a.x0 / kTW + (int)blockIdx.x) * kTW, ty0 = a.y0 + blockIdx.y * kTH;
    if constexpr (Pattern::kParamsInLds) {
        stage_params(a, s_p, tid);
        __syncthreads();
    }
    const typename Pattern::Params& p = params_of<Pattern>(a, s_p);
    // the rows this call may read (the entry point has checked that the source window holds them)
    const int ry0 = a.y0 - kReachY > 0 ? a.y0 - kReachY : 0, ry1 = a.y1 + kReachY < a.H ? a.y1 + kReachY : a.H;

    for (int i = tid; i < kSH * (kSW / 2); i += 256) {
        const int r = i / (kSW / 2), c = 2 * (i % (kSW / 2));
        const int y = ty0 - kReachY + r, x = tx0 - kApronX + c;  // (x is even: Staged)
        int s0 = 0, s1 = 0;
        if (y >= ry0 && y < ry1) load_pair<Pattern>(a, p, y, x, s0, s1);
        s_s[r * kSW + c] = (uint16_t)s0, s_s[r * kSW + c + 1] = (uint16_t)s1;
    }
    __syncthreads();

    const Tile<uint16_t, kSW> S{s_s, ty0 - kReachY, tx0 - kApronX};
    // the auxiliary plane where this call's rows read it: rows [y0 - 1, y1 + 1) of the frame, inside the pattern's ring
    constexpr int kRing = Pattern::kAuxRing;
    const int ay0 = a.y0 - 1 > kRing ? a.y0 - 1 : kRing, ay1 = a.y1 + 1 < a.H - kRing ? a.y1 + 1 : a.H - kRing;
    for (int i = tid; i < kAH * kAW; i += 256) {
        const int r = i / kAW, c = i % kAW;
        const int y = ty0 - 1 + r, x = tx0 - 1 + c;
        int v = 0;
        if (y >= ay0 && y < ay1 && x >= kRing && x < a.W - kRing) v = Pattern::aux_at(p, S, a.H, a.W, y, x);
        s_a[i] = (Aux)v;
    }
    __syncthreads();

    const Tile<Aux, kAW> A{s_a, ty0 - 1, tx0 - 1};
    const int x = tx0 + tx;
    // this tile's share of a row of the window: columns [xa, xb), n elements
    const int xa = tx0 > a.x0 ? tx0 : a.x0, xb = tx0 + kTW < a.x1 ? tx0 + kTW : a.x1, n = 3 * (xb - xa);
    if constexpr (Cls == kTurned) {
        // The tile's rows of D, [ty0, ye), are columns [c0, c0 + ye - ty0) of O, backwards with the rows mirrored; its column x of D is
        // row x of O, or out_w - 1 - x with the columns mirrored.  All pixels into the buffer first, then a wave takes every fourth
        // row of it to dst as one contiguous run.
        const bool flip_rows = a.orientation & orient::kRows, flip_cols = a.orientation & orient::kCols;
        const int ye = ty0 + kTH < a.y1 ? ty0 + kTH : a.y1, c0 = flip_rows ? a.p.out_h - ye : ty0;
        for (int q = 0; q < kRowsPerLane; ++q) {
            const int y = ty0 + ty + 4 * q;
            if (y < ye && x >= xa && x < xb) {
                int rgb[3];
                uint16_t out[3];
                Pattern::pixel_rgb(p, S, A, a.H, a.W, y, x, rgb);
                if constexpr (Blend) mosaic::blend_pixel(rgb, a.clip);
                mosaic::colour(p.M, rgb, out);
                uint16_t* o = s_out + tx * kTurnPitch + 3 * (flip_rows ? ye - 1 - y : y - ty0);
                o[0] = out[0], o[1] = out[1], o[2] = out[2];
            }
        }
        __syncthreads();
        uint16_t* dst = static_cast<uint16_t*>(a.dst);
        for (int j = ty; j < kTW; j += 4) {  // (the same for all 64 lanes of a wave)
            const int xj = tx0 + j;
            if (xj < xa || xj >= xb) continue;
            const int r = flip_cols ? a.p.out_w - 1 - xj : xj;
            store_segment(dst + ((long long)r * a.p.out_h + c0) * 3, s_out + j * kTurnPitch, 3 * (ye - ty0), tx);
        }
    } else if constexpr (Cls == kMirrored) {
        // The upright walk below with two changes (the window is the frame: x0 = 0, x1 = out_w, dst_y0 = 0).  Row y of D is row
        // out_h - 1 - y of O with bit 2: the segment pointer walks upward.  With bit 1 the tile's columns [xa, xb) are O's
        // [out_w - xb, out_w - xa), and a lane writes its pixel to the mirrored slot of the row buffer.
        const bool flip_rows = a.orientation & orient::kRows, flip_cols = a.orientation & orient::kCols;
        const long long row_elems = 3LL * a.p.out_w, step = flip_rows ? -4 * row_elems : 4 * row_elems;
        const int slot = flip_cols ? xb - 1 - x : x - xa;
        uint16_t* seg = static_cast<uint16_t*>(a.dst) + (flip_rows ? a.p.out_h - 1 - (ty0 + ty) : ty0 + ty) * row_elems +
                        3 * (flip_cols ? a.p.out_w - xb : xa);
        for (int q = 0; q < kRowsPerLane; ++q, seg += step) {
            const int y = ty0 + ty + 4 * q;  // (the same for all 64 lanes of a wave)
            if (y < a.y1 && x >= xa && x < xb) {
                int rgb[3];
                uint16_t out[3];
                Pattern::pixel_rgb(p, S, A, a.H, a.W, y, x, rgb);
                if constexpr (Blend) mosaic::blend_pixel(rgb, a.clip);
                mosaic::colour(p.M, rgb, out);
                uint16_t* o = s_out[ty] + 3 * slot;
                o[0] = out[0], o[1] = out[1], o[2] = out[2];
            }
            __syncthreads();
            if (y < a.y1) store_segment(seg, s_out[ty], n, tx);
            __syncthreads();
        }
    } else {
        // the wave's row segment, n contiguous elements of dst: that of its first row, then four rows on per step (one 64-bit product
        // here, none per row)
        const long long row_elems = 3LL * (a.x1 - a.x0);
        OutT<F32>* seg = static_cast<OutT<F32>*>(a.dst) + (ty0 + ty - a.dst_y0) * row_elems + 3 * (xa - a.x0);
        for (int q = 0; q < kRowsPerLane; ++q, seg += 4 * row_elems) {
            const int y = ty0 + ty + 4 * q;  // (the same for all 64 lanes of a wave)
            if (y < a.y1 && x >= xa && x < xb) {
                int rgb[3];
                uint16_t out[3];
                Pattern::pixel_rgb(p, S, A, a.H, a.W, y, x, rgb);
                if constexpr (Blend) mosaic::blend_pixel(rgb, a.clip);
                mosaic::colour(p.M, rgb, out);
                OutT<F32>* o = s_out[ty] + 3 * (x - xa);
                o[0] = finish_sample<F32>(a, out[0]), o[1] = finish_sample<F32>(a, out[1]), o[2] = finish_sample<F32>(a, out[2]);
            }
            __syncthreads();
            if (y < a.y1) store_segment(seg, s_out[ty], n, tx);
            __syncthreads();
        }
    }
}

// Oriented: the lane stores its pixel where orient::from_frame puts it in O (a quarter or a ninth of the samples: no transpose buffer).
template <typename Pattern, bool F32, bool Oriented = false, bool Blend = false>
__global__ __launch_bounds__(256) void mosaic_reduced_kernel(const MosaicArgs<typename Pattern::Params> a) {
    __shared__ typename Pattern::Params s_p;  // (as above)
    if constexpr (Pattern::kParamsInLds) {
        stage_params(a, s_p, threadIdx.y * 64 + threadIdx.x);
        __syncthreads();
    }
    const typename Pattern::Params& p = params_of<Pattern>(a, s_p);
    const int x = a.x0 + blockIdx.x * 64 + threadIdx.x, y = a.y0 + blockIdx.y * 4 + threadIdx.y;
    if (x >= a.x1 || y >= a.y1) return;
    int rgb[3];
    uint16_t out[3];
    Pattern::reduced_rgb(a, p, y, x, rgb);
    if constexpr (Blend) mosaic::blend_pixel(rgb, a.clip);
    mosaic::colour(p.M, rgb, out);
    OutT<F32>* d;
    if constexpr (Oriented) {
        static_assert(!F32, "the float epilogue is upright");
        int r, c;
        orient::from_frame(a.orientation, a.p.out_h, a.p.out_w, y, x, r, c);
        d = static_cast<OutT<F32>*>(a.dst) + ((long long)r * orient::cols(a.orientation, a.p.out_h, a.p.out_w) + c) * 3;
    } else {
        d = static_cast<OutT<F32>*>(a.dst) + ((long long)(y - a.dst_y0) * (a.x1 - a.x0) + (x - a.x0)) * 3;
    }
    d[0] = finish_sample<F32>(a, out[0]), d[1] = finish_sample<F32>(a, out[1]), d[2] = finish_sample<F32>(a, out[2]);
}

// ------------------------------------------------------------------------------------------------------------------------ step M
// The median kernels (include/r2f.h, step M: LibRaw's med_passes): the two kernels above with n passes of the 3 x 3 median of R - G
// and B - G between the interpolation and Blend / step C.  A block holds the three planes of its tile plus an n-pixel ring in LDS
// (sized for the cap: the kernels keep static LDS), filled once from pixel_rgb / reduced_rgb; the passes run in LDS, ping-pong for
// red and blue, and the region that is still exact shrinks by one ring per pass down to the tile.  The ring is the frame's, not
// the call's: a window or row-range edge that is no frame edge reads beyond it, so the staged samples reach n further
// (kReachY + n rows; the entry point has checked the source window for them).  Blend is a uniform run-time branch on `clip` here
// (0: none), not a template flag: half the instantiations, the same bytes.  The argument record is the kernels' own: MosaicArgs and
// the kernels above are what they were.
constexpr int kMedN = R2F_MEDIAN_MAX_PASSES;
constexpr int kMedW = kTW + 2 * kMedN, kMedH = kTH + 2 * kMedN;  // the region of the cap: 72 x 40 pixels
static_assert(kMedN % 2 == 0, "the staged samples start at an even column");

template <typename Params>
struct MedianArgs {
    MosaicArgs<Params> m;  // (clip: 0 for no Blend)
    int passes;            // n, 1 .. kMedN
};

// A block's planes: green, and red / blue twice: I_k is in r0, b0 for an even k, in r1, b1 for an odd one.  (Selects, not a pointer
// array: a register array indexed by a variable goes to scratch.)
struct MedianPlanes {
    uint16_t *g, *r0, *b0, *r1, *b1;
    __device__ __forceinline__ uint16_t* r(int odd) const { return odd ? r1 : r0; }
    __device__ __forceinline__ uint16_t* b(int odd) const { return odd ? b1 : b0; }
};

// The n passes.  The planes hold kMedH x kMedW pixels from frame position (y_org, x_org); on entry g, r0, b0 are I_0 on the
// block's rectangle [ya, yb) x [xa, xb) of D grown by n rings and clipped to the frame (written by these lanes: the barrier is
// here).  Pass k writes that rectangle grown by n - k rings: an interior pixel of the frame by median::pass_pixel, a border pixel
// carried over.  I_n on the rectangle itself is then in r(n & 1), b(n & 1), which is returned; a barrier stands behind the last pass.
__device__ __forceinline__ int median_passes(const MedianPlanes& pl, int y_org, int x_org, int ya, int yb, int xa, int xb, int n, int out_h,
                                             int out_w, int tid) {
    __syncthreads();
    const Tile<uint16_t, kMedW> G{pl.g, y_org, x_org};
    for (int k = 1; k <= n; ++k) {
        const int m = n - k, from = (k - 1) & 1;
        const int py0 = ya - m > 0 ? ya - m : 0, py1 = yb + m < out_h ? yb + m : out_h;
        const int px0 = xa - m > 0 ? xa - m : 0, px1 = xb + m < out_w ? xb + m : out_w;
        const Tile<uint16_t, kMedW> R{pl.r(from), y_org, x_org}, B{pl.b(from), y_org, x_org};
        uint16_t *to_r = pl.r(from ^ 1), *to_b = pl.b(from ^ 1);
        for (int i = tid; i < kMedH * kMedW; i += 256) {
            const int y = y_org + i / kMedW, x = x_org + i % kMedW;
            if (y < py0 || y >= py1 || x < px0 || x >= px1) continue;
            int r, b;
            if (mosaic::in_ring(out_h, out_w, y, x, 1))
                r = R(y, x), b = B(y, x);
            else
                median::pass_pixel(R, B, G, y, x, r, b);
            to_r[i] = (uint16_t)r, to_b[i] = (uint16_t)b;
        }
        __syncthreads();
    }
    return n & 1;
}

// How a tile's finished pixels leave, by OrientClass: mosaic_full_kernel's three epilogues from the point where they call pixel_rgb,
// as a function.  `rgb_of(y, x, rgb)` yields the three planes of pixel (y, x) of D ahead of the matrix M (step C), s_out is the
// block's row buffers (the turned class: the whole tile).  Called by all 256 lanes of a (64, 4) block whose tile has its origin at
// (ty0, tx0).  (mosaic_full_kernel keeps its own text: calling this function from it left its registers and LDS alone but reordered
// its instructions, and it ran 1 - 3 % slower beside the build of before in one process.  The comments on the index arithmetic are
// there.)
template <bool F32, int Cls, typename Params, typename OutBuffer, typename RgbFn>
__device__ __forceinline__ void leave_tile(const MosaicArgs<Params>& a, const float (&M)[9], OutBuffer& s_out, int tx0, int ty0,
                                           const RgbFn& rgb_of) {
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int x = tx0 + tx;
    // this tile's share of a row of the window: columns [xa, xb), n elements
    const int xa = tx0 > a.x0 ? tx0 : a.x0, xb = tx0 + kTW < a.x1 ? tx0 + kTW : a.x1, n = 3 * (xb - xa);
    if constexpr (Cls == kTurned) {
        // The tile's rows of D, [ty0, ye), are columns [c0, c0 + ye - ty0) of O, backwards with the rows mirrored; its column x of D is
        // row x of O, or out_w - 1 - x with the columns mirrored.  All pixels into the buffer first, then a wave takes every fourth
        // row of it to dst as one contiguous run.
        const bool flip_rows = a.orientation & orient::kRows, flip_cols = a.orientation & orient::kCols;
        const int ye = ty0 + kTH < a.y1 ? ty0 + kTH : a.y1, c0 = flip_rows ? a.p.out_h - ye : ty0;
        for (int q = 0; q < kRowsPerLane; ++q) {
            const int y = ty0 + ty + 4 * q;
            if (y < ye && x >= xa && x < xb) {
                int rgb[3];
                uint16_t out[3];
                rgb_of(y, x, rgb);
                mosaic::colour(M, rgb, out);
                uint16_t* o = s_out + tx * kTurnPitch + 3 * (flip_rows ? ye - 1 - y : y - ty0);
                o[0] = out[0], o[1] = out[1], o[2] = out[2];
            }
        }
        __syncthreads();
        uint16_t* dst = static_cast<uint16_t*>(a.dst);
        for (int j = ty; j < kTW; j += 4) {  // (the same for all 64 lanes of a wave)
            const int xj = tx0 + j;
            if (xj < xa || xj >= xb) continue;
            const int r = flip_cols ? a.p.out_w - 1 - xj : xj;
            store_segment(dst + ((long long)r * a.p.out_h + c0) * 3, s_out + j * kTurnPitch, 3 * (ye - ty0), tx);
        }
    } else if constexpr (Cls == kMirrored) {
        // The upright walk below with two changes (the window is the frame: x0 = 0, x1 = out_w, dst_y0 = 0).  Row y of D is row
        // out_h - 1 - y of O with bit 2: the segment pointer walks upward.  With bit 1 the tile's columns [xa, xb) are O's
        // [out_w - xb, out_w - xa), and a lane writes its pixel to the mirrored slot of the row buffer.
        const bool flip_rows = a.orientation & orient::kRows, flip_cols = a.orientation & orient::kCols;
        const long long row_elems = 3LL * a.p.out_w, step = flip_rows ? -4 * row_elems : 4 * row_elems;
        const int slot = flip_cols ? xb - 1 - x : x - xa;
        uint16_t* seg = static_cast<uint16_t*>(a.dst) + (flip_rows ? a.p.out_h - 1 - (ty0 + ty) : ty0 + ty) * row_elems +
                        3 * (flip_cols ? a.p.out_w - xb : xa);
        for (int q = 0; q < kRowsPerLane; ++q, seg += step) {
            const int y = ty0 + ty + 4 * q;  // (the same for all 64 lanes of a wave)
            if (y < a.y1 && x >= xa && x < xb) {
                int rgb[3];
                uint16_t out[3];
                rgb_of(y, x, rgb);
                mosaic::colour(M, rgb, out);
                uint16_t* o = s_out[ty] + 3 * slot;
                o[0] = out[0], o[1] = out[1], o[2] = out[2];
            }
            __syncthreads();
            if (y < a.y1) store_segment(seg, s_out[ty], n, tx);
            __syncthreads();
        }
    } else {
        // the wave's row segment, n contiguous elements of dst: that of its first row, then four rows on per step (one 64-bit product
        // here, none per row)
        const long long row_elems = 3LL * (a.x1 - a.x0);
        OutT<F32>* seg = static_cast<OutT<F32>*>(a.dst) + (ty0 + ty - a.dst_y0) * row_elems + 3 * (xa - a.x0);
        for (int q = 0; q < kRowsPerLane; ++q, seg += 4 * row_elems) {
            const int y = ty0 + ty + 4 * q;  // (the same for all 64 lanes of a wave)
            if (y < a.y1 && x >= xa && x < xb) {
                int rgb[3];
                uint16_t out[3];
                rgb_of(y, x, rgb);
                mosaic::colour(M, rgb, out);
                OutT<F32>* o = s_out[ty] + 3 * (x - xa);
                o[0] = finish_sample<F32>(a, out[0]), o[1] = finish_sample<F32>(a, out[1]), o[2] = finish_sample<F32>(a, out[2]);
            }
            __syncthreads();
            if (y < a.y1) store_segment(seg, s_out[ty], n, tx);
            __syncthreads();
        }
    }
}

// The full size.  LDS: the three planes of I_0, and behind them one range that first holds the staged samples and the auxiliary
// plane (dead once the planes exist) and then the second red and blue planes and the epilogue's buffer.
template <typename Pattern, bool F32, int Cls = kUpright>
__global__ __launch_bounds__(256) void mosaic_median_full_kernel(const MedianArgs<typename Pattern::Params> ma) {
    static_assert(Cls == kUpright || !F32, "the float epilogue is upright");
    using Aux = typename Pattern::Aux;
    constexpr int kReachY = Pattern::kReachY + kMedN, kApronX = Pattern::kApronX + kMedN;  // of the cap; a call loads what its n reaches
    constexpr int kSW = kTW + 2 * kApronX, kSH = kTH + 2 * kReachY, kAW = kMedW + 2, kAH = kMedH + 2, kPlane = kMedH * kMedW;
    using OutBuffer = std::conditional_t<Cls == kTurned, uint16_t[kTW * kTurnPitch], OutT<F32>[4][3 * kTW]>;
    constexpr int kSamplesBytes = (kSH * kSW * 2 + 15) / 16 * 16, kStageBytes = kSamplesBytes + kAH * kAW * (int)sizeof(Aux);
    constexpr int kLateBytes = 2 * kPlane * 2 + (int)sizeof(OutBuffer);
    static_assert(kSW % 2 == 0 && (kPlane * 2) % 16 == 0, "pairs at even columns; 16-byte aligned planes and buffer");
    __shared__ typename Pattern::Params s_p;  // (no use of it, and so no LDS, unless the pattern keeps its params there)
    __shared__ __align__(16) uint16_t s_i0[3 * kPlane];
    __shared__ __align__(16) unsigned char s_u[kStageBytes > kLateBytes ? kStageBytes : kLateBytes];
    uint16_t* s_s = reinterpret_cast<uint16_t*>(s_u);
    Aux* s_a = reinterpret_cast<Aux*>(s_u + kSamplesBytes);
    uint16_t* s_i1 = reinterpret_cast<uint16_t*>(s_u);
    OutBuffer& s_out = *reinterpret_cast<OutBuffer*>(s_u + 2 * kPlane * 2);
    const MedianPlanes pl{s_i0, s_i0 + kPlane, s_i0 + 2 * kPlane, s_i1, s_i1 + kPlane};

    const MosaicArgs<typename Pattern::Params>& a = ma.m;
    const int n = ma.passes;
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * 64 + tx;
    const int tx0 = (a.x0 / kTW + (int)blockIdx.x) * kTW, ty0 = a.y0 + blockIdx.y * kTH;
    if constexpr (Pattern::kParamsInLds) {
        stage_params(a, s_p, tid);
        __syncthreads();
    }
    const typename Pattern::Params& p = params_of<Pattern>(a, s_p);
    // the block's rectangle of D, and the rows and columns of I_0 it needs: n rings more, inside the frame
    const int ya = ty0, yb = ty0 + kTH < a.y1 ? ty0 + kTH : a.y1;
    const int xa = tx0 > a.x0 ? tx0 : a.x0, xb = tx0 + kTW < a.x1 ? tx0 + kTW : a.x1;
    const int iy0 = ya - n > 0 ? ya - n : 0, iy1 = yb + n < a.H ? yb + n : a.H, ix0 = xa - n > 0 ? xa - n : 0, ix1 = xb + n < a.W ? xb + n : a.W;
    // the samples those pixels read (the entry point has checked that the source window holds the rows)
    const int ry0 = iy0 - Pattern::kReachY > 0 ? iy0 - Pattern::kReachY : 0, ry1 = iy1 + Pattern::kReachY < a.H ? iy1 + Pattern::kReachY : a.H;

    for (int i = tid; i < kSH * (kSW / 2); i += 256) {
        const int r = i / (kSW / 2), c = 2 * (i % (kSW / 2));
        const int y = ty0 - kReachY + r, x = tx0 - kApronX + c;  // (x is even: the tile origin, the apron and the cap are)
        int s0 = 0, s1 = 0;
        if (y >= ry0 && y < ry1) load_pair<Pattern>(a, p, y, x, s0, s1);
        s_s[r * kSW + c] = (uint16_t)s0, s_s[r * kSW + c + 1] = (uint16_t)s1;
    }
    __syncthreads();

    const Tile<uint16_t, kSW> S{s_s, ty0 - kReachY, tx0 - kApronX};
    // the auxiliary plane where those pixels read it: one sample around them, inside the pattern's ring
    constexpr int kRing = Pattern::kAuxRing;
    const int ay0 = iy0 - 1 > kRing ? iy0 - 1 : kRing, ay1 = iy1 + 1 < a.H - kRing ? iy1 + 1 : a.H - kRing;
    const int ax0 = ix0 - 1 > kRing ? ix0 - 1 : kRing, ax1 = ix1 + 1 < a.W - kRing ? ix1 + 1 : a.W - kRing;
    for (int i = tid; i < kAH * kAW; i += 256) {
        const int r = i / kAW, c = i % kAW;
        const int y = ty0 - kMedN - 1 + r, x = tx0 - kMedN - 1 + c;
        int v = 0;
        if (y >= ay0 && y < ay1 && x >= ax0 && x < ax1) v = Pattern::aux_at(p, S, a.H, a.W, y, x);
        s_a[i] = (Aux)v;
    }
    __syncthreads();

    const Tile<Aux, kAW> A{s_a, ty0 - kMedN - 1, tx0 - kMedN - 1};
    const int y_org = ty0 - kMedN, x_org = tx0 - kMedN;
    for (int i = tid; i < kPlane; i += 256) {  // I_0: pixel_rgb once per pixel of the region
        const int y = y_org + i / kMedW, x = x_org + i % kMedW;
        if (y < iy0 || y >= iy1 || x < ix0 || x >= ix1) continue;
        int rgb[3];
        Pattern::pixel_rgb(p, S, A, a.H, a.W, y, x, rgb);
        pl.r0[i] = (uint16_t)rgb[0], pl.g[i] = (uint16_t)rgb[1], pl.b0[i] = (uint16_t)rgb[2];
    }
    const int last = median_passes(pl, y_org, x_org, ya, yb, xa, xb, n, a.H, a.W, tid);  // (full size: D has the mosaic's sides)

    const Tile<uint16_t, kMedW> R{pl.r(last), y_org, x_org}, G{pl.g, y_org, x_org}, B{pl.b(last), y_org, x_org};
    leave_tile<F32, Cls>(a, p.M, s_out, tx0, ty0, [&](int y, int x, int (&rgb)[3]) {
        rgb[0] = R(y, x), rgb[1] = G(y, x), rgb[2] = B(y, x);
        if (a.clip) mosaic::blend_pixel(rgb, a.clip);
    });
}

// The reduced form: the same region from reduced_rgb (each lane loads its cells itself), the same passes; a lane then stores its
// pixels as mosaic_reduced_kernel does.  Tiles are anchored to the call's rectangle.
template <typename Pattern, bool F32, bool Oriented = false>
__global__ __launch_bounds__(256) void mosaic_median_reduced_kernel(const MedianArgs<typename Pattern::Params> ma) {
    constexpr int kPlane = kMedH * kMedW;
    __shared__ typename Pattern::Params s_p;  // (as above)
    __shared__ __align__(16) uint16_t s_i[5 * kPlane];
    const MedianPlanes pl{s_i, s_i + kPlane, s_i + 2 * kPlane, s_i + 3 * kPlane, s_i + 4 * kPlane};
    const MosaicArgs<typename Pattern::Params>& a = ma.m;
    const int n = ma.passes;
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * 64 + tx;
    if constexpr (Pattern::kParamsInLds) {
        stage_params(a, s_p, tid);
        __syncthreads();
    }
    const typename Pattern::Params& p = params_of<Pattern>(a, s_p);
    const int out_h = a.p.out_h, out_w = a.p.out_w;
    const int xa = a.x0 + blockIdx.x * kTW, ya = a.y0 + blockIdx.y * kTH;
    const int xb = xa + kTW < a.x1 ? xa + kTW : a.x1, yb = ya + kTH < a.y1 ? ya + kTH : a.y1;
    const int iy0 = ya - n > 0 ? ya - n : 0, iy1 = yb + n < out_h ? yb + n : out_h, ix0 = xa - n > 0 ? xa - n : 0, ix1 = xb + n < out_w ? xb + n : out_w;
    const int y_org = ya - kMedN, x_org = xa - kMedN;
    for (int i = tid; i < kPlane; i += 256) {
        const int y = y_org + i / kMedW, x = x_org + i % kMedW;
        if (y < iy0 || y >= iy1 || x < ix0 || x >= ix1) continue;
        int rgb[3];
        Pattern::reduced_rgb(a, p, y, x, rgb);
        pl.r0[i] = (uint16_t)rgb[0], pl.g[i] = (uint16_t)rgb[1], pl.b0[i] = (uint16_t)rgb[2];
    }
    const int last = median_passes(pl, y_org, x_org, ya, yb, xa, xb, n, out_h, out_w, tid);

    const Tile<uint16_t, kMedW> R{pl.r(last), y_org, x_org}, G{pl.g, y_org, x_org}, B{pl.b(last), y_org, x_org};
    const int x = xa + tx;
    if (x >= xb) return;  // (no barrier below)
    for (int y = ya + ty; y < yb; y += 4) {
        int rgb[3] = {R(y, x), G(y, x), B(y, x)};
        uint16_t out[3];
        if (a.clip) mosaic::blend_pixel(rgb, a.clip);
        mosaic::colour(p.M, rgb, out);
        OutT<F32>* d;
        if constexpr (Oriented) {
            static_assert(!F32, "the float epilogue is upright");
            int r, c;
            orient::from_frame(a.orientation, out_h, out_w, y, x, r, c);
            d = static_cast<OutT<F32>*>(a.dst) + ((long long)r * orient::cols(a.orientation, out_h, out_w) + c) * 3;
        } else {
            d = static_cast<OutT<F32>*>(a.dst) + ((long long)(y - a.dst_y0) * (a.x1 - a.x0) + (x - a.x0)) * 3;
        }
        d[0] = finish_sample<F32>(a, out[0]), d[1] = finish_sample<F32>(a, out[1]), d[2] = finish_sample<F32>(a, out[2]);
    }
}

// What an entry point passes to mosaic_rows: the head and the tail all eleven share, in the header's order, then by name what it alone
// takes.  The form says which of clip and passes it has: the blend form a clip inside [1, 65535]; the median form its passes n and a
// clip that may be 0 (no Blend), and its rows of D read I_0 n rows further.
enum class MosaicForm { kPlain, kBlend, kMedian };
struct MosaicCall {
    const char* what;  // names the entry point in messages
    const uint16_t* src_rows;  // the source window: mosaic rows [src_gy0, src_gy0 + src_nrows), src_pitch samples apart
    int src_gy0, src_nrows;
    int64_t src_pitch;
    int H, W;
    void* dst;
    int y0, y1;  // rows of the window, [y0, y1)
    void* stream;
    MosaicForm form = MosaicForm::kPlain;
    int orientation = 0;  // not 0 (uint16, no window): [y0, y1) are rows of O, dst is O, the launch walks orient::rect_of's rectangle of D
    int clip = 0, passes = 0;  // (0 where the form has none)
    const int* window = nullptr;  // (row0, col0, rows, cols) of the demosaiced frame: what dst holds (none: all of it)
    float divisor = 1.f, factor = 1.f;  // the float epilogue's
};

// An entry point: the checks, then one launch.
template <typename Pattern, bool F32>
int mosaic_rows(r2f_ctx* ctx, const typename Pattern::Params* params, const MosaicCall& c) {
    constexpr int kMaxSide = 1 << 17;  // (the reduced grid has a block per four rows; indices go through long long)
    constexpr int kMin = Pattern::kMinSide, kReduction = Pattern::kReduction, kReachY = Pattern::kReachY;
    const char* what = c.what;
    const int H = c.H, W = c.W, y0 = c.y0, y1 = c.y1, orientation = c.orientation, clip = c.clip, passes = c.passes;
    const int* window = c.window;
    const bool blend = c.form == MosaicForm::kBlend, median = c.form == MosaicForm::kMedian;
    if (!c.src_rows || !params || !c.dst || H < kMin || W < kMin || H > kMaxSide || W > kMaxSide || c.src_pitch < W || c.src_gy0 < 0 ||
        c.src_nrows < 0)
        return fail(ctx, R2F_EINVAL, "%s: a mosaic of at least %d x %d samples, a pitch of at least W and a source window are required", what,
                    kMin, kMin);
    const typename Pattern::Params& p = *params;
    if (const int rc = Pattern::check_params(ctx, what, p, H, W)) return rc;
    const bool reduced = Pattern::reduced(p);
    if (p.out_h != (reduced ? H / kReduction : H) || p.out_w != (reduced ? W / kReduction : W))
        return fail(ctx, R2F_EINVAL, "%s: the params are those of another frame size (%s)", what, Pattern::kPlanner);
    if (!orient::valid(orientation) || (orientation && (F32 || window)))
        return fail(ctx, R2F_EINVAL, "%s: orientation %d is not one of 0 .. 7 (LibRaw's sizes.flip bits)", what, orientation);
    if (blend && (clip < 1 || clip > 65535)) return fail(ctx, R2F_EINVAL, "%s: clip %d is not inside [1, 65535]", what, clip);
    if (median && (clip < 0 || clip > 65535)) return fail(ctx, R2F_EINVAL, "%s: clip %d is neither 0 (no Blend) nor inside [1, 65535]", what, clip);
    if (median && (passes < 1 || passes > R2F_MEDIAN_MAX_PASSES))
        return fail(ctx, R2F_EINVAL, "%s: passes %d is not inside [1, R2F_MEDIAN_MAX_PASSES = %d] (LibRaw's med_passes)", what, passes,
                    R2F_MEDIAN_MAX_PASSES);
    const int frame_rows = orient::rows(orientation, p.out_h, p.out_w);  // (an oriented call has no window: dst is all of O)
    const int row0 = window ? window[0] : 0, col0 = window ? window[1] : 0, rows = window ? window[2] : frame_rows,
              cols = window ? window[3] : p.out_w;
    if (row0 < 0 || col0 < 0 || rows <= 0 || cols <= 0 || rows > frame_rows - row0 || cols > p.out_w - col0)
        return fail(ctx, R2F_EINVAL, "%s: the window (%d, %d, %d, %d) is empty or not inside the %d x %d frame", what, row0, col0, rows, cols,
                    p.out_h, p.out_w);
    if (y0 < 0 || y1 > rows || y0 > y1) return fail(ctx, R2F_EINVAL, "%s: rows [%d, %d) not inside the output's [0, %d)", what, y0, y1, rows);
    if (F32 && (!(c.divisor > 0.f) || (reinterpret_cast<uintptr_t>(c.dst) & 3u)))
        return fail(ctx, R2F_EINVAL, "%s: a positive divisor and a 4-byte aligned destination are required", what);
    if (y0 == y1) return R2F_OK;
    // the rectangle of the demosaiced frame this call takes: the window's rows [y0, y1) over its columns, or what O's rows hold
    const orient::Rect d = orientation ? orient::rect_of(orientation, p.out_h, p.out_w, y0, y1) : orient::Rect{row0 + y0, row0 + y1, col0, col0 + cols};
    // the rows of D whose I_0 it reads: its own, and with step M `passes` more either side, inside the frame
    const orient::Rect read{d.y0 - passes > 0 ? d.y0 - passes : 0, d.y1 + passes < p.out_h ? d.y1 + passes : p.out_h, d.x0, d.x1};
    int lo, hi;
    orient::source_rows(orientation, read, H, kReachY, reduced ? kReduction : 0, lo, hi);
    if (lo < c.src_gy0 || (long long)hi > (long long)c.src_gy0 + c.src_nrows)
        return fail(ctx, R2F_EINVAL, "%s: rows [%d, %d) read mosaic rows [%d, %d), the source window holds [%d, %lld)", what, y0, y1, lo, hi,
                    c.src_gy0, (long long)c.src_gy0 + c.src_nrows);
    const int wide = ((reinterpret_cast<uintptr_t>(c.src_rows) & 3u) == 0 && c.src_pitch % 2 == 0) ? 1 : 0;
    const MosaicArgs<typename Pattern::Params> a{c.src_rows, c.src_gy0, (long long)c.src_pitch, H, W, p, c.dst, d.y0, d.y1, wide,
                                                 orientation ? 0 : row0, d.x0, d.x1, c.divisor, c.factor, orientation, clip};
    hipStream_t s = static_cast<hipStream_t>(c.stream);
    const dim3 reduced_grid((d.x1 - d.x0 + 63) / 64, (d.y1 - d.y0 + 3) / 4);
    // (the whole frame: ceil(W / 64) tiles from column 0)
    const dim3 full_grid((d.x1 - 1) / kTW - d.x0 / kTW + 1, (d.y1 - d.y0 + kTH - 1) / kTH);
    const dim3 tiles((d.x1 - d.x0 + kTW - 1) / kTW, full_grid.y), block(64, 4);  // (the median reduced form's: anchored to the rectangle)
    // The choice among reduced, turned, mirrored and upright, once for the three forms (the reduced kernels know oriented or not).
    auto launch = [&](auto cls) {
        constexpr int Cls = decltype(cls)::value;
        constexpr bool Oriented = Cls != kUpright;
        if (median)
            launch_k(reduced ? mosaic_median_reduced_kernel<Pattern, F32, Oriented> : mosaic_median_full_kernel<Pattern, F32, Cls>,
                     reduced ? tiles : full_grid, block, 0, s, MedianArgs<typename Pattern::Params>{a, passes});
        else if (blend)
            launch_k(reduced ? mosaic_reduced_kernel<Pattern, F32, Oriented, true> : mosaic_full_kernel<Pattern, F32, Cls, true>,
                     reduced ? reduced_grid : full_grid, block, 0, s, a);
        else
            launch_k(reduced ? mosaic_reduced_kernel<Pattern, F32, Oriented, false> : mosaic_full_kernel<Pattern, F32, Cls, false>,
                     reduced ? reduced_grid : full_grid, block, 0, s, a);
    };
    if constexpr (F32)  // (upright: the float epilogue has no oriented kernels, and the checks have refused an orientation)
        launch(std::integral_constant<int, kUpright>{});
    else if (orientation & orient::kSwap)
        launch(std::integral_constant<int, kTurned>{});
    else if (orientation)
        launch(std::integral_constant<int, kMirrored>{});
    else
        launch(std::integral_constant<int, kUpright>{});
    R2F_HIP(ctx, take_launch_status());
    return R2F_OK;
}

}  // namespace
}  // namespace r2f
