// r2f_lens.hip -- the lens step in front of the render path, with its three entry points (include/r2f.h) below its four kernels:
//   lens_correct                  radial map, cv2.remap(INTER_LANCZOS4, zero border), clamp, vignetting gain
//   lens_correct_tca              the same with red and blue sampling at coordinates of their own
//   lens_correct_projected<kTca>  the fisheye-to-rectilinear step in front of the map, without or with a TCA record
// The arithmetic is r2f_lens_math.h's (the text the CPU check programs compile), the profile's planner r2f_lens_plan.cpp.  The
// kernels differ in what a lane keeps between its two passes and in when a block stages (each kernel's comment says why that shape);
// what a block stages, and how a lane samples it, is one skeleton, stated once ahead of them.  None of this runs in a timed step.
#include <climits>

#include "r2f_ctx.h"
#include "r2f_lens_math.h"

using namespace r2f;

namespace r2f {

// ------------------------------------------------------------------------------ the staging skeleton
// effects.lens_correction (effects.py:22-43) from caller-supplied numbers; the definition is in include/r2f.h.  Lanes along x, four
// output rows per lane; the 32 x 8 phase table sits in LDS (1 KiB, one float per thread to fill).
// A block of 256 threads makes a 64 x 16 tile (four rows per lane), finds the box of source texels its taps touch,
// and -- when the box fits kLensBoxTexels -- copies it into LDS once (a texel outside the frame as 0, which is what such a tap
// reads), so that a texel crosses the memory system once per block instead of once per tap.  The sums are sample64's over another
// view: the same samples in the same order, so the result does not depend on whether a block staged.  A block whose box
// does not fit (a strong magnification: scale well below 1) gathers its taps from global memory.  Against one lane per pixel
// gathering every tap from global memory: 5.0 instead of 7.7 ms at 100 MP; two or eight rows per lane and an interleaved float4
// box were slower (profiles/r15_lens_correct.txt).
// Three things are written out in the kernels and not shared, because as a shared piece each moved a kernel's registers (hipcc -O3,
// gfx950; profiles/r29_lens_skeleton_codeobj_diff.txt has the numbers the kernels are held to):
//   - the three-channel sampling body (sample64 staged or global, three finish) in lens_correct_kernel and the projected kernel
//     without a record: as one helper it took them from 253 to 246 and 245 VGPRs, as a helper for the sums alone the latter to 255
//     (fewer registers at the same two waves are no cost, but the kernels are held to the parent's numbers exactly, and nobody has
//     timed the 246-register form);
//   - channel_coord and split_phase ahead of lens_sample_channel: inside it, lens_correct_tca_kernel went from 145 to 147 VGPRs;
//   - split_phase and add() inside lens_extent_channels: as a helper of their own, that kernel spilled 23 SGPRs for 21.
// And the projected kernel keeps its prologue and its extent pass written out: over lens_prologue, LensExtent and
// lens_extent_channels its registers stayed, but beside the parent's build in one process its form with a TCA record ran 1.01 x the
// parent's time at 24 and 100 MP in every round, where two copies of one build differ by 0.4 %, and with them written out 0.99 x
// (profiles/r29_lens_skeleton_bench.txt, the second and third part).
struct LensArgs {
    const void* in;
    int in_layout, H, W;
    DevPlanes dst;
    int out_h, out_w, oy, ox;
    r2f_lens_params p;
    const float* table;  // 32 x 8, device
};

constexpr int kLensRows = 4;            // rows per lane
constexpr int kLensBoxTexels = 3072;    // 36 KiB of LDS for three planes: 71 x 23 texels for an undistorted tile

// The two places a tap reads from, each in sample64's call shape (three channels of a texel) and sample64_channel's (one).
struct LensSource {
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
    __device__ __forceinline__ float operator()(int ch, int y, int x) const {
        if (in_layout == R2F_LAYOUT_CHW) return src[(long long)ch * H * W + (long long)y * W + x];
        return src[((long long)y * W + x) * (in_layout == R2F_LAYOUT_HWC4 ? 4 : 3) + ch];
    }
};

struct LensBoxView {
    const float* box;  // [3][kLensBoxTexels], rows bw apart
    int x0, y0, bw;
    __device__ __forceinline__ void operator()(int y, int x, float (&v)[3]) const {
        const int o = (y - y0) * bw + (x - x0);
        v[0] = box[o], v[1] = box[kLensBoxTexels + o], v[2] = box[2 * kLensBoxTexels + o];
    }
    __device__ __forceinline__ float operator()(int ch, int y, int x) const { return box[ch * kLensBoxTexels + (y - y0) * bw + (x - x0)]; }
};

__device__ __forceinline__ LensSource lens_source(const LensArgs& a) { return LensSource{static_cast<const float*>(a.in), a.in_layout, a.H, a.W}; }

// The block prologue: the phase table into LDS and the extent quadruple (min ix, max ix, min iy, max iy) reset; ends in a barrier.
__device__ __forceinline__ void lens_prologue(const LensArgs& a, float* table, int* ext, int tid) {
    table[tid] = a.table[tid];
    if (tid < 4) ext[tid] = (tid & 1) ? INT_MIN : INT_MAX;
    __syncthreads();
}

// What one lane's inside pixels touch, and its fold into a quadruple of the block.
struct LensExtent {
    int lo_x = INT_MAX, hi_x = INT_MIN, lo_y = INT_MAX, hi_y = INT_MIN;
    __device__ __forceinline__ void add(int ix, int iy) { lo_x = min(lo_x, ix), hi_x = max(hi_x, ix), lo_y = min(lo_y, iy), hi_y = max(hi_y, iy); }
    __device__ __forceinline__ void fold(int* ext) const {
        if (lo_x <= hi_x) {
            atomicMin(&ext[0], lo_x), atomicMax(&ext[1], hi_x);
            atomicMin(&ext[2], lo_y), atomicMax(&ext[3], hi_y);
        }
    }
};

// The per-channel extent pass: the three channels' coordinates at one offset.
__device__ __forceinline__ void lens_extent_channels(const LensArgs& a, const r2f_lens_tca_params& tca, float ox, float oy, LensExtent& e) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float sx, sy;
        lens::channel_coord(a.p, tca, ch, ox, oy, sx, sy);
        int ix, iy, fx, fy;
        if (!lens::split_phase(sx, a.W, ix, fx) || !lens::split_phase(sy, a.H, iy, fy)) continue;
        e.add(ix, iy);
    }
}

// The box of an extent quadruple: the taps of index i are i - 3 .. i + 4.  `any`: some pixel sampled; `staged`: the box fits the LDS.
// (ix, iy lie in [-4, n + 2] (split_phase), so the extents are small ints and their products cannot overflow)
struct LensBox {
    int x0, y0, bw, bh;
    bool any, staged;
};

__device__ __forceinline__ LensBox lens_box(int lo_x, int hi_x, int lo_y, int hi_y) {
    LensBox b;
    b.any = lo_x <= hi_x;
    b.x0 = lo_x - 3, b.y0 = lo_y - 3;
    b.bw = b.any ? hi_x + 4 - b.x0 + 1 : 0, b.bh = b.any ? hi_y + 4 - b.y0 + 1 : 0;
    b.staged = b.any && (long long)b.bw * b.bh <= kLensBoxTexels;
    return b;
}

// The box fill of a staged block: three planes kLensBoxTexels apart, a texel outside the frame as 0.  The caller's barrier follows.
__device__ __forceinline__ void lens_fill_box(const LensArgs& a, const LensBox& b, float* box, int tid) {
    if (!b.staged) return;
    const LensSource global = lens_source(a);
    for (int i = tid; i < b.bw * b.bh; i += 256) {
        const int y = b.y0 + i / b.bw, x = b.x0 + i % b.bw;
        float v[3] = {0.f, 0.f, 0.f};
        if (y >= 0 && y < a.H && x >= 0 && x < a.W) global(y, x, v);
        box[i] = v[0], box[kLensBoxTexels + i] = v[1], box[2 * kLensBoxTexels + i] = v[2];
    }
}

__device__ __forceinline__ LensBoxView lens_box_view(const float* box, const LensBox& b) { return LensBoxView{box, b.x0, b.y0, b.bw}; }

// The per-channel sampling body: indices and phases of channel ch's coordinate -> its finished value.
__device__ __forceinline__ float lens_sample_channel(const LensArgs& a, const float* table, const float* box, const LensBox& b, int ch, int ix, int iy,
                                                     int fx, int fy, float ddx, float ddy) {
    const float *wx = table + fx * lens::kTaps, *wy = table + fy * lens::kTaps;
    const float acc = b.staged ? lens::sample64_channel(lens_box_view(box, b), ch, a.H, a.W, ix, iy, wx, wy)
                               : lens::sample64_channel(lens_source(a), ch, a.H, a.W, ix, iy, wx, wy);
    return lens::finish(a.p, acc, ddx, ddy);
}

// Output pixel (dy, dx) of the window in plane 0; the other planes are plane_stride apart.
__device__ __forceinline__ float* lens_dst(const LensArgs& a, int dy, int dx) { return a.dst.data + (long long)(dy - a.dst.gy0) * a.out_w + dx; }

__device__ __forceinline__ void lens_store3(const LensArgs& a, int dy, int dx, const float (&v)[3]) {
    float* p0 = lens_dst(a, dy, dx);
    p0[0] = v[0];
    p0[a.dst.plane_stride] = v[1];
    p0[2 * a.dst.plane_stride] = v[2];
}

// ------------------------------------------------------------------------------ lens correction (pre-path)
// r2f_lens_correct: one coordinate per pixel.  The four rows of a lane are unrolled copies, and their indices, phases and ddx / ddy
// stay in registers between the extent pass and the sampling pass.
__global__ __launch_bounds__(256) void lens_correct_kernel(const LensArgs a) {
    __shared__ float table[lens::kPhases * lens::kTaps];
    __shared__ float box[3 * kLensBoxTexels];
    __shared__ int ext[4];  // over the block's inside pixels
    const int tid = threadIdx.y * 64 + threadIdx.x;
    lens_prologue(a, table, ext, tid);
    const int dx = blockIdx.x * 64 + threadIdx.x, dy0 = blockIdx.y * (4 * kLensRows) + threadIdx.y;
    int ix[kLensRows], iy[kLensRows], ph[kLensRows];  // ph: fx | fy << 8, or -1 for a pixel that samples nothing
    float ddx[kLensRows], ddy[kLensRows];
    LensExtent e;
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
        e.add(ix[r], iy[r]);
    }
    e.fold(ext);
    __syncthreads();
    // (block-uniform from here: every thread reads the same four words)
    const LensBox b = lens_box(ext[0], ext[1], ext[2], ext[3]);
    lens_fill_box(a, b, box, tid);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kLensRows; ++r) {
        const int dy = dy0 + 4 * r;
        if (dx >= a.out_w || dy >= a.out_h) continue;
        float v[3] = {0.f, 0.f, 0.f};
        if (ph[r] >= 0) {
            float acc[3];
            const float *wx = table + (ph[r] & 31) * lens::kTaps, *wy = table + (ph[r] >> 8) * lens::kTaps;
            if (b.staged)
                lens::sample64(lens_box_view(box, b), a.H, a.W, ix[r], iy[r], wx, wy, acc);
            else
                lens::sample64(lens_source(a), a.H, a.W, ix[r], iy[r], wx, wy, acc);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = lens::finish(a.p, acc[c], ddx[r], ddy[r]);
        }
        lens_store3(a, dy, dx, v);
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
// The sums are lens::sample64_channel's over either view: results do not depend on whether a block staged.
// The compiler reports (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage) 145 VGPRs, no VGPR spills, no scratch, 21 SGPRs
// spilled into VGPR lanes, 37,904 B of LDS and 3 waves per SIMD, against lens_correct_kernel's 253 VGPRs and 2 waves.  Beside that
// kernel in one process: 1.08 x its time with factors of 1, 1.15 x / 1.23 x at 24 / 100 MP with a poly3 record that parts red and
// blue by up to 12 px at 100 MP, where a tenth of the blocks' unions no longer fit the box (profiles/r25_lens_tca_probe.txt).
struct LensTcaArgs {
    LensArgs lens;
    r2f_lens_tca_params tca;
};

__global__ __launch_bounds__(256) void lens_correct_tca_kernel(const LensTcaArgs t) {
    const LensArgs& a = t.lens;
    __shared__ float table[lens::kPhases * lens::kTaps];
    __shared__ float box[3 * kLensBoxTexels];
    __shared__ int ext[4];  // over the block's inside pixels, all channels
    const int tid = threadIdx.y * 64 + threadIdx.x;
    lens_prologue(a, table, ext, tid);
    const int dx = blockIdx.x * 64 + threadIdx.x, dy0 = blockIdx.y * (4 * kLensRows) + threadIdx.y;
    LensExtent e;
    if (dx < a.out_w) {
#pragma unroll 1
        for (int dy = dy0; dy < min(a.out_h, dy0 + 4 * kLensRows); dy += 4) {
            float ox, oy, ddx, ddy;
            lens::source_offset(a.p, dx + a.ox, dy + a.oy, ox, oy, ddx, ddy);
            lens_extent_channels(a, t.tca, ox, oy, e);
        }
    }
    e.fold(ext);
    __syncthreads();
    // (block-uniform from here: every thread reads the same four words)
    const LensBox b = lens_box(ext[0], ext[1], ext[2], ext[3]);
    lens_fill_box(a, b, box, tid);
    __syncthreads();
    if (dx >= a.out_w) return;  // (no barrier below)
#pragma unroll 1
    for (int dy = dy0; dy < min(a.out_h, dy0 + 4 * kLensRows); dy += 4) {
        float ox, oy, ddx, ddy;
        lens::source_offset(a.p, dx + a.ox, dy + a.oy, ox, oy, ddx, ddy);
        float* p0 = lens_dst(a, dy, dx);
#pragma unroll 1
        for (int ch = 0; ch < 3; ++ch) {
            float sx, sy;
            lens::channel_coord(a.p, t.tca, ch, ox, oy, sx, sy);
            int ix, iy, fx, fy;
            float v = 0.f;
            if (lens::split_phase(sx, a.W, ix, fx) && lens::split_phase(sy, a.H, iy, fy))
                v = lens_sample_channel(a, table, box, b, ch, ix, iy, fx, fy, ddx, ddy);
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
// The sums are lens::sample64's / sample64_channel's over either view in the same order: the result does not depend on the
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
    __shared__ int ext[2][4];  // per half, over its inside pixels, all channels
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
    // (block-uniform from here: every thread reads the same eight words)
    const int un_lo_x = min(ext[0][0], ext[1][0]), un_hi_x = max(ext[0][1], ext[1][1]);
    const int un_lo_y = min(ext[0][2], ext[1][2]), un_hi_y = max(ext[0][3], ext[1][3]);
    const LensBox un_box = lens_box(un_lo_x, un_hi_x, un_lo_y, un_hi_y);
    const bool whole = !un_box.any || un_box.staged;  // (nothing sampled: one pass that stages nothing)
#pragma unroll 1
    for (int pass = 0; pass < (whole ? 1 : 2); ++pass) {
        const LensBox b = lens_box(whole ? un_lo_x : ext[pass][0], whole ? un_hi_x : ext[pass][1], whole ? un_lo_y : ext[pass][2], whole ? un_hi_y : ext[pass][3]);
        const int r_begin = whole ? 0 : pass * kHalfRows, r_end = whole ? kLensRows : (pass + 1) * kHalfRows;
        if (pass) __syncthreads();  // (the first half's lanes are done with the box)
        lens_fill_box(a, b, box, tid);
        __syncthreads();
        if (!col_in) continue;  // (block-uniform trip count: such a lane still meets every barrier)
#pragma unroll 1
        for (int r = r_begin; r < r_end; ++r) {
            const int dy = dy0 + 4 * r;
            if (dy >= a.out_h) break;
            float ox, oy, ddx, ddy;
            lens::source_offset(a.p, t.proj, dx + a.ox, dy + a.oy, ox, oy, ddx, ddy);
            if constexpr (kTca) {
                float* p0 = lens_dst(a, dy, dx);
#pragma unroll 1
                for (int ch = 0; ch < 3; ++ch) {
                    float sx, sy;
                    lens::channel_coord(a.p, t.tca, ch, ox, oy, sx, sy);
                    int ix, iy, fx, fy;
                    float v = 0.f;
                    if (lens::split_phase(sx, a.W, ix, fx) && lens::split_phase(sy, a.H, iy, fy))
                        v = lens_sample_channel(a, table, box, b, ch, ix, iy, fx, fy, ddx, ddy);
                    p0[ch * a.dst.plane_stride] = v;
                }
            } else {
                float sx, sy;
                lens::centre_coord(a.p, ox, oy, sx, sy);
                int ix, iy, fx, fy;
                float v[3] = {0.f, 0.f, 0.f};
                if (lens::split_phase(sx, a.W, ix, fx) && lens::split_phase(sy, a.H, iy, fy)) {
                    float acc[3];
                    const float *wx = table + fx * lens::kTaps, *wy = table + fy * lens::kTaps;
                    if (b.staged)
                        lens::sample64(lens_box_view(box, b), a.H, a.W, ix, iy, wx, wy, acc);
                    else
                        lens::sample64(lens_source(a), a.H, a.W, ix, iy, wx, wy, acc);
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[c] = lens::finish(a.p, acc[c], ddx, ddy);
                }
                lens_store3(a, dy, dx, v);
            }
        }
    }
}

}  // namespace r2f

// =============================================================================== C ABI
// What every lens entry point checks and sets up: the arguments, the rows of `dst`, the phase table on the device -> the kernel's args.
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

// The tail of every lens entry point: `kernel` over the 64 x 16 tiles of the window of `lens` (the LensArgs inside `a`).
template <typename Args>
static int lens_launch(r2f_ctx* ctx, void (*kernel)(Args), const Args& a, const LensArgs& lens, void* stream) {
    launch_k(kernel, lens_grid(lens.out_h, lens.out_w), dim3(64, 4), 0, static_cast<hipStream_t>(stream), a);
    R2F_HIP(ctx, take_launch_status());
    return R2F_OK;
}

extern "C" {

int r2f_lens_correct(r2f_ctx* ctx, const void* in, int in_layout, int H, int W, const r2f_lens_params* params, const r2f_planes* dst,
                     int out_h, int out_w, int oy, int ox, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    LensArgs a;
    const int rc = lens_args(ctx, "lens_correct", in, in_layout, H, W, params, dst, out_h, out_w, oy, ox, &a);
    if (rc) return rc;
    return lens_launch(ctx, lens_correct_kernel, a, a, stream);
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
    return lens_launch(ctx, lens_correct_tca_kernel, a, a.lens, stream);
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
    return lens_launch(ctx, tca_params ? lens_correct_projected_kernel<true> : lens_correct_projected_kernel<false>, a, a.lens, stream);
}

}  // extern "C"
