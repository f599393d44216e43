// r2f_plan.h -- the host-side planners of libr2f_hip.so, free of HIP: everything the host units (r2f_api.hip, r2f_stencil.hip)
// decide on the CPU before they upload a table or launch a kernel (the option table, tap boxes and their device entry lists, every decision of a call of the FFT form (fft_call: window, scratch element, batches and their walk), tile orders,
// LANCZOS4 / Gaussian tables, curve cells, workspace sizes).  Plain C++ so that the same translation unit also builds with
// `g++ -fsanitize=address,undefined` into the fuzz harness of tests/test_plan_sanitizers.py (GPU-side sanitizers are not available on
// this pool; this is the part of the library that can run under one).  Nothing here touches the device.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace r2f {
namespace plan {

// ------------------------------------------------------------------------------------------------ stencil taps
// A stencil as handed to r2f_set_kernel: (kh, kw, kc) row-major floats, kc in {1, 3}; channel c reads plane kc == 1 ? 0 : c.
struct Taps {
    const float* k;
    int kh, kw, kc;
    float at(int i, int j, int c) const { return k[((size_t)i * kw + j) * kc + (kc == 1 ? 0 : c)]; }
};

// Bounding box of channel c's non-zero taps {i_lo, i_hi, j_lo, j_hi}; an all-zero plane keeps its centre tap.
void tap_box(const Taps& t, int c, int box[4]);
// Is channel c a single tap at the anchor (kh / 2, kw / 2)?  (*w = its weight)
bool single_tap_channel(const Taps& t, int c, float* w);
// Channel c's box {i_lo, i_hi, j_lo, j_hi}: odd width >= 9, centred on the anchor column, left-right mirror symmetric bit for bit?
bool mirror_symmetric(const Taps& t, int c, const int box[4]);

// Device form of one channel (mirrors DevStencil's geometry fields; the pointers are filled in by the uploader).
struct StencilGeom {
    int kh = 0, kw = 0, kw_pad = 0, RS = 0, ay = 0, ax = 0, sym = 0;
    int n_phases = 0, n_rowsteps = 0, n_entries = 0, mask_first_or = 0, mask_last_or = 0, max_lds_rows = 0;
};
// The entry list stencil_accumulate<Q> consumes (layout: r2f_device.h, DevStencil).
struct StreamHost {
    std::vector<float> w;
    std::vector<int> rowinfo, phases;  // rowinfo: 4 ints per non-empty row step (+ 2 dummy records); phases: 4 ints per phase + terminator
    int n_phases = 0, n_rowsteps = 0, n_entries = 0, max_lds_rows = 0, mask_first_or = 0, mask_last_or = 0;
};
// Channel c of `t` cropped to `box` (the caller may have widened it to a box common to all channels) for a tile of TW x TH
// outputs, Q rows per lane and an LDS budget in bytes (0 = the whole stencil height in one phase).  allow_sym: pair mirrored taps
// when the channel allows it (force_sym_off overrides a shared-geometry decision).  Returns 0, or -3 (R2F_ETOOLARGE) when a
// single row step does not fit the budget.
int plan_stencil_channel(const Taps& t, int c, const int box[4], bool sym, int Q, int TW, int TH, size_t lds_budget, StencilGeom* g,
                         StreamHost* sh);

constexpr int fixed_ax(int R) { return R < 4 ? R : (R <= 6 ? 6 : (R <= 10 ? 10 : 14)); }  // = fixed_stencil_ax of r2f_device.h
// R if the channels `chans` all fill the same square (2 R + 1)^2 box around the anchor, 1 <= R <= max_r, mirror symmetric, and
// their device geometry `geom[c]` is what stencil_fixed expects; else 0.
int fixed_stencil_radius(const Taps& t, const StencilGeom* geom, const int* chans, int nch, int max_r);
// stencil_fixed<R, Q>'s weight table for the three channels ([(2 R + Q)][R + 1][Q / 2] pairs each); *same: identical tables.
std::vector<float> fixed_stencil_weights(const Taps& t, int R, int Q, bool* same);
// Is every channel's (2 R + 1)^2 box K = u v^T to 6e-7 of its largest tap?  Fills u[c][0 .. 2 R], v[c][0 .. R] (left half).
bool separable_taps(const Taps& t, int R, float u[3][19], float v[3][10]);

// Source rows [lo, hi) a stencil reaching `above` / `below` rows needs for outputs [y0, y1) of an H-row frame (reflect-101): exactly
// the hull of the rows read.  above + below >= 0; either may be negative (a tap box that does not hold the anchor row).
void stencil_source_rows(int y0, int y1, int above, int below, int H, int* lo, int* hi);

// ------------------------------------------------------------------------------------------------ FFT form
struct FftOptions {
    int window = 0;        // columns forced (0 = choose)
    int window_max = 512;  // widest the automatic choice may take
    int window_rows = 0;   // rows forced (0 = choose)
    int batch_mib = 192;   // scratch in flight, MiB (a 256 x 256 complex128 pair = 1 MiB)
    int streams = 2;
    int even = 1;          // equal numbers of launch triples per stream
};
constexpr int kFftMaxTaps = 400;
// Window shape {ny, nx} for a bh x bw tap box on a W x H frame (the one whose three passes move the fewest scratch bytes).
// rows_hint > 0: the rows of THIS call (a row shard) -- the window rows are then chosen for the shard, not for the whole frame.
bool fft_window(const FftOptions& o, int bh, int bw, int W, int H, bool s32, int* ny, int* nx);
struct FftBatches {
    int ny = 0, nx = 0, vy = 0, vx = 0, gx = 0, ntiles = 0, ppc = 0, pairs = 0;
    int nstreams = 1, batch = 0, launches = 0;
    size_t img_bytes = 0, scratch_bytes = 0;
};
// Outputs a window keeps of a bh x bw tap box (the one statement of the rule: fft_window prices with it, fft_batches tiles with it).
inline void fft_valid(int ny, int nx, int bh, int bw, int* vy, int* vx) {
    *vy = ny - bh + 1;
    *vx = (nx - bw + 1) & ~3;  // a multiple of 4: window origins stay 16-byte aligned for the float4 stores of pass 3
}
// Tiling of output rows [y0, y1) x W columns into window pairs and their batches; elem_bytes: 16 (complex128), 8 or 12.
FftBatches fft_batches(const FftOptions& o, int ny, int nx, int bh, int bw, int W, int y0, int y1, int nch, int elem_bytes);

struct Options;
// Every host decision of ONE call of the FFT form (run_stencil_fft), from plain facts: what the device call launches and what
// r2f_plan_fft reports are both read off the FftCall this returns.
struct FftCallIn {
    int bh = 0, bw = 0;  // the group's tap box
    int ay = 0, ax = 0;  // the anchor inside it (kh / 2 - box[0], kw / 2 - box[2]: cv.filter2D's default anchor)
    int nch = 1, which = 0, W = 0, y0 = 0, y1 = 0;
    // the group's channels: any with taps of both signs?  all of unit gain?  all centrally symmetric (centrally_symmetric)?
    bool any_mixed_sign = false, all_unit_gain = false, symmetric = false;
    // the caller: its epilogue, whether it vouches for the exposure-range record (run_stencil's dyn), whether a density curve is set
    int epilogue = 0;
    bool dyn = false, curve_set = false;
    FftOptions fo;
    int fft_s32 = 0, fft_s96 = 0, fft_s96_auto = 0, fft_real = 0, fft_mixed_sign = 0, fft_cols_walk = 0;  // as in Options
    void take_options(const Options& o);
};
struct FftBatch {
    int pair0, npairs, lane;
    size_t scratch_offset;  // bytes into the call's scratch: a lane's batches share one slice of it
};
struct FftCall {
    bool ok = false;  // false: no window shape fits the box under the window options (nothing else is filled in)
    int kreal = 0, oy = 0, ox = 0;  // real spectrum (the box laid out with its anchor on the window origin), and that origin shift
    // scratch element (FftConvArgs::s32): 0 complex128, 1 complex64, 2 the 12-byte element, 3 complex128 or 12 bytes per window
    // pair, chosen on the device (batches are sized for complex128)
    int element = 0;
    int elem_bytes = 16;   // what the batches are sized by
    int timing_offset = 0;  // added to a pass's timing class (kernel_timing: complex64 launches are classes 3-5)
    FftBatches b;           // window, valid outputs, tiling, batches (ny, nx, vy, vx, gx, ntiles, ppc, pairs, nstreams, batch, ...)
    // algorithmic bytes of the three passes PER PAIR: window floats in (2 per pair) + scratch image out; scratch in + valid rows
    // out; valid rows in + valid outputs out.  (The kernel spectrum, 1 MB, stays in L2.)
    double pass_bytes[3] = {0, 0, 0};
    // batch i of b.launches: `batch` pairs from pair i * batch on, dealt to the lanes in turn
    FftBatch batch(int i) const {
        const int p0 = i * b.batch, lane = i % b.nstreams;
        return {p0, b.pairs - p0 < b.batch ? b.pairs - p0 : b.batch, lane, (size_t)lane * b.batch * b.img_bytes};
    }
};
FftCall fft_call(const FftCallIn& in);

// Is every channel of `chans` centrally symmetric bit for bit (k[i][j] == k[bh-1-i][bw-1-j]) inside `box`, an odd x odd box whose
// centre is the anchor (kh / 2, kw / 2)?  Such a box, laid out with its anchor on the window origin, has a real spectrum.
bool centrally_symmetric(const Taps& t, const int* chans, int nch, const int box[4]);
// The zero-padded ny x nx kernel image of channel c's `box`: in the window's top left corner (outputs from row / column 0 on), or,
// wrap = true (a real spectrum), wrapped around the window with the anchor on the origin.
std::vector<float> fft_kernel_image(const Taps& t, int c, const int box[4], int ny, int nx, bool wrap);

// ------------------------------------------------------------------------------------------------ options
// The integer options of r2f_set_option with their defaults.  (Bits `which` of the masks: R2F_KERNEL_HALATION / _MTF / _GRAIN.)
struct Options {
    int fft_window = 0;      // window columns: 0 = the cheapest of 256 / 512 / 1024 per stencil and frame, or one of them forced
    int fft_window_max = 512;  // widest window the automatic choice may take (1024 columns: 9 % fewer window elements for the
                               // 87-tap disc, but the passes run 10-25 % slower per element)
    int fft_window_rows = 0;  // window rows, likewise
    // optional per-launch timing of the FFT passes with events on the launch stream (bench.py's roofline): class 0 / 1 / 2 =
    // pass 1 / 2 / 3; algorithmic bytes are summed alongside
    int timing = 0;
    int fft = 1;             // 1: stencil channels with a large enough kernel take the FFT form
    int fft_min_taps = 400;  // ... "large enough": cropped box of at least this many taps (and at most 200 x 200);
                             // measured crossover with the direct form: 17 x 17 ties, 23 x 23 is 1.5x faster by FFT
    int fft_streams = 2;     // internal streams taking alternate batches (r2f_ctx::Fft)
    int fft_even = 1;        // batches sized so that every internal stream gets the same number of launch triples
    int fft_batch = 192;     // window pairs per launch triple: 192 MB of scratch stay inside the 256 MB Infinity Cache
    // bit `which`: that stencil's FFT scratch images hold complex64 instead of complex128 elements (r2f_fft.hip, sld / sst).
    // Default: the MTF only -- it acts on density, whose values are bounded, so two fp32 roundings of the spectrum cost ~1e-7
    // absolute; the halation acts on linear exposure, where the same roundings are relative to the brightest pixel of the window.
    int fft_s32 = 1 << 1;
    int fft_s96 = 0;  // bit `which`: 12-byte scratch elements (doubles rounded to 48 bits, 2^-37) whatever the frame holds -- A/B
    // 1: the halation's FFT passes choose between complex128 and the 12-byte element ON THE DEVICE, per frame and per WINDOW PAIR,
    // from the range of the exposure samples the pair's windows hold (the record's tiles, filled by the front kernel): the 12-byte
    // element costs a shadow at most 1.46e-11 x (max |x| / shadow) of itself (two roundings at 2^-37; kDynCoefficient adds a
    // factor 1.5) -- which the density curve turns into 0.434 x slope x that; the bound keeps it under three fp32 ulps of a density
    // in [1, 2), what the MTF's complex64 scratch is allowed, and window pairs with a wider range keep complex128 (the stand-in Portra
    // curve: max / shadow <= 6.2e4; the headline's noise frame spans 1.4e5 as a whole, ~2e4 per window: 99 % of its pairs qualify).
    int fft_s96_auto = 1;
    int fft_epi_lds = 1;  // pass 3's epilogue gathers its curve cells from LDS (0: from global memory; A/B)
    // 1: a centrally symmetric tap box (k[i][j] == k[bh-1-i][bw-1-j] bit for bit, anchor at its centre -- every halation disc and
    // |ifft2| MTF kernel the reference builds, effects.py:200-217, :123-143) is laid out with its anchor on the window origin, so its
    // spectrum is real: pass 2 reads 8 instead of 16 bytes of it per element (FftConvArgs::kreal).  0: complex spectra for all (A/B).
    int fft_real = 1;
    int fft_mixed_sign = 1;  // channels with taps of both signs take the float64 FFT form on complex128 scratch whatever their size
    int fft_cols_walk = 1;  // pass 2 of real-spectrum launches as a resident grid walking the launch's pairs (0: one workgroup per pair; A/B)
    int xcd_band = 0;  // tile columns per band of the xcd_remap = 2 order; 0 = auto
    int variant = -1;  // -1 auto
    int xcd_remap = 2;  // 0 = launch order, 1 = one contiguous row-major run of tiles per XCD, 2 = that run walked in column bands
    int ablate = 0;
    int sym = 1;      // use the mirror-symmetric entry form when a channel's taps allow it
    int grain_fixed = 1;  // 0: always the generic entry list (A/B)
    int grain_sep = 1;    // 0: never take the separable form (A/B)
    int grain_xpass_lds = 0;  // 1: the separable form's pass along x through LDS at every R (A/B; 0: in registers up to R = 4)
    int stencil_fixed = 1;
    int front_fast = 1;    // the fused LUT-only pass may take the specialised kernel (r2f_front.hip); 0 = always the generic one (A/B)
    int front_blocks = 6;  // front kernel with the curve in LDS: workgroups per CU in its grid (3 are resident at 48 KB each)
    int lds_kb = 80;  // LDS budget per stencil workgroup; 80 KB -> two workgroups per CU
    int render_graph = 1;
};
// One row per option name: how a value is checked and stored, and what r2f_last_error says when it is refused.
//   Switch: stored as value ? 1 : 0.   Range: a <= value <= b.   OneOf: value among v[0 .. n).   Raw: stored unchecked.
//   Mask: stored as value & a, nothing refused.
enum class OptionKind { Switch, Range, OneOf, Raw, Mask };
struct OptionRow {
    const char* name;
    int Options::*field;
    OptionKind kind;
    int a, b;  // Range: bounds; Mask: a; OneOf: a = n
    int v[4];
    const char* error;
};
constexpr int kNumStencilVariants = 3;  // = r2f_launch.h's (restated for the range of stencil_variant)
const OptionRow* find_option(const char* name);  // nullptr: unknown
bool store_option(Options* o, const OptionRow& row, int value);  // false: refused (row.error), *o untouched

// ------------------------------------------------------------------------------------------------ tables
// Tile order of a gx x gy grid of stencil workgroups: entry i = tile index of linear workgroup id i (XCD-contiguous runs walked
// in bands of tile columns; band = 0: automatic).
std::vector<int> tile_order(int gx, int gy, int band);
// cv::interpolateLanczos4 weights for fractional position x.
void lanczos4_coeffs(float x, float* coeffs8);
int lanczos4_table_u8(int ssize, int dsize, int* ofs, short* coef);
int lanczos4_table_f32(int ssize, int dsize, int* ofs, float* coef);
// gaussian_kernel_1d(2 size + 1, 0.3 ((taps - 1) / 2 - 1) + 0.8) normalised by its float32 pairwise sum (effects.py:421-435).
constexpr int kChromaMaxTaps = 63;
bool chroma_weights(int size, float* w);
// scipy's gaussian kernel for sigma = 3, truncate = 2 (13 taps, doubles).
void burn_weights(double* w13);

// One cell {xp[i], xp[i + 1], fp[i], slope[i]} per interval and channel of a (4, m) curve table; slopes in double like np.interp.
struct CurveCells {
    std::vector<float> cells;  // 3 x (m - 1) x 4
    float x0 = 0, x1 = 0, inv_step = 0, f_first[3] = {0, 0, 0}, f_last[3] = {0, 0, 0};
    int m = 0, near = 0;
};
// 0, or -1 when the table is unusable (m < 2, xp decreasing).
int curve_cells(const float* lut4xm, int m, CurveCells* out);

// Plane sets + burn scratch of r2f_render, in floats.
size_t plane_set_floats(int H, int W);
bool burn_geometry(int burn_cell, int H, int W, int* h_lo, int* w_lo);
size_t workspace_floats(unsigned flags, int burn_cell, int H, int W);

}  // namespace plan
}  // namespace r2f
