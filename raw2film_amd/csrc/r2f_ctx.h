// r2f_ctx.h -- what the host units of the library share (r2f_api.hip, r2f_stencil.hip, r2f_graph.hip, r2f_jpeg_api.hip and the
// entries of r2f_resample.hip, r2f_lens.hip and r2f_post.hip): the
// context, its owned device buffers, the error and device-binding macros, and the functions one unit calls in another.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/r2f.h"
#include "r2f_launch.h"
#include "r2f_plan.h"

namespace r2f {

// How DeviceBuf::reserve replaces an allocation that is too small.
enum class Grow {
    Quiet,           // nothing can be using the old one (first use, or the caller has synchronised already); `generation` stays
    Sync,            // the device is synchronised first; `generation` stays (no captured graph holds the address)
    SyncGeneration,  // ... and `generation` moves: captured launches hold the old address
};

// A device allocation the context owns: freed with it.
struct DeviceBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DeviceBuf() = default;
    DeviceBuf(DeviceBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
    DeviceBuf& operator=(DeviceBuf&& o) noexcept {
        if (this != &o) release(), p = o.p, bytes = o.bytes, o.p = nullptr, o.bytes = 0;
        return *this;
    }
    ~DeviceBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    // At least `n` bytes (contents are not kept when it grows).
    int reserve(r2f_ctx* ctx, size_t n, Grow how);
};

// Host copy of one stencil as handed to r2f_set_kernel, plus its device form per Q.
struct StencilSet {
    bool present = false;
    int kh = 0, kw = 0, kc = 0;
    std::vector<float> host;  // (kh, kw, kc)
    int built_q = 0;          // 0 = device form stale
    int built_tw = 0, built_th = 0;
    size_t built_budget = 0;
    bool built_sym = false;
    bool common_box = false;
    DevStencil dev[3];
    plan::StencilGeom geom[3];  // the host-side geometry dev[] was filled from
    bool mixed_sign[3] = {false, false, false};  // the channel has taps of both signs (set by r2f_set_kernel)
    bool unit_gain[3] = {false, false, false};   // no negative tap and the taps sum to 1 (>= 0.99): an output is no smaller than the
                                                 // smallest sample under the stencil -- what the 12-byte element's guard presumes
    int single_tap_mask = 0;  // channels whose stencil is ONE tap at the anchor (set by r2f_set_kernel: a scan of every tap, which
                              // the per-frame front / range calls of a row shard must not repeat -- 15 us of host time per call)
    DeviceBuf wbuf[3], mbuf[3];
    plan::Taps taps() const { return plan::Taps{host.data(), kh, kw, kc}; }
};

// r2f_render's graph cache (r2f_graph.hip): one entry per (buffers, shape, parameters without the seed).  An entry is rendered
// kernel by kernel the first time the context sees its structure (tables, scratch and spectra get built then), captured on
// `cap_stream` afterwards and replayed on the caller's stream from then on.  Everything is dropped when `generation` moves.
struct RenderGraph {
    const void* in = nullptr;
    int in_layout = 0;
    HwcOut out{};  // which output a frame writes (r2f_render's u8, r2f_render16's u16) is part of its key
    int H = 0, W = 0;
    void* workspace = nullptr;
    r2f_params p{};  // seed zeroed
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipEvent_t done = nullptr;  // recorded behind every launch of `exec`: the executable graph must outlive its last replay
    uint64_t last_use = 0;
    bool never = false;  // a capture of this entry failed: kernel by kernel from now on
    bool dyn_armed = false;  // the captured halation launches choose their scratch element on the device
};
// The LANCZOS4 tables of one geometry on the device, [xofs | yofs | pad to 16 bytes | xcoef | ycoef], kept until another geometry is
// asked for.  Coef is short (r2f_lanczos4_table: the uint8 resize) or float (r2f_lanczos4_table_f32: the uint16 and float32 ones).
struct LanczosTables {
    DeviceBuf buf;
    int key[4] = {0, 0, 0, 0};  // H, W, out_h, out_w
    // Make sure `buf` holds this geometry's tables (a new geometry is an upload: it synchronises and moves `generation`) and hand
    // out where they are.  Defined in r2f_resample.hip, for its three LANCZOS4 entries.
    template <typename Coef>
    int tables(r2f_ctx* ctx, int H, int W, int out_h, int out_w, const int** xofs, const int** yofs, const Coef** xcoef, const Coef** ycoef);
};

// The auto-exposure record of the context (exposure_finish_kernel writes it, decode_u16_auto_kernel reads the factor): 16 bytes.
struct ExposureRecord {
    double stops;
    float factor;
    unsigned pad;
};

struct RenderGraphCache {
    std::vector<RenderGraph> graphs;
    // Executable graphs that left the cache (evicted, or dropped because the generation moved) while a replay of them may still be
    // running: destroyed once their `done` event has completed -- polled at the next r2f_render, no device-wide synchronisation
    // inside a render (a caller cycling through more than 8 buffer sets would otherwise stall every stream of the device per eviction).
    struct Retired {
        hipGraph_t graph;
        hipGraphExec_t exec;
        hipEvent_t done;
    };
    std::vector<Retired> retired;
    uint64_t generation = 0;  // the context's `generation` the entries (and `warm`) belong to
    uint64_t clock = 0;
    RenderGraph warm;         // structure (shape, layout, parameters) of the last frame launched kernel by kernel
    bool warm_valid = false;
    // buffer sets seen on frames launched kernel by kernel (keys only, most recent last, at most 16): an entry is captured the
    // SECOND time its buffers come by -- a caller that hands in fresh buffers every frame never pays for a capture it cannot reuse
    std::vector<RenderGraph> seen;
    hipStream_t cap_stream = nullptr;
    uint64_t replays = 0, captures = 0, eager = 0, dropped = 0;  // r2f_render_stats

    ~RenderGraphCache();
    int find(const RenderGraph& key) const;  // the entry with the key's buffers and structure, or -1
    void note_eager(const RenderGraph& key);  // a frame of this key went kernel by kernel: it is warm, and its buffers are seen
    bool should_capture(const RenderGraph& key, int slot) const;
    int insert(const RenderGraph& key);  // a new entry (the least recently used one leaves when there are 8); its index
    void retire(RenderGraph& g);  // out of service: its executable graph may still be replaying, so it is parked behind `done`
    void drop_all();
    void follow(uint64_t ctx_generation);  // a table, stencil, option or internal buffer moved: frozen pointers are stale
    void reap(bool wait);  // destroy the retired graphs whose last replay has completed (wait = true: all of them -- r2f_destroy)
};

}  // namespace r2f

struct r2f_ctx {
    int device = 0;
    std::string err;
    // Bumped whenever something a captured HIP graph may have frozen changes: a table or stencil upload, a context buffer that
    // was re-allocated (its old address is dangling), the matrix, an option.  r2f_generation() reports it; a caller that replays
    // captured launches (raw2film_amd/sharding.py) re-captures when it moves.
    uint64_t generation = 0;
    r2f::plan::Options opt;  // r2f_set_option
    bool has_matrix = false;
    r2f::Mat3 mat;
    r2f::DeviceBuf lut2d_buf, lut3d_buf, curve_buf, grain_lut_buf;
    r2f::DevLut2D lut2d{nullptr, 0};
    r2f::DevLut3D lut3d{nullptr, 0};
    r2f::DevCurve curve{};
    r2f::DevCurve grain_lut{};
    r2f::StencilSet stencil[3];
    // tile-order tables of the stencil launches (xcd_remap = 2), keyed by the tile grid
    struct TileOrder {
        int gx = 0, gy = 0;
        r2f::DeviceBuf buf;
    } tile_order[4];
    int tile_order_next = 0;
    // FFT form of large stencils (r2f_fft.hip, run_stencil_fft): twiddles, per stencil and channel the kernel spectrum, pass scratch
    // (one spectrum per WINDOW SHAPE: the calls of one frame may differ in it -- a row shard's interior halation and its boundary
    // bands cover different numbers of rows, and the window choice follows the rows of the call -- and must not evict each other)
    struct Fft {
        static constexpr int kShapes = 6;  // {256, 512} rows x {256, 512, 1024} columns
        static int shape_index(int ny, int nx) { return (ny == 512 ? 3 : 0) + (nx == 256 ? 0 : (nx == 512 ? 1 : 2)); }
        r2f::DeviceBuf tw, s1, kimg;
        struct Spectrum {  // of one (stencil, channel, window shape)
            r2f::DeviceBuf buf;
            bool valid = false, real = false;  // built for the stencil's current taps; laid out for a real spectrum
        } spectrum[3][3][kShapes];
        struct Last {  // one (stencil, channel)'s last launch, for r2f_stencil_stats: its window (ny * 4096 + nx), a real spectrum?
            int dims = 0, real = 0;
        } last[3][3];
        void forget(int which, int c) {  // the stencil's taps changed (r2f_set_kernel)
            last[which][c] = Last();
            for (Spectrum& sp : spectrum[which][c]) sp.valid = false;
        }
        // two internal streams take alternate batches (each with its own half of the scratch), so the tail of one launch
        // overlaps the head of the other stream's; fenced against the caller's stream with events
        hipStream_t stream[4] = {nullptr, nullptr, nullptr, nullptr};
        hipEvent_t ev_in = nullptr, ev_out[4] = {nullptr, nullptr, nullptr, nullptr};
        ~Fft();
    } fft;
    int cu_count = 0;  // multiprocessors of the context's device, asked for once (device_cu_count)
    // kernel_timing: the event pairs of the timed launches, [pass + 3 * (complex64 scratch ? 1 : 0)], until r2f_kernel_timing reads them
    std::vector<std::pair<hipEvent_t, hipEvent_t>> timing_ev[6];
    double timing_bytes[6] = {0, 0, 0, 0, 0, 0};
    float curve_slope_max = 0.f;  // max |d density / d log10 exposure| over the density curve's cells (host copy, r2f_set_curve1d)
    bool frame_dyn_armed = false;  // the last whole-frame render's halation launches carried the rule (r2f_frame_exposure_range)
    bool capturing = false;        // r2f_render is capturing render_launches: the frame-block write stays outside the graph
    // one per entry point: the float32 up-scale before the path and the final resize of one process() call differ in geometry
    r2f::LanczosTables lanczos_u8, lanczos_u16, lanczos_f32;
    r2f::DeviceBuf lens_table;  // r2f_lens_correct's 32 x 8 phase table (r2f_lens_phase_table), uploaded on first use
    // the grain stencil as weight pairs for grain_stencil_fixed (small square symmetric kernels), built on first use
    r2f::DeviceBuf grain_fixed_w;
    bool grain_fixed_valid = false;
    int grain_fixed_r = 0, grain_fixed_same = 0;
    // the grain stencil as two 1-D passes when every channel is u v^T to fp32 rounding (ensure_grain_fixed)
    bool grain_sep = false;
    float grain_sep_u[3][19] = {}, grain_sep_v[3][10] = {};
    r2f::DeviceBuf stencil_fixed_w[3];  // the same for the direct stencil kernel (stencil_fixed<R, 4>), per stencil
    bool stencil_fixed_valid[3] = {false, false, false};
    // Per-render values the kernels read through a pointer (FrameParams: the grain seed), so that a captured frame can be
    // replayed with a new seed; written in stream order by write_frame_params ahead of a frame's launches.
    r2f::DeviceBuf frame_buf;
    // The exposure-range record's tile grid (r2f_device.h RangeRecord: 64 x 256 tiles of the GLOBAL frame, {min, max |.|} each) and
    // the per-pair flags fft_decide_kernel derives from it for the halation's FFT passes of the call at hand (one per pair-in-channel)
    r2f::DeviceBuf range_tiles, dyn_flags;
    int tiles_tyn = 0, tiles_txn = 0;
    int dyn_flags_ppc = 0;  // pairs per channel of the last call that chose per pair (r2f_frame_scratch_choice)
    // The auto exposure measured on the device (r2f_exposure_rows / _finish): the fp64 sums of the sampled rows, sized by capacity
    // (ceil(H / 2) doubles of the tallest frame so far; no captured graph reads it: growing it leaves `generation` alone), and the
    // record {stops, factor} r2f_decode_u16_auto reads.  A copy of the record follows every finish into pinned host memory on a
    // stream of the context's own, so that r2f_exposure_result waits for the finish kernel and not for the render queued behind it.
    struct Exposure {
        r2f::DeviceBuf sums, rec;
        int rows_cap = 0;  // sampled rows `sums` holds
        r2f::ExposureRecord* host = nullptr;
        hipStream_t stream = nullptr;
        hipEvent_t done = nullptr;
        bool measured = false;  // a finish has been queued: the record holds (or will hold) a frame's values
        ~Exposure();
    } exposure;
    r2f::RenderGraphCache graphs;  // (retired and reaped by r2f_destroy ahead of the buffers its graphs point into)
    struct Jpeg {
        // r2f_jpeg_encode's scratch (r2f_jpeg_plan.h Scratch): grows to the largest frame encoded so far and stays, so that frames of
        // alternating sizes neither re-allocate nor synchronise (no captured graph reads it: growing it leaves `generation` alone)
        r2f::DeviceBuf scratch;
        // the open row-wise encode (r2f_jpeg_rows_begin): its frame, the next row it takes and where its file goes; the carry (bits
        // and 0xFF bytes so far) stays on the device.  A one-shot encode, a new begin or the frame's last rows end it.
        struct Rows {
            bool open = false;
            int H = 0, W = 0, next_y = 0;
            int sampling = 2, header_len = 0, restart = 0;
            uint8_t* out = nullptr;
            uint64_t* out_len = nullptr;
        } rows;
        r2f::DeviceBuf carry;
        r2f::DeviceBuf freq;  // r2f_jpeg_encode_ex with optimize: the frame's symbol counts, uint64 [4][256]
    } jpeg;
    ~r2f_ctx();  // the timing event pairs nobody read; the members free what they own
};

namespace r2f {

int fail(r2f_ctx* ctx, int code, const char* fmt, ...);

#define R2F_HIP(ctx, expr)                                                                      \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) return fail(ctx, R2F_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// The multiprocessors of the context's device, asked for once: what the resident grids (the FFT's column walk, r2f_mosaic_maximum)
// are sized by.
inline int device_cu_count(r2f_ctx* ctx, int* out) {
    if (!ctx->cu_count) {
        int n = 0;
        R2F_HIP(ctx, hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, ctx->device));
        ctx->cu_count = n > 0 ? n : 256;
    }
    *out = ctx->cu_count;
    return R2F_OK;
}

// Every entry point that touches HIP binds the context's device for the duration of the call and puts the caller's
// current device back on return: two contexts on two GPUs can be driven from one thread (and torch's notion of the current
// device is left alone).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t status = hipSuccess;
    explicit DeviceGuard(int device) {
        // (no hipGetLastError() here: a pending error of another user of the runtime in this process -- PyTorch, RCCL -- is theirs to
        // read; the library clears only what it produced itself, right after an abandoned capture in r2f_render)
        status = hipGetDevice(&prev);
        if (status == hipSuccess && prev != device) {
            status = hipSetDevice(device);
            switched = status == hipSuccess;
        }
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define R2F_GUARD(ctx)                  \
    DeviceGuard guard_((ctx)->device); \
    if (guard_.status != hipSuccess) return fail(ctx, R2F_EHIP, "cannot bind device %d: %s", (ctx)->device, hipGetErrorString(guard_.status))

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool planes_vec_ok(const r2f_planes* pl, int W) { return W % 4 == 0 && aligned16(pl->data) && pl->plane_stride % 4 == 0; }
inline DevPlanes to_dev(const r2f_planes* pl) {
    DevPlanes d;
    d.data = pl->data;
    d.plane_stride = pl->plane_stride;
    d.gy0 = pl->gy0;
    d.rows = pl->rows;
    return d;
}

// r2f_api.hip
int upload(r2f_ctx* ctx, DeviceBuf& buf, const void* host, size_t bytes);
bool planes_overlap(const r2f_planes* a, const r2f_planes* b, int W);
int check_rows(r2f_ctx* ctx, const char* what, const r2f_planes* pl, int lo, int hi);
RangeRecord record_of(const r2f_ctx* ctx);
int ensure_range_tiles(r2f_ctx* ctx, int H_global, int W);
// mode 1: seed + reset of the exposure range (the start of a render); 0: a stage entry's own seed write in the middle of one;
// 2: the range reset alone (a render whose caller keeps the seed resident); 3: the range made unusable (frame_params_kernel).
// Modes 1 and 2 reset the tile grid too.
int write_frame_params(r2f_ctx* ctx, const r2f_params* p, hipStream_t s, int mode);
// r2f_stage_front / r2f_stage_front_split; tracked: r2f_render's front call asks whether the exposure range was recorded
int stage_front_impl(r2f_ctx* ctx, const r2f_params* p, const void* in, int in_layout, int in_gy0, int in_rows, int upto,
                     const r2f_planes* dst, const HwcOut& out, int y0, int y1, int W, int H_global, void* stream,
                     const r2f_planes* finish_dst = nullptr, int* finished_mask = nullptr, bool* tracked = nullptr);
// r2f_stage_tail / r2f_stage_tail16 (r2f_graph.hip's renders call it too)
int stage_tail_impl(r2f_ctx* ctx, const r2f_params* p, const r2f_planes* density, const float* burn_map, const HwcOut& out, int y0, int y1,
                    int W, int H_global, void* stream);

// r2f_stencil.hip
constexpr int kFixedMaxR = 11;  // largest unrolled direct form (23 x 23)
int ensure_stencil(r2f_ctx* ctx, int which, int Q, int TW, int TH, size_t lds_budget, bool common_box);
bool fft_eligible(const r2f_ctx* ctx, const StencilSet& s, int c);
void dyn_rule(const r2f_ctx* ctx, float* bound, float* floor);
// skip_identity: the single-tap channels were finished by the front kernel (r2f_stage_front_split) -- leave them alone.
// dyn: the caller vouches that the exposure-range record was kept for the samples `src` holds this frame (run_stencil_fft).
int run_stencil(r2f_ctx* ctx, int which, const r2f_planes* src, const r2f_planes* dst, int y0, int y1, int W, int H, int epilogue,
                float log_eps, hipStream_t s, bool skip_identity = false, bool dyn = false);

}  // namespace r2f
