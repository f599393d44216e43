// r2f_api.hip -- C ABI (include/r2f.h) over the gfx950 kernels: context, options, table and stencil upload and the stage entry
// points of the render path.  The stencil dispatch (r2f_stencil.hip), the whole-frame render with its graph cache (r2f_graph.hip),
// the JPEG entries (r2f_jpeg_api.hip) and the stages off the path with their entries (r2f_resample.hip, r2f_lens.hip, r2f_post.hip) are units of
// their own; r2f_ctx.h is what they share.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "r2f_ctx.h"

using namespace r2f;

static_assert(plan::kNumStencilVariants == kNumStencilVariants, "plan::kNumStencilVariants restates r2f_launch.h's");

namespace r2f {

int fail(r2f_ctx* ctx, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return code;
}

int DeviceBuf::reserve(r2f_ctx* ctx, size_t n, Grow how) {
    if (bytes >= n) return R2F_OK;
    if (how != Grow::Quiet) R2F_HIP(ctx, hipDeviceSynchronize());
    release();
    R2F_HIP(ctx, hipMalloc(&p, n));
    bytes = n;
    if (how == Grow::SyncGeneration) ++ctx->generation;
    return R2F_OK;
}

// Tables change only when a render parameter changes (the reference's caching rule), so the upload path
// is allowed to be slow: wait for every render still in flight on any stream before overwriting a table
// that those kernels may be reading, then copy synchronously.
int upload(r2f_ctx* ctx, DeviceBuf& buf, const void* host, size_t bytes) {
    R2F_HIP(ctx, hipDeviceSynchronize());
    int rc = buf.reserve(ctx, bytes, Grow::Quiet);  // (synchronised above, whether it grows or not)
    if (rc) return rc;
    R2F_HIP(ctx, hipMemcpy(buf.p, host, bytes, hipMemcpyHostToDevice));
    ++ctx->generation;
    return R2F_OK;
}

// (4, m) table -> per channel m-1 cells {xp[i], xp[i+1], fp[i], slope[i]} (plan::curve_cells), uploaded.
static int upload_curve(r2f_ctx* ctx, DeviceBuf& buf, DevCurve& cv, const float* lut, int m) {
    if (!lut || m < 2) return fail(ctx, R2F_EINVAL, "curve: need a (4, m) table with m >= 2");
    plan::CurveCells cc;
    if (plan::curve_cells(lut, m, &cc)) return fail(ctx, R2F_EINVAL, "curve: xp must be non-decreasing");
    static_assert(sizeof(float4) == 4 * sizeof(float), "a cell is one float4");
    int rc = upload(ctx, buf, cc.cells.data(), cc.cells.size() * sizeof(float));
    if (rc) return rc;
    cv.cells = static_cast<const float4*>(buf.p);
    cv.m = cc.m;
    cv.x0 = cc.x0;
    cv.x1 = cc.x1;
    cv.inv_step = cc.inv_step;
    cv.near = cc.near;
    for (int c = 0; c < 3; ++c) cv.f_first[c] = cc.f_first[c], cv.f_last[c] = cc.f_last[c];
    return R2F_OK;
}
// Does any plane of `a` (rows x W floats, plane_stride apart) share bytes with any plane of `b`?
bool planes_overlap(const r2f_planes* a, const r2f_planes* b, int W) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const float* a0 = a->data + i * a->plane_stride;
            const float* b0 = b->data + j * b->plane_stride;
            const float* a1 = a0 + (int64_t)a->rows * W;
            const float* b1 = b0 + (int64_t)b->rows * W;
            if (reinterpret_cast<uintptr_t>(a0) < reinterpret_cast<uintptr_t>(b1) &&
                reinterpret_cast<uintptr_t>(b0) < reinterpret_cast<uintptr_t>(a1))
                return true;
        }
    return false;
}

int check_rows(r2f_ctx* ctx, const char* what, const r2f_planes* pl, int lo, int hi) {
    if (!pl || !pl->data) return fail(ctx, R2F_EINVAL, "%s: null planes", what);
    if (lo < pl->gy0 || hi > pl->gy0 + pl->rows)
        return fail(ctx, R2F_EINVAL, "%s: rows [%d, %d) not inside the buffer's [%d, %d)", what, lo, hi, pl->gy0,
                    pl->gy0 + pl->rows);
    return R2F_OK;
}

RangeRecord record_of(const r2f_ctx* ctx) {
    RangeRecord r;
    r.blk = static_cast<FrameParams*>(ctx->frame_buf.p);
    r.tiles = static_cast<int2*>(ctx->range_tiles.p);
    r.tyn = ctx->tiles_tyn, r.txn = ctx->tiles_txn;
    return r;
}

// The record's tile grid for an H x W frame (allocated on first use and when the frame grows; a fresh grid says "unknown").
int ensure_range_tiles(r2f_ctx* ctx, int H_global, int W) {
    const int tyn = (H_global + kRangeTileRows - 1) / kRangeTileRows, txn = (W + kRangeTileCols - 1) / kRangeTileCols;
    if (ctx->range_tiles.p && tyn <= ctx->tiles_tyn && txn == ctx->tiles_txn) return R2F_OK;
    R2F_HIP(ctx, hipDeviceSynchronize());  // (kernels of an earlier frame may still be reading the old grid)
    const int new_tyn = std::max(tyn, ctx->tiles_txn == txn ? ctx->tiles_tyn : 0);
    const size_t n = (size_t)new_tyn * txn;
    std::vector<int2> init(n, make_int2((int)kFrameMinReset, (int)kFrameMaxReset));
    int rc = ctx->range_tiles.reserve(ctx, n * sizeof(int2), Grow::Quiet);
    if (rc) return rc;
    R2F_HIP(ctx, hipMemcpy(ctx->range_tiles.p, init.data(), n * sizeof(int2), hipMemcpyHostToDevice));
    ctx->tiles_tyn = new_tyn, ctx->tiles_txn = txn;
    ++ctx->generation;  // (captured launches hold the grid's address and dimensions)
    return R2F_OK;
}

// p->seed -> the context's device-side frame block, in stream order (a one-lane kernel: its by-value argument is copied at
// launch time, so no host staging buffer has to outlive the call).  The modes: r2f_ctx.h.
int write_frame_params(r2f_ctx* ctx, const r2f_params* p, hipStream_t s, int mode) {
    FrameParams v{};
    v.seed = p->seed;
    v.e_min = kFrameMinReset, v.e_max = kFrameMaxReset;
    R2F_HIP(ctx, launch_frame_params(record_of(ctx), v, mode, s));
    return R2F_OK;
}
}  // namespace r2f

// Event pairs of timed launches that r2f_kernel_timing never read.
r2f_ctx::~r2f_ctx() {
    for (auto& cls : timing_ev)
        for (auto& ev : cls) {
            (void)hipEventDestroy(ev.first);
            (void)hipEventDestroy(ev.second);
        }
}

r2f_ctx::Exposure::~Exposure() {
    if (stream) (void)hipStreamDestroy(stream);
    if (done) (void)hipEventDestroy(done);
    if (host) (void)hipHostFree(host);
}

// =============================================================================== C ABI
extern "C" {

const char* r2f_version(void) { return "r2f-hip 0.6 gfx950 abi7"; }

int r2f_create(int device, r2f_ctx** out) {
    if (!out) return R2F_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return R2F_EHIP;
    DeviceGuard guard(device);  // the caller's current device is restored on return
    if (guard.status != hipSuccess) return R2F_EHIP;
    if (init_kernel_attributes() != hipSuccess || front_fast_init_attributes() != hipSuccess) return R2F_EHIP;
    r2f_ctx* ctx = new r2f_ctx();
    ctx->device = device;
    if (ctx->frame_buf.reserve(ctx, sizeof(FrameParams), Grow::Quiet) != R2F_OK || hipMemset(ctx->frame_buf.p, 0, sizeof(FrameParams)) != hipSuccess ||
        ctx->exposure.rec.reserve(ctx, sizeof(ExposureRecord), Grow::Quiet) != R2F_OK) {
        delete ctx;  // (frees the block if it was the hipMemset that failed)
        return R2F_EHIP;
    }
    *out = ctx;
    return R2F_OK;
}

void r2f_destroy(r2f_ctx* ctx) {
    if (!ctx) return;
    DeviceGuard guard(ctx->device);
    (void)hipDeviceSynchronize();  // nothing in flight may still read what is freed below
    ctx->graphs.drop_all();  // the graphs go before the buffers they point into
    ctx->graphs.reap(true);  // (the device has been synchronised: entries without a usable event go too)
    delete ctx;
}

const char* r2f_last_error(const r2f_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

uint64_t r2f_generation(const r2f_ctx* ctx) { return ctx ? ctx->generation : 0; }

int r2f_set_option(r2f_ctx* ctx, const char* name, int value) {
    if (!ctx || !name) return R2F_EINVAL;
    ++ctx->generation;  // by-value launch arguments and the choice of kernels depend on the options
    const plan::OptionRow* row = plan::find_option(name);  // (r2f_plan.cpp has the table: names, ranges, error texts)
    if (!row) return fail(ctx, R2F_EINVAL, "unknown option %s", name);
    if (!plan::store_option(&ctx->opt, *row, value)) return fail(ctx, R2F_EINVAL, "%s", row->error);
    if (row->field == &plan::Options::xcd_band)
        for (auto& t : ctx->tile_order) t.gx = t.gy = 0;  // rebuild the tables
    return R2F_OK;
}

int r2f_set_matrix3x3(r2f_ctx* ctx, const float* m) {
    if (!ctx) return R2F_EINVAL;
    ctx->has_matrix = m != nullptr;
    if (m) memcpy(ctx->mat.m, m, sizeof ctx->mat.m);
    ++ctx->generation;
    return R2F_OK;
}

int r2f_set_lut2d(r2f_ctx* ctx, const float* lut, int n) {
    if (!ctx) return R2F_EINVAL;
    if (!lut || n < 2) return fail(ctx, R2F_EINVAL, "lut2d: need (n, n, 3) with n >= 2");
    R2F_GUARD(ctx);
    std::vector<float4> tex((size_t)n * n);
    for (size_t i = 0; i < tex.size(); ++i) tex[i] = make_float4(lut[3 * i], lut[3 * i + 1], lut[3 * i + 2], 0.f);
    int rc = upload(ctx, ctx->lut2d_buf, tex.data(), tex.size() * sizeof(float4));
    if (rc) return rc;
    ctx->lut2d.tex = static_cast<const float4*>(ctx->lut2d_buf.p);
    ctx->lut2d.n = n;
    return R2F_OK;
}

int r2f_set_lut3d(r2f_ctx* ctx, const float* lut, int n) {
    if (!ctx) return R2F_EINVAL;
    if (!lut || n < 2 || n > 256) return fail(ctx, R2F_EINVAL, "lut3d: need (n, n, n, 3) with 2 <= n <= 256");
    R2F_GUARD(ctx);
    std::vector<float4> tex((size_t)n * n * n);
    for (size_t i = 0; i < tex.size(); ++i) tex[i] = make_float4(lut[3 * i], lut[3 * i + 1], lut[3 * i + 2], 0.f);
    int rc = upload(ctx, ctx->lut3d_buf, tex.data(), tex.size() * sizeof(float4));
    if (rc) return rc;
    ctx->lut3d.tex = static_cast<const float4*>(ctx->lut3d_buf.p);
    ctx->lut3d.n = n;
    return R2F_OK;
}

int r2f_set_curve1d(r2f_ctx* ctx, const float* lut4xm, int m) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    int rc = upload_curve(ctx, ctx->curve_buf, ctx->curve, lut4xm, m);
    if (rc) return rc;
    double smax = 0.0;
    for (int c = 1; c <= 3; ++c)
        for (int i = 0; i + 1 < m; ++i) {
            const double dx = (double)lut4xm[i + 1] - (double)lut4xm[i];
            if (dx > 0.0) smax = std::max(smax, std::fabs(((double)lut4xm[(size_t)c * m + i + 1] - (double)lut4xm[(size_t)c * m + i]) / dx));
        }
    ctx->curve_slope_max = (float)smax;
    return R2F_OK;
}

int r2f_set_grain_lut(r2f_ctx* ctx, const float* lut4xm, int m) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    return upload_curve(ctx, ctx->grain_lut_buf, ctx->grain_lut, lut4xm, m);
}

int r2f_set_kernel(r2f_ctx* ctx, int which, const float* k, int kh, int kw, int kc) {
    if (!ctx) return R2F_EINVAL;
    if (which < 0 || which > 2) return fail(ctx, R2F_EINVAL, "set_kernel: which must be 0..2");
    if (!k || kh < 1 || kw < 1 || (kc != 1 && kc != 3)) return fail(ctx, R2F_EINVAL, "set_kernel: need (kh, kw, 1|3)");
    R2F_GUARD(ctx);
    StencilSet& s = ctx->stencil[which];
    s.present = true;
    s.kh = kh;
    s.kw = kw;
    s.kc = kc;
    s.host.assign(k, k + (size_t)kh * kw * kc);
    for (int c = 0; c < 3; ++c) {
        bool pos = false, neg = false;
        double sum = 0.0;
        for (size_t i = 0; i < (size_t)kh * kw; ++i) {
            const float v = k[i * kc + (kc == 1 ? 0 : c)];
            pos = pos || v > 0.f, neg = neg || v < 0.f;
            sum += (double)v;
        }
        s.mixed_sign[c] = pos && neg;
        s.unit_gain[c] = !neg && sum >= 0.99;  // (NaN taps: false)
    }
    s.single_tap_mask = 0;
    for (int c = 0; c < 3; ++c) {
        float w;
        if (plan::single_tap_channel(s.taps(), c, &w)) s.single_tap_mask |= 1 << c;
    }
    ++ctx->generation;
    s.built_q = 0;
    for (int c = 0; c < 3; ++c) ctx->fft.forget(which, c);
    if (which == R2F_KERNEL_GRAIN) ctx->grain_fixed_valid = false;
    ctx->stencil_fixed_valid[which] = false;
    return R2F_OK;
}

// ------------------------------------------------------------------------------- stages
int r2f_stage_front(r2f_ctx* ctx, const r2f_params* p, const void* in, int in_layout, int in_gy0, int in_rows, int upto,
                    const r2f_planes* dst, float* out_f32, uint8_t* out_u8, int out_gy0, int y0, int y1, int W,
                    int H_global, void* stream) {
    return stage_front_impl(ctx, p, in, in_layout, in_gy0, in_rows, upto, dst, HwcOut{out_f32, out_u8, nullptr, out_gy0}, y0, y1, W,
                            H_global, stream);
}

int r2f_stage_front_split(r2f_ctx* ctx, const r2f_params* p, const void* in, int in_layout, int in_gy0, int in_rows,
                          const r2f_planes* exposure, const r2f_planes* density, int y0, int y1, int W, int H_global,
                          int* finished_mask, void* stream) {
    if (!finished_mask) return R2F_EINVAL;
    *finished_mask = 0;
    return stage_front_impl(ctx, p, in, in_layout, in_gy0, in_rows, R2F_UPTO_EXPOSURE, exposure, HwcOut{}, y0, y1, W, H_global, stream,
                            density, finished_mask);
}

}  // extern "C"

// What an entry point that writes an interleaved output asks of it, in the order the callers have always reported it (the tail
// folds "y0 above the buffer" into its geometry check, ahead of this).  *vec: may the float4 / packed stores be used?
static int check_hwc_out(r2f_ctx* ctx, const char* who, const HwcOut& out, int y0, bool* vec) {
    if (!out.any()) return fail(ctx, R2F_EINVAL, "%s: no output buffer", who);
    if (y0 < out.gy0) return fail(ctx, R2F_EINVAL, "%s: y0 above the output buffer", who);
    if (reinterpret_cast<uintptr_t>(out.u16) & 1u) return fail(ctx, R2F_EINVAL, "%s: the uint16 output must be 2-byte aligned", who);
    *vec = *vec && out.vec_ok();
    return R2F_OK;
}

// tracked (whole-frame renders): when given, the fast kernel records the range of the exposure planes it writes in the context's frame
// block and *tracked says whether that happened (only the split fast kernel does it).
int r2f::stage_front_impl(r2f_ctx* ctx, const r2f_params* p, const void* in, int in_layout, int in_gy0, int in_rows, int upto,
                            const r2f_planes* dst, const HwcOut& out, int y0, int y1, int W, int H_global, void* stream,
                            const r2f_planes* finish_dst, int* finished_mask, bool* tracked) {
    if (tracked) *tracked = false;
    if (!ctx || !p) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (y1 <= y0) return R2F_OK;
    // R2F_F_TRACK_RANGE (a row shard's front calls): record like a whole-frame render's front kernel, or say that it did not happen
    const bool want_track = upto == R2F_UPTO_EXPOSURE && (tracked || (p->flags & R2F_F_TRACK_RANGE)) && ctx->opt.fft_s96_auto;
    auto cannot_track = [&]() -> int {
        if (!(p->flags & R2F_F_TRACK_RANGE) || upto != R2F_UPTO_EXPOSURE) return R2F_OK;
        return write_frame_params(ctx, p, static_cast<hipStream_t>(stream), 3);
    };
    if (!in || W <= 0 || y0 < in_gy0 || y1 > in_gy0 + in_rows || in_layout < 0 || in_layout > 2)
        return fail(ctx, R2F_EINVAL, "front: bad input geometry");
    if (!ctx->lut2d.tex) return fail(ctx, R2F_EINVAL, "input LUT not set (r2f_set_lut2d)");
    if ((p->flags & R2F_F_MATRIX) && !ctx->has_matrix) return fail(ctx, R2F_EINVAL, "matrix not set (r2f_set_matrix3x3)");
    FrontArgs a;
    memset(&a, 0, sizeof a);
    a.in = in;
    a.in_layout = in_layout;
    a.in_gy0 = in_gy0;
    a.in_rows = in_rows;
    a.upto = upto;
    a.y0 = y0;
    a.y1 = y1;
    a.W = W;
    a.H_global = H_global;
    a.use_matrix = (p->flags & R2F_F_MATRIX) ? 1 : 0;
    a.mat = ctx->mat;
    a.lut2d = ctx->lut2d;
    a.curve = ctx->curve;
    a.lut3d = ctx->lut3d;
    a.log_eps = p->log_eps;
    a.lut3d_scale = p->lut3d_scale;
    a.lut3d_mode = p->lut3d_mode;
    bool vec = W % 4 == 0 && aligned16(in);
    if (upto >= R2F_UPTO_DENSITY && !ctx->curve.cells) return fail(ctx, R2F_EINVAL, "density curve not set (r2f_set_curve1d)");
    if (upto == R2F_UPTO_OUTPUT) {
        if (!ctx->lut3d.tex) return fail(ctx, R2F_EINVAL, "output LUT not set (r2f_set_lut3d)");
        int rc = check_hwc_out(ctx, "front", out, y0, &vec);
        if (rc) return rc;
        a.out = out;
    } else if (upto == R2F_UPTO_EXPOSURE || upto == R2F_UPTO_DENSITY) {
        int rc = check_rows(ctx, "front dst", dst, y0, y1);
        if (rc) return rc;
        a.dst = to_dev(dst);
        vec = vec && planes_vec_ok(dst, W);
    } else {
        return fail(ctx, R2F_EINVAL, "front: bad upto");
    }
    a.vec = vec ? 1 : 0;
    a.blocks_per_cu = ctx->opt.front_blocks;
    a.fast = ctx->opt.front_fast;
    if (finish_dst && upto == R2F_UPTO_EXPOSURE && a.fast && ctx->stencil[R2F_KERNEL_HALATION].present && ctx->curve.cells) {
        // channels the halation leaves to a single tap: finish them here when the fast kernel can take the job
        int rc = check_rows(ctx, "front density dst", finish_dst, y0, y1);
        if (rc) return rc;
        FrontArgs f = a;
        f.finish_dst = to_dev(finish_dst);
        for (int c = 0; c < 3; ++c)
            if (plan::single_tap_channel(ctx->stencil[R2F_KERNEL_HALATION].taps(), c, &f.finish_w[c])) f.finish_mask |= 1 << c;
        f.vec = (vec && planes_vec_ok(finish_dst, W)) ? 1 : 0;
        if (f.finish_mask && f.finish_mask != 7 && front_fast_eligible(f)) {
            *finished_mask = f.finish_mask;
            if (want_track) {  // the exposure planes' range for the FFT passes
                rc = ensure_range_tiles(ctx, H_global, W);
                if (rc) return rc;
                f.track = record_of(ctx);
                f.track_mask = 7 & ~f.finish_mask;
                if (tracked) *tracked = true;
            }
            R2F_HIP(ctx, launch_front_fast(f, static_cast<hipStream_t>(stream)));
            return R2F_OK;
        }
    }
    if (want_track && !tracked && a.fast && front_fast_eligible(a)) {
        // a row shard writes every channel's exposure (its neighbours need them); the record covers the channels the halation's FFT
        // passes read, i.e. not the single-tap ones -- the same samples a whole-frame render records
        int rc = ensure_range_tiles(ctx, H_global, W);
        if (rc) return rc;
        a.track = record_of(ctx);
        a.track_mask = 7;
        if (ctx->stencil[R2F_KERNEL_HALATION].present) a.track_mask &= ~ctx->stencil[R2F_KERNEL_HALATION].single_tap_mask;
    } else {
        int rc = cannot_track();
        if (rc) return rc;
    }
    R2F_HIP(ctx, launch_front(a, static_cast<hipStream_t>(stream)));
    return R2F_OK;
}

extern "C" {

int r2f_stage_halation(r2f_ctx* ctx, const r2f_params* p, const r2f_planes* exposure, const r2f_planes* density, int y0,
                       int y1, int W, int H_global, void* stream) {
    if (!ctx || !p) return R2F_EINVAL;
    R2F_GUARD(ctx);
    ctx->frame_dyn_armed = false;  // (set again by the FFT launches when they carry the rule: r2f_frame_exposure_range)
    return run_stencil(ctx, R2F_KERNEL_HALATION, exposure, density, y0, y1, W, H_global, 1, p->log_eps,
                       static_cast<hipStream_t>(stream), (p->flags & R2F_F_IDENTITY_DONE) != 0, (p->flags & R2F_F_RANGE_VALID) != 0);
}

int r2f_stage_exposure_range(r2f_ctx* ctx, const r2f_planes* exposure, int y0, int y1, int y2, int y3, int W, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (y1 <= y0 && y3 <= y2) return R2F_OK;
    if (W <= 0) return fail(ctx, R2F_EINVAL, "exposure range: bad geometry");
    int rc = y1 > y0 ? check_rows(ctx, "exposure range", exposure, y0, y1) : R2F_OK;
    if (rc) return rc;
    rc = y3 > y2 ? check_rows(ctx, "exposure range", exposure, y2, y3) : R2F_OK;
    if (rc) return rc;
    int mask = 7;  // the channels the halation's FFT passes read: not the single-tap ones (as the front kernel records them)
    if (ctx->stencil[R2F_KERNEL_HALATION].present) mask &= ~ctx->stencil[R2F_KERNEL_HALATION].single_tap_mask;
    rc = ensure_range_tiles(ctx, std::max(std::max(y1, y3), exposure->gy0 + exposure->rows), W);
    if (rc) return rc;
    R2F_HIP(ctx, launch_exposure_range(to_dev(exposure), y0, y1, y2, y3, W, mask, record_of(ctx), static_cast<hipStream_t>(stream)));
    return R2F_OK;
}

int r2f_stage_mtf(r2f_ctx* ctx, const r2f_params* p, const r2f_planes* din, const r2f_planes* dout, int y0, int y1,
                  int W, int H_global, void* stream) {
    if (!ctx || !p) return R2F_EINVAL;
    R2F_GUARD(ctx);
    return run_stencil(ctx, R2F_KERNEL_MTF, din, dout, y0, y1, W, H_global, 0, 0.f, static_cast<hipStream_t>(stream));
}

int r2f_stage_stencil(r2f_ctx* ctx, int which, const r2f_planes* src, const r2f_planes* dst, int y0, int y1, int W,
                      int H_global, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (which < 0 || which > 2) return fail(ctx, R2F_EINVAL, "stencil: which must be 0..2");
    return run_stencil(ctx, which, src, dst, y0, y1, W, H_global, 0, 0.f, static_cast<hipStream_t>(stream));
}

int r2f_kernel_timing(r2f_ctx* ctx, int cls, double* total_ms, int* launches, double* bytes) {
    if (!ctx || cls < 0 || cls > 5 || !total_ms || !launches || !bytes) return R2F_EINVAL;
    R2F_GUARD(ctx);
    double sum = 0.0;
    hipError_t err = hipSuccess;  // the first failure; the class's events are destroyed and its record cleared whatever happens
    for (auto& ev : ctx->timing_ev[cls]) {
        float ms = 0.f;
        hipError_t e = hipEventSynchronize(ev.second);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev.first, ev.second);
        if (err == hipSuccess) err = e;
        sum += ms;
        (void)hipEventDestroy(ev.first);
        (void)hipEventDestroy(ev.second);
    }
    const int n = (int)ctx->timing_ev[cls].size();
    const double b = ctx->timing_bytes[cls];
    ctx->timing_ev[cls].clear();
    ctx->timing_bytes[cls] = 0.0;
    if (err != hipSuccess) return fail(ctx, R2F_EHIP, "kernel timing: %s", hipGetErrorString(err));
    *total_ms = sum, *launches = n, *bytes = b;
    return R2F_OK;
}

int r2f_stencil_stats(r2f_ctx* ctx, int which, int* out) {
    if (!ctx || !out) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (which < 0 || which > 2) return fail(ctx, R2F_EINVAL, "stencil: which must be 0..2");
    StencilSet& set = ctx->stencil[which];
    if (!set.present) return fail(ctx, R2F_EINVAL, "stencil %d not set (r2f_set_kernel)", which);
    if (!set.built_q) {  // not launched yet: build the device form the default launch would use
        const StencilVariant& sv = kStencilVariants[ctx->opt.variant >= 0 ? ctx->opt.variant : 0];
        int rc = ensure_stencil(ctx, which, sv.Q, sv.TW(), sv.TH(), (size_t)ctx->opt.lds_kb * 1024, which == 2);
        if (rc) return rc;
    }
    for (int c = 0; c < 3; ++c) {
        const DevStencil& d = set.dev[c];
        int* o = out + 8 * c;
        // bit 0: mirrored taps are paired in the entry list; bits 1..: R when the channel takes the unrolled stencil_fixed form
        // (the grain stencil: all three channels together, and the geometry of the tail tile, which this call may not have built)
        const int all[3] = {0, 1, 2};
        const int fr = which == R2F_KERNEL_GRAIN ? (ctx->opt.grain_fixed ? plan::fixed_stencil_radius(set.taps(), set.geom, all, 3, 9) : 0)
                                                 : (ctx->opt.stencil_fixed && ctx->opt.variant <= 0 && !fft_eligible(ctx, set, c)
                                                        ? plan::fixed_stencil_radius(set.taps(), set.geom, &c, 1, kFixedMaxR)
                                                        : 0);
        // bit 8: the grain stencil runs as two 1-D passes (known once a tail launch has looked at the taps)
        const int sep = which == R2F_KERNEL_GRAIN && fr && ctx->grain_fixed_valid && ctx->grain_sep && ctx->opt.grain_sep;
        // bit 9: ... with the pass along x in registers (launch_tail: R <= kTailXRegMaxR unless grain_xpass_lds)
        const int xreg = sep && fr <= kTailXRegMaxR && !ctx->opt.grain_xpass_lds;
        o[0] = d.n_entries, o[1] = d.n_rowsteps, o[2] = d.n_phases, o[3] = d.sym | (fr << 1) | (sep << 8) | (xreg << 9);
        o[4] = d.kh, o[5] = d.kw, o[6] = set.built_q;
        o[7] = fft_eligible(ctx, set, c) ? 1 | (ctx->fft.last[which][c].dims << 1) | (ctx->fft.last[which][c].real << 30) : 0;
    }
    return R2F_OK;
}

static bool burn_geometry(const r2f_params* p, int H, int W, int* h_lo, int* w_lo) { return plan::burn_geometry(p->burn_cell, H, W, h_lo, w_lo); }

// density == nullptr && planes_out: the grain field alone (K_g * noise) -> planes_out.
// gfield: a grain field computed that way is applied pointwise instead of being generated here.
// The grain stencil in the form stencil_fixed<R, 2> wants, when it has one (fixed_stencil_radius); grain_fixed_r = 0
// otherwise (the generic entry list runs).
static int ensure_grain_fixed(r2f_ctx* ctx) {
    if (ctx->grain_fixed_valid) return R2F_OK;
    StencilSet& set = ctx->stencil[R2F_KERNEL_GRAIN];
    ctx->grain_fixed_valid = true;
    const int chans[3] = {0, 1, 2};
    ctx->grain_fixed_r = plan::fixed_stencil_radius(set.taps(), set.geom, chans, 3, 9);
    ctx->grain_sep = false;
    if (!ctx->grain_fixed_r) return R2F_OK;
    bool same = false;
    const std::vector<float> w = plan::fixed_stencil_weights(set.taps(), ctx->grain_fixed_r, kTailQ, &same);
    ctx->grain_fixed_same = same ? 1 : 0;
    // separable (K = u v^T to 6e-7 of the largest tap: plan::separable_taps)?  Then two 1-D passes of 2 R + 1 taps replace (2 R + 1)^2
    ctx->grain_sep = plan::separable_taps(set.taps(), ctx->grain_fixed_r, ctx->grain_sep_u, ctx->grain_sep_v);
    return upload(ctx, ctx->grain_fixed_w, w.data(), w.size() * sizeof(float));
}

static int run_tail(r2f_ctx* ctx, const r2f_params* p, const r2f_planes* density, const r2f_planes* planes_out,
                    const float* burn_map, const HwcOut& out, int y0, int y1, int W, int H_global, void* stream,
                    const r2f_planes* gfield = nullptr) {
    if (y1 <= y0) return R2F_OK;
    const bool field_only = density == nullptr && planes_out != nullptr;
    if (field_only) {
        static const r2f_planes none = {nullptr, 0, 0, 0};
        density = &none;
    }
    const bool to_planes = planes_out != nullptr;
    if (W <= 0 || y0 < 0 || y1 > H_global || (!to_planes && y0 < out.gy0)) return fail(ctx, R2F_EINVAL, "tail: bad geometry");
    bool out_vec = true;
    int rc = to_planes ? R2F_OK : check_hwc_out(ctx, "tail", out, y0, &out_vec);
    if (rc) return rc;
    if (!to_planes && !ctx->lut3d.tex) return fail(ctx, R2F_EINVAL, "output LUT not set (r2f_set_lut3d)");
    rc = field_only ? R2F_OK : check_rows(ctx, "tail src", density, y0, y1);
    if (rc) return rc;
    TailArgs a;
    memset(&a, 0, sizeof a);
    a.src = to_dev(density);
    a.out = out;
    a.y0 = y0;
    a.y1 = y1;
    a.W = W;
    a.H_global = H_global;
    a.grain = (p->flags & R2F_F_GRAIN) ? 1 : 0;
    if (gfield) {  // the field was made ahead of time: this call is the pointwise half
        if (!a.grain) return fail(ctx, R2F_EINVAL, "tail: a grain field was passed but the grain flag is off");
        rc = check_rows(ctx, "grain field", gfield, y0, y1);
        if (rc) return rc;
        if (!ctx->grain_lut.cells) return fail(ctx, R2F_EINVAL, "grain LUT not set (r2f_set_grain_lut)");
        a.grain = 0;
        a.gfield = to_dev(gfield);
        a.has_gfield = 1;
        a.grain_lut = ctx->grain_lut;
    }
    a.mono = (p->flags & R2F_F_GRAIN_MONO) ? 1 : 0;
    a.frame = static_cast<const FrameParams*>(ctx->frame_buf.p);
    a.lut3d = ctx->lut3d;
    a.lut3d_scale = p->lut3d_scale;
    a.lut3d_mode = p->lut3d_mode;
    bool vec = field_only ? true : planes_vec_ok(density, W);
    if (gfield) vec = vec && planes_vec_ok(gfield, W);
    if (to_planes) {
        if (!a.grain) return fail(ctx, R2F_EINVAL, "grain stage called with the grain flag off");
        rc = check_rows(ctx, "grain dst", planes_out, y0, y1);
        if (rc) return rc;
        // pointwise on the density, so exactly in place (same base, stride and first row) is fine; anything else that
        // overlaps would have one pixel's store land on another pixel's load
        if (!field_only && planes_overlap(density, planes_out, W) &&
            !(density->data == planes_out->data && density->plane_stride == planes_out->plane_stride && density->gy0 == planes_out->gy0))
            return fail(ctx, R2F_EINVAL, "grain: source and destination planes overlap without being the same buffer");
        a.to_planes = field_only ? 2 : 1;
        a.dst = to_dev(planes_out);
        vec = vec && planes_vec_ok(planes_out, W);
    } else {
        vec = vec && out_vec;
        if (burn_map) {
            if (a.grain || a.has_gfield)
                return fail(ctx, R2F_EINVAL, "tail with a burn map: apply the grain first (r2f_stage_grain) and clear R2F_F_GRAIN");
            int h_lo, w_lo;
            if (!burn_geometry(p, H_global, W, &h_lo, &w_lo)) return fail(ctx, R2F_EINVAL, "burn: bad burn_cell");
            a.burn.map = burn_map;
            a.burn.h_lo = h_lo;
            a.burn.w_lo = w_lo;
            a.burn.h_up = h_lo * p->burn_cell;
            a.burn.w_up = w_lo * p->burn_cell;
            a.burn.zy = a.burn.h_up > 1 ? (double)(h_lo - 1) / (double)(a.burn.h_up - 1) : 0.0;
            a.burn.zx = a.burn.w_up > 1 ? (double)(w_lo - 1) / (double)(a.burn.w_up - 1) : 0.0;
            a.burn.strength = p->burn_strength;
        }
    }
    a.vec = vec ? 1 : 0;
    if (a.grain) {
        if (!ctx->grain_lut.cells) return fail(ctx, R2F_EINVAL, "grain LUT not set (r2f_set_grain_lut)");
        if (!ctx->stencil[R2F_KERNEL_GRAIN].present) {
            // gpu_processor.py:931-932: no grain kernel -> 1x1 ones
            const float one = 1.f;
            rc = r2f_set_kernel(ctx, R2F_KERNEL_GRAIN, &one, 1, 1, 1);
            if (rc) return rc;
        }
        rc = ensure_stencil(ctx, R2F_KERNEL_GRAIN, kTailQ, 4 * kTailBX, kTailQ * kTailBY, 0, true);
        if (rc) return rc;
        for (int c = 0; c < 3; ++c) a.gk[c] = ctx->stencil[R2F_KERNEL_GRAIN].dev[c];
        rc = ensure_grain_fixed(ctx);
        if (rc) return rc;
        a.fixed_r = ctx->opt.grain_fixed ? ctx->grain_fixed_r : 0;
        a.fixed_same = ctx->grain_fixed_same;
        a.fixed_w = static_cast<const float*>(ctx->grain_fixed_w.p);
        // (monochrome noise with per-channel taps: the one noise plane cannot be filtered in place three ways -> 2-D form)
        a.sep = (a.fixed_r && ctx->opt.grain_sep && ctx->grain_sep && (!a.mono || ctx->grain_fixed_same)) ? 1 : 0;
        a.xpass_lds = ctx->opt.grain_xpass_lds ? 1 : 0;
        memcpy(a.sep_u, ctx->grain_sep_u, sizeof a.sep_u);
        memcpy(a.sep_v, ctx->grain_sep_v, sizeof a.sep_v);
        if (tail_lds_bytes(a.gk, a.mono) > kMaxLds)
            return fail(ctx, R2F_ETOOLARGE, "grain stencil %dx%d does not fit the LDS noise tile", a.gk[0].kh, a.gk[0].kw);
        a.grain_lut = ctx->grain_lut;
    }
    if (a.grain && !(p->flags & R2F_F_FRAME_RESIDENT)) {  // the seed of THIS call, ahead of the kernel that reads it
        rc = write_frame_params(ctx, p, static_cast<hipStream_t>(stream), 0);
        if (rc) return rc;
    }
    R2F_HIP(ctx, launch_tail(a, static_cast<hipStream_t>(stream)));
    return R2F_OK;
}

int r2f_stage_tail(r2f_ctx* ctx, const r2f_params* p, const r2f_planes* density, const float* burn_map, float* out_f32,
                   uint8_t* out_u8, int out_gy0, int y0, int y1, int W, int H_global, void* stream) {
    return stage_tail_impl(ctx, p, density, burn_map, HwcOut{out_f32, out_u8, nullptr, out_gy0}, y0, y1, W, H_global, stream);
}

}  // extern "C"

int r2f::stage_tail_impl(r2f_ctx* ctx, const r2f_params* p, const r2f_planes* density, const float* burn_map, const HwcOut& out, int y0,
                         int y1, int W, int H_global, void* stream) {
    if (!ctx || !p) return R2F_EINVAL;
    R2F_GUARD(ctx);
    return run_tail(ctx, p, density, nullptr, burn_map, out, y0, y1, W, H_global, stream);
}

extern "C" {

int r2f_stage_tail16(r2f_ctx* ctx, const r2f_params* p, const r2f_planes* density, const float* burn_map, float* out_f32,
                     uint8_t* out_u8, uint16_t* out_u16, int out_gy0, int y0, int y1, int W, int H_global, void* stream) {
    return stage_tail_impl(ctx, p, density, burn_map, HwcOut{out_f32, out_u8, out_u16, out_gy0}, y0, y1, W, H_global, stream);
}

int r2f_stage_tail_field16(r2f_ctx* ctx, const r2f_params* p, const r2f_planes* density, const r2f_planes* field, float* out_f32,
                           uint8_t* out_u8, uint16_t* out_u16, int out_gy0, int y0, int y1, int W, int H_global, void* stream) {
    if (!ctx || !p) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (!field) return fail(ctx, R2F_EINVAL, "tail: null grain field");
    return run_tail(ctx, p, density, nullptr, nullptr, HwcOut{out_f32, out_u8, out_u16, out_gy0}, y0, y1, W, H_global, stream, field);
}

int r2f_stage_front16(r2f_ctx* ctx, const r2f_params* p, const void* in, int in_layout, int in_gy0, int in_rows, float* out_f32,
                      uint16_t* out_u16, int out_gy0, int y0, int y1, int W, int H_global, void* stream) {
    return stage_front_impl(ctx, p, in, in_layout, in_gy0, in_rows, R2F_UPTO_OUTPUT, nullptr, HwcOut{out_f32, nullptr, out_u16, out_gy0}, y0,
                            y1, W, H_global, stream);
}

int r2f_stage_grain_field(r2f_ctx* ctx, const r2f_params* p, const r2f_planes* field, int y0, int y1, int W, int H_global,
                          void* stream) {
    if (!ctx || !p) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (!field) return fail(ctx, R2F_EINVAL, "grain field: null destination");
    return run_tail(ctx, p, nullptr, field, nullptr, HwcOut{}, y0, y1, W, H_global, stream);
}

int r2f_stage_tail_field(r2f_ctx* ctx, const r2f_params* p, const r2f_planes* density, const r2f_planes* field, float* out_f32,
                         uint8_t* out_u8, int out_gy0, int y0, int y1, int W, int H_global, void* stream) {
    if (!ctx || !p) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (!field) return fail(ctx, R2F_EINVAL, "tail: null grain field");
    return run_tail(ctx, p, density, nullptr, nullptr, HwcOut{out_f32, out_u8, nullptr, out_gy0}, y0, y1, W, H_global, stream, field);
}

int r2f_stage_grain(r2f_ctx* ctx, const r2f_params* p, const r2f_planes* din, const r2f_planes* dout, int y0, int y1, int W,
                    int H_global, void* stream) {
    if (!ctx || !p) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (!dout) return fail(ctx, R2F_EINVAL, "grain: null destination");
    return run_tail(ctx, p, din, dout, nullptr, HwcOut{}, y0, y1, W, H_global, stream);
}

int r2f_stage_burn_sums(r2f_ctx* ctx, const r2f_params* p, const r2f_planes* density, float* cell_sums, int y0, int y1, int W,
                        int H_global, void* stream) {
    if (!ctx || !p) return R2F_EINVAL;
    R2F_GUARD(ctx);
    int h_lo, w_lo;
    if (!cell_sums || !burn_geometry(p, H_global, W, &h_lo, &w_lo)) return fail(ctx, R2F_EINVAL, "burn sums: bad arguments");
    if (y0 < 0 || y1 > H_global || y1 < y0) return fail(ctx, R2F_EINVAL, "burn sums: bad rows");
    if (y1 > y0) {
        int rc = check_rows(ctx, "burn src", density, y0, y1);
        if (rc) return rc;
    }
    BurnSumsArgs a;
    a.src = to_dev(density);
    a.cell_sums = cell_sums;
    a.y0 = y0;
    a.y1 = y1;
    a.W = W;
    a.H_global = H_global;
    a.h_lo = h_lo;
    a.w_lo = w_lo;
    R2F_HIP(ctx, launch_burn_sums(a, static_cast<hipStream_t>(stream)));
    return R2F_OK;
}

int r2f_stage_burn_map(r2f_ctx* ctx, const r2f_params* p, const float* cell_sums, float* burn_map, float* scratch, int W,
                       int H_global, void* stream) {
    if (!ctx || !p) return R2F_EINVAL;
    R2F_GUARD(ctx);
    int h_lo, w_lo;
    if (!cell_sums || !burn_map || !scratch || !burn_geometry(p, H_global, W, &h_lo, &w_lo))
        return fail(ctx, R2F_EINVAL, "burn map: bad arguments");
    BurnMapArgs a;
    a.cell_sums = cell_sums;
    a.map = burn_map;
    a.scratch = scratch;
    a.h_lo = h_lo;
    a.w_lo = w_lo;
    a.d_ref = p->burn_d_ref;
    plan::burn_weights(a.w);  // scipy's gaussian kernel for sigma = 3, truncate = 2
    R2F_HIP(ctx, launch_burn_map(a, static_cast<hipStream_t>(stream)));
    return R2F_OK;
}

int r2f_stage_noise(r2f_ctx* ctx, const r2f_params* p, uint32_t* hash_planes, float* noise_planes, int y0, int y1, int W,
                    void* stream) {
    if (!ctx || !p) return R2F_EINVAL;
    R2F_GUARD(ctx);
    NoiseArgs a;
    a.hash = hash_planes;
    a.noise = noise_planes;
    a.y0 = y0;
    a.y1 = y1;
    a.W = W;
    a.frame = static_cast<const FrameParams*>(ctx->frame_buf.p);
    a.mono = (p->flags & R2F_F_GRAIN_MONO) ? 1 : 0;
    if (!(p->flags & R2F_F_FRAME_RESIDENT)) {
        int rc = write_frame_params(ctx, p, static_cast<hipStream_t>(stream), 0);
        if (rc) return rc;
    }
    R2F_HIP(ctx, launch_noise(a, static_cast<hipStream_t>(stream)));
    return R2F_OK;
}

// ------------------------------------------------------------------------------- the frame record
int r2f_frame_exposure_range(r2f_ctx* ctx, float* out4, int* armed, int* packed) {
    if (!ctx || !out4 || !armed || !packed) return R2F_EINVAL;
    R2F_GUARD(ctx);
    R2F_HIP(ctx, hipDeviceSynchronize());
    FrameParams v{};
    R2F_HIP(ctx, hipMemcpy(&v, ctx->frame_buf.p, sizeof v, hipMemcpyDeviceToHost));
    // the frame's extremes = the extremes over the record's tiles (the kernels merge into tiles only: nothing decides on the frame's
    // range any more); a record marked unusable (a front kernel that could not record) reads as max = +inf
    int lo = (int)kFrameMinReset, hi = (int)kFrameMaxReset;
    if (ctx->range_tiles.p && ctx->tiles_tyn > 0) {
        std::vector<int2> tiles((size_t)ctx->tiles_tyn * ctx->tiles_txn);
        R2F_HIP(ctx, hipMemcpy(tiles.data(), ctx->range_tiles.p, tiles.size() * sizeof(int2), hipMemcpyDeviceToHost));
        for (const int2& t : tiles) lo = std::min(lo, t.x), hi = std::max(hi, t.y);
    }
    if (v.e_max == 0x7f800000u) hi = 0x7f800000;
    memcpy(&out4[0], &lo, 4);
    memcpy(&out4[1], &hi, 4);
    dyn_rule(ctx, &out4[2], &out4[3]);
    *armed = ctx->frame_dyn_armed ? 1 : 0;
    // the choice is made per window pair (r2f_frame_scratch_choice has the counts): *packed says whether EVERY pair of the last
    // halation call took the 12-byte element
    int pairs = 0, packed_pairs = 0;
    int rc = r2f_frame_scratch_choice(ctx, &pairs, &packed_pairs);
    if (rc) return rc;
    *packed = (*armed && pairs > 0 && packed_pairs == pairs) ? 1 : 0;
    return R2F_OK;
}

int r2f_frame_scratch_choice(r2f_ctx* ctx, int* pairs, int* packed_pairs) {
    if (!ctx || !pairs || !packed_pairs) return R2F_EINVAL;
    R2F_GUARD(ctx);
    *pairs = *packed_pairs = 0;
    if (!ctx->frame_dyn_armed || !ctx->dyn_flags.p || ctx->dyn_flags_ppc <= 0) return R2F_OK;
    R2F_HIP(ctx, hipDeviceSynchronize());
    std::vector<int> flags((size_t)ctx->dyn_flags_ppc);
    R2F_HIP(ctx, hipMemcpy(flags.data(), ctx->dyn_flags.p, flags.size() * sizeof(int), hipMemcpyDeviceToHost));
    *pairs = ctx->dyn_flags_ppc;
    for (int f : flags) *packed_pairs += f != 0;
    return R2F_OK;
}

int r2f_frame_scratch_flags(r2f_ctx* ctx, int32_t* out, int capacity, int* count) {
    if (!ctx || !count || capacity < 0 || (capacity > 0 && !out)) return R2F_EINVAL;
    R2F_GUARD(ctx);
    *count = 0;
    if (!ctx->frame_dyn_armed || !ctx->dyn_flags.p || ctx->dyn_flags_ppc <= 0) return R2F_OK;
    R2F_HIP(ctx, hipDeviceSynchronize());
    *count = ctx->dyn_flags_ppc;
    const int n = std::min(capacity, ctx->dyn_flags_ppc);
    if (n > 0) R2F_HIP(ctx, hipMemcpy(out, ctx->dyn_flags.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return R2F_OK;
}

int r2f_write_frame_params(r2f_ctx* ctx, const r2f_params* p, void* stream) {
    if (!ctx || !p) return R2F_EINVAL;
    R2F_GUARD(ctx);
    return write_frame_params(ctx, p, static_cast<hipStream_t>(stream), 1);
}

}  // extern "C"
