// r2f_stencil.hip -- the stencil stages' dispatch: a stencil's device forms (entry lists, tile orders, the unrolled fixed form, FFT
// spectra) built on demand, and the choice between them per channel (run_stencil).  The FFT form's call (run_stencil_fft) is a
// sequence of named steps around plan::fft_call: see the section "FFT form" below.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "r2f_ctx.h"

namespace r2f {

static_assert(plan::fixed_ax(4) == fixed_stencil_ax(4) && plan::fixed_ax(7) == fixed_stencil_ax(7) && plan::fixed_ax(11) == fixed_stencil_ax(11),
              "plan::fixed_ax restates fixed_stencil_ax");

// Build (or reuse) the device form of stencil `which` for a tile TW x TH, Q rows per lane, and an LDS
// budget in bytes (0 = whole stencil height in one phase).
int ensure_stencil(r2f_ctx* ctx, int which, int Q, int TW, int TH, size_t lds_budget, bool common_box) {
    const bool allow_sym = ctx->opt.sym != 0;
    StencilSet& s = ctx->stencil[which];
    if (!s.present) return fail(ctx, R2F_EINVAL, "stencil %d not set (r2f_set_kernel)", which);
    if (s.built_q == Q && s.built_tw == TW && s.built_th == TH && s.built_budget == lds_budget && s.common_box == common_box &&
        s.built_sym == allow_sym)
        return R2F_OK;
    const plan::Taps taps = s.taps();
    int box[3][4];
    for (int c = 0; c < 3; ++c) plan::tap_box(taps, c, box[c]);
    if (common_box) {
        for (int c = 1; c < 3; ++c) {
            box[0][0] = std::min(box[0][0], box[c][0]);
            box[0][1] = std::max(box[0][1], box[c][1]);
            box[0][2] = std::min(box[0][2], box[c][2]);
            box[0][3] = std::max(box[0][3], box[c][3]);
        }
        for (int c = 1; c < 3; ++c) memcpy(box[c], box[0], sizeof box[0]);
    }
    plan::StreamHost sh;
    for (int c = 0; c < 3; ++c) {
        // mirror symmetry about the anchor column, bit for bit?  (needs an odd box centred on the anchor)
        bool sym = allow_sym && plan::mirror_symmetric(taps, c, box[c]);
        if (sym && common_box)  // shared geometry (grain): pair taps only if every channel allows it
            sym = plan::mirror_symmetric(taps, 0, box[c]) && plan::mirror_symmetric(taps, 1, box[c]) && plan::mirror_symmetric(taps, 2, box[c]);
        plan::StencilGeom g;
        if (plan::plan_stencil_channel(taps, c, box[c], sym, Q, TW, TH, lds_budget, &g, &sh))
            return fail(ctx, R2F_ETOOLARGE, "stencil %d: %d-tap rows do not fit the LDS budget", which, g.kw);
        DevStencil& d = s.dev[c];
        d.kh = g.kh, d.kw = g.kw, d.kw_pad = g.kw_pad, d.RS = g.RS, d.ay = g.ay, d.ax = g.ax, d.sym = g.sym;
        d.wmul = 1;
        d.n_phases = g.n_phases, d.n_rowsteps = g.n_rowsteps, d.n_entries = g.n_entries;
        d.mask_first_or = g.mask_first_or, d.mask_last_or = g.mask_last_or, d.max_lds_rows = g.max_lds_rows;
        s.geom[c] = g;
        int rc = upload(ctx, s.wbuf[c], sh.w.data(), sh.w.size() * sizeof(float));
        if (rc) return rc;
        // row-step records (16-byte aligned: read with s_load_dwordx4) and phase records share one allocation
        std::vector<int> meta(sh.rowinfo);
        const size_t n_ri = meta.size();
        meta.insert(meta.end(), sh.phases.begin(), sh.phases.end());
        rc = upload(ctx, s.mbuf[c], meta.data(), meta.size() * sizeof(int));
        if (rc) return rc;
        d.wstream = static_cast<const float*>(s.wbuf[c].p);
        d.rowinfo = static_cast<const int*>(s.mbuf[c].p);
        d.phases = d.rowinfo + n_ri;
    }
    s.built_q = Q;
    s.built_tw = TW;
    s.built_th = TH;
    s.built_budget = lds_budget;
    s.built_sym = allow_sym;
    s.common_box = common_box;
    return R2F_OK;
}

// Source rows a stencil with `above`/`below` taps needs for outputs [y0, y1), after reflect-101.
static int check_stencil_source(r2f_ctx* ctx, const char* what, const r2f_planes* src, int y0, int y1, int above, int below,
                         int H) {
    int lo, hi;
    plan::stencil_source_rows(y0, y1, above, below, H, &lo, &hi);
    return check_rows(ctx, what, src, lo, hi);
}

// Tile order for a gx x gy grid of stencil workgroups (plan::tile_order: one contiguous run of tiles per XCD, walked in bands
// of tile columns), cached per grid.
static int ensure_tile_order(r2f_ctx* ctx, int gx, int gy, const int** out) {
    for (auto& t : ctx->tile_order)
        if (t.gx == gx && t.gy == gy && t.buf.p) {
            *out = static_cast<const int*>(t.buf.p);
            return R2F_OK;
        }
    const std::vector<int> order = plan::tile_order(gx, gy, ctx->opt.xcd_band);
    r2f_ctx::TileOrder& slot = ctx->tile_order[ctx->tile_order_next];
    ctx->tile_order_next = (ctx->tile_order_next + 1) % 4;
    int rc = upload(ctx, slot.buf, order.data(), order.size() * sizeof(int));
    if (rc) return rc;
    slot.gx = gx;
    slot.gy = gy;
    *out = static_cast<const int*>(slot.buf.p);
    return R2F_OK;
}

// Up to which radius the unrolled direct form is preferred over the FFT form (tools/fft_probe.py, 24 MP x 3 channels): against
// complex128 scratch it wins up to 23 x 23 (0.54 vs 0.55 ms; 25 x 25: 0.81 vs 0.57); against the complex64 scratch of the MTF
// passes (0.42-0.45 ms whatever the taps) only up to 19 x 19 (0.40; 21 x 21: 0.45 vs 0.45, 23 x 23: 0.54 vs 0.43).
static int fixed_preferred_max_r(const r2f_ctx* ctx, int which) { return ((ctx->opt.fft_s32 >> which) & 1) ? 9 : kFixedMaxR; }

// Does channel c of stencil `which` take the overlap-save FFT form?
bool fft_eligible(const r2f_ctx* ctx, const StencilSet& s, int c) {
    if (!ctx->opt.fft) return false;
    int b[4];
    plan::tap_box(s.taps(), c, b);
    const int bh = b[1] - b[0] + 1, bw = b[3] - b[2] + 1;
    // up to 400 taps a side: a 512-point window then still yields 113 x 112 outputs (boxes over 200 taps on an axis take the
    // 512-point window there, see fft_window)
    if (!(bh <= plan::kFftMaxTaps && bw <= plan::kFftMaxTaps)) return false;
    // A channel with taps of BOTH signs (the unsharp-masked MTF kernel, effects.py:179-183 with sharpening_strength > 0) cancels:
    // a float32 sum is accurate relative to sum |w x|, not to the result -- 4-8 ulp of a density, which a stepped grain LUT or a
    // steep output LUT then multiplies (found by the round-4 fuzz criterion against the float64 evaluation: one case of 1 100 at
    // 1.46 x its bound).  Such a channel takes the float64 FFT form whatever its size, on complex128 scratch (run_stencil_fft):
    // one rounding, like the oracle's.  Preview-scale unsharp masking is rare and its frames are small; the headline has none.
    // (`stencil_fft_mixed_sign = 0` hands such channels back to the size rules below -- the A/B switch, and the way to keep the
    // stencil_fft_min_taps / stencil_fft_scratch32 knobs in charge of them)
    if (s.mixed_sign[c] && ctx->opt.fft_mixed_sign) return true;
    if (bh * bw < ctx->opt.fft_min_taps) return false;
    // square mirror-symmetric stencils up to 23 x 23 are faster in the unrolled direct form (needs the device form: callers
    // run ensure_stencil first)
    const int which = (int)(&s - ctx->stencil);
    if (ctx->opt.stencil_fixed && ctx->opt.variant <= 0 && s.built_q && plan::fixed_stencil_radius(s.taps(), s.geom, &c, 1, fixed_preferred_max_r(ctx, which)))
        return false;
    return true;
}

// The rule of the halation's scratch element (FftConvArgs::dyn): the 12-byte element when max |x| <= bound x max(min x, floor).
//   |delta density| <= 0.434 x steepest curve cell x kDynCoefficient x (max / shadow) <= 3.6e-7  (three ulps of a density in [1, 2));
//   below the curve's first breakpoint np.interp clamps: no slope, so shadows under it do not count.
// kDynCoefficient = what the element costs a shadow's exposure, as a multiple of max / shadow: 1.5 x 2^-36.  The element keeps 36
// mantissa bits per component (half an ulp = 2^-37 of the value) and a scratch value is rounded twice (pass 1's store, pass 2's);
// the worst frame is a nearly flat bright field around a dark hole: all of a window's energy sits in one spectral line per row,
// whose two roundings reach every output of the window undiminished (the stencil's taps sum to 1) -- 2 x 2^-37 = 1.46e-11 of
// max / shadow.  A search over 1 050 random frames of seven families x five bright-region statistics found exactly that and nothing
// above it (1.43e-11 for holes in a jittered flat field; noise-like windows 1.0e-11, isolated speculars 4.5e-12:
// profiles/r06_scratch96_probe.txt; tests/test_gpu_fft.py repeats the search on a fixed budget).  Round 5 shipped 6.0e-12, the
// maximum of 16 hand-made probes without a flat field among them: too small by 2.4.  The factor
// 1.5 covers what no search of 7e5-pixel frames sees of a 1e8-pixel frame's tail.
constexpr double kDynCoefficient = 1.5 * 1.4551915228366852e-11;  // 1.5 x 2^-36 = 2.18e-11
void dyn_rule(const r2f_ctx* ctx, float* bound, float* floor) {
    const double slope = std::max((double)ctx->curve_slope_max, 1e-3);
    *bound = (float)std::min(3.6e-7 / (0.4343 * slope * kDynCoefficient), 1e7);
    *floor = (float)std::pow(10.0, (double)ctx->curve.x0);
}

// ------------------------------------------------------------------------------------------------ FFT form
// One call = the channels `chans` of a stencil (all with the same tap box) as fp64 overlap-save FFT correlations (r2f_fft.hip); their
// window pairs share the launches.  Everything the host decides about the call is plan::fft_call's (window, real spectrum, scratch
// element, batches, timing classes and bytes: r2f_plan.cpp, pinned on the CPU by tests/test_fft_call_host.py); what follows owns
// the device side of it -- the twiddle table, the spectrum cache, the lanes, the timing bracket -- and run_stencil_fft strings them.

// The facts fft_call plans from: the group's tap box and anchor, what r2f_set_kernel noted of its channels, the caller, the options.
static plan::FftCallIn fft_call_facts(const r2f_ctx* ctx, int which, const int* chans, int nch, const int box[4], int y0, int y1, int W,
                                      int epilogue, bool dyn) {
    const StencilSet& set = ctx->stencil[which];
    plan::FftCallIn in;
    in.bh = box[1] - box[0] + 1, in.bw = box[3] - box[2] + 1;
    in.ay = set.kh / 2 - box[0], in.ax = set.kw / 2 - box[2];
    in.nch = nch, in.which = which, in.W = W, in.y0 = y0, in.y1 = y1;
    in.all_unit_gain = true;
    for (int i = 0; i < nch; ++i) {
        in.any_mixed_sign = in.any_mixed_sign || set.mixed_sign[chans[i]];
        in.all_unit_gain = in.all_unit_gain && set.unit_gain[chans[i]];
    }
    in.symmetric = plan::centrally_symmetric(set.taps(), chans, nch, box);
    in.epilogue = epilogue, in.dyn = dyn, in.curve_set = ctx->curve.cells != nullptr;
    in.take_options(ctx->opt);
    return in;
}

// W_256^k, k < 256, then W_512^k, k < 256, then W_1024^k, k < 64: built and uploaded once per context.
static int ensure_twiddles(r2f_ctx* ctx) {
    if (ctx->fft.tw.p) return R2F_OK;
    std::vector<double> tw(4 * kFftN + 2 * 64);
    const double pi = 3.14159265358979323846264338327950288;
    for (int k = 0; k < kFftN; ++k) {
        tw[2 * k] = std::cos(-2.0 * pi * k / kFftN), tw[2 * k + 1] = std::sin(-2.0 * pi * k / kFftN);
        tw[2 * (kFftN + k)] = std::cos(-pi * k / kFftN), tw[2 * (kFftN + k) + 1] = std::sin(-pi * k / kFftN);
    }
    for (int k = 0; k < 64; ++k)
        tw[2 * (2 * kFftN + k)] = std::cos(-2.0 * pi * k / 1024.0), tw[2 * (2 * kFftN + k) + 1] = std::sin(-2.0 * pi * k / 1024.0);
    return upload(ctx, ctx->fft.tw, tw.data(), tw.size() * sizeof(double));
}

// What every launch of the call -- a spectrum build or a batch -- is told of its windows.
static FftConvArgs fft_window_args(const r2f_ctx* ctx, const plan::FftCallIn& in, const plan::FftCall& call, int cus) {
    FftConvArgs a;
    memset(&a, 0, sizeof a);
    a.tw = static_cast<const double2*>(ctx->fft.tw.p);
    a.tw512 = a.tw + kFftN;
    a.tw1024 = a.tw + 2 * kFftN;
    a.ny = call.b.ny, a.nx = call.b.nx;
    a.ay = in.ay, a.ax = in.ax;
    a.vy = call.b.vy, a.vx = call.b.vx;
    a.kreal = call.kreal, a.oy = call.oy, a.ox = call.ox;
    a.cols_walk = ctx->opt.fft_cols_walk;
    a.cols_slots = 2 * cus;
    return a;
}

// The spectrum of channel c's tap box for the call's window, from the cache; a missing or stale one (r2f_set_kernel, another
// stencil_fft_real) is built by the same two forward passes on the zero-padded kernel image -- the box in the window's top left
// corner (outputs from row / column 0 on), or, for a real spectrum, wrapped around the window with its anchor on the origin.
// `wa`: fft_window_args of the call; the passes use the start of the scratch (one complex128 image, reserved by the caller).
static int ensure_spectrum(r2f_ctx* ctx, int which, int c, const int box[4], const FftConvArgs& wa, hipStream_t s, const double2** out) {
    const size_t img = (size_t)wa.ny * wa.nx;
    ctx->fft.last[which][c] = {wa.ny * 4096 + wa.nx, wa.kreal};
    r2f_ctx::Fft::Spectrum& sp = ctx->fft.spectrum[which][c][r2f_ctx::Fft::shape_index(wa.ny, wa.nx)];
    if (!(sp.valid && sp.real == (wa.kreal != 0))) {
        const std::vector<float> kimg = plan::fft_kernel_image(ctx->stencil[which].taps(), c, box, wa.ny, wa.nx, wa.kreal != 0);
        int rc = upload(ctx, ctx->fft.kimg, kimg.data(), img * sizeof(float));
        if (rc) return rc;
        rc = sp.buf.reserve(ctx, img * sizeof(double2), Grow::SyncGeneration);
        if (rc) return rc;
        sp.real = wa.kreal != 0;
        FftConvArgs k = wa;
        k.src.data = static_cast<float*>(ctx->fft.kimg.p);
        k.raw = 1;
        k.s32 = 0;  // spectra are always built and kept in complex128
        k.nch = 1, k.chan[0] = 0, k.ppc = 1;
        k.ntiles = 1, k.gx = 1, k.npairs = 1, k.pair0 = 0;
        k.s1 = static_cast<double2*>(ctx->fft.s1.p);
        k.kf_out = static_cast<double2*>(sp.buf.p);
        R2F_HIP(ctx, launch_fft_rows_fwd(k, s));
        R2F_HIP(ctx, launch_fft_cols(k, 1, s));
        sp.valid = true;
    }
    *out = static_cast<const double2*>(sp.buf.p);
    return R2F_OK;
}

// The per-pair element of a call whose passes choose it on the device (element 3), from the exposure-range tiles its caller vouches
// for: one small launch on the caller's stream ahead of the passes (they fan out to the internal streams behind it).
static int queue_pair_flags(r2f_ctx* ctx, FftConvArgs* a, int W, hipStream_t s) {
    int rc = ensure_range_tiles(ctx, a->H_global, W);
    if (rc) return rc;
    rc = ctx->dyn_flags.reserve(ctx, (size_t)std::max(a->ppc, 1) * sizeof(int), Grow::SyncGeneration);
    if (rc) return rc;
    float bound, floor_;
    dyn_rule(ctx, &bound, &floor_);
    a->dyn_flags = static_cast<const int*>(ctx->dyn_flags.p);
    ctx->dyn_flags_ppc = a->ppc;
    R2F_HIP(ctx, launch_fft_decide(*a, record_of(ctx), bound, floor_, static_cast<int*>(ctx->dyn_flags.p), s));
    return R2F_OK;
}

// The lanes of a call: the caller's stream alone, or n internal streams (created on first use) that start behind everything queued
// on the caller's stream so far (src, spectra, flags) ...
static int fork_lanes(r2f_ctx* ctx, hipStream_t s, int n, hipStream_t lane[4]) {
    r2f_ctx::Fft& f = ctx->fft;
    for (int i = 0; i < 4; ++i) lane[i] = s;
    if (n <= 1) return R2F_OK;
    for (int i = 0; i < n; ++i) {
        if (!f.stream[i]) R2F_HIP(ctx, hipStreamCreateWithFlags(&f.stream[i], hipStreamNonBlocking));
        if (!f.ev_out[i]) R2F_HIP(ctx, hipEventCreateWithFlags(&f.ev_out[i], hipEventDisableTiming));
        lane[i] = f.stream[i];
    }
    if (!f.ev_in) R2F_HIP(ctx, hipEventCreateWithFlags(&f.ev_in, hipEventDisableTiming));
    R2F_HIP(ctx, hipEventRecord(f.ev_in, s));
    for (int i = 0; i < n; ++i) R2F_HIP(ctx, hipStreamWaitEvent(lane[i], f.ev_in, 0));
    return R2F_OK;
}
// ... and that the caller's stream waits for at the end.
static int join_lanes(r2f_ctx* ctx, hipStream_t s, int n, const hipStream_t lane[4]) {
    for (int i = 0; i < n && n > 1; ++i) {
        R2F_HIP(ctx, hipEventRecord(ctx->fft.ev_out[i], lane[i]));
        R2F_HIP(ctx, hipStreamWaitEvent(s, ctx->fft.ev_out[i], 0));
    }
    return R2F_OK;
}

// One launch, bracketed by timing events on its stream when kernel_timing asks for its class (r2f_kernel_timing reads them).
template <typename Launch>
static int timed_launch(r2f_ctx* ctx, int pass, int cls, double bytes, hipStream_t st, Launch&& launch) {
    if (!(ctx->opt.timing & (1 << pass))) {
        R2F_HIP(ctx, launch());
        return R2F_OK;
    }
    hipEvent_t e0, e1;
    R2F_HIP(ctx, hipEventCreate(&e0));
    R2F_HIP(ctx, hipEventCreate(&e1));
    R2F_HIP(ctx, hipEventRecord(e0, st));
    R2F_HIP(ctx, launch());
    R2F_HIP(ctx, hipEventRecord(e1, st));
    ctx->timing_ev[cls].push_back({e0, e1});
    ctx->timing_bytes[cls] += bytes;
    return R2F_OK;
}

// The launch arguments of the call, from its plan: fft_window_args `wa` plus what the call reads and writes.  (Per channel the
// spectrum, per batch pair0 / npairs / s1 and, when the element is chosen per pair, the flags are filled in where they are made.)
static FftConvArgs fft_call_args(const r2f_ctx* ctx, const FftConvArgs& wa, const plan::FftCall& call, const int* chans, int nch,
                                 const r2f_planes* src, const r2f_planes* dst, int y0, int y1, int W, int H, int epilogue, float log_eps) {
    FftConvArgs a = wa;
    a.src = to_dev(src), a.dst = to_dev(dst);
    a.nch = nch;
    for (int i = 0; i < nch; ++i) a.chan[i] = chans[i];
    a.y0 = y0, a.y1 = y1, a.W = W, a.H_global = H;
    a.s32 = call.element;
    a.gx = call.b.gx, a.ntiles = call.b.ntiles, a.ppc = call.b.ppc;
    a.epilogue = epilogue, a.epi_lds = ctx->opt.fft_epi_lds, a.curve = ctx->curve, a.log_eps = log_eps;
    a.vec4 = planes_vec_ok(dst, W) ? 1 : 0;
    return a;
}

// dyn: the caller vouches that the context's exposure-range record (its tiles) was kept for the samples `src` holds this frame: the
// passes may then choose their scratch element on the device, per window pair (FftConvArgs::dyn_flags, fft_decide_kernel).
static int run_stencil_fft(r2f_ctx* ctx, int which, const int* chans, int nch, const r2f_planes* src, const r2f_planes* dst, int y0,
                           int y1, int W, int H, int epilogue, float log_eps, hipStream_t s, bool dyn) {
    int box[4];
    plan::tap_box(ctx->stencil[which].taps(), chans[0], box);
    const plan::FftCallIn in = fft_call_facts(ctx, which, chans, nch, box, y0, y1, W, epilogue, dyn);
    const plan::FftCall call = plan::fft_call(in);
    if (!call.ok)
        return fail(ctx, R2F_EINVAL, "stencil %d: no FFT window shape fits a %d x %d tap box under the current stencil_fft_window* options",
                    which, in.bh, in.bw);
    const plan::FftBatches& fb = call.b;
    int rc = ensure_twiddles(ctx), cus = 0;
    if (rc || (rc = device_cu_count(ctx, &cus))) return rc;
    const FftConvArgs wa = fft_window_args(ctx, in, call, cus);
    FftConvArgs a = fft_call_args(ctx, wa, call, chans, nch, src, dst, y0, y1, W, H, epilogue, log_eps);
    rc = ctx->fft.s1.reserve(ctx, (size_t)fb.ny * fb.nx * sizeof(double2), Grow::SyncGeneration);  // (a spectrum build's image)
    for (int i = 0; i < nch && !rc; ++i) rc = ensure_spectrum(ctx, which, chans[i], box, wa, s, &a.kfs[i]);
    if (rc) return rc;
    if (call.element == 3) ctx->frame_dyn_armed = true;
    rc = ctx->fft.s1.reserve(ctx, fb.scratch_bytes, Grow::SyncGeneration);
    if (!rc && call.element == 3) rc = queue_pair_flags(ctx, &a, W, s);
    if (rc) return rc;
    hipStream_t lane[4];
    if ((rc = fork_lanes(ctx, s, fb.nstreams, lane))) return rc;
    for (int i = 0; i < fb.launches; ++i) {
        const plan::FftBatch bt = call.batch(i);
        hipStream_t st = lane[bt.lane];
        a.pair0 = bt.pair0, a.npairs = bt.npairs;
        a.s1 = reinterpret_cast<double2*>(static_cast<char*>(ctx->fft.s1.p) + bt.scratch_offset);
        const int cls = call.timing_offset;
        if ((rc = timed_launch(ctx, 0, cls + 0, bt.npairs * call.pass_bytes[0], st, [&] { return launch_fft_rows_fwd(a, st); }))) return rc;
        if ((rc = timed_launch(ctx, 1, cls + 1, bt.npairs * call.pass_bytes[1], st, [&] { return launch_fft_cols(a, 0, st); }))) return rc;
        if ((rc = timed_launch(ctx, 2, cls + 2, bt.npairs * call.pass_bytes[2], st, [&] { return launch_fft_rows_inv(a, st); }))) return rc;
    }
    return join_lanes(ctx, s, fb.nstreams, lane);
}

int run_stencil(r2f_ctx* ctx, int which, const r2f_planes* src, const r2f_planes* dst, int y0, int y1, int W, int H, int epilogue,
                float log_eps, hipStream_t s, bool skip_identity, bool dyn) {
    if (y1 <= y0) return R2F_OK;
    if (W <= 0 || H <= 0 || y0 < 0 || y1 > H) return fail(ctx, R2F_EINVAL, "stencil: bad geometry");
    StencilSet& set = ctx->stencil[which];
    if (!set.present) return fail(ctx, R2F_EINVAL, "stencil %d not set (r2f_set_kernel)", which);
    // choose the tile variant and LDS budget: the widest tile whose rows fit; wide stencils fall back to the
    // narrow tile and, if need be, to one workgroup per CU (the whole 160 KB)
    int variant = -1;
    const size_t budgets[2] = {(size_t)ctx->opt.lds_kb * 1024, kMaxLds};
    for (int b = 0; b < 2 && variant < 0; ++b) {
        for (int v = 0; v < kNumStencilVariants; ++v) {
            if (ctx->opt.variant >= 0 && v != ctx->opt.variant) continue;
            const StencilVariant& sv = kStencilVariants[v];
            int rc = ensure_stencil(ctx, which, sv.Q, sv.TW(), sv.TH(), budgets[b], false);
            if (rc == R2F_ETOOLARGE) continue;
            if (rc) return rc;
            if (stencil_lds_bytes(sv, set.dev, 3) <= kMaxLds) {
                variant = v;
                break;
            }
        }
    }
    if (variant < 0) return fail(ctx, R2F_ETOOLARGE, "stencil %d: %dx%d taps do not fit an LDS tile", which, set.kh, set.kw);
    int rc = check_rows(ctx, "stencil dst", dst, y0, y1);
    if (rc) return rc;
    for (int c = 0; c < 3; ++c) {
        const DevStencil& d = set.dev[c];
        rc = check_stencil_source(ctx, "stencil src", src, y0, y1, d.ay, d.kh - 1 - d.ay, H);
        if (rc) return rc;
    }
    if (epilogue == 1 && !ctx->curve.cells) return fail(ctx, R2F_EINVAL, "density curve not set (r2f_set_curve1d)");
    if (planes_overlap(src, dst, W))  // tiles (and FFT batches) read halo rows that others have already overwritten
        return fail(ctx, R2F_EINVAL, "stencil %d: source and destination planes overlap (the stencil stages are out of place)", which);
    StencilArgs a;
    for (int c = 0; c < 3; ++c) {
        a.st[c] = set.dev[c];
        if (ctx->opt.ablate == 3) a.st[c].wmul = 0;
    }
    a.src = to_dev(src);
    a.dst = to_dev(dst);
    a.y0 = y0;
    a.y1 = y1;
    a.W = W;
    a.H_global = H;
    a.epilogue = epilogue;
    a.curve = ctx->curve;
    a.log_eps = log_eps;
    // large kernels take the fp64 FFT form (channels with the same tap box share their launches); single taps are
    // pointwise; the direct kernel runs the rest
    a.nchan = 0;
    bool done[3] = {false, false, false};
    for (int c = 0; c < 3; ++c) {
        if (done[c]) continue;
        int tb[4];
        plan::tap_box(set.taps(), c, tb);
        if (fft_eligible(ctx, set, c)) {
            int group[3], ng = 0;
            for (int d = c; d < 3; ++d) {
                int ob[4];
                plan::tap_box(set.taps(), d, ob);
                if (!done[d] && fft_eligible(ctx, set, d) && !memcmp(ob, tb, sizeof tb)) group[ng++] = d, done[d] = true;
            }
            rc = run_stencil_fft(ctx, which, group, ng, src, dst, y0, y1, W, H, epilogue, log_eps, s, dyn);
            if (rc) return rc;
        } else if (tb[0] == tb[1] && tb[2] == tb[3] && tb[0] == set.kh / 2 && tb[2] == set.kw / 2 && ctx->opt.ablate == 0) {
            if (skip_identity) continue;
            TapArgs t;  // a single tap at the anchor: pointwise
            t.src = to_dev(src), t.dst = to_dev(dst);
            t.ch = c, t.y0 = y0, t.y1 = y1, t.W = W;
            t.w = set.host[((size_t)tb[0] * set.kw + tb[2]) * set.kc + (set.kc == 1 ? 0 : c)];
            t.epilogue = epilogue, t.curve = ctx->curve, t.log_eps = log_eps;
            t.vec = (planes_vec_ok(src, W) && planes_vec_ok(dst, W)) ? 1 : 0;
            R2F_HIP(ctx, launch_single_tap(t, s));
        } else {
            a.chan[a.nchan++] = c;
        }
    }
    if (a.nchan == 0) return R2F_OK;
    a.vec = planes_vec_ok(dst, W) ? 1 : 0;
    a.xcd_remap = ctx->opt.xcd_remap;
    a.order = nullptr;
    if (a.xcd_remap == 2) {
        const StencilVariant& sv = kStencilVariants[variant];
        rc = ensure_tile_order(ctx, (W + sv.TW() - 1) / sv.TW(), (y1 - y0 + sv.TH() - 1) / sv.TH(), &a.order);
        if (rc) return rc;
    }
    a.ablate = ctx->opt.ablate;
    // small square mirror-symmetric stencils (below the FFT threshold: up to 19 x 19) take the unrolled form
    a.fixed_r = 0;
    a.fixed_w = nullptr;
    if (variant == 0 && ctx->opt.stencil_fixed && ctx->opt.ablate == 0) {
        const int R = plan::fixed_stencil_radius(set.taps(), set.geom, a.chan, a.nchan, kFixedMaxR);
        if (R) {
            if (!ctx->stencil_fixed_valid[which]) {
                bool same;
                const std::vector<float> w = plan::fixed_stencil_weights(set.taps(), R, kStencilVariants[0].Q, &same);
                rc = upload(ctx, ctx->stencil_fixed_w[which], w.data(), w.size() * sizeof(float));
                if (rc) return rc;
                ctx->stencil_fixed_valid[which] = true;
            }
            a.fixed_r = R;
            a.fixed_w = static_cast<const float*>(ctx->stencil_fixed_w[which].p);
        }
    }
    R2F_HIP(ctx, launch_stencil(a, variant, s));
    return R2F_OK;
}

}  // namespace r2f

// The internal streams and their fences (created by fork_lanes on first use); the buffers free themselves.
r2f_ctx::Fft::~Fft() {
    for (int i = 0; i < 4; ++i) {
        if (stream[i]) (void)hipStreamDestroy(stream[i]);
        if (ev_out[i]) (void)hipEventDestroy(ev_out[i]);
    }
    if (ev_in) (void)hipEventDestroy(ev_in);
}
