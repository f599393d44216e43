// r2f_stencil.hip -- the stencil stages' dispatch: a stencil's device forms (entry lists, tile orders, the unrolled fixed form, FFT
// spectra) built on demand, and the choice between them per channel (run_stencil).
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

static plan::FftOptions fft_options(const r2f_ctx* ctx) {
    plan::FftOptions o;
    o.window = ctx->opt.fft_window;
    o.window_max = ctx->opt.fft_window_max;
    o.window_rows = ctx->opt.fft_window_rows;
    o.batch_mib = ctx->opt.fft_batch;
    o.streams = ctx->opt.fft_streams;
    o.even = ctx->opt.fft_even;
    return o;
}

// The channels `chans` of a stencil (all with the same tap box) as fp64 overlap-save FFT correlations (r2f_fft.hip);
// their window pairs share the launches.
// dyn: the caller vouches that the context's exposure-range record (its tiles) was kept for the samples `src` holds this frame: the
// passes may then choose their scratch element on the device, per window pair (FftConvArgs::dyn_flags, fft_decide_kernel).
static int run_stencil_fft(r2f_ctx* ctx, int which, const int* chans, int nch, const r2f_planes* src, const r2f_planes* dst, int y0,
                           int y1, int W, int H, int epilogue, float log_eps, hipStream_t s, bool dyn) {
    StencilSet& set = ctx->stencil[which];
    int b[4];
    plan::tap_box(set.taps(), chans[0], b);
    const int bh = b[1] - b[0] + 1, bw = b[3] - b[2] + 1;
    int ny = 256, nx = 256;
    // (the rows of THIS call, not of the global frame: a row shard's 1 058-row call is 6.15 window rows of 172 and should not be
    // planned as if the seventh were free -- VERDICT r3, next 4; a whole-frame call sees the frame as before)
    const plan::FftOptions fo = fft_options(ctx);
    // scratch element of THIS launch: complex64 only where the stencil's bit says so and no channel of the group has cancelling taps
    // (those keep complex128: no float32 rounding between the passes either) -- the window choice is priced with it
    bool s32_eff = (ctx->opt.fft_s32 >> which) & 1;
    for (int i = 0; i < nch; ++i)
        if (set.mixed_sign[chans[i]] && ctx->opt.fft_mixed_sign) s32_eff = false;
    if (!plan::fft_window(fo, bh, bw, W, y1 - y0, s32_eff, &ny, &nx))
        return fail(ctx, R2F_EINVAL, "stencil %d: no FFT window shape fits a %d x %d tap box under the current stencil_fft_window* options",
                    which, bh, bw);
    const size_t img = (size_t)ny * nx;
    const int shape = r2f_ctx::Fft::shape_index(ny, nx);
    if (!ctx->fft.tw.p) {
        // W_256^k, k < 256, then W_512^k, k < 256, then W_1024^k, k < 64
        std::vector<double> tw(4 * kFftN + 2 * 64);
        const double pi = 3.14159265358979323846264338327950288;
        for (int k = 0; k < kFftN; ++k) {
            tw[2 * k] = std::cos(-2.0 * pi * k / kFftN), tw[2 * k + 1] = std::sin(-2.0 * pi * k / kFftN);
            tw[2 * (kFftN + k)] = std::cos(-pi * k / kFftN), tw[2 * (kFftN + k) + 1] = std::sin(-pi * k / kFftN);
        }
        for (int k = 0; k < 64; ++k)
            tw[2 * (2 * kFftN + k)] = std::cos(-2.0 * pi * k / 1024.0), tw[2 * (2 * kFftN + k) + 1] = std::sin(-2.0 * pi * k / 1024.0);
        int rc = upload(ctx, ctx->fft.tw, tw.data(), tw.size() * sizeof(double));
        if (rc) return rc;
    }
    FftConvArgs a;
    memset(&a, 0, sizeof a);
    a.tw = static_cast<const double2*>(ctx->fft.tw.p);
    a.tw512 = a.tw + kFftN;
    a.tw1024 = a.tw + 2 * kFftN;
    a.ny = ny, a.nx = nx;
    a.ay = set.kh / 2 - b[0];  // anchor (kh/2, kw/2): cv.filter2D's default
    a.ax = set.kw / 2 - b[2];
    a.vy = ny - bh + 1;
    a.vx = (nx - bw + 1) & ~3;  // a multiple of 4: window origins stay 16-byte aligned for the float4 stores of pass 3
    // Real spectra: every channel of the group centrally symmetric around an anchor at the centre of its (odd x odd) box
    const bool kreal = ctx->opt.fft_real && plan::centrally_symmetric(set.taps(), chans, nch, b);
    a.kreal = kreal ? 1 : 0;
    a.oy = kreal ? a.ay : 0;
    a.ox = kreal ? a.ax : 0;
    int cus = 0;
    if (const int rc = device_cu_count(ctx, &cus)) return rc;
    a.cols_walk = ctx->opt.fft_cols_walk;
    a.cols_slots = 2 * cus;
    int rc = ctx->fft.s1.reserve(ctx, img * sizeof(double2), Grow::SyncGeneration);
    if (rc) return rc;
    for (int i = 0; i < nch; ++i) {
        const int c = chans[i];
        ctx->fft.kf_dims[which][c] = ny * 4096 + nx;
        ctx->fft.last_real[which][c] = kreal ? 1 : 0;
        if (ctx->fft.kf_valid[which][c][shape] && ctx->fft.kf_real[which][c][shape] == kreal) continue;
        // the kernel's spectrum: the same two forward passes on its zero-padded image -- the box in the window's top left corner
        // (outputs from row / column 0 on), or, for a real spectrum, wrapped around the window with its anchor on the origin
        const std::vector<float> kimg = plan::fft_kernel_image(set.taps(), c, b, ny, nx, kreal);
        rc = upload(ctx, ctx->fft.kimg, kimg.data(), img * sizeof(float));
        if (rc) return rc;
        rc = ctx->fft.kf[which][c][shape].reserve(ctx, img * sizeof(double2), Grow::SyncGeneration);
        if (rc) return rc;
        ctx->fft.kf_real[which][c][shape] = kreal;
        FftConvArgs k = a;
        k.src.data = static_cast<float*>(ctx->fft.kimg.p);
        k.raw = 1;
        k.s32 = 0;  // spectra are always built and kept in complex128
        k.nch = 1, k.chan[0] = 0, k.ppc = 1;
        k.ntiles = 1, k.gx = 1, k.npairs = 1, k.pair0 = 0;
        k.s1 = static_cast<double2*>(ctx->fft.s1.p);
        k.kf_out = static_cast<double2*>(ctx->fft.kf[which][c][shape].p);
        R2F_HIP(ctx, launch_fft_rows_fwd(k, s));
        R2F_HIP(ctx, launch_fft_cols(k, 1, s));
        ctx->fft.kf_valid[which][c][shape] = true;
    }
    a.src = to_dev(src);
    a.dst = to_dev(dst);
    a.nch = nch;
    for (int i = 0; i < nch; ++i) {
        a.chan[i] = chans[i];
        a.kfs[i] = static_cast<const double2*>(ctx->fft.kf[which][chans[i]][shape].p);
    }
    a.y0 = y0, a.y1 = y1, a.W = W, a.H_global = H;
    a.s32 = ((ctx->opt.fft_s96 >> which) & 1) ? 2 : (s32_eff ? 1 : 0);
    for (int i = 0; i < nch; ++i)
        if (set.mixed_sign[chans[i]] && ctx->opt.fft_mixed_sign) a.s32 = 0;  // (the 12-byte element neither)
    // the halation of a whole-frame render whose front kernel recorded the range of the exposure planes: element chosen on the device.
    // The guard compares a window's SAMPLES; it speaks for the outputs only under a stencil of unit gain (the reference's halation
    // kernels are normalised and non-negative, effects.py:200-217): taps that cancel or sum to 0.01 make outputs far below the samples
    bool unit_gain = true;
    for (int i = 0; i < nch; ++i) unit_gain = unit_gain && set.unit_gain[chans[i]];
    if (a.s32 == 0 && which == R2F_KERNEL_HALATION && epilogue == 1 && dyn && ctx->opt.fft_s96_auto && a.kreal && unit_gain &&
        ny == 256 && ctx->opt.fft_cols_walk && ctx->curve.cells) {
        a.s32 = 3;  // (the flags are worked out below, once the call's tiling is known)
        ctx->frame_dyn_armed = true;
    }
    const plan::FftBatches fb = plan::fft_batches(fo, ny, nx, bh, bw, W, y0, y1, nch, a.s32 == 1 ? 8 : (a.s32 == 2 ? 12 : 16));  // (3: sized for 16)
    a.gx = fb.gx;
    a.ntiles = fb.ntiles;
    a.ppc = fb.ppc;
    a.epilogue = epilogue;
    a.epi_lds = ctx->opt.fft_epi_lds;
    a.curve = ctx->curve;
    a.log_eps = log_eps;
    a.vec4 = planes_vec_ok(dst, W) ? 1 : 0;
    const size_t img_bytes = fb.img_bytes;
    const int pairs = fb.pairs, nstreams = fb.nstreams, batch = fb.batch;
    rc = ctx->fft.s1.reserve(ctx, fb.scratch_bytes, Grow::SyncGeneration);
    if (rc) return rc;
    if (a.s32 == 3) {
        // the element of every window pair of this call, from the exposure-range tiles its caller vouches for: one small launch on the
        // caller's stream ahead of the passes (they fan out to the internal streams behind it)
        rc = ensure_range_tiles(ctx, H, W);
        if (rc) return rc;
        rc = ctx->dyn_flags.reserve(ctx, (size_t)std::max(fb.ppc, 1) * sizeof(int), Grow::SyncGeneration);
        if (rc) return rc;
        float bound, floor_;
        dyn_rule(ctx, &bound, &floor_);
        a.dyn_flags = static_cast<const int*>(ctx->dyn_flags.p);
        ctx->dyn_flags_ppc = fb.ppc;
        R2F_HIP(ctx, launch_fft_decide(a, record_of(ctx), bound, floor_, static_cast<int*>(ctx->dyn_flags.p), s));
    }
    hipStream_t lanes[4] = {s, s, s, s};
    if (nstreams > 1) {
        for (int i = 0; i < nstreams; ++i) {
            if (!ctx->fft.stream[i]) R2F_HIP(ctx, hipStreamCreateWithFlags(&ctx->fft.stream[i], hipStreamNonBlocking));
            if (!ctx->fft.ev_out[i]) R2F_HIP(ctx, hipEventCreateWithFlags(&ctx->fft.ev_out[i], hipEventDisableTiming));
            lanes[i] = ctx->fft.stream[i];
        }
        if (!ctx->fft.ev_in) R2F_HIP(ctx, hipEventCreateWithFlags(&ctx->fft.ev_in, hipEventDisableTiming));
        R2F_HIP(ctx, hipEventRecord(ctx->fft.ev_in, s));  // everything queued on the caller's stream so far (src, spectra)
        for (int i = 0; i < nstreams; ++i) R2F_HIP(ctx, hipStreamWaitEvent(lanes[i], ctx->fft.ev_in, 0));
    }
    auto timed = [&](int cls, double bytes, hipStream_t st, auto&& launch) -> int {
        if (!(ctx->opt.timing & (1 << cls))) {
            R2F_HIP(ctx, launch());
            return R2F_OK;
        }
        hipEvent_t e0, e1;
        R2F_HIP(ctx, hipEventCreate(&e0));
        R2F_HIP(ctx, hipEventCreate(&e1));
        R2F_HIP(ctx, hipEventRecord(e0, st));
        R2F_HIP(ctx, launch());
        R2F_HIP(ctx, hipEventRecord(e1, st));
        ctx->timing_ev[cls + 3 * (a.s32 == 1)].push_back({e0, e1});
        ctx->timing_bytes[cls + 3 * (a.s32 == 1)] += bytes;
        return R2F_OK;
    };
    int turn = 0;
    for (int p0 = 0; p0 < pairs; p0 += batch, turn = (turn + 1) % nstreams) {
        const int li = turn;
        hipStream_t st = lanes[li];
        a.pair0 = p0;
        a.npairs = std::min(batch, pairs - p0);
        a.s1 = reinterpret_cast<double2*>(static_cast<char*>(ctx->fft.s1.p) + (size_t)li * batch * img_bytes);
        // algorithmic bytes of the passes: window floats in (2 per pair) + scratch image out; scratch in + valid rows out;
        // valid rows in + valid outputs out.  The kernel spectrum (1 MB) stays in L2.
        const double np = a.npairs, full = (double)img_bytes, part = full * a.vy / ny;
        rc = timed(0, np * (2.0 * img * sizeof(float) + full), st, [&] { return launch_fft_rows_fwd(a, st); });
        if (rc) return rc;
        rc = timed(1, np * (full + part), st, [&] { return launch_fft_cols(a, 0, st); });
        if (rc) return rc;
        rc = timed(2, np * (part + 2.0 * a.vy * a.vx * sizeof(float)), st, [&] { return launch_fft_rows_inv(a, st); });
        if (rc) return rc;
    }
    if (nstreams > 1)
        for (int i = 0; i < nstreams; ++i) {
            R2F_HIP(ctx, hipEventRecord(ctx->fft.ev_out[i], lanes[i]));
            R2F_HIP(ctx, hipStreamWaitEvent(s, ctx->fft.ev_out[i], 0));
        }
    return R2F_OK;
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

// The internal streams and their fences (created by run_stencil_fft on first use); the buffers free themselves.
r2f_ctx::Fft::~Fft() {
    for (int i = 0; i < 4; ++i) {
        if (stream[i]) (void)hipStreamDestroy(stream[i]);
        if (ev_out[i]) (void)hipEventDestroy(ev_out[i]);
    }
    if (ev_in) (void)hipEventDestroy(ev_in);
}
