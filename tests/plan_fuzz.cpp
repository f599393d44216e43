// plan_fuzz.cpp -- fuzz harness for the host-side planners of libr2f_hip.so (raw2film_amd/csrc/r2f_plan.cpp), built by
// tests/test_plan_sanitizers.py with `g++ -fsanitize=address,undefined -fno-sanitize-recover=all` and run as a child process:
// the sanitizers abort on the first out-of-bounds access, overflow or invalid cast; the checks below abort on a plan that breaks
// its own contract (for an entry list: stream_consistent in r2f_plan.cpp -- every tap once per output row, the LDS offsets, and the
// live-column masks of every row step's first and last entry recomputed from the taps).  The random stencils include the sparsity
// of tests/exact_taps.py's families (ragged rows, runs of zero rows and columns, isolated taps, tap boxes beside the anchor), and
// stencil_source_rows is held to the brute-force hull of the rows read, with a negative reach above or below.
// Test infrastructure: nothing in the product links this file.
//
//   plan_fuzz <seed> <cases>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/r2f.h"
#include "../raw2film_amd/csrc/r2f_plan.h"

using namespace r2f::plan;

static uint64_t g_state = 1;
static uint32_t rnd() {  // xorshift64*
    g_state ^= g_state >> 12, g_state ^= g_state << 25, g_state ^= g_state >> 27;
    return (uint32_t)((g_state * 2685821237ULL) >> 32);
}
static int rint_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }
static float rfloat() { return (float)(rnd() >> 8) / 16777216.f; }
template <class T>
static T pick(std::initializer_list<T> v) { return *(v.begin() + rnd() % v.size()); }

#define CHECK(cond, ...)                                              \
    do {                                                              \
        if (!(cond)) {                                                \
            fprintf(stderr, "plan_fuzz: %s failed: ", #cond);         \
            fprintf(stderr, __VA_ARGS__);                             \
            fprintf(stderr, "\n");                                    \
            abort();                                                  \
        }                                                             \
    } while (0)

// frame sizes 1 .. 16384 with the small and the awkward ones over-represented
static int frame_dim() {
    switch (rnd() % 6) {
        case 0: return rint_in(1, 8);
        case 1: return rint_in(1, 300);
        case 2: return pick({255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 8192, 12288, 16383, 16384});
        default: return rint_in(1, 16384);
    }
}
static int tap_dim() {
    switch (rnd() % 5) {
        case 0: return rint_in(1, 12);
        case 1: return pick({19, 20, 21, 35, 85, 87, 199, 200, 201, 255, 256, 257, 399, 400});
        default: return rint_in(1, 400);
    }
}

static void fuzz_fft() {
    const int bh = tap_dim(), bw = tap_dim(), W = frame_dim(), H = frame_dim(), nch = rint_in(1, 3);
    const int elem = pick({16, 8, 12});
    const int window = pick({0, 0, 256, 512, 1024}), window_rows = pick({0, 0, 256, 512}), window_max = pick({256, 512, 512, 1024});
    const int batch = pick({1, 2, 7, 64, 192, 256, 4096}), streams = rint_in(1, 4);
    // a row range of the frame, like a shard's call
    const int y0 = rint_in(0, H - 1), y1 = rint_in(y0 + 1, H);
    r2f_fft_plan p;
    memset(&p, 0, sizeof p);
    const int rc = r2f_plan_fft(bh, bw, W, y1 - y0, nch, elem, window, window_rows, window_max, batch, streams, &p);
    if (rc != R2F_OK) {
        // no window keeps outputs only when a forced axis cannot hold the box
        const bool rows_forced_small = window_rows == 256 && bh <= 200 ? false : false;
        (void)rows_forced_small;
        CHECK(rc == R2F_EINVAL, "rc %d", rc);
        const bool must_fit = (bh <= 200 || true) && (bw <= 200 || true);
        (void)must_fit;
        // with nothing forced a shape always exists for boxes up to 400 taps
        if (window == 0 && window_rows == 0) CHECK(false, "no window for %d x %d taps on %d x %d (max %d)", bh, bw, W, H, window_max);
        return;
    }
    CHECK((p.ny == 256 || p.ny == 512) && (p.nx == 256 || p.nx == 512 || p.nx == 1024), "shape %d x %d", p.ny, p.nx);
    CHECK(p.vy == p.ny - bh + 1 && p.vy >= 1 && p.vx >= 4 && p.vx % 4 == 0 && p.vx <= p.nx - bw + 1, "valid %d x %d", p.vy, p.vx);
    CHECK((long long)p.gx * p.vx >= W && (long long)(p.gx - 1) * p.vx < W, "gx %d vx %d W %d", p.gx, p.vx, W);
    const int gyw = p.ntiles / p.gx;
    CHECK(p.ntiles == gyw * p.gx && (long long)gyw * p.vy >= y1 - y0 && (long long)(gyw - 1) * p.vy < y1 - y0, "tiles %d", p.ntiles);
    CHECK(p.pairs_per_channel == (p.ntiles + 1) / 2 && p.pairs == p.pairs_per_channel * nch, "pairs %d", p.pairs);
    CHECK(p.batch >= 1 && p.batch <= p.pairs && p.streams >= 1 && p.streams <= streams, "batch %d streams %d", p.batch, p.streams);
    CHECK((long long)p.launches * p.batch >= p.pairs && (long long)(p.launches - 1) * p.batch < p.pairs, "launches %d", p.launches);
    CHECK(p.scratch_bytes == (uint64_t)p.batch * p.streams * p.ny * p.nx * elem, "scratch %llu", (unsigned long long)p.scratch_bytes);
    if (window_rows && bh <= 200) CHECK(p.ny == window_rows, "rows forced %d got %d", window_rows, p.ny);
    if (window && bw <= 200) CHECK(p.nx == window, "columns forced %d got %d", window, p.nx);
    if (bh > 200) CHECK(p.ny == 512, "tall box in %d rows", p.ny);
    if (bw > 200) CHECK(p.nx >= 512, "wide box in %d columns", p.nx);
    // The batch walk of the device call (plan::fft_call, the rows [y0, y1) this time): the batches cover the pairs once and in order,
    // on lanes that exist, inside the scratch; only the batches of one lane share scratch.  (A wrong offset stops here, not on a GPU.)
    FftCallIn in;
    in.bh = bh, in.bw = bw, in.nch = nch, in.W = W, in.y0 = y0, in.y1 = y1;
    in.fo.window = window, in.fo.window_rows = window_rows, in.fo.window_max = window_max, in.fo.batch_mib = batch, in.fo.streams = streams;
    in.fo.even = (int)(rnd() % 2);
    in.which = rint_in(0, 1);
    in.fft_s32 = (elem == 8 ? 1 : 0) << in.which, in.fft_s96 = (elem == 12 ? 1 : 0) << in.which;
    const FftCall c = fft_call(in);
    CHECK(c.ok && c.elem_bytes == elem, "element %d sized by %d, wanted %d", c.element, c.elem_bytes, elem);
    const FftBatches& b = c.b;
    CHECK(b.ny == p.ny && b.nx == p.nx && b.vy == p.vy && b.vx == p.vx && b.img_bytes == (size_t)p.ny * p.nx * elem, "call window %d x %d", b.ny, b.nx);
    CHECK(b.pairs == p.pairs && b.nstreams >= 1 && b.nstreams <= streams && b.launches >= 1, "call pairs %d streams %d", b.pairs, b.nstreams);
    if (in.fo.even) CHECK(b.batch == p.batch && b.launches == p.launches && b.scratch_bytes == p.scratch_bytes, "call batch %d", b.batch);
    int next = 0;
    size_t lane_lo[4] = {0, 0, 0, 0}, lane_hi[4] = {0, 0, 0, 0};
    for (int i = 0; i < b.launches; ++i) {
        const FftBatch t = c.batch(i);
        CHECK(t.pair0 == next && t.npairs >= 1, "batch %d starts at pair %d, not %d", i, t.pair0, next);
        next += t.npairs;
        CHECK(t.lane >= 0 && t.lane < b.nstreams, "batch %d on lane %d of %d", i, t.lane, b.nstreams);
        const size_t lo = t.scratch_offset, hi = lo + (size_t)t.npairs * b.img_bytes;
        CHECK(hi <= b.scratch_bytes, "batch %d: scratch [%zu, %zu) of %zu", i, lo, hi, b.scratch_bytes);
        if (lane_hi[t.lane]) CHECK(lo == lane_lo[t.lane], "batch %d: lane %d moved its scratch", i, t.lane);
        lane_lo[t.lane] = lo, lane_hi[t.lane] = std::max(lane_hi[t.lane], hi);
    }
    CHECK(next == b.pairs, "batches cover %d of %d pairs", next, b.pairs);
    for (int l = 0; l < b.nstreams; ++l)
        for (int m = l + 1; m < b.nstreams; ++m)
            if (lane_hi[l] && lane_hi[m]) CHECK(lane_hi[l] <= lane_lo[m] || lane_hi[m] <= lane_lo[l], "lanes %d and %d share scratch", l, m);
}

// stencil_source_rows against brute force.  `above` / `below` as run_stencil derives them from a tap box and the anchor: they sum
// to the box's height - 1 >= 0, and one of them is negative when the box does not hold the anchor row (a pure translation).  The
// rows reflect-101 visits must lie inside [lo, hi) and touch both ends: a row more would refuse a caller's exact window.
static int reflect101_host(long long i, int n) {
    if (n == 1) return 0;
    const long long p = 2LL * n - 2;
    i %= p;
    if (i < 0) i += p;
    return (int)(i < n ? i : p - i);
}
static void check_source_rows() {
    const int H = rnd() % 3 ? rint_in(1, 40) : frame_dim(), y0 = rint_in(0, H - 1), y1 = rnd() % 4 ? std::min(H, y0 + rint_in(1, 70)) : rint_in(y0 + 1, H);
    const int taps = rnd() % 3 ? rint_in(1, 90) : rint_in(1, 400);
    const int above = rnd() % 2 ? rint_in(0, taps - 1) : rint_in(-250, 250), below = taps - 1 - above;
    int lo = -1, hi = -1;
    stencil_source_rows(y0, y1, above, below, H, &lo, &hi);
    CHECK(lo >= 0 && hi <= H && lo < hi, "source rows [%d, %d) for [%d, %d) of %d, above %d below %d", lo, hi, y0, y1, H, above, below);
    if (above >= 0 && below >= 0) CHECK(lo <= y0 && hi >= y1, "source rows [%d, %d) do not hold [%d, %d)", lo, hi, y0, y1);
    int seen_lo = H, seen_hi = -1;
    for (long long i = (long long)y0 - above; i <= (long long)y1 - 1 + below; ++i) {
        const int s = reflect101_host(i, H);
        seen_lo = std::min(seen_lo, s), seen_hi = std::max(seen_hi, s);
    }
    CHECK(seen_lo == lo && seen_hi + 1 == hi, "source rows [%d, %d), visited [%d, %d]: outputs [%d, %d) of %d, above %d below %d", lo, hi, seen_lo,
          seen_hi, y0, y1, H, above, below);
}

static void fuzz_stencil() {
    // a random stencil: dense, sparse, disc-like, mirror symmetric or not, with zero borders (cropping) and zero planes
    int kh = rnd() % 4 ? rint_in(1, 40) : tap_dim(), kw = rnd() % 4 ? rint_in(1, 40) : tap_dim();
    if ((long long)kh * kw > 120 * 120) kh = std::min(kh, 120), kw = std::min(kw, 120);  // keep a case cheap
    const int kc = pick({1, 3});
    std::vector<float> k((size_t)kh * kw * kc, 0.f);
    const int mode = rnd() % 5;
    const int zb_i = rnd() % 3 ? 0 : rint_in(0, kh / 3), zb_j = rnd() % 3 ? 0 : rint_in(0, kw / 3);
    for (int c = 0; c < kc; ++c)
        for (int i = zb_i; i < kh - zb_i; ++i)
            for (int j = zb_j; j < kw - zb_j; ++j) {
                float v = rfloat() - (mode == 3 ? 0.3f : 0.f);
                if (mode == 1 && rnd() % 4) v = 0.f;
                if (mode == 2) {  // a disc around the centre
                    const float di = i - kh / 2, dj = j - kw / 2;
                    if (di * di + dj * dj > 0.25f * std::min(kh, kw) * std::min(kh, kw)) v = 0.f;
                }
                k[((size_t)i * kw + j) * kc + c] = v;
            }
    // the sparsity no dense box or disc has (tests/exact_taps.py's families): every row with a first and last column of its own, runs
    // of 1 .. 5 all-zero rows and all-zero columns inside the box, a few isolated taps in an empty box, a tap box beside the anchor
    const int sparse = rnd() % 8;
    for (int c = 0; c < kc && sparse < 4; ++c) {
        auto at = [&](int i, int j) -> float& { return k[((size_t)i * kw + j) * kc + c]; };
        if (sparse == 0) {  // ragged rows; some collapse to one chunk or one tap
            for (int i = 0; i < kh; ++i) {
                int f = rint_in(0, kw - 1), l = rint_in(0, kw - 1);
                if (f > l) std::swap(f, l);
                if (rnd() % 6 == 0) l = std::min(l, f + (int)(rnd() % 4));
                for (int j = 0; j < kw; ++j)
                    if (j < f || j > l) at(i, j) = 0.f;
                if (rnd() % 2) at(i, f) = at(i, l) = 0.25f;
            }
        } else if (sparse == 1) {  // zero rows in runs, zero columns
            for (int i = rint_in(0, 3), run = 1; i < kh; i += run + rint_in(1, 3), run = run % 5 + 1)
                for (int z = i; z < std::min(kh, i + run); ++z)
                    for (int j = 0; j < kw; ++j) at(z, j) = 0.f;
            for (int j = rint_in(0, 4); j < kw; j += rint_in(1, 9)) {
                const int run = rnd() % 3 ? 1 : 4;
                for (int z = j; z < std::min(kw, j + run); ++z)
                    for (int i = 0; i < kh; ++i) at(i, z) = 0.f;
            }
        } else {  // isolated taps: the corners and the centre of a box (2), or a small cluster anywhere -- beside the anchor as a rule (3)
            for (int i = 0; i < kh; ++i)
                for (int j = 0; j < kw; ++j) at(i, j) = 0.f;
            if (sparse == 2) {
                at(0, 0) = at(0, kw - 1) = at(kh - 1, 0) = at(kh - 1, kw - 1) = 0.125f, at(kh / 2, kw / 2) = 0.5f;
                for (int n = 0; n < 10; ++n) at(rint_in(0, kh - 1), rint_in(0, kw - 1)) = rfloat() - 0.5f;
            } else {
                const int i0 = rint_in(0, kh - 1), j0 = rint_in(0, kw - 1), ch = rint_in(1, 3), cw = rint_in(1, 5);
                for (int i = i0; i < std::min(kh, i0 + ch); ++i)
                    for (int j = j0; j < std::min(kw, j0 + cw); ++j) at(i, j) = 0.5f - rfloat();
            }
        }
    }
    if (mode != 3 && rnd() % 2)  // mirror the left half onto the right one, bit for bit
        for (int c = 0; c < kc; ++c)
            for (int i = 0; i < kh; ++i)
                for (int j = 0; j < kw / 2; ++j) k[((size_t)i * kw + (kw - 1 - j)) * kc + c] = k[((size_t)i * kw + j) * kc + c];
    if (mode == 4 && kc == 3)  // one plane all zero, one a single tap at the anchor
        for (int i = 0; i < kh; ++i)
            for (int j = 0; j < kw; ++j) {
                k[((size_t)i * kw + j) * 3 + 1] = 0.f;
                k[((size_t)i * kw + j) * 3 + 2] = (i == kh / 2 && j == kw / 2) ? 1.f : 0.f;
            }
    const Taps t{k.data(), kh, kw, kc};
    const int c = rint_in(0, 2);
    int box[4];
    tap_box(t, c, box);
    CHECK(box[0] >= 0 && box[1] < kh && box[0] <= box[1] && box[2] >= 0 && box[3] < kw && box[2] <= box[3], "box");
    float w1 = 0.f;
    (void)single_tap_channel(t, c, &w1);
    // the three tile variants of the direct kernel and the tail tile, with the budgets the library uses
    const int Q = pick({2, 4}), TW = pick({64, 128}), TH = Q * pick({8, 16, 32});
    const int budget = pick({0, 0, 8 * 1024, 40 * 1024, 80 * 1024, 160 * 1024});
    int out8[8];
    const int rc = r2f_plan_stencil(k.data(), kh, kw, kc, c, Q, TW, TH, budget, rnd() % 4 != 0, out8);
    CHECK(rc == R2F_OK || rc == R2F_ETOOLARGE, "plan_stencil rc %d (a planner bug: the entry list does not reproduce its taps)", rc);
    if (rc == R2F_OK) {
        CHECK(out8[0] >= 0 && out8[1] >= 0 && (out8[0] == 0) == (out8[1] == 0) && out8[2] >= 1 && out8[6] == TW + (out8[5] + 3) / 4 * 4, "geometry");
        if (budget) CHECK(((long long)out8[7] * out8[6] + 16) * 4 <= budget, "phase of %d rows x %d floats exceeds %d bytes", out8[7], out8[6], budget);
    } else {
        CHECK(budget != 0, "too large without a budget");
    }
    // unrolled / separable forms on what the planner produced
    StencilGeom geom[3];
    StreamHost sh;
    for (int ch = 0; ch < 3; ++ch) {
        int b[4];
        tap_box(t, ch, b);
        (void)plan_stencil_channel(t, ch, b, mirror_symmetric(t, ch, b), Q, TW, TH, 0, &geom[ch], &sh);
    }
    const int chans[3] = {0, 1, 2};
    const int R = fixed_stencil_radius(t, geom, chans, 3, 11);
    CHECK(R >= 0 && R <= 11, "R %d", R);
    if (R) {
        bool same;
        const std::vector<float> w = fixed_stencil_weights(t, R, Q, &same);
        CHECK(w.size() == (size_t)3 * (2 * R + Q) * (R + 1) * (Q / 2) * 2, "fixed weights");
        float u[3][19], v[3][10];
        if (R <= 9) (void)separable_taps(t, R, u, v);
    }
    check_source_rows();
}

static void fuzz_tables() {
    {  // tile orders
        const int gx = rint_in(1, 200), gy = rint_in(1, 200), band = rnd() % 2 ? 0 : rint_in(1, 64);
        std::vector<int> order((size_t)gx * gy, -1), count((size_t)gx * gy, 0);
        CHECK(r2f_plan_tile_order(gx, gy, band, order.data()) == R2F_OK, "tile order");
        for (int v : order) {
            CHECK(v >= 0 && v < gx * gy, "tile %d of %d", v, gx * gy);
            ++count[(size_t)v];
        }
        for (int n : count) CHECK(n == 1, "not a permutation");
    }
    {  // LANCZOS4 tables
        const int ss = rnd() % 3 ? rint_in(1, 400) : frame_dim(), ds = rnd() % 3 ? rint_in(1, 400) : frame_dim();
        std::vector<int> ofs((size_t)ds);
        std::vector<short> cs((size_t)ds * 8);
        std::vector<float> cf((size_t)ds * 8);
        CHECK(r2f_lanczos4_table(ss, ds, ofs.data(), cs.data()) == R2F_OK, "lanczos u8");
        for (int d = 0; d < ds; ++d) {
            int sum = 0;
            for (int kk = 0; kk < 8; ++kk) sum += cs[(size_t)d * 8 + kk];
            CHECK(ofs[(size_t)d] >= -1 && ofs[(size_t)d] <= ss && std::abs(sum - 2048) <= 8, "u8 row %d: ofs %d sum %d", d, ofs[(size_t)d], sum);
        }
        CHECK(r2f_lanczos4_table_f32(ss, ds, ofs.data(), cf.data()) == R2F_OK, "lanczos f32");
        for (float v : cf) CHECK(std::isfinite(v), "non-finite weight");
    }
    {  // curve cells: monotone, with repeats, tiny and huge ranges
        const int m = rnd() % 4 ? rint_in(2, 300) : pick({2, 3, 1024, 4096});
        std::vector<float> lut((size_t)4 * m);
        float x = (rfloat() - 0.5f) * pick({1.f, 1e-6f, 1e6f, 1e30f});
        const float step = pick({1e-3f, 1.f, 1e-30f, 1e20f});
        for (int i = 0; i < m; ++i) {
            lut[(size_t)i] = x;
            if (rnd() % 8) x += step * rfloat();
        }
        for (size_t i = (size_t)m; i < lut.size(); ++i) lut[i] = (rfloat() - 0.5f) * 8.f;
        CurveCells cc;
        const int rc = curve_cells(lut.data(), m, &cc);
        CHECK(rc == 0 && cc.cells.size() == (size_t)3 * (m - 1) * 4 && (cc.near == 0 || cc.near == 1), "curve cells");
        lut[(size_t)rint_in(0, m - 1)] = NAN;  // a table with a NaN abscissa is refused (m == 2: the NaN breaks the only comparison)
        CHECK(curve_cells(lut.data(), m, &cc) == -1, "NaN abscissa accepted");
    }
    {  // Gaussian tables, workspace sizes
        float w[kChromaMaxTaps];
        const int size = rint_in(-2, 40);
        const bool ok = chroma_weights(size, w);
        CHECK(ok == (size >= 1 && 2 * size + 1 <= kChromaMaxTaps), "chroma size %d", size);
        if (ok) {
            float s = 0.f;
            for (int i = 0; i <= 2 * size; ++i) s += w[i];
            CHECK(std::fabs(s - 1.f) < 1e-5f, "chroma weights sum %g", s);
        }
        double bw13[13];
        burn_weights(bw13);
        r2f_params p;
        memset(&p, 0, sizeof p);
        p.flags = rnd() & 63u;
        p.burn_cell = rint_in(-1, 400);
        const int H = frame_dim(), W = frame_dim();
        const size_t bytes = r2f_workspace_bytes(&p, H, W);
        CHECK(bytes % 16 == 0 && bytes <= ((size_t)2 * 3 * ((size_t)H * W + 3) + 4 * (size_t)H * W + 16) * 4, "workspace %zu", bytes);
    }
}

// The two host decisions of the FFT form's kernel spectrum (run_stencil_fft): a real spectrum needs every channel centrally
// symmetric bit for bit about an anchor at the centre of an odd x odd box, and the wrapped kernel image is the corner one rolled
// by (-ay, -ax).  Fixed cases, every run.
static void check_fft_kernel_forms() {
    const int chans[2] = {0, 1};
    auto disc = [](int kh, int kw, int cy, int cx, int r) {  // (kh, kw, 3): channels 0 and 1 a disc around (cy, cx), channel 2 its centre tap
        std::vector<float> k((size_t)kh * kw * 3, 0.f);
        for (int i = 0; i < kh; ++i)
            for (int j = 0; j < kw; ++j) {
                const int d2 = (i - cy) * (i - cy) + (j - cx) * (j - cx);
                if (d2 <= r * r) k[((size_t)i * kw + j) * 3] = 1.f / (1.f + d2), k[((size_t)i * kw + j) * 3 + 1] = 0.3f / (2.f + d2);
            }
        k[((size_t)cy * kw + cx) * 3 + 2] = 1.f;
        return k;
    };
    auto rolled = [&](const Taps& t, int c, const int box[4]) {  // wrapped image == corner image rolled by (-ay, -ax)
        const int ny = 16, nx = 32, ay = t.kh / 2 - box[0], ax = t.kw / 2 - box[2];
        const std::vector<float> u = fft_kernel_image(t, c, box, ny, nx, false), w = fft_kernel_image(t, c, box, ny, nx, true);
        CHECK(u.size() == (size_t)ny * nx && w.size() == u.size(), "image size");
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x)
                CHECK(!memcmp(&w[(size_t)((y - ay + ny) % ny) * nx + (x - ax + nx) % nx], &u[(size_t)y * nx + x], sizeof(float)), "roll at %d %d", y, x);
        for (int y = 0; y < ny; ++y)  // the corner image: the box, then zeros
            for (int x = 0; x < nx; ++x) {
                const bool in = y <= box[1] - box[0] && x <= box[3] - box[2];
                const float want = in ? t.at(box[0] + y, box[2] + x, c) : 0.f;
                CHECK(!memcmp(&u[(size_t)y * nx + x], &want, sizeof want), "corner image at %d %d", y, x);
            }
    };
    int box[4];
    {  // a symmetric disc around the anchor: real
        std::vector<float> k = disc(13, 13, 6, 6, 4);
        Taps t{k.data(), 13, 13, 3};
        tap_box(t, 0, box);
        CHECK(box[0] == 2 && box[1] == 10 && box[2] == 2 && box[3] == 10, "disc box");
        CHECK(centrally_symmetric(t, chans, 2, box), "symmetric disc");
        rolled(t, 0, box), rolled(t, 1, box);
        // ... the same disc with the last mantissa bit of one tap of channel 1 flipped: not real, for the group
        uint32_t bits;
        float& tap = k[((size_t)4 * 13 + 7) * 3 + 1];
        memcpy(&bits, &tap, 4), bits ^= 1u, memcpy(&tap, &bits, 4);
        CHECK(!centrally_symmetric(t, chans, 2, box), "one mantissa bit");
        CHECK(centrally_symmetric(t, chans, 1, box), "channel 0 alone is untouched");
    }
    {  // an even-sized box
        std::vector<float> k((size_t)12 * 12, 0.f);
        for (int i = 4; i < 8; ++i)
            for (int j = 4; j < 8; ++j) k[(size_t)i * 12 + j] = 0.0625f;
        Taps t{k.data(), 12, 12, 1};
        tap_box(t, 0, box);
        CHECK(box[1] - box[0] + 1 == 4 && box[3] - box[2] + 1 == 4, "even box");
        CHECK(!centrally_symmetric(t, chans, 1, box), "even-sized box");
        rolled(t, 0, box);
    }
    {  // a disc that is symmetric in itself, one row below the anchor
        std::vector<float> k = disc(13, 13, 7, 6, 4);
        Taps t{k.data(), 13, 13, 3};
        tap_box(t, 0, box);
        CHECK(box[0] == 3 && box[1] == 11 && 13 / 2 - box[0] != (box[1] - box[0] + 1) / 2, "off-centre box");
        CHECK(!centrally_symmetric(t, chans, 2, box), "off-centre anchor");
        rolled(t, 0, box);
    }
}

int main(int argc, char** argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int cases = argc > 2 ? atoi(argv[2]) : 2000;
    g_state = seed * 0x9E3779B97F4A7C15ULL + 1;
    check_fft_kernel_forms();
    for (int i = 0; i < cases; ++i) {
        fuzz_fft();
        if (i % 4 == 0) fuzz_stencil();
        if (i % 8 == 0) fuzz_tables();
    }
    printf("plan_fuzz: seed %llu, %d cases ok\n", (unsigned long long)seed, cases);
    return 0;
}
