// r2f_jpeg_api.hip -- the JPEG entry points of include/r2f.h over the encoder's launchers (r2f_jpeg.hip, r2f_jpeg_prog.hip) and
// host-side tables (r2f_jpeg_plan.cpp).
#include <cstring>
#include <vector>

#include "r2f_ctx.h"
#include "r2f_jpeg.h"

using namespace r2f;

namespace {

// What r2f_jpeg_encode_ex and r2f_jpeg_rows_begin_ex check of a frame and its output; then the scratch grown to the frame.
// (row_stride < 0: no image yet)
int jpeg_prepare(r2f_ctx* ctx, int H, int W, int64_t row_stride, const r2f_jpeg_opts* o, uint8_t* out, uint64_t out_cap,
                 uint64_t* out_len) {
    if (!out || !out_len || !o) return fail(ctx, R2F_EINVAL, "jpeg: null output, length or options pointer");
    if (H < 1 || W < 1 || H > jpeg::kMaxDim || W > jpeg::kMaxDim)
        return fail(ctx, R2F_EINVAL, "jpeg: a %d x %d frame (JPEG holds 1 .. %d pixels per side)", H, W, jpeg::kMaxDim);
    if (o->quality < 0 || o->quality > 100) return fail(ctx, R2F_EINVAL, "jpeg: quality %d is not in 0 .. 100", o->quality);
    if (!jpeg::valid_sampling(o->sampling))
        return fail(ctx, R2F_EINVAL, "jpeg: sampling %d is not 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0)", o->sampling);
    if (o->optimize != 0 && o->optimize != 1) return fail(ctx, R2F_EINVAL, "jpeg: optimize %d is not 0 or 1", o->optimize);
    if (o->progressive != 0 && o->progressive != 1)
        return fail(ctx, R2F_EINVAL, "jpeg: progressive %d is not 0 or 1", o->progressive);
    if (!jpeg::valid_restart(o->restart_interval))
        return fail(ctx, R2F_EINVAL, "jpeg: restart_interval %d is not in 0 .. %d", o->restart_interval, jpeg::kMaxRestart);
    if (o->progressive && o->restart_interval)
        return fail(ctx, R2F_EINVAL, "jpeg: progressive with a restart_interval is not supported (baseline only)");
    if (o->x_density < 0 || o->y_density < 0 || o->x_density > jpeg::kMaxDensity || o->y_density > jpeg::kMaxDensity)
        return fail(ctx, R2F_EINVAL, "jpeg: density %d x %d is not in 0 .. %d", o->x_density, o->y_density, jpeg::kMaxDensity);
    if (row_stride >= 0 && row_stride < 3LL * W)
        return fail(ctx, R2F_EINVAL, "jpeg: row stride %lld < 3 W = %lld", (long long)row_stride, 3LL * W);
    if ((uintptr_t)out_len % 8) return fail(ctx, R2F_EINVAL, "jpeg: out_len must be 8-byte aligned");
    const uint64_t bound =
        o->progressive ? jpeg::prog_bound_bytes(H, W, o->sampling) : jpeg::bound_bytes(H, W, o->sampling, o->restart_interval);
    if (out_cap < bound)
        return fail(ctx, R2F_EINVAL, "jpeg: output capacity %llu < bound %llu", (unsigned long long)out_cap, (unsigned long long)bound);
    const size_t total = o->progressive ? jpeg::prog_scratch_layout(H, W, o->sampling).total : jpeg::scratch_layout(H, W, o->sampling, o->restart_interval).total;
    // (an earlier encode may still be working in the old buffer; no captured graph reads it)
    return ctx->jpeg.scratch.reserve(ctx, total, Grow::Sync);
}

jpeg::HeaderExtras header_extras(const r2f_jpeg_opts* o) { return jpeg::HeaderExtras{o->restart_interval, o->x_density, o->y_density}; }

// The standard tables and header of an encode.
int jpeg_std_setup(r2f_ctx* ctx, const r2f_jpeg_opts* o, int H, int W, JpegEncodeArgs* a, uint8_t* hdr, size_t cap) {
    jpeg::Huffman h;
    jpeg::std_huffman(&h);
    jpeg::make_tables(o->quality, h, &a->tables);
    const int n = jpeg::header(o->quality, o->sampling, h, H, W, header_extras(o), hdr, cap);
    if (n < 0) return fail(ctx, R2F_EINVAL, "jpeg: header");
    a->header = hdr, a->header_len = n, a->sampling = o->sampling, a->restart = o->restart_interval;
    return R2F_OK;
}

// progressive=True: the ten scans' symbol counts (the first synchronisation), every scan's tables and header on the host, the
// packing queued, and the file's length read back (the second).
int jpeg_encode_progressive(r2f_ctx* ctx, const r2f_jpeg_opts* o, JpegEncodeArgs& a, uint64_t out_cap, hipStream_t s) {
    const int H = a.H, W = a.W;
    R2F_HIP(ctx, launch_jpeg_prog_stats(a, s));
    const jpeg::ProgScratch P = jpeg::prog_scratch_layout(H, W, o->sampling);
    std::vector<uint64_t> freq(jpeg::kProgFreqWords);
    R2F_HIP(ctx, hipMemcpyAsync(freq.data(), static_cast<uint8_t*>(a.scratch) + P.freq, jpeg::kProgScans * 513 * sizeof(uint64_t),
                                hipMemcpyDeviceToHost, s));
    R2F_HIP(ctx, hipStreamSynchronize(s));
    uint8_t frame[jpeg::kProgFrameHeaderBytes];
    if (jpeg::prog_frame_header(o->quality, o->sampling, H, W, frame, sizeof frame, o->x_density, o->y_density) != jpeg::kProgFrameHeaderBytes)
        return fail(ctx, R2F_EINVAL, "jpeg: progressive frame header");
    std::vector<ProgScanPlan> plans(jpeg::kProgScans);
    uint64_t file = jpeg::kProgFrameHeaderBytes + 2;
    const uint64_t scan_bound = jpeg::prog_scratch_layout(H, W, o->sampling).scan_words * 32ull;
    for (int scan = 0; scan < jpeg::kProgScans; ++scan) {
        const jpeg::ProgScan& sc = jpeg::prog_scan(scan);
        const uint64_t(*f)[256] = reinterpret_cast<const uint64_t(*)[256]>(freq.data() + (size_t)scan * 512);
        jpeg::ProgTables t{};
        for (int k = 0; k < jpeg::prog_slots(sc); ++k) {
            uint8_t bits[17];
            const int n = jpeg::optimal_table(f[k], bits, t.huffval[k]);
            if (n < 0) return fail(ctx, R2F_ETOOLARGE, "jpeg: the symbol counts of scan %d pass libjpeg's 10^9 sentinel", scan);
            if (n > (sc.Ss ? jpeg::kProgAcSymbols : 12)) return fail(ctx, R2F_EHIP, "jpeg: scan %d's table has %d symbols", scan, n);
            for (int i = 0; i < 16; ++i) t.bits[k][i] = bits[i + 1];
            t.n[k] = n;
        }
        ProgScanPlan& pl = plans[scan];
        std::memset(&pl, 0, sizeof pl);
        // (a table slot's codes: the same canonical derivation the baseline tables take)
        jpeg::Huffman h{};
        for (int k = 0; k < jpeg::prog_slots(sc); ++k) {
            std::memcpy(h.bits[1], t.bits[k], 16), std::memcpy(h.huffval[1], t.huffval[k], 256), h.n[1] = t.n[k];
            std::memcpy(h.bits[0], t.bits[k], 16), std::memcpy(h.huffval[0], t.huffval[k], 256), h.n[0] = t.n[k];
            jpeg::Tables dt;
            jpeg::make_tables(o->quality, h, &dt);
            for (int v = 0; v < 256; ++v) pl.codes[k][v] = sc.Ss ? dt.ac[0][v] : (v < 16 ? dt.dc[0][v] : 0);
        }
        pl.header_len = jpeg::prog_scan_header(scan, t, pl.header, sizeof pl.header);
        if (pl.header_len < 0) return fail(ctx, R2F_EHIP, "jpeg: scan %d's header", scan);
        const uint64_t n_blocks = jpeg::prog_geom(H, W, o->sampling, scan).n;
        const uint64_t extra = sc.Ss == 0 ? (sc.Ah ? n_blocks : 0) : freq[(size_t)jpeg::kProgScans * 512 + scan];
        const uint64_t bits = jpeg::prog_scan_bits(scan, f, t, extra);
        if (bits > scan_bound || bits > n_blocks * jpeg::kProgScanBlockBits)
            return fail(ctx, R2F_EHIP, "jpeg: scan %d's %llu bits pass its bound", scan, (unsigned long long)bits);
        file += (uint64_t)pl.header_len + (bits + 7) / 8;
    }
    if (file > out_cap)  // (before stuffing: too large already, nothing is written)
        return fail(ctx, R2F_ETOOLARGE, "jpeg: the progressive file takes at least %llu bytes, out_cap is %llu",
                    (unsigned long long)file, (unsigned long long)out_cap);
    R2F_HIP(ctx, launch_jpeg_prog_pack(a, frame, plans.data(), out_cap, s));
    uint64_t len = 0;
    R2F_HIP(ctx, hipMemcpyAsync(&len, a.out_len, sizeof len, hipMemcpyDeviceToHost, s));
    R2F_HIP(ctx, hipStreamSynchronize(s));
    if (len == 0)
        return fail(ctx, R2F_ETOOLARGE, "jpeg: the progressive file with its stuffed bytes exceeds out_cap %llu",
                    (unsigned long long)out_cap);
    return R2F_OK;
}

}  // namespace

extern "C" {

int r2f_jpeg_encode_ex(r2f_ctx* ctx, const uint8_t* image, int H, int W, int64_t row_stride, const r2f_jpeg_opts* opts, uint8_t* out,
                       uint64_t out_cap, uint64_t* out_len, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    ctx->jpeg.rows.open = false;  // (this encode works in the scratch an open row-wise one keeps its frame's state in)
    if (!image || !out || !out_len) return fail(ctx, R2F_EINVAL, "jpeg: null image, output or length pointer");
    int rc = jpeg_prepare(ctx, H, W, row_stride < 0 ? 0 : row_stride, opts, out, out_cap, out_len);
    if (rc) return rc;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    JpegEncodeArgs a;
    a.image = image, a.row_stride = row_stride, a.H = H, a.W = W, a.scratch = ctx->jpeg.scratch.p;
    a.out = out, a.out_len = reinterpret_cast<unsigned long long*>(out_len);
    uint8_t hdr[jpeg::kHeaderBytes + jpeg::kDriBytes];
    if ((rc = jpeg_std_setup(ctx, opts, H, W, &a, hdr, sizeof hdr))) return rc;
    if (opts->progressive) return jpeg_encode_progressive(ctx, opts, a, out_cap, s);
    if (opts->optimize) {
        // the frame's symbol counts (the one synchronisation), then its tables and header (libjpeg's optimize_coding)
        if ((rc = ctx->jpeg.freq.reserve(ctx, 4 * 256 * sizeof(uint64_t), Grow::Quiet))) return rc;
        unsigned long long* freq_dev = static_cast<unsigned long long*>(ctx->jpeg.freq.p);
        R2F_HIP(ctx, launch_jpeg_stats(a, freq_dev, s));
        uint64_t freq[4][256];
        R2F_HIP(ctx, hipMemcpyAsync(freq, freq_dev, sizeof freq, hipMemcpyDeviceToHost, s));
        R2F_HIP(ctx, hipStreamSynchronize(s));
        jpeg::Huffman h{};
        for (int t = 0; t < 4; ++t) {
            uint8_t bits[17];
            const int n = jpeg::optimal_table(freq[t], bits, h.huffval[t]);
            if (n < 0) return fail(ctx, R2F_ETOOLARGE, "jpeg: the symbol counts of table %d pass libjpeg's 10^9 sentinel", t);
            if (n < 1 || n > (t % 2 ? 162 : 12)) return fail(ctx, R2F_EHIP, "jpeg: optimized table %d has %d symbols", t, n);
            for (int i = 0; i < 16; ++i) h.bits[t][i] = bits[i + 1];
            h.n[t] = n;
        }
        if (jpeg::scan_bits(freq, h) > jpeg::scan_bound_bits(H, W, opts->sampling))
            return fail(ctx, R2F_ETOOLARGE, "jpeg: the optimized scan exceeds the bound");
        jpeg::make_tables(opts->quality, h, &a.tables);
        const int n = jpeg::header(opts->quality, opts->sampling, h, H, W, header_extras(opts), hdr, sizeof hdr);
        if (n < 0) return fail(ctx, R2F_EINVAL, "jpeg: header");
        a.header_len = n, a.recount = true;
    }
    R2F_HIP(ctx, launch_jpeg_encode(a, s));
    return R2F_OK;
}

int r2f_jpeg_encode(r2f_ctx* ctx, const uint8_t* image, int H, int W, int64_t row_stride, int quality, uint8_t* out,
                    uint64_t out_cap, uint64_t* out_len, void* stream) {
    const r2f_jpeg_opts o{quality, 2, 0, 0};
    return r2f_jpeg_encode_ex(ctx, image, H, W, row_stride, &o, out, out_cap, out_len, stream);
}

int r2f_jpeg_rows_begin_ex(r2f_ctx* ctx, int H, int W, const r2f_jpeg_opts* opts, uint8_t* out, uint64_t out_cap, uint64_t* out_len,
                           void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    ctx->jpeg.rows.open = false;
    if (opts && opts->progressive) return fail(ctx, R2F_EINVAL, "jpeg rows: every progressive scan spans the whole frame");
    int rc = jpeg_prepare(ctx, H, W, -1, opts, out, out_cap, out_len);
    if (rc) return rc;
    if (opts->optimize)
        return fail(ctx, R2F_EINVAL, "jpeg rows: optimize needs the whole frame's statistics before the first scan byte");
    if ((rc = ctx->jpeg.carry.reserve(ctx, 64, Grow::Quiet))) return rc;
    JpegEncodeArgs a;
    a.image = nullptr, a.row_stride = 0, a.H = H, a.W = W, a.scratch = ctx->jpeg.scratch.p, a.carry = ctx->jpeg.carry.p;
    uint8_t hdr[jpeg::kHeaderBytes + jpeg::kDriBytes];
    if ((rc = jpeg_std_setup(ctx, opts, H, W, &a, hdr, sizeof hdr))) return rc;
    a.out = out, a.out_len = reinterpret_cast<unsigned long long*>(out_len);
    R2F_HIP(ctx, launch_jpeg_rows_begin(a, static_cast<hipStream_t>(stream)));
    ctx->jpeg.rows.open = true;
    ctx->jpeg.rows.H = H, ctx->jpeg.rows.W = W, ctx->jpeg.rows.next_y = 0;
    ctx->jpeg.rows.sampling = opts->sampling, ctx->jpeg.rows.header_len = a.header_len;
    ctx->jpeg.rows.restart = opts->restart_interval;
    ctx->jpeg.rows.out = out, ctx->jpeg.rows.out_len = out_len;
    return R2F_OK;
}

int r2f_jpeg_rows_begin(r2f_ctx* ctx, int H, int W, int quality, uint8_t* out, uint64_t out_cap, uint64_t* out_len, void* stream) {
    const r2f_jpeg_opts o{quality, 2, 0, 0};
    return r2f_jpeg_rows_begin_ex(ctx, H, W, &o, out, out_cap, out_len, stream);
}

int r2f_jpeg_rows(r2f_ctx* ctx, const uint8_t* image, int64_t row_stride, int y0, int y1, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    auto& r = ctx->jpeg.rows;
    if (!r.open) return fail(ctx, R2F_EINVAL, "jpeg rows: no row-wise encode is open (r2f_jpeg_rows_begin; a one-shot encode, a new "
                                              "begin or the frame's last rows end one)");
    if (!image) return fail(ctx, R2F_EINVAL, "jpeg rows: null image pointer");
    if (row_stride < 3LL * r.W)
        return fail(ctx, R2F_EINVAL, "jpeg rows: row stride %lld < 3 W = %lld", (long long)row_stride, 3LL * r.W);
    if (y0 != r.next_y) return fail(ctx, R2F_EINVAL, "jpeg rows: rows from %d, but the encode is at row %d", y0, r.next_y);
    jpeg::RowsGrid g;
    if (!jpeg::rows_grid(r.H, r.W, r.sampling, y0, y1, &g, r.restart))
        return fail(ctx, R2F_EINVAL, "jpeg rows: rows [%d, %d) of %d: the end must lie past the start and be a multiple of %d or %d",
                    y0, y1, r.H, jpeg::layout(r.sampling).mh, r.H);
    JpegEncodeArgs a;
    a.image = image, a.row_stride = row_stride, a.H = r.H, a.W = r.W, a.scratch = ctx->jpeg.scratch.p, a.carry = ctx->jpeg.carry.p;
    a.sampling = r.sampling, a.header_len = r.header_len, a.restart = r.restart;
    a.header = nullptr, a.out = r.out, a.out_len = reinterpret_cast<unsigned long long*>(r.out_len);
    const bool last = y1 == r.H;
    R2F_HIP(ctx, launch_jpeg_rows(a, g, last, static_cast<hipStream_t>(stream)));
    r.next_y = y1;
    r.open = !last;
    return R2F_OK;
}

}  // extern "C"
