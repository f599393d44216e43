// jpeg_restart_plan_check.cpp -- harness for the host side of the JPEG export's restart intervals and JFIF density
// (r2f_jpeg_plan.cpp: the header's DRI segment and APP0, the bounds, scratch_layout and rows_grid with an interval), built by
// tests/test_jpeg_restart_host.py with `g++ -fsanitize=address,undefined -fno-sanitize-recover=all` and run as a child process.
// Test infrastructure: nothing in the product links this file.
//
//   jpeg_restart_plan_check fuzz <seed> <cases>                     random frames, samplings, intervals and densities
//   jpeg_restart_plan_check header <q> <s> <H> <W> <restart> <xd> <yd>   r2f_jpeg_header_ex's bytes as hex, then the bound
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../include/r2f.h"
#include "../raw2film_amd/csrc/r2f_jpeg_plan.h"

using namespace r2f::jpeg;

#define CHECK(cond, ...)                                                    \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "jpeg_restart_plan_check: %s failed: ", #cond); \
            fprintf(stderr, __VA_ARGS__);                                   \
            fprintf(stderr, "\n");                                          \
            abort();                                                        \
        }                                                                   \
    } while (0)

static uint64_t g_state = 1;
static uint32_t rnd() {  // xorshift64*
    g_state ^= g_state >> 12, g_state ^= g_state << 25, g_state ^= g_state >> 27;
    return (uint32_t)((g_state * 2685821237ULL) >> 32);
}

static int random_restart() {
    switch (rnd() % 5) {
        case 0: return 1;
        case 1: return 1 + (int)(rnd() % 12);
        case 2: return 1 + (int)(rnd() % 3000);
        case 3: return kMaxRestart;
        default: return 1 + (int)(rnd() % kMaxRestart);
    }
}

// The header with extras against the plain one: the same bytes but for APP0's units and densities and the DRI in front of SOS.
static void one_header(int q, int s, int H, int W, int restart, int xd, int yd) {
    Huffman h;
    std_huffman(&h);
    uint8_t plain[kHeaderBytes], buf[kHeaderBytes + kDriBytes + 1];
    const int n0 = header(q, s, h, H, W, plain, sizeof plain);
    CHECK(n0 == kHeaderBytes, "plain header %d", n0);
    buf[kHeaderBytes + kDriBytes] = 0xA5;
    const int need = n0 + (restart ? kDriBytes : 0);
    const int n = header(q, s, h, H, W, HeaderExtras{restart, xd, yd}, buf, (size_t)need);
    CHECK(n == need && buf[kHeaderBytes + kDriBytes] == 0xA5, "header length %d, need %d", n, need);
    CHECK(header(q, s, h, H, W, HeaderExtras{restart, xd, yd}, buf, (size_t)need - 1) == -1, "a short cap accepted");
    const bool dpi = xd > 0 && yd > 0;
    const uint8_t app0[5] = {(uint8_t)(dpi ? 1 : 0), (uint8_t)(dpi ? xd >> 8 : 0), (uint8_t)(dpi ? xd & 255 : 1),
                             (uint8_t)(dpi ? yd >> 8 : 0), (uint8_t)(dpi ? yd & 255 : 1)};
    CHECK(!memcmp(buf, plain, 13) && !memcmp(buf + 13, app0, 5) && !memcmp(buf + 18, plain + 18, (size_t)n0 - 14 - 18), "up to SOS");
    if (restart) {
        const uint8_t dri[6] = {0xFF, 0xDD, 0, 4, (uint8_t)(restart >> 8), (uint8_t)(restart & 255)};
        CHECK(!memcmp(buf + n0 - 14, dri, 6), "DRI");
    }
    CHECK(!memcmp(buf + n - 14, plain + n0 - 14, 14), "SOS");
    // the C ABI writes the same
    r2f_jpeg_opts o{q, s, 0, 0, restart, xd, yd};
    uint8_t abi[kHeaderBytes + kDriBytes];
    size_t len = 0;
    CHECK(r2f_jpeg_header_ex(&o, H, W, abi, sizeof abi, &len) == R2F_OK && len == (size_t)n && !memcmp(abi, buf, len), "header_ex");
}

static void one_frame(int H, int W, int s, int restart) {
    const Layout l = layout(s);
    const Scratch P = scratch_layout(H, W, s), L = scratch_layout(H, W, s, restart);
    const uint64_t n = mcus(H, W, s), k = restart_intervals(n, restart);
    CHECK(k >= 1 && k == (n + restart - 1) / restart && restart_intervals(n, 0) == 0, "intervals");
    CHECK(scan_bound_bits(H, W, s, 0) == scan_bound_bits(H, W, s) && bound_bytes(H, W, s, 0) == bound_bytes(H, W, s), "interval 0");
    CHECK(scan_bound_bits(H, W, s, restart) == scan_bound_bits(H, W, s) + 23 * k - 16, "scan bound");
    CHECK(bound_bytes(H, W, s, restart) == bound_bytes(H, W, s) + kDriBytes + 4 * k, "bound");
    // the bound holds for the longest scan the bit bound allows: data bytes (B + 7 k) / 8, all stuffed, 2 (k - 1) marker bytes
    const uint64_t B = scan_bound_bits(H, W, s);
    CHECK(kHeaderBytes + kDriBytes + 2 * ((B + 7 * k) / 8) + 2 * (k - 1) + 2 <= bound_bytes(H, W, s, restart), "worst case");
    CHECK(L.n_mcus == n && L.coefs == P.coefs && L.offsets == P.offsets && L.words == P.words, "leading regions");
    CHECK(L.scan_words * 32 >= scan_bound_bits(H, W, s, restart) && L.stuff_chunks * kStuffChunk * 8 >= scan_bound_bits(H, W, s, restart), "words");
    CHECK(L.intervals >= L.tables + sizeof(Tables) && L.total >= L.intervals + (k + 1) * 8 && L.total % 16 == 0, "intervals region");
    CHECK(scan_partials(k) <= L.partial_elems && P.total == P.intervals, "partials");
    r2f_jpeg_opts o{90, s, 0, 0, restart, 0, 0};
    CHECK(r2f_jpeg_bound_bytes_opts(&o, H, W) == bound_bytes(H, W, s, restart), "bound_opts");
    RowsGrid g;
    uint64_t m_next = 0;
    int y = 0;
    while (y < H) {
        const int rows = (H - y + l.mh - 1) / l.mh;
        const int y1 = std::min(y + l.mh * (1 + (int)(rnd() % (uint32_t)rows)), H);
        RowsGrid p;
        CHECK(rows_grid(H, W, s, y, y1, &g, restart) && rows_grid(H, W, s, y, y1, &p), "rows [%d, %d) of %d refused", y, y1, H);
        CHECK(g.m0 == m_next && g.m0 == p.m0 && g.m1 == p.m1 && g.stuff_chunks >= p.stuff_chunks && g.stuff_chunks <= L.stuff_chunks, "grid");
        // intervals that end in the call, and the bytes its stuffing passes must cover
        uint64_t ends = 0;
        for (uint64_t e = (g.m0 / restart + 1) * (uint64_t)restart; e <= g.m1; e += restart) ++ends;
        if (g.m1 == n && n % restart) ++ends;
        const uint64_t bits = (g.m1 - g.m0) * l.nb * kBlockBoundBits + 23 * ends;
        CHECK(g.stuff_chunks == L.stuff_chunks || g.stuff_chunks * kStuffChunk >= (bits + 7) / 8 + 1, "stuff chunks");
        CHECK(g.zero_words >= (bits + 31) / 32 && scan_partials(g.m1 - g.m0) <= L.partial_elems, "grid sizes");
        CHECK((g.m1 - 1) / restart - g.m0 / restart + 1 <= k, "local intervals");
        m_next = g.m1, y = y1;
    }
    CHECK(m_next == n, "the calls end at MCU %llu of %llu", (unsigned long long)m_next, (unsigned long long)n);
    CHECK(!rows_grid(H, W, s, 0, H, &g, -1) && !rows_grid(H, W, s, 0, H, &g, kMaxRestart + 1), "bad interval accepted");
}

int main(int argc, char** argv) {
    if (argc == 9 && !strcmp(argv[1], "header")) {
        r2f_jpeg_opts o{atoi(argv[2]), atoi(argv[3]), 0, 0, atoi(argv[6]), atoi(argv[7]), atoi(argv[8])};
        uint8_t buf[kHeaderBytes + kDriBytes];
        size_t len = 0;
        if (r2f_jpeg_header_ex(&o, atoi(argv[4]), atoi(argv[5]), buf, sizeof buf, &len) != R2F_OK) return 3;
        for (size_t i = 0; i < len; ++i) printf("%02x", buf[i]);
        printf("\n%llu\n", (unsigned long long)r2f_jpeg_bound_bytes_opts(&o, atoi(argv[4]), atoi(argv[5])));
        return 0;
    }
    if (argc != 4 || strcmp(argv[1], "fuzz")) return 2;
    g_state = 0x9E3779B97F4A7C15ULL ^ strtoull(argv[2], nullptr, 10);
    const int cases = atoi(argv[3]);
    uint8_t buf[kHeaderBytes + kDriBytes];
    size_t len = 0;
    // the first four fields alone mean "no interval, no density": the results of before
    r2f_jpeg_opts four{50, 0, 0, 0};
    CHECK(four.restart_interval == 0 && four.x_density == 0 && four.y_density == 0, "appended fields");
    CHECK(r2f_jpeg_header_ex(&four, 8, 8, buf, sizeof buf, &len) == R2F_OK && len == (size_t)kHeaderBytes, "four fields");
    CHECK(r2f_jpeg_bound_bytes_opts(&four, 100, 200) == r2f_jpeg_bound_bytes_ex(100, 200, 0), "four fields' bound");
    for (int bad : {-1, kMaxRestart + 1, 70000}) {
        r2f_jpeg_opts o{50, 0, 0, 0, bad, 0, 0};
        CHECK(r2f_jpeg_header_ex(&o, 8, 8, buf, sizeof buf, &len) == R2F_EINVAL && r2f_jpeg_bound_bytes_opts(&o, 8, 8) == 0, "interval %d", bad);
    }
    for (int bad : {-1, kMaxDensity + 1}) {
        r2f_jpeg_opts o{50, 0, 0, 0, 0, bad, 72}, p{50, 0, 0, 0, 0, 72, bad};
        CHECK(r2f_jpeg_header_ex(&o, 8, 8, buf, sizeof buf, &len) == R2F_EINVAL, "x density %d", bad);
        CHECK(r2f_jpeg_header_ex(&p, 8, 8, buf, sizeof buf, &len) == R2F_EINVAL, "y density %d", bad);
    }
    r2f_jpeg_opts prog{50, 0, 0, 1, 5, 0, 0};
    CHECK(r2f_jpeg_bound_bytes_opts(&prog, 8, 8) == 0, "progressive with an interval has no bound");
    prog.restart_interval = 0, prog.x_density = prog.y_density = 300;
    CHECK(r2f_jpeg_bound_bytes_opts(&prog, 8, 8) == prog_bound_bytes(8, 8, 0), "progressive with a density");
    uint8_t frame[kProgFrameHeaderBytes], frame0[kProgFrameHeaderBytes];
    CHECK(prog_frame_header(50, 0, 8, 8, frame0, sizeof frame0) == kProgFrameHeaderBytes, "progressive header");
    CHECK(prog_frame_header(50, 0, 8, 8, frame, sizeof frame, 300, 73) == kProgFrameHeaderBytes, "progressive header, dpi");
    const uint8_t dpi[5] = {1, 1, 0x2C, 0, 73};
    CHECK(!memcmp(frame + 13, dpi, 5) && !memcmp(frame, frame0, 13) && !memcmp(frame + 18, frame0 + 18, sizeof frame - 18), "progressive APP0");
    CHECK(prog_frame_header(50, 0, 8, 8, frame, sizeof frame, -1, 73) == -1, "progressive header, bad density");
    for (int i = 0; i < cases; ++i) {
        const int s = (int)(rnd() % 3), q = (int)(rnd() % 101);
        const int big = rnd() % 8 == 0;
        const int H = 1 + (int)(rnd() % (big ? 65535u : 300u)), W = 1 + (int)(rnd() % (big ? 65535u : 300u));
        const int restart = random_restart();
        const int xd = rnd() % 3 ? (int)(rnd() % 65536u) : 0, yd = rnd() % 3 ? (int)(rnd() % 65536u) : 0;
        one_header(q, s, H, W, rnd() % 4 ? restart : 0, xd, yd);
        one_frame(big ? H : 1 + H % 200, big ? W % 3000 + 1 : W, s, restart);
    }
    one_frame(65535, 17, 0, 1);
    one_frame(1, 1, 1, 1);
    one_frame(2400, 2400, 0, kMaxRestart);  // (the clamp of 219 MCU rows of 300)
    printf("%d cases ok\n", cases);
    return 0;
}
