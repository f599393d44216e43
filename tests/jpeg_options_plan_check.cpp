// jpeg_options_plan_check.cpp -- harness for the JPEG options' host side (r2f_jpeg_plan.cpp: optimal_table, the sampling-aware
// header, scratch_layout and rows_grid), built by tests/test_jpeg_options_host.py with
// `g++ -fsanitize=address,undefined -fno-sanitize-recover=all` and run as a child process.  Test infrastructure: nothing in the
// product links this file.
//
//   jpeg_options_plan_check fuzz <seed> <cases>            random histograms through optimal_table and the header; random frames
//                                                          and samplings through scratch_layout and rows_grid
//   jpeg_options_plan_check header <q> <s> <H> <W> <f..>   the header with the optimized tables of 4 x 256 counts, as hex
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
            fprintf(stderr, "jpeg_options_plan_check: %s failed: ", #cond); \
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

// Optimized tables of freq[4][256]; false when a table has no symbol.
static bool tables_of(const uint64_t freq[4][256], Huffman* h) {
    *h = Huffman{};
    for (int t = 0; t < 4; ++t) {
        uint8_t bits[17];
        bool adjusted = false;
        const int n = optimal_table(freq[t], bits, h->huffval[t], &adjusted);
        if (n < 0) return false;
        CHECK(bits[0] == 0, "bits[0]");
        int sum = 0, kraft = 0;  // sum of 2^(16 - len): the code must leave the all-ones code free
        for (int i = 1; i <= 16; ++i) sum += bits[i], kraft += bits[i] << (16 - i);
        CHECK(sum == n && kraft < 65536, "table %d: %d symbols, Kraft sum %d", t, n, kraft);
        uint8_t seen[256] = {};
        for (int i = 0; i < n; ++i) CHECK(!seen[h->huffval[t][i]]++ && freq[t][h->huffval[t][i]], "symbol %d", h->huffval[t][i]);
        std::memcpy(h->bits[t], bits + 1, 16);
        h->n[t] = n;
    }
    return true;
}

// A histogram whose symbols are those the encoder can count for table t (DC: 0..11; AC: EOB, ZRL, run/size).
static void random_freq(uint64_t f[256], int t) {
    std::memset(f, 0, 256 * sizeof(uint64_t));
    const int mode = rnd() % 4;
    const uint64_t cap = mode == 0 ? 3 : mode == 1 ? 1000 : 3000000;  // (162 symbols stay below libjpeg's 10^9 sentinel)
    for (int s = 0; s < 256; ++s) {
        const bool valid = t % 2 == 0 ? s <= 11 : (s == 0 || s == 0xF0 || ((s & 15) >= 1 && (s & 15) <= 10));
        if (valid && rnd() % 3) f[s] = 1 + (((uint64_t)rnd() << 32 | rnd()) % cap);
    }
    if (rnd() % 8 == 0) {  // Fibonacci-like: code lengths over 16 before the K.3 folding
        uint64_t a = 2, b = 2;
        int run = 0;
        for (int s = 0; s < 256; ++s)
            if (f[s]) {
                f[s] = a, b += a, a = b - a;
                if (++run % 32 == 0) a = b = 2;  // (runs of 32: the sums stay below libjpeg's 10^9 sentinel)
            }
    }
    f[t % 2 ? 0 : 1] += 1;  // (never empty)
}

static void one_frame(int H, int W, int s) {
    const Layout l = layout(s);
    const Scratch L = scratch_layout(H, W, s);
    CHECK(L.n_mcus == mcus(H, W, s) && L.coefs == 0 && L.offsets >= L.n_mcus * l.nb * 128, "coefs");
    CHECK(L.words - L.offsets >= (L.n_mcus + 1) * 8 && L.scan_words * 32 >= scan_bound_bits(H, W, s), "scan words");
    CHECK(L.total >= L.tables + sizeof(Tables), "total");
    if (s == 2) {
        const Scratch D = scratch_layout(H, W);
        CHECK(D.total == L.total && D.words == L.words && bound_bytes(H, W) == bound_bytes(H, W, 2), "4:2:0 = default");
    }
    CHECK(r2f_jpeg_bound_bytes_ex(H, W, s) == bound_bytes(H, W, s), "bound");
    RowsGrid g;
    if (l.mh < H) CHECK(!rows_grid(H, W, s, 0, l.mh + 1, &g) || l.mh + 1 == H, "misaligned end accepted");
    CHECK(!rows_grid(H, W, s, 4, H, &g), "misaligned start accepted");
    uint64_t m_next = 0;
    int y = 0;
    while (y < H) {
        const int rows = (H - y + l.mh - 1) / l.mh;
        const int y1 = std::min(y + l.mh * (1 + (int)(rnd() % (uint32_t)rows)), H);
        CHECK(rows_grid(H, W, s, y, y1, &g), "rows [%d, %d) of %d refused (sampling %d)", y, y1, H, s);
        CHECK(g.m0 == m_next && g.m1 > g.m0 && g.stuff_chunks >= 1 && g.stuff_chunks <= L.stuff_chunks, "grid");
        CHECK(scan_partials(g.m1 - g.m0) <= L.partial_elems && g.zero_words <= L.scan_words + 1, "grid sizes");
        if (s == 2) {
            RowsGrid d;
            CHECK(rows_grid(H, W, y, y1, &d) && d.m0 == g.m0 && d.m1 == g.m1 && d.stuff_chunks == g.stuff_chunks, "4:2:0 = default");
        }
        m_next = g.m1, y = y1;
    }
    CHECK(m_next == L.n_mcus, "the calls end at MCU %llu of %llu", (unsigned long long)m_next, (unsigned long long)L.n_mcus);
}

int main(int argc, char** argv) {
    if (argc == 6 + 1024 && !strcmp(argv[1], "header")) {
        static uint64_t freq[4][256];
        for (int i = 0; i < 1024; ++i) freq[i / 256][i % 256] = strtoull(argv[6 + i], nullptr, 10);
        Huffman h;
        if (!tables_of(freq, &h)) return 3;
        uint8_t buf[kHeaderBytes];
        const int n = header(atoi(argv[2]), atoi(argv[3]), h, atoi(argv[4]), atoi(argv[5]), buf, sizeof buf);
        if (n < 0) return 2;
        for (int i = 0; i < n; ++i) printf("%02x", buf[i]);
        printf("\n");
        return 0;
    }
    if (argc != 4 || strcmp(argv[1], "fuzz")) return 2;
    g_state = 0x9E3779B97F4A7C15ULL ^ strtoull(argv[2], nullptr, 10);
    const int cases = atoi(argv[3]);
    uint8_t bits[17], hv[256];
    static const uint64_t zero[256] = {};
    CHECK(optimal_table(zero, bits, hv) == -1 && r2f_jpeg_optimal_table(zero, bits, hv, nullptr) == R2F_EINVAL, "empty histogram");
    uint64_t past[256] = {};
    past[1] = 2000000000ULL, past[2] = 5;  // (never merged: symbol 1 would have no code)
    CHECK(optimal_table(past, bits, hv) == -1, "a count past the sentinel");
    r2f_jpeg_opts o{50, 0, 1, 0};
    uint8_t buf[kHeaderBytes];
    size_t len = 0;
    CHECK(r2f_jpeg_header_ex(&o, 8, 8, buf, sizeof buf, &len) == R2F_EINVAL, "optimize header");
    for (int s : {-1, 3}) {
        o = {50, s, 0, 0};
        CHECK(r2f_jpeg_header_ex(&o, 8, 8, buf, sizeof buf, &len) == R2F_EINVAL && r2f_jpeg_bound_bytes_ex(8, 8, s) == 0, "s %d", s);
    }
    for (int i = 0; i < cases; ++i) {
        static uint64_t freq[4][256];
        for (int t = 0; t < 4; ++t) random_freq(freq[t], t);
        Huffman h;
        CHECK(tables_of(freq, &h), "tables");
        const int s = (int)(rnd() % 3), q = (int)(rnd() % 101);
        const int big = rnd() % 4 == 0;
        const int H = 1 + (int)(rnd() % (big ? 65535u : 300u)), W = 1 + (int)(rnd() % (big ? 65535u : 300u));
        const size_t cap = rnd() % 8 == 0 ? rnd() % kHeaderBytes : kHeaderBytes;
        const int n = header(q, s, h, H, W, buf, cap);
        const int need = 275 + h.n[0] + h.n[1] + h.n[2] + h.n[3];
        CHECK(n == (cap >= (size_t)need ? need : -1) && need <= kHeaderBytes, "header length %d (need %d, cap %zu)", n, need, cap);
        CHECK(scan_bits(freq, h) != UINT64_MAX, "scan bits");
        if (i % 4 == 0) one_frame(big ? H : 1 + H % 200, big ? W % 3000 + 1 : W, s);
    }
    one_frame(65535, 17, 0);
    one_frame(1, 1, 1);
    printf("%d cases ok\n", cases);
    return 0;
}
