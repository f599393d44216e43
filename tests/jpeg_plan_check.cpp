// jpeg_plan_check.cpp -- harness for the JPEG encoder's host side (raw2film_amd/csrc/r2f_jpeg_plan.cpp), built by
// tests/test_jpeg_host.py with `g++ -fsanitize=address,undefined -fno-sanitize-recover=all` and run as a child process.
// Test infrastructure: nothing in the product links this file.
//
//   jpeg_plan_check header <quality> <H> <W>   the header's bytes, hex, written into a buffer of exactly their size
//   jpeg_plan_check fuzz <seed> <cases>        header, tables, bound and scratch layout over random qualities and sizes
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/r2f.h"
#include "../raw2film_amd/csrc/r2f_jpeg_plan.h"

using namespace r2f::jpeg;

#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            fprintf(stderr, "jpeg_plan_check: %s failed: ", #cond); \
            fprintf(stderr, __VA_ARGS__);                     \
            fprintf(stderr, "\n");                            \
            abort();                                          \
        }                                                     \
    } while (0)

static uint64_t g_state = 1;
static uint32_t rnd() {  // xorshift64*
    g_state ^= g_state >> 12, g_state ^= g_state << 25, g_state ^= g_state >> 27;
    return (uint32_t)((g_state * 2685821237ULL) >> 32);
}

static void one_case(int q, int H, int W) {
    std::vector<uint8_t> buf(kHeaderBytes);  // exactly the header's size: a write past it is an ASan report
    size_t len = 0;
    CHECK(r2f_jpeg_header(q, H, W, buf.data(), buf.size(), &len) == 0 && len == (size_t)kHeaderBytes, "q %d %d x %d", q, H, W);
    CHECK(buf[0] == 0xFF && buf[1] == 0xD8 && buf[len - 14] == 0xFF && buf[len - 13] == 0xDA, "markers");
    CHECK(r2f_jpeg_header(q, H, W, buf.data(), buf.size() - 1, &len) == R2F_EINVAL, "short buffer accepted");
    Tables t;
    make_tables(q, &t);
    for (int c = 0; c < 2; ++c) {
        for (int i = 0; i < 64; ++i) CHECK(t.qdiv[c][i] >= 8 && t.qdiv[c][i] <= 8 * 255 && t.qdiv[c][i] % 8 == 0, "divisor");
        for (int n = 0; n <= 11; ++n) CHECK((t.dc[c][n] & 0xFF) >= 2 && (t.dc[c][n] & 0xFF) <= 11, "dc length");
        for (int s = 0; s < 256; ++s) {
            const int len8 = t.ac[c][s] & 0xFF, n = s & 15;
            if (s == 0x00 || s == 0xF0 || (n >= 1 && n <= 10)) CHECK(len8 >= 2 && len8 <= 16, "ac symbol %02x missing", s);
            if (len8) CHECK((t.ac[c][s] >> 8) < (1u << len8), "code wider than its length");
            if (len8) CHECK(len8 + n <= 26, "per-position bound");
        }
    }
    const uint64_t bound = r2f_jpeg_bound_bytes(H, W);
    CHECK(bound == bound_bytes(H, W) && bound > (uint64_t)kHeaderBytes + 2 * mcus(H, W) * 6 * 2, "bound");
    const Scratch s = scratch_layout(H, W);
    CHECK(s.coefs < s.offsets && s.offsets < s.words && s.words < s.chunks && s.chunks < s.partial && s.partial <= s.tables &&
              s.tables < s.total, "layout order");
    CHECK(s.offsets - s.coefs >= s.n_mcus * 768 && s.words - s.offsets >= (s.n_mcus + 1) * 8, "layout sizes");
    CHECK(s.scan_words * 32 >= scan_bound_bits(H, W) && (s.chunks - s.words) >= s.scan_words * 4, "scan words");
    CHECK((s.partial - s.chunks) >= (s.stuff_chunks + 1) * 8 && (s.tables - s.partial) >= s.partial_elems * 8, "chunks");
    CHECK(s.partial_elems >= scan_partials(s.n_mcus) && s.partial_elems >= scan_partials(s.stuff_chunks), "partials");
}

int main(int argc, char** argv) {
    if (argc == 5 && !strcmp(argv[1], "header")) {
        uint8_t buf[kHeaderBytes];
        size_t len = 0;
        if (r2f_jpeg_header(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), buf, sizeof buf, &len) != 0) return 2;
        for (size_t i = 0; i < len; ++i) printf("%02x", buf[i]);
        printf("\n");
        return 0;
    }
    if (argc != 4 || strcmp(argv[1], "fuzz")) return 2;
    g_state = 0x9E3779B97F4A7C15ULL ^ strtoull(argv[2], nullptr, 10);
    const int cases = atoi(argv[3]);
    for (int bad : {-1, 101}) CHECK(r2f_jpeg_header(bad, 8, 8, nullptr, 0, nullptr) == R2F_EINVAL, "quality %d", bad);
    uint8_t tmp[kHeaderBytes];
    size_t len;
    for (int d : {0, -3, 65536}) {
        CHECK(r2f_jpeg_header(50, d, 8, tmp, sizeof tmp, &len) == R2F_EINVAL && r2f_jpeg_bound_bytes(8, d) == 0, "size %d", d);
    }
    one_case(100, 65535, 65535);
    one_case(0, 1, 1);
    for (int i = 0; i < cases; ++i) {
        const int big = rnd() % 4 == 0;
        const int H = 1 + (int)(rnd() % (big ? 65535u : 300u)), W = 1 + (int)(rnd() % (big ? 65535u : 300u));
        one_case((int)(rnd() % 101), H, W);
    }
    printf("%d cases ok\n", cases + 2);
    return 0;
}
