// jpeg_rows_plan_check.cpp -- harness for the row-wise encoder's host side (rows_grid in raw2film_amd/csrc/r2f_jpeg_plan.cpp),
// built by tests/test_jpeg_stream_host.py with `g++ -fsanitize=address,undefined -fno-sanitize-recover=all` and run as a child
// process.  Test infrastructure: nothing in the product links this file.
//
//   jpeg_rows_plan_check fuzz <seed> <cases>   random frames split into random 16-aligned calls: the calls' MCUs partition the
//                                              frame in order, and for bit counts drawn per MCU (none, random, the worst case) every
//                                              range a call's passes touch fits its fixed grid and the frame's scratch and output
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/r2f.h"
#include "../raw2film_amd/csrc/r2f_jpeg_plan.h"

using namespace r2f::jpeg;

#define CHECK(cond, ...)                                                \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "jpeg_rows_plan_check: %s failed: ", #cond); \
            fprintf(stderr, __VA_ARGS__);                               \
            fprintf(stderr, "\n");                                      \
            abort();                                                    \
        }                                                               \
    } while (0)

static uint64_t g_state = 1;
static uint32_t rnd() {  // xorshift64*
    g_state ^= g_state >> 12, g_state ^= g_state << 25, g_state ^= g_state >> 27;
    return (uint32_t)((g_state * 2685821237ULL) >> 32);
}

// Bits of MCU m under `mode`: 0 none, 1 random, 2 the worst case.
static uint64_t mcu_bits(int mode) {
    const uint64_t worst = 6 * (uint64_t)kBlockBoundBits;
    return mode == 0 ? 0 : mode == 2 ? worst : rnd() % (worst + 1);
}

static void one_frame(int H, int W, int mode) {
    const Scratch L = scratch_layout(H, W);
    const uint64_t scan_bytes = (scan_bound_bits(H, W) + 7) / 8, bound = bound_bytes(H, W);
    RowsGrid g;
    for (int bad : {-16, 1, 15}) CHECK(!rows_grid(H, W, bad, H, &g) && g.m1 == 0, "y0 %d accepted", bad);
    CHECK(!rows_grid(H, W, 0, 0, &g) && !rows_grid(H, W, 0, H + 1, &g), "empty or overlong rows accepted");
    if (H != 17) CHECK(!rows_grid(H, W, 0, 17, &g), "misaligned end accepted");
    uint64_t m_next = 0, bits = 0, ff = 0;
    int y = 0, calls = 0;
    while (y < H) {
        // the next end: a random multiple of 16 past y (often one MCU row), or H
        const int rows16 = (H - y + 15) / 16;
        const int step = rnd() % 3 == 0 ? 1 : 1 + (int)(rnd() % (uint32_t)rows16);
        const int y1 = std::min(y + 16 * step, H);
        CHECK(rows_grid(H, W, y, y1, &g), "rows [%d, %d) of %d refused", y, y1, H);
        CHECK(g.m0 == m_next && g.m1 > g.m0, "calls do not partition the MCUs: %llu after %llu", (unsigned long long)g.m0,
              (unsigned long long)m_next);
        CHECK(g.m1 - g.m0 == (uint64_t)((y1 + 15) / 16 - y / 16) * ((W + 15) / 16), "MCU rows");
        CHECK(g.stuff_chunks >= 1 && g.stuff_chunks <= L.stuff_chunks, "stuff chunks %llu of %llu", (unsigned long long)g.stuff_chunks,
              (unsigned long long)L.stuff_chunks);
        CHECK(scan_partials(g.m1 - g.m0) <= L.partial_elems && scan_partials(g.stuff_chunks) <= L.partial_elems, "scan partials");
        const uint64_t before = bits;
        for (uint64_t m = g.m0; m < g.m1; ++m) bits += mcu_bits(mode);
        const bool last = y1 == H;
        // zero pass: words [ceil(before / 32), ceil(bits / 32)); stuffing: bytes [floor(before / 8), hi)
        const uint64_t w0 = (before + 31) / 32, w1 = (bits + 31) / 32;
        CHECK(w1 - w0 <= g.zero_words && w1 <= L.scan_words, "words [%llu, %llu)", (unsigned long long)w0, (unsigned long long)w1);
        const uint64_t lo = before / 8, hi = last ? (bits + 7) / 8 : bits / 8;
        CHECK(hi >= lo && hi - lo <= g.stuff_chunks * (uint64_t)kStuffChunk, "bytes [%llu, %llu) over %llu chunks",
              (unsigned long long)lo, (unsigned long long)hi, (unsigned long long)g.stuff_chunks);
        CHECK(hi <= L.scan_words * 4 && hi <= scan_bytes, "bytes past the scan");
        ff += mode == 2 ? hi - lo : 0;  // (worst case: every byte stuffed)
        CHECK(kHeaderBytes + hi + ff + (last ? 2 : 0) <= bound, "file past the bound");
        m_next = g.m1, y = y1, ++calls;
    }
    CHECK(m_next == mcus(H, W) && calls >= 1, "the calls end at MCU %llu of %llu", (unsigned long long)m_next,
          (unsigned long long)mcus(H, W));
}

int main(int argc, char** argv) {
    if (argc != 4 || strcmp(argv[1], "fuzz")) return 2;
    g_state = 0x9E3779B97F4A7C15ULL ^ strtoull(argv[2], nullptr, 10);
    const int cases = atoi(argv[3]);
    RowsGrid g;
    CHECK(!rows_grid(0, 8, 0, 0, &g) && !rows_grid(8, 65536, 0, 8, &g), "frame size");
    one_frame(1, 1, 2);
    one_frame(16, 16, 2);
    one_frame(65535, 17, 2);
    for (int i = 0; i < cases; ++i) {
        const int big = rnd() % 8 == 0;
        const int H = 1 + (int)(rnd() % (big ? 20000u : 400u)), W = 1 + (int)(rnd() % (big ? 2000u : 400u));
        one_frame(H, W, (int)(rnd() % 3));
    }
    printf("%d cases ok\n", cases + 3);
    return 0;
}
