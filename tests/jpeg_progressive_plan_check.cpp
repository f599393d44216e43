// jpeg_progressive_plan_check.cpp -- drives the progressive side of raw2film_amd/csrc/r2f_jpeg_plan.cpp under
// -fsanitize=address,undefined for tests/test_jpeg_progressive_host.py:
//   fuzz SEED N             random sizes, samplings and symbol counts through every progressive planner function
//   frame Q S H W           prints the SOF2 frame header (hex)
//   scan I EXTRA F[512]     prints scan I's DHT + SOS (hex) from the counts F[slot][256], then its exact bits
#include "../raw2film_amd/csrc/r2f_jpeg_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

using namespace r2f::jpeg;

namespace {

void hex(const uint8_t* b, int n) {
    for (int i = 0; i < n; ++i) std::printf("%02x", b[i]);
}

bool tables_of(int scan, const uint64_t freq[2][256], ProgTables* t) {
    std::memset(t, 0, sizeof *t);
    for (int k = 0; k < prog_slots(prog_scan(scan)); ++k) {
        uint8_t bits[17];
        const int n = optimal_table(freq[k], bits, t->huffval[k]);
        if (n < 0) return false;
        std::memcpy(t->bits[k], bits + 1, 16);
        t->n[k] = n;
    }
    return true;
}

int fuzz(unsigned seed, int cases) {
    std::mt19937_64 rng(seed);
    auto pick = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    for (int c = 0; c < cases; ++c) {
        const int H = rng() % 4 ? pick(1, 300) : pick(1, kMaxDim), W = rng() % 4 ? pick(1, 300) : pick(1, kMaxDim);
        const int s = pick(0, 2), q = pick(0, 100);
        const ProgScratch P = prog_scratch_layout(H, W, s);
        const Scratch B = scratch_layout(H, W, s);
        if (P.coefs != B.coefs || P.tables != B.tables || P.runs < B.total || P.total < P.freq + kProgFreqWords * 8) return 1;
        for (size_t off : {P.runs, P.ecount, P.bcount, P.ccount, P.jump, P.mark, P.offsets, P.words, P.chunks, P.partial, P.freq})
            if (off % 16 || off > P.total) return 2;
        if (P.scan_words * 32 < P.n_max * (uint64_t)kProgScanBlockBits) return 3;
        if ((1ull << P.levels) <= P.n_max / 15 + 2) return 4;
        uint64_t runs = 0;
        for (int i = 0; i < kProgScans; ++i) {
            const ProgGeom g = prog_geom(H, W, s, i);
            if (g.n > P.n_max || g.n == 0) return 5;
            if (prog_scan(i).Ss) {
                if (P.run_at[i] != runs) return 6;
                runs += g.n;
                if (prog_levels(g.n, prog_scan(i).Ah != 0) > P.levels) return 7;
            }
        }
        if (runs != P.run_elems) return 8;
        if (prog_bound_bytes(H, W, s) <= bound_bytes(H, W, s)) return 9;
        uint8_t frame[kProgFrameHeaderBytes];
        if (prog_frame_header(q, s, H, W, frame, sizeof frame) != kProgFrameHeaderBytes) return 10;
        if (prog_frame_header(q, s, H, W, frame, sizeof frame - 1) != -1) return 11;
        for (int i = 0; i < kProgScans; ++i) {
            uint64_t freq[2][256] = {};
            std::vector<int> syms;  // the symbols a scan can count: DC categories; AC run / size, ZRL and EOB runs
            if (prog_scan(i).Ss == 0)
                for (int v = 0; v < 12; ++v) syms.push_back(v);
            else
                for (int v = 0; v < 256; ++v)
                    if ((v & 15) <= 10) syms.push_back(v);  // (low nibble 0: ZRL and EOB0 .. EOB14)
            for (int k = 0; k < 2; ++k) {
                const int m = pick(1, (int)syms.size());
                for (int j = 0; j < m; ++j) freq[k][syms[rng() % syms.size()]] += rng() % 1000000;
                freq[k][0] += 1;
            }
            ProgTables t;
            if (!tables_of(i, freq, &t)) return 12;
            uint8_t hdr[kProgScanHeaderMax];
            const int n = prog_scan_header(i, t, hdr, sizeof hdr);
            if (n < 0 || n > kProgScanHeaderMax) return 13;
            if (n > 0 && prog_scan_header(i, t, hdr, (size_t)n - 1) != -1) return 14;
            const uint64_t bits = prog_scan_bits(i, freq, t, 17);
            if (prog_slots(prog_scan(i)) && (bits == UINT64_MAX || bits < 17)) return 15;
        }
    }
    std::printf("%d cases ok\n", cases);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc >= 4 && !std::strcmp(argv[1], "fuzz")) return fuzz((unsigned)std::strtoul(argv[2], nullptr, 10), std::atoi(argv[3]));
    if (argc == 6 && !std::strcmp(argv[1], "frame")) {
        uint8_t b[kProgFrameHeaderBytes];
        const int n = prog_frame_header(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), b, sizeof b);
        if (n < 0) return 2;
        hex(b, n);
        std::printf("\n");
        return 0;
    }
    if (argc == 4 + 512 && !std::strcmp(argv[1], "scan")) {
        const int scan = std::atoi(argv[2]);
        const uint64_t extra = std::strtoull(argv[3], nullptr, 10);
        uint64_t freq[2][256];
        for (int i = 0; i < 512; ++i) freq[i / 256][i % 256] = std::strtoull(argv[4 + i], nullptr, 10);
        ProgTables t;
        if (!tables_of(scan, freq, &t)) return 3;
        uint8_t hdr[kProgScanHeaderMax];
        const int n = prog_scan_header(scan, t, hdr, sizeof hdr);
        if (n < 0) return 4;
        hex(hdr, n);
        std::printf(" %llu\n", (unsigned long long)prog_scan_bits(scan, freq, t, extra));
        return 0;
    }
    std::fprintf(stderr, "usage: fuzz SEED N | frame Q S H W | scan I EXTRA F[512]\n");
    return 1;
}
