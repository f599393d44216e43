// repair_check.cpp -- the hot-pixel repair's shared text (raw2film_amd/csrc/r2f_repair_math.h) and its planner (r2f_repair_plan.cpp)
// on the CPU, built by tests/test_repair_host.py with g++ -fsanitize=address,undefined.
//   repair_check run IN OUT   IN: int32 H, W, P, threshold, q, min_neighbours; P * P doubles of black; 36 int32 colour ids when P is 6;
//                             H * W uint16.  OUT: uint32 replaced, H * W uint16: the planner's params through repair_sample.
//   repair_check table        the canonical X-Trans pattern and its 36 cyclic shifts: "dy dx" and the 36 * 4 * 2 offsets per line
//   repair_check refuse       every refusal of the planner leaves *out alone
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../include/r2f.h"
#include "../raw2film_amd/csrc/r2f_repair_math.h"

namespace {

const char* kCanonical[6] = {"GBGGRG", "RGRBGB", "GBGGRG", "GRGGBG", "BGBRGR", "GRGGBG"};

void shifted(int dy, int dx, int32_t (&cfa)[36]) {
    for (int y = 0; y < 6; ++y)
        for (int x = 0; x < 6; ++x) {
            const char c = kCanonical[(y + dy) % 6][(x + dx) % 6];
            cfa[y * 6 + x] = c == 'R' ? 0 : c == 'G' ? 1 : 2;
        }
}

int fail(const char* what) {
    std::fprintf(stderr, "repair_check: %s\n", what);
    return 1;
}

int run(const char* in_path, const char* out_path) {
    FILE* f = std::fopen(in_path, "rb");
    if (!f) return fail("cannot open the input");
    int32_t head[6];
    if (std::fread(head, sizeof(int32_t), 6, f) != 6) return fail("short header");
    const int H = head[0], W = head[1], P = head[2];
    if (H < 1 || W < 1 || H > 4096 || W > 4096 || (P != 2 && P != 6)) return fail("bad header");
    std::vector<double> black(P * P);
    if (std::fread(black.data(), sizeof(double), black.size(), f) != black.size()) return fail("short black table");
    int32_t cfa[36] = {};
    if (P == 6 && std::fread(cfa, sizeof(int32_t), 36, f) != 36) return fail("short pattern");
    std::vector<uint16_t> raw((size_t)H * W), out((size_t)H * W);
    if (std::fread(raw.data(), 2, raw.size(), f) != raw.size()) return fail("short mosaic");
    std::fclose(f);
    r2f_repair_params p;
    if (r2f_mosaic_repair_plan(P, P == 6 ? cfa : nullptr, black.data(), head[3], head[4], head[5], H, W, &p) != R2F_OK)
        return fail("the planner refused");
    const auto at = [&](int y, int x) { return (int)raw[(size_t)y * W + x]; };
    int replaced = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int v = P == 6 ? r2f::repair::repair_sample(at, r2f::repair::TableOffsets{p.offset}, at(y, x), H, W, y, x, p.black,
                                                              p.threshold, p.q, p.min_neighbours, &replaced)
                                 : r2f::repair::repair_sample(at, r2f::repair::BayerOffsets{}, at(y, x), H, W, y, x, p.black, p.threshold,
                                                              p.q, p.min_neighbours, &replaced);
            out[(size_t)y * W + x] = (uint16_t)v;
        }
    FILE* g = std::fopen(out_path, "wb");
    if (!g) return fail("cannot open the output");
    const uint32_t n = (uint32_t)replaced;
    std::fwrite(&n, 4, 1, g);
    std::fwrite(out.data(), 2, out.size(), g);
    std::fclose(g);
    return 0;
}

int table() {
    const double black[36] = {};
    for (int dy = 0; dy < 6; ++dy)
        for (int dx = 0; dx < 6; ++dx) {
            int32_t cfa[36];
            shifted(dy, dx, cfa);
            r2f_repair_params p;
            if (r2f_mosaic_repair_plan(6, cfa, black, 1000, 32, 4, 6, 6, &p) != R2F_OK) return fail("the planner refused a shift");
            std::printf("%d %d", dy, dx);
            for (int ph = 0; ph < 36; ++ph)
                for (int d = 0; d < 4; ++d) {
                    for (int e = 0; e < d; ++e)  // four DISTINCT neighbours at every phase
                        if (p.offset[ph][d][0] == p.offset[ph][e][0] && p.offset[ph][d][1] == p.offset[ph][e][1]) return fail("two quadrants share a neighbour");
                    std::printf(" %d %d", p.offset[ph][d][0], p.offset[ph][d][1]);
                }
            std::printf("\n");
        }
    return 0;
}

int refuse() {
    int32_t cfa[36];
    shifted(0, 0, cfa);
    double black2[4] = {512, 520, 500, 512}, black6[36];
    for (int i = 0; i < 36; ++i) black6[i] = 1000 + i;
    r2f_repair_params untouched;
    std::memset(&untouched, 0x5a, sizeof(untouched));
    int n = 0;
    const auto refused = [&](int period, const int32_t* c, const double* b, int thr, int q, int mn, int H, int W) {
        r2f_repair_params p = untouched;
        ++n;
        return r2f_mosaic_repair_plan(period, c, b, thr, q, mn, H, W, &p) == R2F_EINVAL && std::memcmp(&p, &untouched, sizeof(p)) == 0;
    };
    bool ok = true;
    ok &= refused(4, cfa, black2, 1000, 32, 4, 64, 64) && refused(0, cfa, black2, 1000, 32, 4, 64, 64);
    ok &= refused(2, nullptr, nullptr, 1000, 32, 4, 64, 64) && refused(6, nullptr, black6, 1000, 32, 4, 64, 64);
    ok &= refused(2, nullptr, black2, -1, 32, 4, 64, 64) && refused(2, nullptr, black2, 65536, 32, 4, 64, 64);
    ok &= refused(2, nullptr, black2, 1000, 0, 4, 64, 64) && refused(2, nullptr, black2, 1000, 256, 4, 64, 64);
    ok &= refused(2, nullptr, black2, 1000, 32, 2, 64, 64) && refused(2, nullptr, black2, 1000, 32, 5, 64, 64);
    ok &= refused(2, nullptr, black2, 1000, 32, 4, 5, 64) && refused(6, cfa, black6, 1000, 32, 4, 64, 5);
    for (const double bad : {-1.0, 65536.0, 512.5, std::numeric_limits<double>::quiet_NaN()}) {
        double b[4] = {512, bad, 500, 512};
        ok &= refused(2, nullptr, b, 1000, 32, 4, 64, 64);
        double b6[36];
        std::memcpy(b6, black6, sizeof(b6));
        b6[35] = bad;
        ok &= refused(6, cfa, b6, 1000, 32, 4, 64, 64);
    }
    int32_t bad_id[36];
    std::memcpy(bad_id, cfa, sizeof(bad_id));
    bad_id[7] = 3;
    ok &= refused(6, bad_id, black6, 1000, 32, 4, 64, 64);
    int32_t lone[36];  // one red site in a green field: no red inside ring 2 of it
    for (int i = 0; i < 36; ++i) lone[i] = 1;
    lone[0] = 0, lone[1] = 2;
    ok &= refused(6, lone, black6, 1000, 32, 4, 64, 64);
    if (r2f_mosaic_repair_plan(2, nullptr, black2, 1000, 32, 4, 64, 64, nullptr) != R2F_EINVAL) ok = false;
    r2f_repair_params p;
    if (r2f_mosaic_repair_plan(2, nullptr, black2, 0, 1, 3, 6, 6, &p) != R2F_OK || p.period != 2 || p.black[7] != 512 || p.black[6] != 500) ok = false;
    if (!ok) return fail("a refusal wrote the output, or was none");
    std::printf("refusals ok %d\n", n);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "run" && argc == 4) return run(argv[2], argv[3]);
    if (mode == "table") return table();
    if (mode == "refuse") return refuse();
    return fail("usage: repair_check run IN OUT | table | refuse");
}
