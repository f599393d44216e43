// denoise_check.cpp -- the wavelet denoise of a Bayer mosaic on the CPU, from the text the kernel compiles: r2f_denoise_math.h and the
// planner (r2f_denoise_plan.cpp).  tests/test_denoise_host.py builds it with g++ -fsanitize=address,undefined -ffp-contract=off
// and holds its bytes against tests/denoise_model.py.
//   denoise_check reflect            walks every (i, c, n), n in 32 .. 80, c in {1, 2, 4, 8, 16}: both taps stay inside [0, n)
//   denoise_check refuse             every refusal of the planner leaves *out alone; the shifts of the maxima the header names
//   denoise_check run IN OUT         IN: int32 H, W, maximum, black[4], then float64 threshold, then H * W uint16; OUT: H * W uint16
// Every line is laid out in heap vectors of its exact size, so an index outside a plane is an AddressSanitizer report.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/r2f.h"
#include "../raw2film_amd/csrc/r2f_denoise_math.h"

using namespace r2f::denoise;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

static int reflect_walk() {
    long taps = 0;
    for (int n = 32; n <= 80; ++n)
        for (int lev = 0; lev < kLevels; ++lev) {
            const int c = 1 << lev;
            std::vector<int> line(n, 1);  // (indexing it is the check ASan makes)
            for (int i = 0; i < n; ++i) {
                const int m = reflect_m(i, c), p = reflect_p(i, c, n);
                CHECK(m >= 0 && m < n && p >= 0 && p < n);
                taps += line[m] + line[p];
            }
        }
    std::printf("reflect ok %ld\n", taps);
    return 0;
}

static bool untouched(const r2f_denoise_params& p) {
    return p.black[0] == -11 && p.black[1] == -12 && p.black[2] == -13 && p.black[3] == -14 && p.shift == -15 && p.threshold == -16.f;
}

static int refusals() {
    const double ok[4] = {512, 515, 509, 512};
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    struct Case {
        double threshold;
        int maximum;
        double black[4];
        int H, W;
        bool null_black, null_out;
    };
    const Case cases[] = {
        {0.0, 16383, {512, 515, 509, 512}, 64, 64, false, false},   {-1.0, 16383, {512, 515, 509, 512}, 64, 64, false, false},
        {nan, 16383, {512, 515, 509, 512}, 64, 64, false, false},   {inf, 16383, {512, 515, 509, 512}, 64, 64, false, false},
        {1000000.5, 16383, {512, 515, 509, 512}, 64, 64, false, false}, {1e-60, 16383, {512, 515, 509, 512}, 64, 64, false, false},
        {100.0, 0, {512, 515, 509, 512}, 64, 64, false, false},     {100.0, 65536, {512, 515, 509, 512}, 64, 64, false, false},
        {100.0, -5, {512, 515, 509, 512}, 64, 64, false, false},    {100.0, 16383, {512, 515.5, 509, 512}, 64, 64, false, false},
        {100.0, 16383, {-1, 515, 509, 512}, 64, 64, false, false},  {100.0, 16383, {512, 515, 509, 65536}, 64, 64, false, false},
        {100.0, 16383, {512, nan, 509, 512}, 64, 64, false, false}, {100.0, 16383, {512, 515, 509, 512}, 62, 64, false, false},
        {100.0, 16383, {512, 515, 509, 512}, 64, 62, false, false}, {100.0, 16383, {512, 515, 509, 512}, 65, 64, false, false},
        {100.0, 16383, {512, 515, 509, 512}, 64, 67, false, false}, {100.0, 16383, {512, 515, 509, 512}, 0, 0, false, false},
        {100.0, 16383, {512, 515, 509, 512}, -64, 64, false, false}, {100.0, 16383, {512, 515, 509, 512}, 64, 64, true, false},
        {100.0, 16383, {512, 515, 509, 512}, 64, 64, false, true},
    };
    int n = 0;
    for (const Case& c : cases) {
        r2f_denoise_params p{{-11, -12, -13, -14}, -15, -16.f};
        const int rc = r2f_mosaic_denoise_plan(c.threshold, c.maximum, c.null_black ? nullptr : c.black, c.H, c.W, c.null_out ? nullptr : &p);
        CHECK(rc == R2F_EINVAL);
        CHECK(untouched(p));
        ++n;
    }
    const int maxima[6] = {1, 255, 16383 - 512, 32767, 32768, 65535}, shifts[6] = {15, 8, 2, 1, 0, 0};
    for (int i = 0; i < 6; ++i) {
        r2f_denoise_params p{};
        CHECK(r2f_mosaic_denoise_plan(100.0, maxima[i], ok, 64, 66, &p) == R2F_OK);
        CHECK(p.shift == shifts[i] && p.threshold == 100.f && p.black[1] == 515 && p.black[2] == 509);
        CHECK(((long long)maxima[i] << p.shift) < 65536 && (p.shift == kMaxShift || ((long long)maxima[i] << (p.shift + 1)) >= 65536));
    }
    CHECK(r2f_mosaic_denoise_workspace_bytes(64, 66) == (size_t)12 * 64 * 66 && r2f_mosaic_denoise_workspace_bytes(62, 66) == 0 &&
          r2f_mosaic_denoise_workspace_bytes(64, 65) == 0);
    std::printf("refusals ok %d\n", n);
    return 0;
}

// steps 2 to 4 of one plane, line by line
static void plane(const std::vector<float>& F, int nr, int nc, float threshold, std::vector<int>& out) {
    std::vector<float> in = F, rows((size_t)nr * nc), low((size_t)nr * nc), D((size_t)nr * nc, 0.f);
    for (int lev = 0; lev < kLevels; ++lev) {
        const int c = 1 << lev;
        const float theta = theta_of(threshold, lev);
        for (int y = 0; y < nr; ++y)
            for (int x = 0; x < nc; ++x)
                rows[(size_t)y * nc + x] = quarter_hat(in[(size_t)y * nc + x], in[(size_t)y * nc + reflect_m(x, c)], in[(size_t)y * nc + reflect_p(x, c, nc)]);
        for (int y = 0; y < nr; ++y)
            for (int x = 0; x < nc; ++x) {
                const size_t i = (size_t)y * nc + x;
                low[i] = quarter_hat(rows[i], rows[(size_t)reflect_m(y, c) * nc + x], rows[(size_t)reflect_p(y, c, nr) * nc + x]);
                const float dd = shrink(in[i], low[i], theta);
                D[i] = lev == 0 ? dd : D[i] + dd;
            }
        in = low;
    }
    out.resize((size_t)nr * nc);
    for (size_t i = 0; i < out.size(); ++i) out[i] = finish(D[i], low[i]);
}

static int run(const char* in_path, const char* out_path) {
    std::FILE* f = std::fopen(in_path, "rb");
    CHECK(f);
    int32_t head[7];
    double threshold;
    CHECK(std::fread(head, sizeof(head), 1, f) == 1 && std::fread(&threshold, sizeof(threshold), 1, f) == 1);
    const int H = head[0], W = head[1], maximum = head[2];
    const double black[4] = {(double)head[3], (double)head[4], (double)head[5], (double)head[6]};
    r2f_denoise_params p{};
    CHECK(r2f_mosaic_denoise_plan(threshold, maximum, black, H, W, &p) == R2F_OK);
    CHECK(params_ok(p.black, p.shift, p.threshold));
    std::vector<uint16_t> mosaic((size_t)H * W), result((size_t)H * W);
    CHECK(std::fread(mosaic.data(), 2, mosaic.size(), f) == mosaic.size());
    std::fclose(f);
    const int nr = H / 2, nc = W / 2;
    for (int k = 0; k < 4; ++k) {
        const int yy = k >> 1, xx = k & 1;
        std::vector<float> F((size_t)nr * nc);
        for (int y = 0; y < nr; ++y)
            for (int x = 0; x < nc; ++x) F[(size_t)y * nc + x] = lift(mosaic[(size_t)(2 * y + yy) * W + 2 * x + xx], p.black[k], p.shift);
        std::vector<int> out;
        plane(F, nr, nc, p.threshold, out);
        for (int y = 0; y < nr; ++y)
            for (int x = 0; x < nc; ++x) {
                const int v = out[(size_t)y * nc + x];
                CHECK(v >= 0 && v <= 65535);
                result[(size_t)(2 * y + yy) * W + 2 * x + xx] = (uint16_t)v;
            }
    }
    std::FILE* g = std::fopen(out_path, "wb");
    CHECK(g);
    CHECK(std::fwrite(result.data(), 2, result.size(), g) == result.size());
    std::fclose(g);
    std::printf("run ok %d %d shift %d\n", H, W, p.shift);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "reflect")) return reflect_walk();
    if (argc == 2 && !std::strcmp(argv[1], "refuse")) return refusals();
    if (argc == 4 && !std::strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    std::fprintf(stderr, "usage: denoise_check reflect | refuse | run IN OUT\n");
    return 2;
}
