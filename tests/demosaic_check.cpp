// demosaic_check.cpp -- the Bayer demosaic's host half as a stand-alone program (tests/test_demosaic_host.py builds it with
// g++ -fsanitize=address,undefined,float-cast-overflow -ffp-contract=off against raw2film_amd/csrc/r2f_demosaic_plan.cpp):
//   demosaic_check fuzz SEED N      N random profiles through r2f_demosaic_plan: what it accepts keeps every trunc of the
//                                   definition inside int (checked on the extreme samples), what it must refuse it refuses
//   demosaic_check render JOB OUT   JOB: int32 H, W, half_size; r2f_raw_profile; uint16 mosaic[H * W].  OUT: r2f_demosaic_params;
//                                   uint16 (out_h, out_w, 3), rendered with r2f_demosaic_math.h -- the text the device kernels compile
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../raw2film_amd/csrc/r2f_demosaic_math.h"

using namespace r2f;

namespace {

struct Plane {
    const std::vector<int>* v;
    int W;
    int operator()(int y, int x) const { return v->at((size_t)y * W + x); }  // (at(): an index outside the frame aborts)
};

std::vector<uint16_t> render(const r2f_demosaic_params& p, const std::vector<uint16_t>& mosaic, int H, int W) {
    std::vector<int> s((size_t)H * W), g((size_t)H * W);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) s[(size_t)y * W + x] = demosaic::scale_sample(p, mosaic[(size_t)y * W + x], demosaic::site(y, x));
    const Plane S{&s, W}, G{&g, W};
    std::vector<uint16_t> out((size_t)p.out_h * p.out_w * 3);
    if (p.half_size) {
        for (int y = 0; y < p.out_h; ++y)
            for (int x = 0; x < p.out_w; ++x) {
                const int q[4] = {S(2 * y, 2 * x), S(2 * y, 2 * x + 1), S(2 * y + 1, 2 * x), S(2 * y + 1, 2 * x + 1)};
                int rgb[3];
                uint16_t o[3];
                demosaic::half_rgb(p, q, rgb);
                demosaic::colour(p, rgb, o);
                memcpy(&out[((size_t)y * p.out_w + x) * 3], o, sizeof o);
            }
        return out;
    }
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) g[(size_t)y * W + x] = demosaic::green_at(p, S, H, W, y, x);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            int rgb[3];
            uint16_t o[3];
            demosaic::pixel_rgb(p, S, G, H, W, y, x, rgb);
            demosaic::colour(p, rgb, o);
            memcpy(&out[((size_t)y * W + x) * 3], o, sizeof o);
        }
    return out;
}

int fail(const char* what, long long i) {
    fprintf(stderr, "case %lld: %s\n", i, what);
    return 1;
}

int fuzz(unsigned seed, long long n) {
    std::mt19937_64 rng(seed);
    auto uni = [&](double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); };
    const double odd[] = {NAN, INFINITY, -INFINITY, -1.0, 65536.0, 0.5, 1e-60, 0.0, 1024.0000001, -64.0000001, 1e300};
    long long accepted = 0;
    for (long long i = 0; i < n; ++i) {
        r2f_raw_profile pr{};
        pr.pattern = (int)(rng() % 6) - 1;  // -1 and 4 are unknown
        pr.half_size = (int)(rng() % 2);
        for (int k = 0; k < 4; ++k) pr.black[k] = std::floor(uni(0, 65536)), pr.mul[k] = uni(1e-6, 1024.0);
        for (int k = 0; k < 9; ++k) pr.matrix[k] = uni(-64.0, 64.0);
        int H = 2 + (int)(rng() % 40), W = 2 + (int)(rng() % 40);
        bool bad = pr.pattern < 0 || pr.pattern > 3;
        switch (rng() % 8) {
            case 0: pr.black[rng() % 4] = odd[rng() % 6], bad = true; break;            // NaN, +-inf, negative, too large, fractional
            case 1: { const double v = odd[rng() % 11]; pr.mul[rng() % 4] = v; bad = bad || !(v > 0 && v <= 1024.0) || (float)v <= 0.f; break; }
            case 2: { const double v = odd[rng() % 11]; pr.matrix[rng() % 9] = v; bad = bad || !(std::fabs(v) <= 64.0); break; }
            case 3: if (rng() % 2) H = (int)(rng() % 2); else W = (int)(rng() % 2); bad = true; break;  // below 2
            default: break;
        }
        if (pr.half_size && ((H | W) & 1)) bad = true;
        r2f_demosaic_params p;
        memset(&p, 0x5A, sizeof p);
        const int rc = r2f_demosaic_plan(&pr, H, W, &p);
        if (bad != (rc == R2F_EINVAL) || (rc != R2F_OK && rc != R2F_EINVAL)) return fail(bad ? "accepted what it must refuse" : "refused a valid profile", i);
        if (rc != R2F_OK) {
            const unsigned char* b = reinterpret_cast<const unsigned char*>(&p);
            for (size_t j = 0; j < sizeof p; ++j)
                if (b[j] != 0x5A) return fail("a refusal wrote to the params", i);
            continue;
        }
        ++accepted;
        if (p.out_h != (pr.half_size ? H / 2 : H) || p.out_w != (pr.half_size ? W / 2 : W)) return fail("output size", i);
        // the extremes of every float step stay inside int (float-cast-overflow aborts otherwise)
        for (int k = 0; k < 4; ++k) (void)demosaic::scale_sample(p, 65535, k), (void)demosaic::scale_sample(p, 0, k);
        const int ext[2] = {0, 65535};
        for (int m = 0; m < 8; ++m) {
            const int rgb[3] = {ext[m & 1], ext[(m >> 1) & 1], ext[(m >> 2) & 1]};
            uint16_t o[3];
            demosaic::colour(p, rgb, o);
        }
        // ... and a small frame renders without an index outside it
        std::vector<uint16_t> mosaic((size_t)H * W);
        for (auto& v : mosaic) v = (uint16_t)(rng() % 3 == 0 ? (rng() % 2) * 65535 : rng());
        if (render(p, mosaic, H, W).size() != (size_t)p.out_h * p.out_w * 3) return fail("render size", i);
    }
    if (r2f_demosaic_plan(nullptr, 4, 4, nullptr) != R2F_EINVAL) return fail("null arguments", -1);
    printf("%lld cases ok (%lld accepted)\n", n, accepted);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "fuzz")) return fuzz((unsigned)strtoul(argv[2], nullptr, 10), atoll(argv[3]));
    if (argc == 4 && !strcmp(argv[1], "render")) {
        FILE* f = fopen(argv[2], "rb");
        if (!f) return 2;
        int32_t head[3];
        r2f_raw_profile pr;
        if (fread(head, sizeof head, 1, f) != 1 || fread(&pr, sizeof pr, 1, f) != 1) return 2;
        const int H = head[0], W = head[1];
        pr.half_size = head[2];
        if (H < 1 || W < 1 || H > 4096 || W > 4096) return 2;
        std::vector<uint16_t> mosaic((size_t)H * W);
        if (fread(mosaic.data(), 2, mosaic.size(), f) != mosaic.size()) return 2;
        fclose(f);
        r2f_demosaic_params p;
        if (r2f_demosaic_plan(&pr, H, W, &p) != R2F_OK) return 3;
        const std::vector<uint16_t> out = render(p, mosaic, H, W);
        FILE* o = fopen(argv[3], "wb");
        if (!o) return 2;
        fwrite(&p, sizeof p, 1, o);
        fwrite(out.data(), 2, out.size(), o);
        fclose(o);
        return 0;
    }
    fprintf(stderr, "usage: demosaic_check fuzz SEED N | render JOB OUT\n");
    return 2;
}
