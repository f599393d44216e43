// lens_tca_check.cpp -- the host half of the lens correction with TCA on the CPU, with its own main (tests/test_lens_tca_host.py
// builds it with g++ -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all -ffp-contract=off together with
// raw2film_amd/csrc/r2f_lens_plan.cpp, r2f_plan.cpp and r2f_lens_math.h -- the text the device kernel compiles).
//   lens_tca_check fuzz SEED CASES  r2f_lens_plan_tca over random profiles and TCA records, huge and non-finite numbers among them,
//                                   each accepted plan checked against its contract; whole pixels through the accepted and through
//                                   hostile constants with a fetch that refuses an index outside the frame
//   lens_tca_check render IN OUT    IN: int32 {H, W, channels, row0, col0, rows, cols}, an r2f_lens_profile, an r2f_lens_tca,
//                                   H*W*channels floats; OUT: the r2f_lens_params, the r2f_lens_tca_params, then rows*cols*3 floats
//                                   (interleaved) of the corrected window
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../include/r2f.h"
#include "../raw2film_amd/csrc/r2f_lens_math.h"

namespace {

int g_failed = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            std::fprintf(stderr, "FAILED %s: ", #cond);   \
            std::fprintf(stderr, __VA_ARGS__);            \
            std::fprintf(stderr, "\n");                   \
            ++g_failed;                                   \
        }                                                 \
    } while (0)

struct Frame {
    const float* data;
    int H, W, C;
    mutable long long bad = 0;
    float operator()(int ch, int y, int x) const {
        if (y < 0 || y >= H || x < 0 || x >= W || ch < 0 || ch > 2) {  // (never reached if the decision holds: counted, nothing indexed)
            ++bad;
            return 0.f;
        }
        return data[((size_t)y * W + x) * C + ch];
    }
};

// the three-channel frame as r2f_lens_math.h's correct_pixel reads it
struct Frame3 {
    const Frame& f;
    void operator()(int y, int x, float (&v)[3]) const {
        for (int c = 0; c < 3; ++c) v[c] = f(c, y, x);
    }
};

bool fits(double v) { return std::isfinite(v) && std::fabs(v) <= 3.0e38; }

int fuzz(uint64_t seed, int cases) {
    std::mt19937_64 rng(seed);
    auto uni = [&](double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); };
    auto pick = [&](int n) { return (int)(rng() % (uint64_t)n); };
    const double hostile[] = {0.0, -0.0, 1e-300, -1e-300, 1e30, -1e30, 1e300, -1e300, INFINITY, -INFINITY, NAN, 1.0, -1.0, 3.4e38, 5e-324};
    const int nh = (int)(sizeof hostile / sizeof hostile[0]);
    const int sides[] = {1, 2, 3, 7, 9, 33, 47, 64, 1000, 4096, 8191, 16384};
    const int ns = (int)(sizeof sides / sizeof sides[0]);
    float table[256];
    CHECK(r2f_lens_phase_table(table) == R2F_OK, "phase table");
    std::vector<float> small(16 * 16 * 3, 1.f);
    long long accepted = 0, identities = 0;
    for (int n = 0; n < cases; ++n) {
        r2f_lens_profile pr{};
        const bool wild = pick(3) == 0;  // a third of the cases: hostile numbers anywhere
        pr.model = pick(4);
        pr.n_coef = pr.model;
        for (int i = 0; i < 3; ++i) pr.coef[i] = wild && pick(6) == 0 ? hostile[pick(nh)] : uni(-0.2, 0.2);
        pr.has_vignetting = pick(2);
        for (int i = 0; i < 3; ++i) pr.vignetting[i] = uni(-0.5, 0.5);
        for (int i = 0; i < 2; ++i) pr.center[i] = uni(-0.05, 0.05);
        pr.auto_scale = pick(3) == 0;
        pr.scale = uni(0.2, 3.0);
        pr.norm_radius_px = pick(3) ? 0.0 : uni(0.5, 20000.0);
        r2f_lens_tca tc{};
        tc.model = wild && pick(6) == 0 ? pick(7) - 2 : 1 + pick(2);
        tc.n_coef = wild && pick(6) == 0 ? pick(5) : (tc.model == R2F_TCA_LINEAR ? 1 : 3);
        const bool identity = !wild && pick(8) == 0;
        for (int i = 0; i < 3; ++i) {
            tc.red[i] = identity ? (i == 0) : wild && pick(3) == 0 ? hostile[pick(nh)] : (i == 0 ? uni(0.9, 1.1) : uni(-0.05, 0.05));
            tc.blue[i] = identity ? (i == 0) : wild && pick(3) == 0 ? hostile[pick(nh)] : (i == 0 ? uni(0.9, 1.1) : uni(-0.05, 0.05));
        }
        const int H = wild && pick(10) == 0 ? pick(3) - 1 : sides[pick(ns)], W = wild && pick(10) == 0 ? pick(3) - 1 : sides[pick(ns)];
        r2f_lens_params out, plain;
        r2f_lens_tca_params tp;
        std::memset(&out, 0x5A, sizeof out);
        std::memset(&tp, 0x5A, sizeof tp);
        const int rc = r2f_lens_plan_tca(&pr, &tc, H, W, &out, &tp);
        CHECK(rc == R2F_OK || rc == R2F_EINVAL, "rc %d", rc);
        const int rc_plain = r2f_lens_plan(&pr, H, W, &plain);
        bool bad = tc.model != R2F_TCA_LINEAR && tc.model != R2F_TCA_POLY3;
        if (!bad) bad = tc.n_coef != (tc.model == R2F_TCA_LINEAR ? 1 : 3);
        if (!bad)
            for (int i = 0; i < tc.n_coef; ++i) bad = bad || !fits(tc.red[i]) || !fits(tc.blue[i]);
        if (bad) CHECK(rc == R2F_EINVAL, "a bad TCA record was accepted (model %d, n_coef %d)", tc.model, tc.n_coef);
        if (rc_plain != R2F_OK && !pr.auto_scale) CHECK(rc == R2F_EINVAL, "a profile r2f_lens_plan refuses was accepted");
        if (rc != R2F_OK) continue;
        ++accepted;
        CHECK(tp.model == tc.model, "TCA model");
        for (int i = 0; i < 3; ++i) {
            const float r = i < tc.n_coef ? (float)tc.red[i] : 0.f, b = i < tc.n_coef ? (float)tc.blue[i] : 0.f;
            CHECK(std::memcmp(&tp.red[i], &r, 4) == 0 && std::memcmp(&tp.blue[i], &b, 4) == 0, "TCA constant %d is not the double rounded to float", i);
        }
        if (!pr.auto_scale) CHECK(rc_plain == R2F_OK && std::memcmp(&out, &plain, sizeof out) == 0, "without auto scale the params are r2f_lens_plan's");
        if (identity) {
            ++identities;
            CHECK(rc_plain == R2F_OK && std::memcmp(&out, &plain, sizeof out) == 0, "an identity record resolves to r2f_lens_plan's params");
        }
        // a few whole pixels of a 16 x 16 frame through these constants (whatever frame they were made for): nothing outside it is
        // fetched, green is r2f_lens_correct's, and with an identity record so are red and blue
        Frame fr{small.data(), 16, 16, 3};
        const Frame3 fr3{fr};
        for (int t = 0; t < 8; ++t) {
            float v[3], w[3];
            const int X = pick(40) - 12, Y = pick(40) - 12;
            r2f::lens::correct_pixel_tca(out, tp, fr, 16, 16, table, X, Y, v);
            r2f::lens::correct_pixel(out, fr3, 16, 16, table, X, Y, w);
            CHECK(std::memcmp(&v[1], &w[1], 4) == 0, "green differs from r2f_lens_correct's at (%d, %d)", X, Y);
            if (identity) CHECK(std::memcmp(v, w, sizeof v) == 0, "an identity record differs from r2f_lens_correct at (%d, %d)", X, Y);
        }
        CHECK(fr.bad == 0, "a tap outside the frame was fetched");
    }
    // whole pixels whose map and TCA constants are hostile
    r2f_lens_params hp{};
    hp.model = R2F_LENS_PTLENS;
    Frame fr{small.data(), 16, 16, 3};
    const float hf[] = {NAN, INFINITY, -INFINITY, 1e30f, -1e30f, 3.4e38f, 0.f, 1.f, -1.f, 1e-40f};
    for (float a : hf)
        for (float b : hf)
            for (int model : {R2F_TCA_LINEAR, R2F_TCA_POLY3})
                for (int benign = 0; benign < 2; ++benign) {
                    r2f_lens_tca_params tp{};
                    tp.model = model;
                    tp.red[0] = a, tp.red[1] = b, tp.red[2] = a, tp.blue[0] = b, tp.blue[1] = a, tp.blue[2] = b;
                    if (benign)  // a sane map under hostile TCA constants ...
                        hp.cx = hp.cy = 7.5f, hp.q = 0.1f, hp.inv_scale = 1.f, hp.c0 = 1.f, hp.k[0] = hp.k[1] = hp.k[2] = 0.f, hp.qv = 0.1f, hp.vignetting = 0;
                    else  // ... and a hostile one
                        hp.cx = a == 0.f ? 7.5f : a, hp.cy = 7.5f, hp.q = b, hp.inv_scale = b, hp.c0 = a, hp.k[0] = b, hp.k[1] = a, hp.k[2] = b,
                        hp.vignetting = 1, hp.qv = b, hp.v[0] = a, hp.v[1] = b, hp.v[2] = a;
                    for (int y = -2; y < 18; y += 3)
                        for (int x = -2; x < 18; x += 3) {
                            float v[3];
                            r2f::lens::correct_pixel_tca(hp, tp, fr, 16, 16, table, x, y, v);
                        }
                }
    CHECK(fr.bad == 0, "a tap outside the frame was fetched (hostile constants)");
    // the planner's own refusals
    {
        r2f_lens_profile pr{};
        pr.scale = 1.0;
        r2f_lens_tca tc{};
        tc.model = R2F_TCA_LINEAR, tc.n_coef = 1, tc.red[0] = tc.blue[0] = 1.0;
        r2f_lens_params out;
        r2f_lens_tca_params tp;
        CHECK(r2f_lens_plan_tca(&pr, &tc, 10, 10, &out, &tp) == R2F_OK, "a plain record");
        CHECK(r2f_lens_plan_tca(nullptr, &tc, 10, 10, &out, &tp) == R2F_EINVAL && r2f_lens_plan_tca(&pr, nullptr, 10, 10, &out, &tp) == R2F_EINVAL &&
                  r2f_lens_plan_tca(&pr, &tc, 10, 10, nullptr, &tp) == R2F_EINVAL && r2f_lens_plan_tca(&pr, &tc, 10, 10, &out, nullptr) == R2F_EINVAL,
              "null arguments");
        tc.model = R2F_TCA_NONE, tc.n_coef = 0;
        CHECK(r2f_lens_plan_tca(&pr, &tc, 10, 10, &out, &tp) == R2F_EINVAL, "R2F_TCA_NONE");
    }
    if (g_failed) return 1;
    std::printf("%d cases ok (%lld accepted, %lld identities)\n", cases, accepted, identities);
    return 0;
}

int render(const char* in_path, const char* out_path) {
    FILE* f = std::fopen(in_path, "rb");
    if (!f) return 2;
    int32_t head[7];
    r2f_lens_profile pr;
    r2f_lens_tca tc;
    if (std::fread(head, sizeof head, 1, f) != 1 || std::fread(&pr, sizeof pr, 1, f) != 1 || std::fread(&tc, sizeof tc, 1, f) != 1) return 2;
    const int H = head[0], W = head[1], C = head[2], r0 = head[3], c0 = head[4], nr = head[5], nc = head[6];
    if (H < 1 || W < 1 || (C != 3 && C != 4) || nr < 1 || nc < 1 || H > 4096 || W > 4096 || nr > 4096 || nc > 4096) return 2;
    std::vector<float> img((size_t)H * W * C);
    if (std::fread(img.data(), sizeof(float), img.size(), f) != img.size()) return 2;
    std::fclose(f);
    r2f_lens_params p;
    r2f_lens_tca_params tp;
    if (r2f_lens_plan_tca(&pr, &tc, H, W, &p, &tp) != R2F_OK) return 3;
    float table[256];
    r2f_lens_phase_table(table);
    const Frame fr{img.data(), H, W, C};
    std::vector<float> out((size_t)nr * nc * 3);
    for (int y = 0; y < nr; ++y)
        for (int x = 0; x < nc; ++x) {
            float v[3];
            r2f::lens::correct_pixel_tca(p, tp, fr, H, W, table, c0 + x, r0 + y, v);
            std::memcpy(&out[((size_t)y * nc + x) * 3], v, sizeof v);
        }
    if (fr.bad) return 4;
    FILE* o = std::fopen(out_path, "wb");
    if (!o) return 2;
    std::fwrite(&p, sizeof p, 1, o);
    std::fwrite(&tp, sizeof tp, 1, o);
    std::fwrite(out.data(), sizeof(float), out.size(), o);
    std::fclose(o);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "fuzz")) return fuzz(std::strtoull(argv[2], nullptr, 10), std::atoi(argv[3]));
    if (argc == 4 && !std::strcmp(argv[1], "render")) return render(argv[2], argv[3]);
    std::fprintf(stderr, "usage: lens_tca_check fuzz SEED CASES | lens_tca_check render IN OUT\n");
    return 64;
}
