// lens_projection_check.cpp -- the host half of the projected lens correction on the CPU, with its own main
// (tests/test_lens_projection_host.py builds it with g++ -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all
// -ffp-contract=off together with raw2film_amd/csrc/r2f_lens_plan.cpp, r2f_plan.cpp and r2f_lens_math.h -- the text the device
// kernels compile).
//   lens_projection_check fuzz SEED CASES  r2f_lens_plan_projected over random profiles, projections and TCA records, huge and
//                                          non-finite numbers among them, each accepted plan checked against its contract; whole
//                                          pixels through the accepted and through hostile constants with a fetch that refuses an
//                                          index outside the frame
//   lens_projection_check render IN OUT    IN: int32 {H, W, channels, row0, col0, rows, cols, has_tca}, an r2f_lens_profile, an
//                                          r2f_lens_projection, an r2f_lens_tca (read when has_tca), H*W*channels floats; OUT: the
//                                          r2f_lens_params, the r2f_lens_projection_params, the r2f_lens_tca_params (zeros without
//                                          a record), then rows*cols*3 floats (interleaved) of the corrected window
//   lens_projection_check atan             the fisheye factor of r2f_lens_math.h against atan(t)/t in double for every float32 t in
//                                          [2^-13, 1] and in (1, 64]: prints the largest error of each range in units of the last
//                                          place of the exact value
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
    const double hostile[] = {0.0, -0.0, 1e-300, -1e-300, 1e30, -1e30, 1e300, -1e300, INFINITY, -INFINITY, NAN, 1.0, -1.0, 3.4e38, 5e-324, 1e-39};
    const int nh = (int)(sizeof hostile / sizeof hostile[0]);
    const int sides[] = {1, 2, 3, 7, 9, 33, 47, 64, 1000, 4096, 8191, 16384};
    const int ns = (int)(sizeof sides / sizeof sides[0]);
    float table[256];
    CHECK(r2f_lens_phase_table(table) == R2F_OK, "phase table");
    std::vector<float> small(16 * 16 * 3, 1.f);
    for (size_t i = 0; i < small.size(); ++i) small[i] = (float)(i % 7) * 0.5f;
    long long accepted = 0, identities = 0, refused_auto = 0;
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
        const bool identity = !wild && pick(8) == 0;
        r2f_lens_projection pj{};
        pj.type = wild && pick(4) == 0 ? pick(9) - 2 : 1 + pick(4);
        pj.focal = identity ? std::ldexp(1.0, 40) : wild && pick(3) == 0 ? hostile[pick(nh)] : uni(0.1, 3.0);
        const bool with_tca = pick(2) == 1;
        r2f_lens_tca tc{};
        tc.model = wild && pick(6) == 0 ? pick(7) - 2 : 1 + pick(2);
        tc.n_coef = wild && pick(6) == 0 ? pick(5) : (tc.model == R2F_TCA_LINEAR ? 1 : 3);
        for (int i = 0; i < 3; ++i) {
            tc.red[i] = wild && pick(3) == 0 ? hostile[pick(nh)] : (i == 0 ? uni(0.9, 1.1) : uni(-0.05, 0.05));
            tc.blue[i] = wild && pick(3) == 0 ? hostile[pick(nh)] : (i == 0 ? uni(0.9, 1.1) : uni(-0.05, 0.05));
        }
        const int H = wild && pick(10) == 0 ? pick(3) - 1 : sides[pick(ns)], W = wild && pick(10) == 0 ? pick(3) - 1 : sides[pick(ns)];
        r2f_lens_params out, plain;
        r2f_lens_projection_params pp;
        r2f_lens_tca_params tp, tp_plain;
        std::memset(&out, 0x5A, sizeof out);
        std::memset(&pp, 0x5A, sizeof pp);
        std::memset(&tp, 0x5A, sizeof tp);
        const int rc = r2f_lens_plan_projected(&pr, &pj, with_tca ? &tc : nullptr, H, W, &out, &pp, with_tca ? &tp : nullptr);
        CHECK(rc == R2F_OK || rc == R2F_EINVAL, "rc %d", rc);
        const int rc_plain = with_tca ? r2f_lens_plan_tca(&pr, &tc, H, W, &plain, &tp_plain) : r2f_lens_plan(&pr, H, W, &plain);
        bool bad = pj.type < R2F_PROJ_FISHEYE || pj.type > R2F_PROJ_ORTHOGRAPHIC;
        bad = bad || !(std::isfinite(pj.focal) && pj.focal > 0) || !fits(1.0 / pj.focal);
        if (bad) CHECK(rc == R2F_EINVAL, "a bad projection was accepted (type %d, focal %g)", pj.type, pj.focal);
        if (rc_plain != R2F_OK && !pr.auto_scale) CHECK(rc == R2F_EINVAL, "a profile the other planners refuse was accepted");
        if (!bad && rc_plain == R2F_OK && !pr.auto_scale) CHECK(rc == R2F_OK, "a sound projection on a sound profile was refused");
        if (rc != R2F_OK) {
            if (!bad && rc_plain == R2F_OK) ++refused_auto;
            continue;
        }
        ++accepted;
        const float inv = (float)(1.0 / pj.focal);
        CHECK(pp.type == pj.type && std::memcmp(&pp.inv_focal, &inv, 4) == 0, "the projection params are not the record's");
        if (with_tca) CHECK(rc_plain != R2F_OK || std::memcmp(&tp, &tp_plain, sizeof tp) == 0, "the TCA params are not r2f_lens_plan_tca's");
        if (!pr.auto_scale) CHECK(rc_plain == R2F_OK && std::memcmp(&out, &plain, sizeof out) == 0, "without auto scale the params are the plain planner's");
        if (identity) {
            ++identities;
            CHECK(rc_plain == R2F_OK && std::memcmp(&out, &plain, sizeof out) == 0, "an identity projection resolves to the plain planner's params");
        }
        // a few whole pixels of a 16 x 16 frame through these constants (whatever frame they were made for): nothing outside it is
        // fetched, and with an identity projection the result is the unprojected form's
        Frame fr{small.data(), 16, 16, 3};
        const Frame3 fr3{fr};
        for (int t = 0; t < 8; ++t) {
            float v[3], w[3];
            const int X = pick(40) - 12, Y = pick(40) - 12;
            if (with_tca) {
                r2f::lens::correct_pixel_tca(out, pp, tp, fr, 16, 16, table, X, Y, v);
                r2f::lens::correct_pixel_tca(out, tp, fr, 16, 16, table, X, Y, w);
            } else {
                r2f::lens::correct_pixel(out, pp, fr3, 16, 16, table, X, Y, v);
                r2f::lens::correct_pixel(out, fr3, 16, 16, table, X, Y, w);
            }
            if (identity) CHECK(std::memcmp(v, w, sizeof v) == 0, "an identity projection differs from the unprojected form at (%d, %d)", X, Y);
        }
        CHECK(fr.bad == 0, "a tap outside the frame was fetched");
    }
    // whole pixels whose map, projection and TCA constants are hostile
    r2f_lens_params hp{};
    hp.model = R2F_LENS_PTLENS;
    Frame fr{small.data(), 16, 16, 3};
    const Frame3 fr3{fr};
    const float hf[] = {NAN, INFINITY, -INFINITY, 1e30f, -1e30f, 3.4e38f, 0.f, 1.f, -1.f, 1e-40f};
    for (float a : hf)
        for (float b : hf)
            for (int type = 0; type <= 5; ++type)
                for (int benign = 0; benign < 2; ++benign) {
                    r2f_lens_projection_params pp{};
                    pp.type = type, pp.inv_focal = a;
                    r2f_lens_tca_params tp{};
                    tp.model = R2F_TCA_POLY3;
                    tp.red[0] = a, tp.red[1] = b, tp.red[2] = a, tp.blue[0] = b, tp.blue[1] = a, tp.blue[2] = b;
                    if (benign)  // a sane map under a hostile projection ...
                        hp.cx = hp.cy = 7.5f, hp.q = 0.1f, hp.inv_scale = 1.f, hp.c0 = 1.f, hp.k[0] = hp.k[1] = hp.k[2] = 0.f, hp.qv = 0.1f, hp.vignetting = 0;
                    else  // ... and a hostile one
                        hp.cx = a == 0.f ? 7.5f : a, hp.cy = 7.5f, hp.q = b, hp.inv_scale = b, hp.c0 = a, hp.k[0] = b, hp.k[1] = a, hp.k[2] = b,
                        hp.vignetting = 1, hp.qv = b, hp.v[0] = a, hp.v[1] = b, hp.v[2] = a;
                    for (int y = -2; y < 18; y += 3)
                        for (int x = -2; x < 18; x += 3) {
                            float v[3];
                            r2f::lens::correct_pixel(hp, pp, fr3, 16, 16, table, x, y, v);
                            r2f::lens::correct_pixel_tca(hp, pp, tp, fr, 16, 16, table, x, y, v);
                        }
                }
    CHECK(fr.bad == 0, "a tap outside the frame was fetched (hostile constants)");
    // the planner's own refusals
    {
        r2f_lens_profile pr{};
        pr.scale = 1.0;
        r2f_lens_projection pj{R2F_PROJ_FISHEYE, 0.6};
        r2f_lens_tca tc{};
        tc.model = R2F_TCA_LINEAR, tc.n_coef = 1, tc.red[0] = tc.blue[0] = 1.0;
        r2f_lens_params out;
        r2f_lens_projection_params pp;
        r2f_lens_tca_params tp;
        CHECK(r2f_lens_plan_projected(&pr, &pj, nullptr, 10, 10, &out, &pp, nullptr) == R2F_OK, "a plain record");
        CHECK(r2f_lens_plan_projected(&pr, &pj, &tc, 10, 10, &out, &pp, &tp) == R2F_OK, "a plain record with TCA");
        CHECK(r2f_lens_plan_projected(nullptr, &pj, nullptr, 10, 10, &out, &pp, nullptr) == R2F_EINVAL &&
                  r2f_lens_plan_projected(&pr, nullptr, nullptr, 10, 10, &out, &pp, nullptr) == R2F_EINVAL &&
                  r2f_lens_plan_projected(&pr, &pj, nullptr, 10, 10, nullptr, &pp, nullptr) == R2F_EINVAL &&
                  r2f_lens_plan_projected(&pr, &pj, nullptr, 10, 10, &out, nullptr, nullptr) == R2F_EINVAL &&
                  r2f_lens_plan_projected(&pr, &pj, &tc, 10, 10, &out, &pp, nullptr) == R2F_EINVAL &&
                  r2f_lens_plan_projected(&pr, &pj, nullptr, 10, 10, &out, &pp, &tp) == R2F_EINVAL,
              "null arguments");
        pj.type = R2F_PROJ_NONE;
        CHECK(r2f_lens_plan_projected(&pr, &pj, nullptr, 10, 10, &out, &pp, nullptr) == R2F_EINVAL, "R2F_PROJ_NONE");
        pj.type = R2F_PROJ_FISHEYE, tc.model = R2F_TCA_NONE, tc.n_coef = 0;
        CHECK(r2f_lens_plan_projected(&pr, &pj, &tc, 10, 10, &out, &pp, &tp) == R2F_EINVAL, "R2F_TCA_NONE");
    }
    if (g_failed) return 1;
    std::printf("%d cases ok (%lld accepted, %lld identities, %lld refused by the auto scale alone)\n", cases, accepted, identities, refused_auto);
    return 0;
}

int render(const char* in_path, const char* out_path) {
    FILE* f = std::fopen(in_path, "rb");
    if (!f) return 2;
    int32_t head[8];
    r2f_lens_profile pr;
    r2f_lens_projection pj;
    r2f_lens_tca tc;
    if (std::fread(head, sizeof head, 1, f) != 1 || std::fread(&pr, sizeof pr, 1, f) != 1 || std::fread(&pj, sizeof pj, 1, f) != 1 ||
        std::fread(&tc, sizeof tc, 1, f) != 1)
        return 2;
    const int H = head[0], W = head[1], C = head[2], r0 = head[3], c0 = head[4], nr = head[5], nc = head[6];
    const bool with_tca = head[7] != 0;
    if (H < 1 || W < 1 || (C != 3 && C != 4) || nr < 1 || nc < 1 || H > 4096 || W > 4096 || nr > 4096 || nc > 4096) return 2;
    std::vector<float> img((size_t)H * W * C);
    if (std::fread(img.data(), sizeof(float), img.size(), f) != img.size()) return 2;
    std::fclose(f);
    r2f_lens_params p;
    r2f_lens_projection_params pp;
    r2f_lens_tca_params tp{};
    if (r2f_lens_plan_projected(&pr, &pj, with_tca ? &tc : nullptr, H, W, &p, &pp, with_tca ? &tp : nullptr) != R2F_OK) return 3;
    float table[256];
    r2f_lens_phase_table(table);
    const Frame fr{img.data(), H, W, C};
    const Frame3 fr3{fr};
    std::vector<float> out((size_t)nr * nc * 3);
    for (int y = 0; y < nr; ++y)
        for (int x = 0; x < nc; ++x) {
            float v[3];
            if (with_tca)
                r2f::lens::correct_pixel_tca(p, pp, tp, fr, H, W, table, c0 + x, r0 + y, v);
            else
                r2f::lens::correct_pixel(p, pp, fr3, H, W, table, c0 + x, r0 + y, v);
            std::memcpy(&out[((size_t)y * nc + x) * 3], v, sizeof v);
        }
    if (fr.bad) return 4;
    FILE* o = std::fopen(out_path, "wb");
    if (!o) return 2;
    std::fwrite(&p, sizeof p, 1, o);
    std::fwrite(&pp, sizeof pp, 1, o);
    std::fwrite(&tp, sizeof tp, 1, o);
    std::fwrite(out.data(), sizeof(float), out.size(), o);
    std::fclose(o);
    return 0;
}

// The largest error of the fisheye factor over every float32 in [lo, hi], in units of the last place of the exact atan(t)/t.
double atan_range(float lo, float hi) {
    uint32_t a, b;
    std::memcpy(&a, &lo, 4);
    std::memcpy(&b, &hi, 4);
    double worst = 0;
    for (uint32_t bits = a; bits <= b; ++bits) {
        float t;
        std::memcpy(&t, &bits, 4);
        const double exact = std::atan((double)t) / (double)t;
        const double ulp = std::ldexp(1.0, std::ilogb(exact) - 23);
        const double err = std::fabs((double)r2f::lens::projection_factor(R2F_PROJ_FISHEYE, t) - exact) / ulp;
        if (err > worst) worst = err;
    }
    return worst;
}

int atan_mode() {
    const double low = atan_range(std::ldexp(1.f, -13), 1.f);
    const double high = atan_range(std::nextafterf(1.f, 2.f), 64.f);
    std::printf("atan max ulp: low %.4f high %.4f\n", low, high);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "fuzz")) return fuzz(std::strtoull(argv[2], nullptr, 10), std::atoi(argv[3]));
    if (argc == 4 && !std::strcmp(argv[1], "render")) return render(argv[2], argv[3]);
    if (argc == 2 && !std::strcmp(argv[1], "atan")) return atan_mode();
    std::fprintf(stderr, "usage: lens_projection_check fuzz SEED CASES | lens_projection_check render IN OUT | lens_projection_check atan\n");
    return 64;
}
