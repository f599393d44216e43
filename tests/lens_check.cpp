// lens_check.cpp -- the host half of the lens correction on the CPU, with its own main (tests/test_lens_host.py builds it with
// g++ -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all -ffp-contract=off together with
// raw2film_amd/csrc/r2f_lens_plan.cpp, r2f_plan.cpp (the LANCZOS4 weights) and r2f_lens_math.h -- the text the device kernel compiles).
//   lens_check fuzz SEED CASES   the planner over shapes 1 x 1 ... 16384^2, all models, hostile coefficients and auto scale, each
//                                accepted plan checked against its contract; the coordinate / inside decision with NaN, +-inf,
//                                +-1e30; whole pixels through hostile constants with a fetch that refuses an index outside the frame
//   lens_check render IN OUT     IN: int32 {H, W, channels, row0, col0, rows, cols}, an r2f_lens_profile, H*W*channels floats;
//                                OUT: the r2f_lens_params, then rows*cols*3 floats (interleaved) of the corrected window
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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
    void operator()(int y, int x, float (&v)[3]) const {
        if (y < 0 || y >= H || x < 0 || x >= W) {  // (never reached if the decision holds: counted, nothing indexed)
            ++bad;
            v[0] = v[1] = v[2] = 0.f;
            return;
        }
        const float* p = data + ((size_t)y * W + x) * C;
        v[0] = p[0], v[1] = p[1], v[2] = p[2];
    }
};

double factor(const r2f_lens_profile& p, double r2) {
    if (p.model == R2F_LENS_POLY3) return (1.0 - p.coef[0]) + p.coef[0] * r2;
    if (p.model == R2F_LENS_POLY5) return 1.0 + r2 * (p.coef[0] + p.coef[1] * r2);
    if (p.model == R2F_LENS_PTLENS) {
        const double r = std::sqrt(r2);
        return (1.0 - p.coef[0] - p.coef[1] - p.coef[2]) + r * (p.coef[2] + r * (p.coef[1] + r * p.coef[0]));
    }
    return 1.0;
}

// How far (pixels) the worst of the eight probes lands outside [0, W - 1] x [0, H - 1] at `scale` (<= 0: all inside).
double probes_outside(const r2f_lens_profile& p, int H, int W, double scale) {
    double norm = p.norm_radius_px;
    if (norm == 0) norm = std::hypot((double)(W - 1), (double)(H - 1)) / 2.0;
    if (norm == 0) norm = 1.0;
    const double cx = (W - 1) / 2.0 + p.center[0] * norm, cy = (H - 1) / 2.0 + p.center[1] * norm;
    const double xs[3] = {0.0, (W - 1) / 2.0, (double)(W - 1)}, ys[3] = {0.0, (H - 1) / 2.0, (double)(H - 1)};
    double worst = -INFINITY;
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) {
            if (i == 1 && j == 1) continue;
            const double dx = xs[i] - cx, dy = ys[j] - cy, q = 1.0 / (norm * scale), u = dx * q, v = dy * q;
            const double g = factor(p, u * u + v * v) / scale;
            const double sx = cx + dx * g, sy = cy + dy * g;
            worst = std::fmax(worst, std::fmax(std::fmax(-sx, sx - (W - 1)), std::fmax(-sy, sy - (H - 1))));
        }
    return worst;
}

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
    CHECK(r2f_lens_phase_table(nullptr) == R2F_EINVAL, "null table");
    for (int p = 0; p < 32; ++p) {
        float s = 0.f;
        for (int k = 0; k < 8; ++k) s += table[8 * p + k];
        CHECK(std::fabs(s - 1.f) < 1e-5f, "phase %d sums to %g", p, (double)s);
    }
    std::vector<float> small(16 * 16 * 3, 1.f);
    long long accepted = 0, autos = 0;
    for (int n = 0; n < cases; ++n) {
        r2f_lens_profile pr{};
        const bool wild = pick(3) == 0;  // a third of the cases: hostile numbers anywhere
        pr.model = wild && pick(8) == 0 ? pick(9) - 3 : pick(4);
        pr.n_coef = wild && pick(8) == 0 ? pick(5) : (pr.model >= 0 && pr.model <= 3 ? pr.model : 0);
        for (int i = 0; i < 3; ++i) pr.coef[i] = wild && pick(3) == 0 ? hostile[pick(nh)] : uni(-0.2, 0.2);
        pr.has_vignetting = pick(2);
        for (int i = 0; i < 3; ++i) pr.vignetting[i] = wild && pick(4) == 0 ? hostile[pick(nh)] : uni(-0.5, 0.5);
        for (int i = 0; i < 2; ++i) pr.center[i] = wild && pick(4) == 0 ? hostile[pick(nh)] : uni(-0.05, 0.05);
        pr.auto_scale = pick(3) == 0;
        pr.scale = wild && pick(3) == 0 ? hostile[pick(nh)] : uni(0.2, 3.0);
        pr.norm_radius_px = pick(3) ? 0.0 : (wild && pick(2) ? hostile[pick(nh)] : uni(0.5, 20000.0));
        const int H = wild && pick(10) == 0 ? pick(3) - 1 : sides[pick(ns)], W = wild && pick(10) == 0 ? pick(3) - 1 : sides[pick(ns)];
        r2f_lens_params out;
        std::memset(&out, 0x5A, sizeof out);
        const int rc = r2f_lens_plan(&pr, H, W, &out);
        CHECK(rc == R2F_OK || rc == R2F_EINVAL, "rc %d", rc);
        // what LensProfile refuses, the planner refuses
        bool bad = pr.model < 0 || pr.model > 3 || H < 1 || W < 1;
        if (!bad) bad = pr.n_coef != pr.model;
        if (!bad)
            for (int i = 0; i < pr.n_coef; ++i) bad = bad || !std::isfinite(pr.coef[i]);
        if (!bad && pr.has_vignetting)
            for (int i = 0; i < 3; ++i) bad = bad || !std::isfinite(pr.vignetting[i]);
        bad = bad || !std::isfinite(pr.center[0]) || !std::isfinite(pr.center[1]);
        bad = bad || !std::isfinite(pr.norm_radius_px) || pr.norm_radius_px < 0;
        bad = bad || (!pr.auto_scale && !(std::isfinite(pr.scale) && pr.scale > 0));
        if (bad) CHECK(rc == R2F_EINVAL, "a bad profile was accepted (model %d, n_coef %d, %d x %d)", pr.model, pr.n_coef, H, W);
        if (rc != R2F_OK) continue;
        ++accepted;
        const float fl[] = {out.cx, out.cy, out.q, out.inv_scale, out.c0, out.k[0], out.k[1], out.k[2], out.qv, out.v[0], out.v[1], out.v[2]};
        for (float v : fl) CHECK(std::isfinite(v), "a constant is not finite");
        CHECK(out.model == pr.model && out.vignetting == (pr.has_vignetting ? 1 : 0), "model / vignetting flag");
        CHECK(std::isfinite(out.scale) && out.scale > 0, "scale %g", out.scale);
        if (!pr.auto_scale) CHECK(out.scale == pr.scale, "a given scale is kept");
        if (pr.auto_scale && !(H == 1 && W == 1)) {
            ++autos;
            // every probe inside (to the resolution of a double at frame coordinates), and one outside just below
            const double tol = 1e-9 * std::fmax(1.0, std::fmax((double)H, (double)W));
            const double at = probes_outside(pr, H, W, out.scale), below = probes_outside(pr, H, W, out.scale * (1 - 1e-6));
            CHECK(at <= tol, "auto scale %.17g leaves a probe %g px outside (%d x %d, model %d)", out.scale, at, H, W, pr.model);
            CHECK(below > 0 || at == -INFINITY, "auto scale %.17g is not the smallest: still inside at scale (1 - 1e-6) (%g)", out.scale, below);
        }
        // a few whole pixels of a 16 x 16 frame through these constants (whatever frame they were made for): nothing outside it is fetched
        Frame fr{small.data(), 16, 16, 3};
        for (int t = 0; t < 8; ++t) {
            float v[3];
            r2f::lens::correct_pixel(out, fr, 16, 16, table, pick(40) - 12, pick(40) - 12, v);
        }
        CHECK(fr.bad == 0, "a tap outside the frame was fetched");
    }
    // the coordinate / inside decision with hostile coordinates
    const float coords[] = {NAN, INFINITY, -INFINITY, 1e30f, -1e30f, 3.4e38f, -3.4e38f, 2147483648.f, -2147483648.f, 67108864.f, -5.f, -4.02f,
                            -4.f, -3.99f, 0.f, -0.f, 0.49f, 15.99f, 18.98f, 19.f, 1e-40f};
    for (float s : coords)
        for (int n : {1, 2, 16, 16384}) {
            int i = 12345, ph = 12345;
            const bool in = r2f::lens::split_phase(s, n, i, ph);
            if (in)
                CHECK(i >= -4 && i <= n + 2 && ph >= 0 && ph < 32 && std::fabs((double)s - (i + ph / 32.0)) <= 1.0 / 64 + 1e-3, "split_phase(%g, %d) -> %d + %d/32",
                      (double)s, n, i, ph);
            else
                CHECK(!(s >= -3.9f && s <= (float)n + 2.9f), "split_phase(%g, %d) refused a coordinate within the tap reach", (double)s, n);
        }
    // ... and whole pixels whose map produces them
    r2f_lens_params hp{};
    hp.model = R2F_LENS_PTLENS;
    Frame fr{small.data(), 16, 16, 3};
    for (float a : {NAN, INFINITY, -INFINITY, 1e30f, -1e30f, 0.f})
        for (float b : {NAN, INFINITY, 1e30f, -1e30f, 1.f}) {
            hp.cx = a == 0.f ? 7.5f : a, hp.cy = 7.5f, hp.q = b, hp.inv_scale = b, hp.c0 = a, hp.k[0] = b, hp.k[1] = a, hp.k[2] = b;
            hp.vignetting = 1, hp.qv = b, hp.v[0] = a, hp.v[1] = b, hp.v[2] = a;
            for (int y = -2; y < 18; y += 3)
                for (int x = -2; x < 18; x += 3) {
                    float v[3];
                    r2f::lens::correct_pixel(hp, fr, 16, 16, table, x, y, v);
                }
        }
    CHECK(fr.bad == 0, "a tap outside the frame was fetched (hostile constants)");
    if (g_failed) return 1;
    std::printf("%d cases ok (%lld accepted, %lld auto scales)\n", cases, accepted, autos);
    return 0;
}

int render(const char* in_path, const char* out_path) {
    FILE* f = std::fopen(in_path, "rb");
    if (!f) return 2;
    int32_t head[7];
    r2f_lens_profile pr;
    if (std::fread(head, sizeof head, 1, f) != 1 || std::fread(&pr, sizeof pr, 1, f) != 1) return 2;
    const int H = head[0], W = head[1], C = head[2], r0 = head[3], c0 = head[4], nr = head[5], nc = head[6];
    if (H < 1 || W < 1 || (C != 3 && C != 4) || nr < 1 || nc < 1 || H > 4096 || W > 4096 || nr > 4096 || nc > 4096) return 2;
    std::vector<float> img((size_t)H * W * C);
    if (std::fread(img.data(), sizeof(float), img.size(), f) != img.size()) return 2;
    std::fclose(f);
    r2f_lens_params p;
    if (r2f_lens_plan(&pr, H, W, &p) != R2F_OK) return 3;
    float table[256];
    r2f_lens_phase_table(table);
    const Frame fr{img.data(), H, W, C};
    std::vector<float> out((size_t)nr * nc * 3);
    for (int y = 0; y < nr; ++y)
        for (int x = 0; x < nc; ++x) {
            float v[3];
            r2f::lens::correct_pixel(p, fr, H, W, table, c0 + x, r0 + y, v);
            std::memcpy(&out[((size_t)y * nc + x) * 3], v, sizeof v);
        }
    if (fr.bad) return 4;
    FILE* o = std::fopen(out_path, "wb");
    if (!o) return 2;
    std::fwrite(&p, sizeof p, 1, o);
    std::fwrite(out.data(), sizeof(float), out.size(), o);
    std::fclose(o);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "fuzz")) return fuzz(std::strtoull(argv[2], nullptr, 10), std::atoi(argv[3]));
    if (argc == 4 && !std::strcmp(argv[1], "render")) return render(argv[2], argv[3]);
    std::fprintf(stderr, "usage: lens_check fuzz SEED CASES | lens_check render IN OUT\n");
    return 64;
}
