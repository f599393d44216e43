// xtrans_check.cpp -- the X-Trans demosaic's host half as a stand-alone program (tests/test_xtrans_host.py builds it with
// g++ -fsanitize=address,undefined,float-cast-overflow -ffp-contract=off against raw2film_amd/csrc/r2f_xtrans_plan.cpp):
//   xtrans_check fuzz SEED N      N random profiles through r2f_xtrans_plan: what it accepts is admissible by a search of the
//                                 pattern written here, keeps every trunc of the definition inside int (checked on the extreme
//                                 samples) and renders without an index outside the frame; what it must refuse it refuses
//   xtrans_check render JOB OUT   JOB: int32 H, W, reduced; r2f_xtrans_profile; uint16 mosaic[H * W].  OUT: r2f_xtrans_params;
//                                 uint16 (out_h, out_w, 3), rendered with r2f_xtrans_math.h -- the text the device kernels compile
//   xtrans_check div              stdin: lines "n d"; stdout: floor_div(n, d, floor(2^32 / d) + 1) per line
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../raw2film_amd/csrc/r2f_xtrans_math.h"

using namespace r2f;

namespace {

struct Plane {
    const std::vector<int>* v;
    int W;
    int operator()(int y, int x) const { return v->at((size_t)y * W + x); }  // (at(): an index outside the frame aborts)
};

std::vector<uint16_t> render(const r2f_xtrans_params& p, const std::vector<uint16_t>& mosaic, int H, int W) {
    std::vector<int> s((size_t)H * W), d((size_t)H * W, 0);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) s[(size_t)y * W + x] = xtrans::scale_sample(p, mosaic[(size_t)y * W + x], xtrans::phase(y, x));
    const Plane S{&s, W}, D{&d, W};
    std::vector<uint16_t> out((size_t)p.out_h * p.out_w * 3);
    if (p.reduced) {
        for (int y = 0; y < p.out_h; ++y)
            for (int x = 0; x < p.out_w; ++x) {
                int q[9], rgb[3];
                for (int k = 0; k < 9; ++k) q[k] = S(3 * y + k / 3, 3 * x + k % 3);
                uint16_t o[3];
                xtrans::reduced_rgb(p, q, y, x, rgb);
                xtrans::colour(p, rgb, o);
                memcpy(&out[((size_t)y * p.out_w + x) * 3], o, sizeof o);
            }
        return out;
    }
    for (int y = 2; y < H - 2; ++y)
        for (int x = 2; x < W - 2; ++x) d[(size_t)y * W + x] = xtrans::diff_at(p, S, y, x);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            int rgb[3];
            uint16_t o[3];
            xtrans::pixel_rgb(p, S, D, H, W, y, x, rgb);
            xtrans::colour(p, rgb, o);
            memcpy(&out[((size_t)y * W + x) * 3], o, sizeof o);
        }
    return out;
}

// The admissibility rules of include/r2f.h by a search of the pattern, for a profile whose ids are all in {0, 1, 2}.
bool admissible(const int32_t (&pat)[36], bool reduced) {
    auto at = [&](int y, int x) { return pat[((y + 12) % 6) * 6 + (x + 12) % 6]; };
    int present[3] = {0, 0, 0};
    for (int i = 0; i < 36; ++i) ++present[pat[i]];
    if (!present[0] || !present[1] || !present[2]) return false;
    for (int y = 0; y < 6; ++y)
        for (int x = 0; x < 6; ++x) {
            const int c0 = at(y, x);
            if (c0 != 1) {
                if (at(y, x - 1) != 1 && at(y, x - 2) != 1) return false;
                if (at(y, x + 1) != 1 && at(y, x + 2) != 1) return false;
                if (at(y - 1, x) != 1 && at(y - 2, x) != 1) return false;
                if (at(y + 1, x) != 1 && at(y + 2, x) != 1) return false;
            }
            bool has[3] = {false, false, false};
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx)
                    if (dy || dx) has[at(y + dy, x + dx)] = true;
            for (int c = 0; c < 3; ++c)
                if (c != c0 && !has[c]) return false;
        }
    if (reduced)
        for (int cy = 0; cy < 6; cy += 3)
            for (int cx = 0; cx < 6; cx += 3) {
                bool has[3] = {false, false, false};
                for (int k = 0; k < 9; ++k) has[at(cy + k / 3, cx + k % 3)] = true;
                if (!has[0] || !has[1] || !has[2]) return false;
            }
    return true;
}

int fail(const char* what, long long i) {
    fprintf(stderr, "case %lld: %s\n", i, what);
    return 1;
}

int fuzz(unsigned seed, long long n) {
    std::mt19937_64 rng(seed);
    auto uni = [&](double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); };
    const double odd[] = {NAN, INFINITY, -INFINITY, -1.0, 65536.0, 0.5, 1e-60, 0.0, 1024.0000001, -64.0000001, 1e300};
    const char* base = "GBGGRGRGRBGBGBGGRGGRGGBGBGBRGRGRGGBG";
    long long accepted = 0, refused_patterns = 0;
    for (long long i = 0; i < n; ++i) {
        r2f_xtrans_profile pr{};
        const int sy = (int)(rng() % 6), sx = (int)(rng() % 6);
        for (int y = 0; y < 6; ++y)
            for (int x = 0; x < 6; ++x) {
                const char ch = base[((y + sy) % 6) * 6 + (x + sx) % 6];
                pr.pattern[y * 6 + x] = ch == 'R' ? 0 : (ch == 'G' ? 1 : 2);
            }
        pr.reduced = (int)(rng() % 2);
        for (int k = 0; k < 36; ++k) pr.black[k] = std::floor(uni(0, 65536));
        for (int k = 0; k < 3; ++k) pr.mul[k] = uni(1e-6, 1024.0);
        for (int k = 0; k < 9; ++k) pr.matrix[k] = uni(-64.0, 64.0);
        int H = 6 + (int)(rng() % 30), W = 6 + (int)(rng() % 30);
        bool bad = false, bad_id = false;
        switch (rng() % 10) {
            case 0: pr.black[rng() % 36] = odd[rng() % 6], bad = true; break;            // NaN, +-inf, negative, too large, fractional
            case 1: { const double v = odd[rng() % 11]; pr.mul[rng() % 3] = v; bad = bad || !(v > 0 && v <= 1024.0) || (float)v <= 0.f; break; }
            case 2: { const double v = odd[rng() % 11]; pr.matrix[rng() % 9] = v; bad = bad || !(std::fabs(v) <= 64.0); break; }
            case 3: if (rng() % 2) H = (int)(rng() % 6); else W = (int)(rng() % 6); bad = true; break;  // below 6
            case 4: pr.pattern[rng() % 36] = (rng() % 2) ? 3 : -1, bad = bad_id = true; break;
            case 5: case 6: {  // a few sites recoloured: admissible or not, by the search above
                const int m = 1 + (int)(rng() % 4);
                for (int k = 0; k < m; ++k) pr.pattern[rng() % 36] = (int)(rng() % 3);
                break;
            }
            case 7: for (int k = 0; k < 36; ++k) pr.pattern[k] = (int)(rng() % 3); break;  // a random array
            default: break;
        }
        if (!bad_id && !admissible(pr.pattern, pr.reduced != 0)) bad = true, ++refused_patterns;
        r2f_xtrans_params p;
        memset(&p, 0x5A, sizeof p);
        const int rc = r2f_xtrans_plan(&pr, H, W, &p);
        if (bad != (rc == R2F_EINVAL) || (rc != R2F_OK && rc != R2F_EINVAL)) return fail(bad ? "accepted what it must refuse" : "refused a valid profile", i);
        if (rc != R2F_OK) {
            const unsigned char* b = reinterpret_cast<const unsigned char*>(&p);
            for (size_t j = 0; j < sizeof p; ++j)
                if (b[j] != 0x5A) return fail("a refusal wrote to the params", i);
            continue;
        }
        ++accepted;
        if (p.out_h != (pr.reduced ? H / 3 : H) || p.out_w != (pr.reduced ? W / 3 : W)) return fail("output size", i);
        for (int ph = 0; ph < 36; ++ph)
            for (int slot = 0; slot < 2; ++slot) {
                const unsigned w = p.wsum[ph][slot];
                if (w > 12 || (p.taps[ph][slot] & ~0x1EFu) || (w > 1 && p.recip[ph][slot] != (uint32_t)(0x100000000ull / w) + 1u)) return fail("tables", i);
            }
        // the extremes of every float step stay inside int (float-cast-overflow aborts otherwise)
        for (int k = 0; k < 36; ++k) (void)xtrans::scale_sample(p, 65535, k), (void)xtrans::scale_sample(p, 0, k);
        const int ext[2] = {0, 65535};
        for (int m = 0; m < 8; ++m) {
            const int rgb[3] = {ext[m & 1], ext[(m >> 1) & 1], ext[(m >> 2) & 1]};
            uint16_t o[3];
            xtrans::colour(p, rgb, o);
        }
        // ... and a small frame renders without an index outside it
        std::vector<uint16_t> mosaic((size_t)H * W);
        for (auto& v : mosaic) v = (uint16_t)(rng() % 3 == 0 ? (rng() % 2) * 65535 : rng());
        if (render(p, mosaic, H, W).size() != (size_t)p.out_h * p.out_w * 3) return fail("render size", i);
    }
    if (r2f_xtrans_plan(nullptr, 12, 12, nullptr) != R2F_EINVAL) return fail("null arguments", -1);
    printf("%lld cases ok (%lld accepted, %lld patterns refused)\n", n, accepted, refused_patterns);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "fuzz")) return fuzz((unsigned)strtoul(argv[2], nullptr, 10), atoll(argv[3]));
    if (argc == 2 && !strcmp(argv[1], "div")) {
        long long nn, d;
        while (scanf("%lld %lld", &nn, &d) == 2) {
            if (d < 1 || d > 12 || nn < -12 * 65535 || nn > 12 * 65535) return 2;
            printf("%d\n", xtrans::floor_div((int)nn, (int)d, (uint32_t)(0x100000000ull / (uint64_t)d) + 1u));
        }
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "render")) {
        FILE* f = fopen(argv[2], "rb");
        if (!f) return 2;
        int32_t head[3];
        r2f_xtrans_profile pr;
        if (fread(head, sizeof head, 1, f) != 1 || fread(&pr, sizeof pr, 1, f) != 1) return 2;
        const int H = head[0], W = head[1];
        pr.reduced = head[2];
        if (H < 1 || W < 1 || H > 4096 || W > 4096) return 2;
        std::vector<uint16_t> mosaic((size_t)H * W);
        if (fread(mosaic.data(), 2, mosaic.size(), f) != mosaic.size()) return 2;
        fclose(f);
        r2f_xtrans_params p;
        if (r2f_xtrans_plan(&pr, H, W, &p) != R2F_OK) return 3;
        const std::vector<uint16_t> out = render(p, mosaic, H, W);
        FILE* o = fopen(argv[3], "wb");
        if (!o) return 2;
        fwrite(&p, sizeof p, 1, o);
        fwrite(out.data(), 2, out.size(), o);
        fclose(o);
        return 0;
    }
    fprintf(stderr, "usage: xtrans_check fuzz SEED N | render JOB OUT | div\n");
    return 2;
}
