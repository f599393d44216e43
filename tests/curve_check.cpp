// curve_check.cpp -- the planner's `near` claim (raw2film_amd/csrc/r2f_plan.cpp, curve_cells) against the look-up the device makes with it
// (r2f_device.h: curve_eval_at and its batch forms).  Built by tests/test_curve_host.py with `g++ -fsanitize=address,undefined
// -fno-sanitize-recover=all` from the translation unit the library links, and run as a child process.  Test infrastructure: nothing in
// the product links this file.
//
//   curve_check search <seed> <cases>
//       Axes of m abscissae from {2, 3, 4, 5, 17, 64, 255, 1024, 4096} on [origin, origin + span]: a uniform grid whose inner breakpoints
//       are moved by jitter x U(-1, 1) of a step, rounded to float32 and sorted (jitter >= 0.5 reorders breakpoints; a large origin or a
//       small span makes float32 repeat abscissae).  A repeated abscissa must give near == 0.  Whenever near == 1: for every breakpoint,
//       its three float neighbours on each side and 20 000 random x in range, the device's guess plus its ONE corrective step must land in
//       upper_bound(xp, x) - 1, the cell np.interp uses -- a `near` that claims too much is a silently wrong cell, nothing walks any more.
//       Prints "<cases> cases, <n> near axes, <points> points, <v> violations"; exit status 1 if v > 0.
//   curve_check flags <tables> [<cells out>]
//       <tables>: int32 count, then per table int32 m and 4 m float32.  Prints per table "near x0 x1 inv_step" (floats as their bit
//       patterns); with a second argument the cells of every table are written there as raw float32, table after table.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../raw2film_amd/csrc/r2f_plan.h"

using namespace r2f::plan;

static uint64_t g_state = 1;
static uint32_t rnd() {  // xorshift64*
    g_state ^= g_state >> 12, g_state ^= g_state << 25, g_state ^= g_state >> 27;
    return (uint32_t)((g_state * 2685821237ULL) >> 32);
}
static double runit() { return (double)(rnd() >> 8) / 16777216.0; }  // [0, 1)
template <class T>
static T pick(std::initializer_list<T> v) { return *(v.begin() + rnd() % v.size()); }

static uint32_t bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// curve_eval_at's choice of the cell on a `near` table: the guess, clamped as an integer, and one corrective step
static int device_cell(const CurveCells& cc, float x) {
    const int last = cc.m - 2;
    const int raw = (int)((x - cc.x0) * cc.inv_step);
    const int i = raw < 0 ? 0 : (raw > last ? last : raw);
    const float* c = &cc.cells[(size_t)i * 4];
    const int adj = (x < c[0] && i > 0) ? -1 : ((x >= c[1] && i < last) ? 1 : 0);
    return i + adj;
}

static long long g_points = 0, g_violations = 0;

static void check_point(const CurveCells& cc, const std::vector<float>& xp, float x, int jitter_pm, double origin, double span) {
    const int last = cc.m - 2;
    int want = (int)(std::upper_bound(xp.begin(), xp.end(), x) - xp.begin()) - 1;
    want = want < 0 ? 0 : (want > last ? last : want);
    const int got = device_cell(cc, x);
    ++g_points;
    if (got != want) {
        if (g_violations < 20)
            fprintf(stderr, "curve_check: m %d jitter %.2f origin %g span %g: x = %.9g lands in cell %d, np.interp uses %d\n", cc.m,
                    jitter_pm / 100.0, origin, span, (double)x, got, want);
        ++g_violations;
    }
}

static int search(uint64_t seed, int cases) {
    g_state = seed * 0x9E3779B97F4A7C15ULL + 1;
    for (int i = 0; i < 16; ++i) rnd();
    int near_axes = 0;
    for (int n = 0; n < cases; ++n) {
        const int m = pick({2, 3, 4, 5, 17, 64, 255, 1024, 4096});
        const int jitter_pm = pick({20, 45, 70, 100, 150, 300});  // in hundredths of a step
        const double origin = pick({-4.0, 0.0, 1000.0, -1e-3, 3e5}), span = pick({5.5, 4.0, 1e-3, 1e4, 0.37});
        const double jitter = jitter_pm / 100.0, step = span / (m - 1);
        std::vector<float> lut((size_t)4 * m);
        for (int k = 0; k < m; ++k) {
            double x = origin + span * k / (m - 1);
            if (k > 0 && k + 1 < m) x += jitter * (2.0 * runit() - 1.0) * step;
            lut[k] = (float)x;
        }
        lut[m - 1] = (float)(origin + span);
        std::sort(lut.begin(), lut.begin() + m);
        for (int k = m; k < 4 * m; ++k) lut[k] = (float)(4.0 * runit());
        CurveCells cc;
        if (curve_cells(lut.data(), m, &cc) != 0) {
            fprintf(stderr, "curve_check: a sorted axis was refused (m %d)\n", m);
            return 1;
        }
        if (cc.near != 0 && cc.near != 1) {
            fprintf(stderr, "curve_check: near = %d\n", cc.near);
            return 1;
        }
        const std::vector<float> xp(lut.begin(), lut.begin() + m);
        bool repeated = false;
        for (int k = 0; k + 1 < m; ++k) repeated |= xp[k] == xp[k + 1];
        // (m = 2 has one cell and no guess to get wrong: its flag decides nothing)
        if (repeated && m >= 3 && cc.near) {
            fprintf(stderr, "curve_check: m %d origin %g span %g: repeated abscissae and near = 1\n", m, origin, span);
            ++g_violations;
        }
        if (!cc.near) continue;
        ++near_axes;
        for (int k = 0; k < m; ++k) {
            check_point(cc, xp, xp[k], jitter_pm, origin, span);
            float up = xp[k], down = xp[k];
            for (int s = 0; s < 3; ++s) {
                up = std::nextafterf(up, INFINITY), down = std::nextafterf(down, -INFINITY);
                check_point(cc, xp, up, jitter_pm, origin, span);
                check_point(cc, xp, down, jitter_pm, origin, span);
            }
        }
        for (int s = 0; s < 20000; ++s) {
            float x = (float)((double)xp[0] + ((double)xp[m - 1] - (double)xp[0]) * runit());
            x = std::min(std::max(x, xp[0]), xp[m - 1]);
            check_point(cc, xp, x, jitter_pm, origin, span);
        }
    }
    printf("%d cases, %d near axes, %lld points, %lld violations\n", cases, near_axes, g_points, g_violations);
    return g_violations ? 1 : 0;
}

static int flags(const char* path, const char* cells_path) {
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "curve_check: cannot open %s\n", path);
        return 2;
    }
    FILE* out = cells_path ? fopen(cells_path, "wb") : nullptr;
    if (cells_path && !out) {
        fprintf(stderr, "curve_check: cannot write %s\n", cells_path);
        fclose(f);
        return 2;
    }
    int rc = 0;
    int32_t count = 0;
    if (fread(&count, 4, 1, f) != 1 || count < 0) rc = 2;
    for (int32_t t = 0; t < count && !rc; ++t) {
        int32_t m = 0;
        if (fread(&m, 4, 1, f) != 1 || m < 2 || m > (1 << 20)) {
            rc = 2;
            break;
        }
        std::vector<float> lut((size_t)4 * m);
        if (fread(lut.data(), 4, lut.size(), f) != lut.size()) {
            rc = 2;
            break;
        }
        CurveCells cc;
        if (curve_cells(lut.data(), m, &cc) != 0) {
            printf("refused\n");
            continue;
        }
        printf("%d %08x %08x %08x\n", cc.near, bits(cc.x0), bits(cc.x1), bits(cc.inv_step));
        if (out && fwrite(cc.cells.data(), 4, cc.cells.size(), out) != cc.cells.size()) rc = 2;
    }
    if (rc) fprintf(stderr, "curve_check: %s is not a table file\n", path);
    fclose(f);
    if (out) fclose(out);
    return rc;
}

int main(int argc, char** argv) {
    if (argc >= 4 && !strcmp(argv[1], "search")) return search(strtoull(argv[2], nullptr, 10), atoi(argv[3]));
    if (argc >= 3 && !strcmp(argv[1], "flags")) return flags(argv[2], argc >= 4 ? argv[3] : nullptr);
    fprintf(stderr, "usage: curve_check search <seed> <cases> | curve_check flags <tables> [<cells out>]\n");
    return 2;
}
