// r2f_repair_math.h -- the hot-pixel repair of a mosaic (include/r2f.h: r2f_mosaic_repair): the neighbour rule N, step T and the hot
// test H.  Like r2f_mosaic_math.h, whose macros it takes, this is text that hipcc compiles for the device (r2f_mosaic_repair.hip),
// for the host planner (r2f_repair_plan.cpp) and g++ for the CPU program (tests/repair_check.cpp).  Integers only.
#pragma once

#include "r2f_mosaic_math.h"

namespace r2f {
namespace repair {

constexpr int kPeriod = 6;            // the tables' period: a 2 x 2 table widened to 6 x 6 keeps every site's level and neighbours
constexpr int kPhases = kPeriod * kPeriod;
constexpr int kReach = 2;             // no neighbour lies further than this from its centre, along rows or columns
constexpr int kMinSide = 6;

R2F_HD int phase_of(int y, int x) { return (y % kPeriod) * kPeriod + x % kPeriod; }

// N, Bayer: quadrant d = up, right, down, left -> the same site of the quad two samples on
R2F_HD int bayer_dy(int d) { return d == 0 ? -2 : d == 2 ? 2 : 0; }
R2F_HD int bayer_dx(int d) { return d == 1 ? 2 : d == 3 ? -2 : 0; }

// N, X-Trans: candidate i = 0 .. 5 of quadrant d: ring r = 1 (i < 2) then r = 2, the lateral offset a in the order 0, 1, -1, 2 over
// -r < a <= r; (dy, dx) = (-r, a), (a, r), (r, -a), (-a, -r) for up, right, down, left
R2F_HD void candidate(int d, int i, int& dy, int& dx) {
    const int r = i < 2 ? 1 : 2;
    const int j = i < 2 ? i : i - 2;
    const int a = j == 0 ? 0 : j == 1 ? 1 : j == 2 ? -1 : 2;
    dy = d == 0 ? -r : d == 1 ? a : d == 2 ? r : -a;
    dx = d == 0 ? a : d == 1 ? r : d == 2 ? -a : -r;
}
// the neighbour of phase (py, px) in quadrant d of a 6 x 6 pattern taken cyclically: the first candidate of the centre's colour;
// false when ring 2 holds none
R2F_HD bool xtrans_neighbour(const int32_t* cfa, int py, int px, int d, int& dy, int& dx) {
    const int32_t c = cfa[py * kPeriod + px];
    for (int i = 0; i < 6; ++i) {
        candidate(d, i, dy, dx);
        if (cfa[((py + dy + kPeriod) % kPeriod) * kPeriod + (px + dx + kPeriod) % kPeriod] == c) return true;
    }
    return false;
}

// T
R2F_HD int t_of(int raw, int black) { return raw > black ? raw - black : 0; }
// H: a neighbour is below its centre (both products stay under 2^24)
R2F_HD bool below(int q, int t_centre, int t_neighbour) { return q * t_centre > 256 * t_neighbour; }
// H: the value of a centre whose four neighbours' t are tk, or -1 when it is not hot (the border rule is the caller's)
R2F_HD int hot_value(int t_centre, const int (&tk)[4], int black_centre, int threshold, int q, int min_neighbours) {
    if (t_centre <= threshold) return -1;
    int n = 0, m = 0;
    R2F_UNROLL
    for (int d = 0; d < 4; ++d)
        if (below(q, t_centre, tk[d])) {
            ++n;
            m = tk[d] > m ? tk[d] : m;
        }
    return n >= min_neighbours ? mosaic::clip16(m + black_centre) : -1;
}

// what the planner produces
R2F_HD bool numbers_ok(int threshold, int q, int min_neighbours) {
    return threshold >= 0 && threshold <= 65535 && q >= 1 && q <= 255 && (min_neighbours == 3 || min_neighbours == 4);
}
R2F_HD bool offset_ok(int dy, int dx) { return dy >= -kReach && dy <= kReach && dx >= -kReach && dx <= kReach && (dy || dx); }

// The output sample at (y, x), whose own value is `raw`, of an H x W frame whose samples `at(yy, xx)` yields; *replaced is incremented
// for a hot centre.  black: the params' table per phase; off(phase, d, dy, dx): the neighbour of quadrant d (the params' table, or
// the Bayer constants).
template <class At, class Off>
R2F_HD int repair_sample(const At& at, const Off& off, int raw, int H, int W, int y, int x, const int32_t* black, int threshold, int q,
                         int min_neighbours, int* replaced) {
    const int ph = phase_of(y, x);
    const int tc = t_of(raw, black[ph]);
    if (tc <= threshold) return raw;
    int tk[4];
    R2F_UNROLL
    for (int d = 0; d < 4; ++d) {
        int dy, dx;
        off(ph, d, dy, dx);
        const int yy = y + dy, xx = x + dx;
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) return raw;  // a sample with a neighbour outside the frame is never hot
        tk[d] = t_of(at(yy, xx), black[phase_of(yy, xx)]);
    }
    const int v = hot_value(tc, tk, black[ph], threshold, q, min_neighbours);
    if (v < 0) return raw;
    ++*replaced;
    return v;
}
struct BayerOffsets {
    R2F_HD void operator()(int, int d, int& dy, int& dx) const { dy = bayer_dy(d), dx = bayer_dx(d); }
};
struct TableOffsets {
    const int8_t (*table)[4][2];
    R2F_HD void operator()(int ph, int d, int& dy, int& dx) const { dy = table[ph][d][0], dx = table[ph][d][1]; }
};

}  // namespace repair
}  // namespace r2f
