// r2f_median_math.h -- the per-pixel arithmetic of step M (include/r2f.h: the median filter of the colour differences, LibRaw's
// med_passes), as text the device kernels (r2f_mosaic_stage.h) and a CPU program (tests/median_check.cpp) both compile: the median
// of nine integers, and one pixel of one pass.  Integer arithmetic only.  No HIP types.
#pragma once

#include "r2f_mosaic_math.h"

namespace r2f {
namespace median {

// (a, b) -> (min, max)
R2F_HD void exchange(int& a, int& b) {
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo, b = hi;
}

// The median of nine integers by the 19-exchange selection network dcraw's median_filter walks (each exchange is a min and a max:
// no branch, no indexed register).  That the network selects the median is proved on the 512 zero-one inputs (tests/median_check.cpp).
R2F_HD int median9(int (&v)[9]) {
    exchange(v[1], v[2]), exchange(v[4], v[5]), exchange(v[7], v[8]);
    exchange(v[0], v[1]), exchange(v[3], v[4]), exchange(v[6], v[7]);
    exchange(v[1], v[2]), exchange(v[4], v[5]), exchange(v[7], v[8]);
    exchange(v[0], v[3]), exchange(v[5], v[8]), exchange(v[4], v[7]);
    exchange(v[3], v[6]), exchange(v[1], v[4]), exchange(v[2], v[5]);
    exchange(v[4], v[7]), exchange(v[4], v[2]), exchange(v[6], v[4]);
    exchange(v[4], v[2]);
    return v[4];
}

// One pass at an interior pixel (y, x), for red and blue: the median of the nine differences C - G around it, plus its own green,
// clamped to 16 bits.  R(y, x), B(y, x) are the planes of the pass before, G(y, x) the green plane (read once for both).
// |C - G| <= 65535.
template <typename RFn, typename BFn, typename GFn>
R2F_HD void pass_pixel(const RFn& R, const BFn& B, const GFn& G, int y, int x, int& r, int& b) {
    int dr[9], db[9];
    R2F_UNROLL
    for (int j = 0; j < 3; ++j) {
        R2F_UNROLL
        for (int i = 0; i < 3; ++i) {
            const int g = G(y + j - 1, x + i - 1);
            dr[3 * j + i] = R(y + j - 1, x + i - 1) - g, db[3 * j + i] = B(y + j - 1, x + i - 1) - g;
        }
    }
    const int g0 = G(y, x);
    r = mosaic::clip16(median9(dr) + g0), b = mosaic::clip16(median9(db) + g0);
}

}  // namespace median
}  // namespace r2f
