// r2f_mosaic_plan.h -- what the two demosaic planners (r2f_demosaic_plan.cpp, r2f_xtrans_plan.cpp) ask of a profile's numbers, once:
// black levels, multipliers and the camera matrix, checked as doubles and stored as the params' types.  Host only, no HIP: hipcc
// compiles it into the library, g++ -fsanitize=address,undefined,float-cast-overflow into the tests' check programs.  Each function
// is false for a value out of range; the comparisons are written so that a NaN fails them, and nothing is converted before it has
// passed.
#pragma once

#include <cmath>
#include <cstdint>

namespace r2f {
namespace mosaic_plan {

// integers in [0, 65535]
template <int N>
inline bool black_levels(const double (&black)[N], int32_t (&out)[N]) {
    for (int i = 0; i < N; ++i) {
        const double b = black[i];
        if (!(b >= 0.0 && b <= 65535.0) || b != std::floor(b)) return false;
        out[i] = (int32_t)b;
    }
    return true;
}

// (0, 1024], as doubles and as the floats they round to
template <int N>
inline bool multipliers(const double (&mul)[N], float (&out)[N]) {
    for (int i = 0; i < N; ++i) {
        const double m = mul[i];
        if (!(m > 0.0 && m <= 1024.0)) return false;
        const float mf = (float)m;
        if (!(mf > 0.f && mf <= 1024.f)) return false;  // (a double below the smallest float rounds to 0)
        out[i] = mf;
    }
    return true;
}

// |entries| <= 64
inline bool matrix(const double (&matrix)[9], float (&out)[9]) {
    for (int i = 0; i < 9; ++i) {
        if (!(std::fabs(matrix[i]) <= 64.0)) return false;
        out[i] = (float)matrix[i];
    }
    return true;
}

}  // namespace mosaic_plan
}  // namespace r2f
