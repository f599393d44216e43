// r2f_mosaic_math.h -- what the per-pixel arithmetic of the two demosaics has in common (r2f_demosaic_math.h the Bayer pattern's,
// r2f_xtrans_math.h the X-Trans one's): the host/device macro set, the integer helpers and step C (colour matrix, clip).  Like the
// two pattern headers this is text that hipcc compiles for the device and g++ -ffp-contract=off for the CPU programs
// (tests/demosaic_check.cpp, tests/xtrans_check.cpp).  No HIP types, no includes beyond <math.h> and <stdint.h>.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define R2F_HD __host__ __device__ __forceinline__
#else
#define R2F_HD inline
#endif
#if defined(__clang__)
#define R2F_NO_CONTRACT _Pragma("clang fp contract(off)")
#define R2F_UNROLL _Pragma("unroll")  // (a loop over a small register array: unrolled, its indices are constants)
#else
#define R2F_NO_CONTRACT  // (g++: the translation unit is compiled with -ffp-contract=off)
#define R2F_UNROLL _Pragma("GCC unroll 9")
#endif

namespace r2f {
namespace mosaic {

constexpr int kRed = 0, kGreen = 1, kBlue = 2;

R2F_HD int clip16(int v) { return v < 0 ? 0 : (v > 65535 ? 65535 : v); }
R2F_HD int iabs(int v) { return v < 0 ? -v : v; }
R2F_HD bool in_ring(int H, int W, int y, int x, int width) { return y < width || y >= H - width || x < width || x >= W - width; }

// C: the matrix and the clip, five fp32 operations per channel in this order.  |acc| <= 3 * 64 * 65535: the truncation stays inside
// int.
R2F_HD void colour(const float (&M)[9], const int (&rgb)[3], uint16_t (&out)[3]) {
    R2F_NO_CONTRACT
    const float r = (float)rgb[0], g = (float)rgb[1], b = (float)rgb[2];
    R2F_UNROLL
    for (int k = 0; k < 3; ++k) {
        float acc = r * M[3 * k];
        const float t1 = g * M[3 * k + 1];
        acc = acc + t1;
        const float t2 = b * M[3 * k + 2];
        acc = acc + t2;
        out[k] = (uint16_t)clip16((int)acc);
    }
}

}  // namespace mosaic
}  // namespace r2f
