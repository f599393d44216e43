// r2f_mosaic_math.h -- what the per-pixel arithmetic of the two demosaics has in common (r2f_demosaic_math.h the Bayer pattern's,
// r2f_xtrans_math.h the X-Trans one's): the host/device macro set, the integer helpers, step C (colour matrix, clip), the row-range
// contract and the index map of the oriented entry points (namespace orient).  Like the two pattern headers this is text that hipcc
// compiles for the device and g++ -ffp-contract=off for the CPU programs (tests/demosaic_check.cpp, tests/xtrans_check.cpp,
// tests/orient_check.cpp).  No HIP types, no includes beyond <math.h> and <stdint.h>.
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

// Blend (include/r2f.h, LibRaw's highlight mode 2): a pixel with a channel above `clip` keeps its lightness and takes the chroma
// magnitude of its clipped version; every other pixel is left alone.  Between the interpolation and step C, on the three integers in
// [0, 65535]; clip in [1, 65535].  Each line is one fp32 operation, in the header's order.  |lab| < 2^19, the squares' sum < 2^41,
// sum0 > 0 where it divides and |acc / 3| < 2^20: no NaN, and the truncation stays inside int.
R2F_HD void blend_pixel(int (&v)[3], int clip) {
    R2F_NO_CONTRACT
    if (v[0] <= clip && v[1] <= clip && v[2] <= clip) return;
    constexpr float kSqrt3 = 0x1.bb67aep+0f, kHalfSqrt3 = 0x1.bb67aep-1f;
    const float fclip = (float)clip;
    float lab[2][3];
    float sum[2];
    R2F_UNROLL
    for (int i = 0; i < 2; ++i) {
        float cam[3];
        R2F_UNROLL
        for (int c = 0; c < 3; ++c) {
            const float f = (float)v[c];
            cam[c] = i && f > fclip ? fclip : f;
        }
        // T = {{1, 1, 1}, {sqrt3, -sqrt3, 0}, {-1, -1, 2}}: a product with 1, -1 or 0 is exact, and x + 0 = x (no -0 arises here
        // that a later step could tell from +0), so only the four roundings that can differ from the plain sum are spelled out
        lab[i][0] = (cam[0] + cam[1]) + cam[2];
        const float a = kSqrt3 * cam[0], b = -kSqrt3 * cam[1];
        lab[i][1] = a + b;
        const float t = 2.f * cam[2];
        lab[i][2] = (-cam[0] + -cam[1]) + t;
        const float s1 = lab[i][1] * lab[i][1], s2 = lab[i][2] * lab[i][2];
        sum[i] = s1 + s2;
    }
    float chratio = 1.f;
    if (sum[0] != 0.f) {
        const float q = sum[1] / sum[0];
        chratio = sqrtf(q);
    }
    const float l0 = lab[0][0], l1 = lab[0][1] * chratio, l2 = lab[0][2] * chratio;
    // I = {{1, h, -1/2}, {1, -h, -1/2}, {1, 0, 1}}, h = sqrt3 / 2
    const float h1 = kHalfSqrt3 * l1, n1 = -kHalfSqrt3 * l1, m2 = -0.5f * l2;
    const float o0 = (l0 + h1) + m2, o1 = (l0 + n1) + m2, o2 = l0 + l2;
    v[0] = clip16((int)(o0 / 3.0f)), v[1] = clip16((int)(o1 / 3.0f)), v[2] = clip16((int)(o2 / 3.0f));
}

// The mosaic rows [lo, hi) that rows [fy0, fy1) of the demosaiced frame D read (the row-range contract of include/r2f.h): full size
// `reach` rows either side, clipped to the H rows of the mosaic; the reduced form (reduction = 2 or 3, else 0) the rows of its cells.
R2F_HD void source_rows(int fy0, int fy1, int H, int reach, int reduction, int& lo, int& hi) {
    lo = reduction ? reduction * fy0 : (fy0 - reach > 0 ? fy0 - reach : 0);
    hi = reduction ? reduction * fy1 : (fy1 + reach < H ? fy1 + reach : H);
}

}  // namespace mosaic

// The sensor's orientation (include/r2f.h, r2f_demosaic_oriented_u16): LibRaw's sizes.flip bits.  D is the demosaiced frame,
// out_h x out_w; O the oriented one, rows(o) x cols(o), with O[r, c] = D[to_frame(r, c)].  One text for the entry points' checks, the
// kernels and tests/orient_check.cpp.
namespace orient {

constexpr int kCols = 1, kRows = 2, kSwap = 4;  // mirror the columns, mirror the rows, swap the axes

R2F_HD bool valid(int o) { return o >= 0 && o <= 7; }
R2F_HD int rows(int o, int out_h, int out_w) { return o & kSwap ? out_w : out_h; }
R2F_HD int cols(int o, int out_h, int out_w) { return o & kSwap ? out_h : out_w; }

// the pixel of D that O[r, c] holds
R2F_HD void to_frame(int o, int out_h, int out_w, int r, int c, int& dy, int& dx) {
    const int a = o & kSwap ? c : r, b = o & kSwap ? r : c;
    dy = o & kRows ? out_h - 1 - a : a;
    dx = o & kCols ? out_w - 1 - b : b;
}
// ... and its inverse: where D[dy, dx] goes (both mirrors are involutions, the swap comes last)
R2F_HD void from_frame(int o, int out_h, int out_w, int dy, int dx, int& r, int& c) {
    const int a = o & kRows ? out_h - 1 - dy : dy, b = o & kCols ? out_w - 1 - dx : dx;
    r = o & kSwap ? b : a;
    c = o & kSwap ? a : b;
}

struct Rect {
    int y0, y1, x0, x1;  // rows [y0, y1) and columns [x0, x1) of D
};
// The pixels of D that rows [y0, y1) of O hold, 0 <= y0 <= y1 <= rows(o): whole rows of D, or with the axes swapped whole columns.
R2F_HD Rect rect_of(int o, int out_h, int out_w, int y0, int y1) {
    if (o & kSwap) return o & kCols ? Rect{0, out_h, out_w - y1, out_w - y0} : Rect{0, out_h, y0, y1};
    return o & kRows ? Rect{out_h - y1, out_h - y0, 0, out_w} : Rect{y0, y1, 0, out_w};
}
// The mosaic rows [lo, hi) a call for that rectangle reads: those of its rows of D; with the axes swapped every row of the mosaic.
R2F_HD void source_rows(int o, const Rect& d, int H, int reach, int reduction, int& lo, int& hi) {
    if (o & kSwap)
        lo = 0, hi = H;
    else
        mosaic::source_rows(d.y0, d.y1, H, reach, reduction, lo, hi);
}

}  // namespace orient
}  // namespace r2f
