// r2f_xtrans_math.h -- the per-pixel arithmetic of the X-Trans demosaic (include/r2f.h, r2f_demosaic_xtrans_u16), as text the
// device kernels (r2f_xtrans.hip) and a CPU program (tests/xtrans_check.cpp, g++ -ffp-contract=off) both compile: step A (black /
// scale), B0 (border ring), B1 (green), B2 (red and blue) and B' (reduced size); step C (colour matrix, clip) is r2f_mosaic_math.h's,
// shared with the Bayer pattern.  Everything is integer arithmetic except the one fp32 multiply of step A (and the five fp32
// operations per channel of step C), for which contraction is off.  Samples come through accessors at frame coordinates inside the
// frame: `S(y, x)` the scaled mosaic, `D(y, x)` the colour-difference plane S - G (diff_at), which the kernel keeps instead of G: B2
// reads nothing else of its neighbours.  The per-phase tables are the planner's (r2f_xtrans_params): no function here searches for
// a neighbour.
//
// The floor divisions, each exact for the numerators the definition allows:
//   by 2 (B1's rounding term floor((a + b) / 2)): a + b >= 2, a shift of a non-negative int.
//   by a + b in {2, 3, 4} (B1's est): the numerator is non-negative and at most 4 * 65535 + 2; floor_div below with the constant
//       multiplier of the span.
//   by wsum in 1 .. 12 (B2): the numerator n may be negative, |n| <= 12 * 65535 < 2^20.  floor_div moves it up by a multiple of the
//       divisor, u = n + d * 2^20 in (0, 13 * 2^20), so that floor(n / d) = floor(u / d) - 2^20 is an unsigned division, and takes
//       floor(u / d) as the high word of u * m with m = floor(2^32 / d) + 1.  Proof of range: m d = 2^32 + e with 0 < e <= d, so
//       u m / 2^32 = u / d + u e / (d 2^32); the second term is below 1 / d when u e < 2^32, which holds for u < 2^32 / 12
//       (3.5e8 > 13 * 2^20 = 1.4e7), and then the floor cannot pass the next multiple of 1 / d: the high word is floor(u / d).
//       d = 1 has no 32-bit m (2^32 + 1): the quotient is u itself.
//   by count in 1 .. 9 (B0, B'): sums of non-negative samples, the integer divide of the language (truncation is the floor).
#pragma once

#include "../../include/r2f.h"
#include "r2f_mosaic_math.h"

namespace r2f {

// The per-phase tables of `out` from its cfa (defined in r2f_xtrans_plan.cpp, host only): false for a pattern that is not admissible
// (with `reduced`, for the reduced size).  The planner fills its params with it and the entry point checks a caller's with it.
bool xtrans_tables(const uint8_t (&cfa)[36], bool reduced, r2f_xtrans_params* out);

namespace xtrans {

using namespace mosaic;  // the macro set, kRed / kGreen / kBlue, clip16, iabs, in_ring and step C (colour)

constexpr int kDivBias = 1 << 20;  // floor_div's: above 12 * 65535

R2F_HD int wrap6(int v) { return v < 0 ? v + 6 : (v >= 6 ? v - 6 : v); }  // v in [-6, 12)
R2F_HD int phase(int y, int x) { return (y % 6) * 6 + x % 6; }            // y, x >= 0
R2F_HD uint32_t mul_hi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}
// floor(n / d) for 1 <= d <= 12 and |n| <= 12 * 65535, m = floor(2^32 / d) + 1 (anything for d = 1): see the head of the file.
R2F_HD int floor_div(int n, int d, uint32_t m) {
    const uint32_t u = (uint32_t)(n + d * kDivBias);
    return (int)(d <= 1 ? u : mul_hi(u, m)) - kDivBias;
}
R2F_HD uint32_t recip_of_span(int span) { return span == 2 ? 0x80000001u : (span == 3 ? 0x55555556u : 0x40000001u); }  // 2, 3, 4

// A: one raw sample at phase ph.  |t * mul| <= 65535 * 1024: the truncation stays inside int.
R2F_HD int scale_sample(const r2f_xtrans_params& p, int raw, int ph) {
    R2F_NO_CONTRACT
    const int c = p.cfa[ph];
    const float m = c == 0 ? p.mul[0] : (c == 1 ? p.mul[1] : p.mul[2]);
    const float f = (float)(raw - p.black[ph]) * m;
    return clip16((int)f);
}

// B1: green at the non-green site (y, x) of phase ph, 2 <= y < H - 2, 2 <= x < W - 2.
template <typename SFn>
R2F_HD int green_est(const r2f_xtrans_params& p, const SFn& S, int y, int x, int ph) {
    const int ah = p.gap[ph][0], bh = p.gap[ph][1], av = p.gap[ph][2], bv = p.gap[ph][3];
    const int hm = S(y, x - ah), hp = S(y, x + bh), vm = S(y - av, x), vp = S(y + bv, x);
    const int span_h = ah + bh, span_v = av + bv;
    const int est_h = floor_div(bh * hm + ah * hp + (span_h >> 1), span_h, recip_of_span(span_h));
    const int est_v = floor_div(bv * vm + av * vp + (span_v >> 1), span_v, recip_of_span(span_v));
    return iabs(hm - hp) * span_v > iabs(vm - vp) * span_h ? est_v : est_h;
}

// S - G at (y, x), 2 <= y < H - 2, 2 <= x < W - 2: 0 at a green site.
template <typename SFn>
R2F_HD int diff_at(const r2f_xtrans_params& p, const SFn& S, int y, int x) {
    const int ph = phase(y, x);
    return p.cfa[ph] == kGreen ? 0 : S(y, x) - green_est(p, S, y, x, ph);
}

// B0: the three planes of a ring pixel, the means over the 3 x 3 neighbourhood clipped to the frame.
template <typename SFn>
R2F_HD void border_rgb(const r2f_xtrans_params& p, const SFn& S, int H, int W, int y, int x, int (&rgb)[3]) {
    int sum[3] = {0, 0, 0}, count[3] = {0, 0, 0};
    const int py = y % 6, px = x % 6;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int yy = y + dy, xx = x + dx;
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
            const int c = p.cfa[wrap6(py + dy) * 6 + wrap6(px + dx)], s = S(yy, xx);
            R2F_UNROLL
            for (int k = 0; k < 3; ++k) sum[k] += c == k ? s : 0, count[k] += c == k ? 1 : 0;
        }
    const int c0 = p.cfa[py * 6 + px], own = S(y, x);
    R2F_UNROLL
    for (int k = 0; k < 3; ++k) rgb[k] = k == c0 ? own : (count[k] ? sum[k] / count[k] : 0);  // (sum >= 0: the division is the floor)
}

// B2: the three planes of an interior pixel from its sample and the colour differences of its centred 3 x 3.
template <typename SFn, typename DFn>
R2F_HD void interior_rgb(const r2f_xtrans_params& p, const SFn& S, const DFn& D, int y, int x, int (&rgb)[3]) {
    const int ph = phase(y, x), c0 = p.cfa[ph];
    const int g0 = S(y, x) - D(y, x);
    const unsigned mr = p.taps[ph][0], mb = p.taps[ph][1];
    int sr = 0, sb = 0;
    R2F_UNROLL
    for (int k = 0; k < 9; ++k) {
        if (k == 4) continue;
        const int dy = k / 3 - 1, dx = k % 3 - 1;
        const int d = D(y + dy, x + dx) * ((k & 1) ? 2 : 1);  // (odd k: the four edge neighbours)
        sr += (mr >> k) & 1u ? d : 0, sb += (mb >> k) & 1u ? d : 0;
    }
    const int r = clip16(g0 + floor_div(sr, p.wsum[ph][0], p.recip[ph][0])), b = clip16(g0 + floor_div(sb, p.wsum[ph][1], p.recip[ph][1]));
    const int own = S(y, x);
    rgb[kRed] = c0 == kRed ? own : r, rgb[kGreen] = g0, rgb[kBlue] = c0 == kBlue ? own : b;
}

template <typename SFn, typename DFn>
R2F_HD void pixel_rgb(const r2f_xtrans_params& p, const SFn& S, const DFn& D, int H, int W, int y, int x, int (&rgb)[3]) {
    if (in_ring(H, W, y, x, 3))
        border_rgb(p, S, H, W, y, x, rgb);
    else
        interior_rgb(p, S, D, y, x, rgb);
}

// B': output pixel (y, x) of the reduced size from the cell at (3 y, 3 x); q[3 j + i] the scaled sample of the cell's (j, i).
R2F_HD void reduced_rgb(const r2f_xtrans_params& p, const int (&q)[9], int y, int x, int (&rgb)[3]) {
    const int cy = y & 1, cx = x & 1;  // (3 y % 6 is 0 or 3)
    int sum[3] = {0, 0, 0};
    R2F_UNROLL
    for (int k = 0; k < 9; ++k) {
        const int c = p.cfa[(3 * cy + k / 3) * 6 + 3 * cx + k % 3];
        sum[0] += c == 0 ? q[k] : 0, sum[1] += c == 1 ? q[k] : 0, sum[2] += c == 2 ? q[k] : 0;
    }
    R2F_UNROLL
    for (int c = 0; c < 3; ++c) rgb[c] = sum[c] / p.cell_count[cy * 2 + cx][c];  // (a planned reduced pattern: every count >= 1)
}

// C with the pattern's params: mosaic::colour (r2f_mosaic_math.h) on their matrix.
R2F_HD void colour(const r2f_xtrans_params& p, const int (&rgb)[3], uint16_t (&out)[3]) { mosaic::colour(p.M, rgb, out); }

}  // namespace xtrans
}  // namespace r2f
