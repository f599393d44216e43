// r2f_demosaic_math.h -- the per-pixel arithmetic of the Bayer demosaic (include/r2f.h, r2f_demosaic_u16), as text the device
// kernels (r2f_demosaic.hip) and a CPU program (tests/demosaic_check.cpp, g++ -ffp-contract=off) both compile: step A (black /
// scale), B0 (border ring), B1 (green), B2 / B3 (red and blue) and B' (half size); step C (colour matrix, clip) is r2f_mosaic_math.h's,
// shared with the X-Trans pattern.  Everything is integer arithmetic except the one fp32 multiply of step A (and the five fp32
// operations per channel of step C), for which contraction is off.  Samples come through accessors: `S(y, x)` the scaled mosaic,
// `G(y, x)` the finished green plane, both at frame coordinates inside the frame.  No HIP types.
#pragma once

#include "../../include/r2f.h"
#include "r2f_mosaic_math.h"

namespace r2f {
namespace demosaic {

using namespace mosaic;  // the macro set, kRed / kGreen / kBlue, clip16, iabs, in_ring and step C (colour)

R2F_HD int site(int y, int x) { return (y & 1) * 2 + (x & 1); }
// (selects, not an indexed load: the params sit in registers on the device, and a register array indexed by a variable goes to scratch)
template <typename T>
R2F_HD T pick4(const T (&v)[4], int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : (k == 2 ? v[2] : v[3])); }
R2F_HD int colour_of(const r2f_demosaic_params& p, int y, int x) { return pick4(p.cfa, site(y, x)); }

// A: one raw sample of site k.  |t * mul| <= 65535 * 1024: the truncation stays inside int.
R2F_HD int scale_sample(const r2f_demosaic_params& p, int raw, int k) {
    R2F_NO_CONTRACT
    const float f = (float)(raw - pick4(p.black, k)) * pick4(p.mul, k);
    return clip16((int)f);
}

// B0: colour c at (y, x) as the floor mean of the sites of that colour in the 3 x 3 neighbourhood clipped to the frame.
template <typename SFn>
R2F_HD int border_mean(const r2f_demosaic_params& p, const SFn& S, int H, int W, int y, int x, int c) {
    int sum = 0, count = 0;
    for (int yy = y - 1; yy <= y + 1; ++yy)
        for (int xx = x - 1; xx <= x + 1; ++xx)
            if (yy >= 0 && yy < H && xx >= 0 && xx < W && colour_of(p, yy, xx) == c) sum += S(yy, xx), ++count;
    return count ? sum / count : 0;  // (sum >= 0: the division is the floor)
}

// B1: green at a non-green site at least 3 samples from every edge.
template <typename SFn>
R2F_HD int green_ppg(const SFn& S, int y, int x) {
    int guess[2], diff[2], lo[2], hi[2];
    R2F_UNROLL
    for (int d = 0; d < 2; ++d) {
        const int dy = d, dx = 1 - d;  // h = (0, 1), then v = (1, 0)
        const int s0 = S(y, x), m1 = S(y - dy, x - dx), p1 = S(y + dy, x + dx), m2 = S(y - 2 * dy, x - 2 * dx),
                  p2 = S(y + 2 * dy, x + 2 * dx), m3 = S(y - 3 * dy, x - 3 * dx), p3 = S(y + 3 * dy, x + 3 * dx);
        guess[d] = 2 * (m1 + s0 + p1) - m2 - p2;
        diff[d] = 3 * (iabs(m2 - s0) + iabs(p2 - s0) + iabs(m1 - p1)) + 2 * (iabs(p3 - p1) + iabs(m3 - m1));
        lo[d] = m1 < p1 ? m1 : p1, hi[d] = m1 < p1 ? p1 : m1;
    }
    const bool v = diff[0] > diff[1];
    const int g = (v ? guess[1] : guess[0]) >> 2, l = v ? lo[1] : lo[0], h = v ? hi[1] : hi[0];
    return g < l ? l : (g > h ? h : g);
}

// The finished green plane at (y, x): native, B0's in rings 0 .. 2, B1's elsewhere.
template <typename SFn>
R2F_HD int green_at(const r2f_demosaic_params& p, const SFn& S, int H, int W, int y, int x) {
    if (colour_of(p, y, x) == kGreen) return S(y, x);
    if (in_ring(H, W, y, x, 3)) return border_mean(p, S, H, W, y, x, kGreen);
    return green_ppg(S, y, x);
}

// B0, B2, B3: the three planes at (y, x), before the matrix.
template <typename SFn, typename GFn>
R2F_HD void pixel_rgb(const r2f_demosaic_params& p, const SFn& S, const GFn& G, int H, int W, int y, int x, int (&rgb)[3]) {
    const int c0 = colour_of(p, y, x), own = S(y, x);
    if (in_ring(H, W, y, x, 1)) {
        R2F_UNROLL
        for (int c = 0; c < 3; ++c) rgb[c] = c == c0 ? own : border_mean(p, S, H, W, y, x, c);
        return;
    }
    if (c0 == kGreen) {
        const int ch = clip16((S(y, x - 1) + S(y, x + 1) + 2 * own - G(y, x - 1) - G(y, x + 1)) >> 1);
        const int cv = clip16((S(y - 1, x) + S(y + 1, x) + 2 * own - G(y - 1, x) - G(y + 1, x)) >> 1);
        const bool red_h = colour_of(p, y, x + 1) == kRed;  // (the neighbours along h are red, those along v blue, or the reverse)
        rgb[kRed] = red_h ? ch : cv, rgb[kGreen] = own, rgb[kBlue] = red_h ? cv : ch;
        return;
    }
    const int g0 = G(y, x);
    int guess[2], diff[2];
    R2F_UNROLL
    for (int d = 0; d < 2; ++d) {
        const int dx = d ? -1 : 1;  // d1 = (1, 1), d2 = (1, -1)
        const int sm = S(y - 1, x - dx), sp = S(y + 1, x + dx), gm = G(y - 1, x - dx), gp = G(y + 1, x + dx);
        diff[d] = iabs(sm - sp) + iabs(gm - g0) + iabs(gp - g0);
        guess[d] = sm + sp + 2 * g0 - gm - gp;
    }
    const int other = diff[0] != diff[1] ? clip16((diff[0] > diff[1] ? guess[1] : guess[0]) >> 1) : clip16((guess[0] + guess[1]) >> 2);
    rgb[kRed] = c0 == kRed ? own : other, rgb[kGreen] = g0, rgb[kBlue] = c0 == kRed ? other : own;
}

// B': output pixel (y, x) of the half-size form from the quad at (2 y, 2 x); q[k] the scaled sample of site k.
R2F_HD void half_rgb(const r2f_demosaic_params& p, const int (&q)[4], int (&rgb)[3]) {
    int r = 0, g = 0, b = 0;  // (a planned pattern has one red, one blue and two green sites)
    R2F_UNROLL
    for (int k = 0; k < 4; ++k) {
        if (p.cfa[k] == kGreen)
            g += q[k];
        else if (p.cfa[k] == kRed)
            r = q[k];
        else
            b = q[k];
    }
    rgb[kRed] = r, rgb[kGreen] = g >> 1, rgb[kBlue] = b;
}

// C with the pattern's params: mosaic::colour (r2f_mosaic_math.h) on their matrix.
R2F_HD void colour(const r2f_demosaic_params& p, const int (&rgb)[3], uint16_t (&out)[3]) { mosaic::colour(p.M, rgb, out); }

}  // namespace demosaic
}  // namespace r2f
