// r2f_lens_math.h -- the arithmetic of the lens correction (include/r2f.h, r2f_lens_correct, r2f_lens_correct_tca and
// r2f_lens_correct_projected), as text the device kernels (r2f_lens.hip) and CPU programs (tests/lens_check.cpp,
// tests/lens_tca_check.cpp, tests/lens_projection_check.cpp, g++ -ffp-contract=off) both compile: the coordinate map, the projection
// factor in front of its distortion model, red's and blue's TCA step on it, the 1/32 phase split with its inside / outside decision, the 64-tap
// sample over a pixel-fetch functor (three channels at one coordinate, or one channel at its own) and the vignetting gain.  Every
// operation is one correctly rounded fp32 operation; contraction is off for each function (a fused multiply-add would round once
// where the definition rounds twice).  No HIP types, no includes beyond <math.h>.
#pragma once

#include <math.h>

#include "../../include/r2f.h"

#if defined(__HIPCC__)
#define R2F_HD __host__ __device__ __forceinline__
#else
#define R2F_HD inline
#endif
#if defined(__clang__)
#define R2F_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define R2F_NO_CONTRACT  // (g++: the translation unit is compiled with -ffp-contract=off)
#endif

namespace r2f {
namespace lens {

constexpr int kPhases = 32;  // INTER_TAB_SIZE = 1 << INTER_BITS
constexpr int kTaps = 8;

// The model factor f of r2 (ptlens: of r = sqrt(r2)).
R2F_HD float model_factor(const r2f_lens_params& p, float r2) {
    R2F_NO_CONTRACT
    float f = 1.f;
    if (p.model == R2F_LENS_POLY3) {
        const float t = p.k[0] * r2;
        f = p.c0 + t;
    } else if (p.model == R2F_LENS_POLY5) {
        const float t0 = p.k[1] * r2;
        const float t1 = p.k[0] + t0;
        const float t2 = r2 * t1;
        f = 1.f + t2;
    } else if (p.model == R2F_LENS_PTLENS) {
        const float r = sqrtf(r2);
        const float t0 = r * p.k[0];
        const float t1 = p.k[1] + t0;
        const float t2 = r * t1;
        const float t3 = p.k[2] + t2;
        const float t4 = r * t3;
        f = p.c0 + t4;
    }
    return f;
}

// The offset (ox, oy) = (dx*g, dy*g) of output pixel (X, Y)'s source coordinate from the optical centre: the map up to the point at
// which the channels part (r2f_lens_correct_tca).  dx, dy are handed on to the vignetting gain.
R2F_HD void source_offset(const r2f_lens_params& p, int X, int Y, float& ox, float& oy, float& dx, float& dy) {
    R2F_NO_CONTRACT
    dx = (float)X - p.cx;
    dy = (float)Y - p.cy;
    const float u = dx * p.q, v = dy * p.q;
    const float uu = u * u, vv = v * v;
    const float r2 = uu + vv;
    const float f = model_factor(p, r2);
    const float g = f * p.inv_scale;
    ox = dx * g, oy = dy * g;
}

// p(x) of include/r2f.h's fisheye factor: atan(t) ~ t*p(t*t) on [0, 1], Horner from c9 down, each product and sum rounded on its own.
R2F_HD float atan_poly(float x) {
    R2F_NO_CONTRACT
    const float c[10] = {0x1p+0f,         -0x1.55554p-2f, 0x1.999278p-3f, -0x1.242702p-3f, 0x1.c0d2e2p-4f,
                         -0x1.58dd68p-4f, 0x1.dd11b4p-5f, -0x1.01b21p-5f, 0x1.6a946ap-7f,  -0x1.df068p-10f};
    float acc = c[9];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 8; k >= 0; --k) {
        acc = acc * x;
        acc = c[k] + acc;
    }
    return acc;
}

// The projection factor P(t) of r2f_lens_correct_projected: the lens's image radius over the rectilinear one, t = tan(theta).
// An unknown type (the entry point refuses it) gives 1.
R2F_HD float projection_factor(int type, float t) {
    R2F_NO_CONTRACT
    const float tt = t * t;
    if (type == R2F_PROJ_FISHEYE) {
        if (t <= 1.f) return atan_poly(tt);
        const float w = 1.f / t;
        const float ww = w * w;
        const float a = w * atan_poly(ww);
        const float b = 0x1.921fb6p+0f - a;
        return b * w;
    }
    const float s1 = 1.f + tt;
    const float s = sqrtf(s1);
    if (type == R2F_PROJ_ORTHOGRAPHIC) return 1.f / s;
    if (type == R2F_PROJ_STEREOGRAPHIC) {
        const float d = 1.f + s;
        return 2.f / d;
    }
    if (type == R2F_PROJ_EQUISOLID) {
        const float n = s + 1.f, m = 2.f * s;
        const float h = n / m;
        const float e = sqrtf(h);
        const float b = s * e;
        return 1.f / b;
    }
    return 1.f;
}

// source_offset through the projection step (r2f_lens_correct_projected): the output pixel's rectilinear radius goes to the lens's
// own projection before the distortion model sees it.  With P == 1 every value below is source_offset's.
R2F_HD void source_offset(const r2f_lens_params& p, const r2f_lens_projection_params& pp, int X, int Y, float& ox, float& oy, float& dx,
                          float& dy) {
    R2F_NO_CONTRACT
    dx = (float)X - p.cx;
    dy = (float)Y - p.cy;
    const float u = dx * p.q, v = dy * p.q;
    const float uu = u * u, vv = v * v;
    const float r2 = uu + vv;
    const float r = sqrtf(r2);
    const float t = r * pp.inv_focal;
    const float P = projection_factor(pp.type, t);
    const float up = u * P, vp = v * P;
    const float upp = up * up, vpp = vp * vp;
    const float r2p = upp + vpp;
    const float f = model_factor(p, r2p);
    const float g0 = f * P;
    const float g = g0 * p.inv_scale;
    ox = dx * g, oy = dy * g;
}

// Source coordinate (sx, sy) of output pixel (X, Y); dx, dy are handed on to the vignetting gain.
R2F_HD void source_coord(const r2f_lens_params& p, int X, int Y, float& sx, float& sy, float& dx, float& dy) {
    R2F_NO_CONTRACT
    float ox, oy;
    source_offset(p, X, Y, ox, oy, dx, dy);
    sx = p.cx + ox;
    sy = p.cy + oy;
}

// The centre plus an offset: the coordinate all three channels share without a TCA record, and green's with one.
R2F_HD void centre_coord(const r2f_lens_params& p, float ox, float oy, float& sx, float& sy) {
    R2F_NO_CONTRACT
    sx = p.cx + ox;
    sy = p.cy + oy;
}

// The coordinate at which channel ch (0 red, 1 green, 2 blue) samples: green at the centre plus the offset, red and blue at the
// centre plus the offset times their TCA factor t (linear: v; poly3: v + r*(c + r*b), r the offset's length in units of the
// normalisation radius).
R2F_HD void channel_coord(const r2f_lens_params& p, const r2f_lens_tca_params& tca, int ch, float ox, float oy, float& sx, float& sy) {
    R2F_NO_CONTRACT
    if (ch != 1) {
        const float* k = ch == 0 ? tca.red : tca.blue;
        float t = k[0];
        if (tca.model == R2F_TCA_POLY3) {
            const float a = ox * p.qv, e = oy * p.qv;
            const float aa = a * a, ee = e * e;
            const float r2 = aa + ee;
            const float r = sqrtf(r2);
            const float t0 = r * k[2];
            const float t1 = k[1] + t0;
            const float t2 = r * t1;
            t = k[0] + t2;
        }
        ox = ox * t, oy = oy * t;
    }
    sx = p.cx + ox;
    sy = p.cy + oy;
}

// One axis of the 1/32 phase split: s -> (i, phase), or false when no tap of i-3 .. i+4 can lie inside [0, n).  Decided on the
// float rint(s*32) -- a NaN fails both comparisons, an infinity or 1e30 one of them -- so the int conversion only ever sees values
// of at most (n + 3)*32 in magnitude.
R2F_HD bool split_phase(float s, int n, int& i, int& phase) {
    R2F_NO_CONTRACT
    const float t = s * 32.f;
    const float qf = rintf(t);
    if (!(qf >= -128.f && qf < (float)(n + 3) * 32.f)) return false;  // i >= -4 and i <= n + 2
    const int q = (int)qf;
    i = q >> 5;
    phase = q & 31;
    return true;
}

// The 64 taps around (ix, iy) with the rows wy, wx of the phase table.  fetch(y, x, v) is called for taps inside the frame only and
// fills the three channels; a tap outside reads 0.  Sum order: a row left to right, rows top to bottom, each from its first product.
template <typename Fetch>
R2F_HD void sample64(const Fetch& fetch, int H, int W, int ix, int iy, const float* wx, const float* wy, float (&acc)[3]) {
    R2F_NO_CONTRACT
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < kTaps; ++k) {
        const int yy = iy - 3 + k;
        const bool row_in = yy >= 0 && yy < H;
        float h[3] = {0.f, 0.f, 0.f};
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < kTaps; ++j) {
            const int xx = ix - 3 + j;
            float v[3] = {0.f, 0.f, 0.f};
            if (row_in && xx >= 0 && xx < W) fetch(yy, xx, v);
            const float w = wy[k] * wx[j];
            for (int c = 0; c < 3; ++c) {
                const float prod = w * v[c];
                h[c] = j == 0 ? prod : h[c] + prod;
            }
        }
        for (int c = 0; c < 3; ++c) acc[c] = k == 0 ? h[c] : acc[c] + h[c];
    }
}

// sample64 for one channel: fetch(ch, y, x) returns that channel's sample of a texel inside the frame.  The same weights, products
// and sum order as sample64's for that channel.
template <typename Fetch>
R2F_HD float sample64_channel(const Fetch& fetch, int ch, int H, int W, int ix, int iy, const float* wx, const float* wy) {
    R2F_NO_CONTRACT
    float acc = 0.f;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < kTaps; ++k) {
        const int yy = iy - 3 + k;
        const bool row_in = yy >= 0 && yy < H;
        float h = 0.f;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < kTaps; ++j) {
            const int xx = ix - 3 + j;
            const float v = row_in && xx >= 0 && xx < W ? fetch(ch, yy, xx) : 0.f;
            const float w = wy[k] * wx[j];
            const float prod = w * v;
            h = j == 0 ? prod : h + prod;
        }
        acc = k == 0 ? h : acc + h;
    }
    return acc;
}

// max(sum, 0), then the vignetting gain of (dx, dy).
R2F_HD float finish(const r2f_lens_params& p, float sum, float dx, float dy) {
    R2F_NO_CONTRACT
    float o = sum < 0.f ? 0.f : sum;
    if (p.vignetting) {
        const float a = dx * p.qv, b = dy * p.qv;
        const float aa = a * a, bb = b * b;
        const float rv2 = aa + bb;
        const float t0 = rv2 * p.v[2];
        const float t1 = p.v[1] + t0;
        const float t2 = rv2 * t1;
        const float t3 = p.v[0] + t2;
        const float t4 = rv2 * t3;
        const float d = 1.f + t4;
        o = o / d;
    }
    return o;
}

// One output pixel, start to end: what the kernel's lane and the CPU program's loop body both run.  `table`: 32 x 8 floats.
template <typename Fetch>
R2F_HD void correct_pixel(const r2f_lens_params& p, const Fetch& fetch, int H, int W, const float* table, int X, int Y, float (&out)[3]) {
    float sx, sy, dx, dy;
    source_coord(p, X, Y, sx, sy, dx, dy);
    int ix, iy, fx, fy;
    out[0] = out[1] = out[2] = 0.f;
    if (!split_phase(sx, W, ix, fx) || !split_phase(sy, H, iy, fy)) return;  // outside: 0, nothing indexed, no gain applied
    float acc[3];
    sample64(fetch, H, W, ix, iy, table + fx * kTaps, table + fy * kTaps, acc);
    for (int c = 0; c < 3; ++c) out[c] = finish(p, acc[c], dx, dy);
}

// One output pixel of r2f_lens_correct_tca, start to end: each channel with its own coordinate, decision, phases and sum.
template <typename Fetch>
R2F_HD void correct_pixel_tca(const r2f_lens_params& p, const r2f_lens_tca_params& tca, const Fetch& fetch, int H, int W, const float* table,
                              int X, int Y, float (&out)[3]) {
    float ox, oy, dx, dy;
    source_offset(p, X, Y, ox, oy, dx, dy);
    for (int ch = 0; ch < 3; ++ch) {
        float sx, sy;
        channel_coord(p, tca, ch, ox, oy, sx, sy);
        int ix, iy, fx, fy;
        out[ch] = 0.f;
        if (!split_phase(sx, W, ix, fx) || !split_phase(sy, H, iy, fy)) continue;  // outside: 0 for this channel alone
        out[ch] = finish(p, sample64_channel(fetch, ch, H, W, ix, iy, table + fx * kTaps, table + fy * kTaps), dx, dy);
    }
}

// correct_pixel through the projection step.
template <typename Fetch>
R2F_HD void correct_pixel(const r2f_lens_params& p, const r2f_lens_projection_params& pp, const Fetch& fetch, int H, int W, const float* table,
                          int X, int Y, float (&out)[3]) {
    R2F_NO_CONTRACT
    float ox, oy, dx, dy;
    source_offset(p, pp, X, Y, ox, oy, dx, dy);
    float sx, sy;
    centre_coord(p, ox, oy, sx, sy);
    int ix, iy, fx, fy;
    out[0] = out[1] = out[2] = 0.f;
    if (!split_phase(sx, W, ix, fx) || !split_phase(sy, H, iy, fy)) return;
    float acc[3];
    sample64(fetch, H, W, ix, iy, table + fx * kTaps, table + fy * kTaps, acc);
    for (int c = 0; c < 3; ++c) out[c] = finish(p, acc[c], dx, dy);
}

// correct_pixel_tca through the projection step.
template <typename Fetch>
R2F_HD void correct_pixel_tca(const r2f_lens_params& p, const r2f_lens_projection_params& pp, const r2f_lens_tca_params& tca, const Fetch& fetch,
                              int H, int W, const float* table, int X, int Y, float (&out)[3]) {
    float ox, oy, dx, dy;
    source_offset(p, pp, X, Y, ox, oy, dx, dy);
    for (int ch = 0; ch < 3; ++ch) {
        float sx, sy;
        channel_coord(p, tca, ch, ox, oy, sx, sy);
        int ix, iy, fx, fy;
        out[ch] = 0.f;
        if (!split_phase(sx, W, ix, fx) || !split_phase(sy, H, iy, fy)) continue;
        out[ch] = finish(p, sample64_channel(fetch, ch, H, W, ix, iy, table + fx * kTaps, table + fy * kTaps), dx, dy);
    }
}

}  // namespace lens
}  // namespace r2f
