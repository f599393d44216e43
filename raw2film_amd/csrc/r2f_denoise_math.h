// r2f_denoise_math.h -- the per-sample arithmetic of the wavelet denoise of a Bayer mosaic (include/r2f.h: r2f_mosaic_denoise): the
// shift, the index reflection, step 2's lift to the square-root domain, step 3's hat and threshold, step 4, and the check of a
// params record.  Like r2f_mosaic_math.h, whose macros it takes, this is text that hipcc compiles for the device and g++
// -ffp-contract=off for the CPU program (tests/denoise_check.cpp).  Every line that rounds is one fp32 operation, in the header's order.
#pragma once

#include "r2f_mosaic_math.h"

namespace r2f {
namespace denoise {

constexpr int kLevels = 5, kMinSide = 64, kMaxShift = 15;
constexpr float kMaxThreshold = 1e6f;

// noise[lev] of step 3 (dcraw's table, its first five entries)
R2F_HD float noise_of(int lev) { return lev == 0 ? 0.8002f : lev == 1 ? 0.2735f : lev == 2 ? 0.1202f : lev == 3 ? 0.0585f : 0.0291f; }
R2F_HD float theta_of(float threshold, int lev) {
    R2F_NO_CONTRACT
    return threshold * noise_of(lev);
}

// 1: the largest s >= 0 with (M << s) < 65536, for M in [1, 65535]
R2F_HD int shift_of(int maximum) {
    int s = 0;
    while ((maximum << (s + 1)) < 65536) ++s;
    return s;
}

R2F_HD bool side_ok(int n) { return n >= kMinSide && n % 2 == 0; }
// what the planner produces: black levels in [0, 65535], a shift in [0, 15], a threshold in (0, 1e6] (a NaN fails the comparison)
R2F_HD bool params_ok(const int32_t (&black)[4], int32_t shift, float threshold) {
    for (int k = 0; k < 4; ++k)
        if (black[k] < 0 || black[k] > 65535) return false;
    return shift >= 0 && shift <= kMaxShift && threshold > 0.f && threshold <= kMaxThreshold;
}

// the taps of hat() at distance c of sample i of a line of n >= 32 samples, c <= 16: both lie in [0, n)
R2F_HD int reflect_m(int i, int c) { return i >= c ? i - c : c - i; }
R2F_HD int reflect_p(int i, int c, int n) { return i + c < n ? i + c : 2 * n - 2 - (i + c); }

// 2: F of one sample (t << s is below 2^31 and has at most 16 significant bits: exact as a float)
R2F_HD float lift(int raw, int black, int shift) {
    R2F_NO_CONTRACT
    const int t = raw > black ? raw - black : 0;
    const float root = sqrtf((float)(t << shift));
    return 256.f * root;
}

// 3: 0.25 * hat (the product 2 b[i] and the quartering are exact)
R2F_HD float quarter_hat(float mid, float m, float p) {
    R2F_NO_CONTRACT
    float acc = 2.f * mid;
    acc = acc + m;
    acc = acc + p;
    return 0.25f * acc;
}
// 3: d' of one level
R2F_HD float shrink(float in, float low, float theta) {
    R2F_NO_CONTRACT
    const float d = in - low;
    if (d < -theta) return d + theta;
    if (d > theta) return d - theta;
    return 0.f;
}
// 4: the sample that leaves (q >= 0 and never a NaN; the clamp comes ahead of the conversion, which then stays inside int)
R2F_HD int finish(float D, float L) {
    R2F_NO_CONTRACT
    const float sum = D + L;
    float q = sum * sum;
    q = q * 0x1p-16f;  // (exact: / 65536)
    return (int)(q < 65535.f ? q : 65535.f);
}

}  // namespace denoise
}  // namespace r2f
