// r2f_levels_plan.cpp -- host planner of a mosaic's scale from the sensor's levels and the frame's measured maximum (include/r2f.h:
// r2f_raw_scale_plan, the Scale steps).  No HIP in this file: hipcc compiles it into the library, g++
// -fsanitize=address,undefined,float-cast-overflow into tests/levels_check.cpp's program.  The comparisons are written so that a NaN
// fails them, and nothing is converted before it has passed.
#include <cmath>

#include "../../include/r2f.h"

extern "C" {

int r2f_raw_scale_plan(const r2f_raw_levels* levels, const double* black, int n_black, uint32_t data_maximum, r2f_raw_scale* out) {
    if (!levels || !black || !out || (n_black != 4 && n_black != 36) || data_maximum > 65535u) return R2F_EINVAL;
    double black_min = 65535.0;
    for (int i = 0; i < n_black; ++i) {
        const double b = black[i];
        if (!(b >= 0.0 && b <= 65535.0) || b != std::floor(b)) return R2F_EINVAL;
        black_min = b < black_min ? b : black_min;
    }
    const double* wb = levels->white_balance;
    double wb_min = wb[0];
    for (int c = 0; c < 3; ++c) {
        if (!(wb[c] > 0.0) || !std::isfinite(wb[c])) return R2F_EINVAL;
        wb_min = wb[c] < wb_min ? wb[c] : wb_min;
    }
    const double thr = levels->adjust_maximum_thr;
    if (levels->white_level < 1 || levels->white_level > 65535 || !(thr >= 0.0 && thr <= 1.0)) return R2F_EINVAL;
    const int m = levels->white_level - (int)black_min;
    if (m < 1) return R2F_EINVAL;
    const int d = (int)data_maximum;
    bool adjusted = false;
    if (!(thr < 0.00001)) {
        const float t = (float)(thr > 0.99999 ? 0.75 : thr);
        const float product = (float)m * t;  // one fp32 multiply (the program is built with contraction off; there is no add to fuse)
        adjusted = d > 0 && d < m && (float)d > product;
    }
    r2f_raw_scale r{};
    r.maximum_used = adjusted ? d : m;
    r.adjusted = adjusted ? 1 : 0;
    for (int c = 0; c < 3; ++c) r.mul[c] = wb[c] / wb_min * 65535.0 / (double)r.maximum_used;
    *out = r;
    return R2F_OK;
}

// Mode 0 is the call above; modes 1 and 2 take its m_eff and normalise by the largest factor.  Both outputs are written together, and
// only once nothing is left to refuse.
int r2f_raw_scale_plan_highlight(const r2f_raw_levels* levels, const double* black, int n_black, uint32_t data_maximum, int mode,
                                 r2f_raw_scale* out, r2f_highlight* hl) {
    if (!out || !hl || mode < R2F_HIGHLIGHT_CLIP || mode > R2F_HIGHLIGHT_BLEND) return R2F_EINVAL;  // (3 .. 9: LibRaw's rebuild modes)
    r2f_raw_scale r{};
    if (const int rc = r2f_raw_scale_plan(levels, black, n_black, data_maximum, &r)) return rc;
    r2f_highlight h{mode, 0};
    if (mode != R2F_HIGHLIGHT_CLIP) {
        const double* wb = levels->white_balance;  // (finite and > 0: the call above has passed them)
        double wb_max = wb[0];
        for (int c = 0; c < 3; ++c) wb_max = wb[c] > wb_max ? wb[c] : wb_max;
        for (int c = 0; c < 3; ++c) r.mul[c] = wb[c] / wb_max * 65535.0 / (double)r.maximum_used;
        if (mode == R2F_HIGHLIGHT_BLEND) {
            int clip = 65535;
            for (int c = 0; c < 3; ++c) {
                const float p = (float)(wb[c] / wb_max);  // in [0, 1]
                const float level = 65535.0f * p;         // one fp32 multiply, in [0, 65535]: the truncation stays inside int
                clip = (int)level < clip ? (int)level : clip;
            }
            if (clip < 1) return R2F_EINVAL;
            h.clip = clip;
        }
    }
    *out = r;
    *hl = h;
    return R2F_OK;
}

}  // extern "C"
