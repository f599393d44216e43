// r2f_lens_plan.cpp -- host planner of the lens correction (include/r2f.h: r2f_lens_plan, r2f_lens_plan_tca, r2f_lens_plan_projected,
// r2f_lens_phase_table).  No HIP in this file: hipcc compiles it into the library, g++ -fsanitize=address,undefined,float-cast-overflow
// into the programs of tests/lens_check.cpp, tests/lens_tca_check.cpp and tests/lens_projection_check.cpp.
#include <cmath>

#include "../../include/r2f.h"
#include "r2f_plan.h"

namespace {

constexpr int kCoefCount[4] = {0, 1, 2, 3};  // none, poly3, poly5, ptlens

// The definition's map in double: f(r) of the profile's model.
double model_factor(const r2f_lens_profile& p, double r2) {
    switch (p.model) {
        case R2F_LENS_POLY3: return (1.0 - p.coef[0]) + p.coef[0] * r2;
        case R2F_LENS_POLY5: return 1.0 + r2 * (p.coef[0] + p.coef[1] * r2);
        case R2F_LENS_PTLENS: {
            const double r = std::sqrt(r2), a = p.coef[0], b = p.coef[1], c = p.coef[2];
            return (1.0 - a - b - c) + r * (c + r * (b + r * a));
        }
        default: return 1.0;
    }
}

// The TCA factor t of one channel's constants (v, c, b) in double, at an offset of length r in units of the normalisation radius.
double tca_factor(const r2f_lens_tca& tca, const double* k, double r) {
    return tca.model == R2F_TCA_POLY3 ? k[0] + r * (k[1] + r * k[2]) : k[0];
}

// The projection factor P of a probe at tangent t: in double, then rounded to float -- the precision at which the kernel applies it,
// so that a projection the kernel cannot resolve (P rounds to 1) leaves the probes, and with them the scale, r2f_lens_plan's.
double projection_factor(const r2f_lens_projection& proj, double t) {
    const double s = std::sqrt(1.0 + t * t);
    double P = 1.0;
    switch (proj.type) {
        case R2F_PROJ_FISHEYE: P = t > 0 ? std::atan(t) / t : 1.0; break;
        case R2F_PROJ_STEREOGRAPHIC: P = 2.0 / (1.0 + s); break;
        case R2F_PROJ_EQUISOLID: P = 1.0 / (s * std::sqrt((s + 1.0) / (2.0 * s))); break;
        case R2F_PROJ_ORTHOGRAPHIC: P = 1.0 / s; break;
        default: break;
    }
    return (double)(float)P;
}

// How far the furthest-reaching of the eight probes lands outside [0, W - 1] x [0, H - 1], in pixels (<= 0: every probe is inside;
// 0: one lies exactly on the boundary).  NaN when the map is not finite at a probe.  With a TCA record each probe is evaluated for
// green, red and blue, and the furthest reach of any channel counts.  With a projection each probe's (u, v) is taken to the lens's own
// projection before the model sees it, and its factor multiplies the model's (P == 1 leaves every value what it is without one).
double outside(const r2f_lens_profile& p, const r2f_lens_projection* proj, const r2f_lens_tca* tca, int H, int W, double cx, double cy,
               double norm, double scale) {
    const double xs[3] = {0.0, (W - 1) / 2.0, (double)(W - 1)}, ys[3] = {0.0, (H - 1) / 2.0, (double)(H - 1)};
    double worst = -INFINITY;
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) {
            if (i == 1 && j == 1) continue;  // (the centre is no probe)
            const double dx = xs[i] - cx, dy = ys[j] - cy;
            const double q = 1.0 / (norm * scale);
            double u = dx * q, v = dy * q, P = 1.0;
            if (proj) {
                P = projection_factor(*proj, std::sqrt(u * u + v * v) / proj->focal);
                u *= P, v *= P;
            }
            const double g = model_factor(p, u * u + v * v) * P / scale;
            const double ox = dx * g, oy = dy * g;
            for (int ch = 0; ch < (tca ? 3 : 1); ++ch) {  // green first: the only one without a record
                double t = 1.0;
                if (ch) {
                    const double a = ox / norm, e = oy / norm;
                    t = tca_factor(*tca, ch == 1 ? tca->red : tca->blue, std::sqrt(a * a + e * e));
                }
                const double sx = cx + ox * t, sy = cy + oy * t;
                if (!std::isfinite(sx) || !std::isfinite(sy)) return NAN;
                worst = std::fmax(worst, std::fmax(std::fmax(-sx, sx - (W - 1)), std::fmax(-sy, sy - (H - 1))));
            }
        }
    return worst;
}

bool fits_float(double v) { return std::isfinite(v) && std::fabs(v) <= 3.0e38; }

// r2f_lens_plan, with the probes of the auto scale going through `proj` and `tca` too when there is one.
int plan(const r2f_lens_profile* p, const r2f_lens_projection* proj, const r2f_lens_tca* tca, int H, int W, r2f_lens_params* out) {
    if (!p || !out || H < 1 || W < 1) return R2F_EINVAL;
    if (p->model < R2F_LENS_NONE || p->model > R2F_LENS_PTLENS || p->n_coef != kCoefCount[p->model]) return R2F_EINVAL;
    for (int i = 0; i < p->n_coef; ++i)
        if (!std::isfinite(p->coef[i])) return R2F_EINVAL;
    if (p->has_vignetting)
        for (int i = 0; i < 3; ++i)
            if (!std::isfinite(p->vignetting[i])) return R2F_EINVAL;
    if (!std::isfinite(p->center[0]) || !std::isfinite(p->center[1])) return R2F_EINVAL;
    if (!std::isfinite(p->norm_radius_px) || p->norm_radius_px < 0) return R2F_EINVAL;
    if (!p->auto_scale && !(std::isfinite(p->scale) && p->scale > 0)) return R2F_EINVAL;

    double norm = p->norm_radius_px;
    if (norm == 0) norm = std::hypot((double)(W - 1), (double)(H - 1)) / 2.0;
    if (norm == 0) norm = 1.0;  // a 1 x 1 frame
    const double cx = (W - 1) / 2.0 + p->center[0] * norm, cy = (H - 1) / 2.0 + p->center[1] * norm;
    if (!std::isfinite(cx) || !std::isfinite(cy)) return R2F_EINVAL;

    double scale = p->scale;
    if (p->auto_scale) {
        if (H == 1 && W == 1) {
            scale = 1.0;  // every probe is the one pixel: nothing to fit
        } else {
            // at `lo` a probe is outside (or the map is not finite there: NaN), at `hi` all are inside; keep that while halving
            double lo = 1.0 / 16, hi = 16.0;
            if (!(outside(*p, proj, tca, H, W, cx, cy, norm, hi) <= 0) || outside(*p, proj, tca, H, W, cx, cy, norm, lo) <= 0)
                return R2F_EINVAL;
            for (int it = 0; it < 200; ++it) {
                const double mid = lo + (hi - lo) / 2;
                if (mid <= lo || mid >= hi) break;
                if (outside(*p, proj, tca, H, W, cx, cy, norm, mid) <= 0)
                    hi = mid;
                else
                    lo = mid;
            }
            scale = hi;
        }
    }

    double a = 0, b = 0, c = 0, c0 = 1.0;
    if (p->model == R2F_LENS_POLY3) a = p->coef[0], c0 = 1.0 - a;
    if (p->model == R2F_LENS_POLY5) a = p->coef[0], b = p->coef[1];
    if (p->model == R2F_LENS_PTLENS) a = p->coef[0], b = p->coef[1], c = p->coef[2], c0 = 1.0 - a - b - c;
    const double q = 1.0 / (norm * scale), inv_scale = 1.0 / scale, qv = 1.0 / norm;
    const double all[] = {cx, cy, q, inv_scale, c0, a, b, c, qv};
    for (double v : all)
        if (!fits_float(v)) return R2F_EINVAL;
    r2f_lens_params r{};
    r.model = p->model;
    r.vignetting = p->has_vignetting ? 1 : 0;
    r.cx = (float)cx, r.cy = (float)cy, r.q = (float)q, r.inv_scale = (float)inv_scale, r.c0 = (float)c0;
    r.k[0] = (float)a, r.k[1] = (float)b, r.k[2] = (float)c;
    r.qv = (float)qv;
    for (int i = 0; i < 3; ++i) {
        const double v = p->has_vignetting ? p->vignetting[i] : 0.0;
        if (!fits_float(v)) return R2F_EINVAL;
        r.v[i] = (float)v;
    }
    r.scale = scale;
    *out = r;
    return R2F_OK;
}

// The TCA record's checks and its constants in float.
int plan_tca_record(const r2f_lens_tca* tca, r2f_lens_tca_params* out_tca) {
    if (tca->model != R2F_TCA_LINEAR && tca->model != R2F_TCA_POLY3) return R2F_EINVAL;
    if (tca->n_coef != (tca->model == R2F_TCA_LINEAR ? 1 : 3)) return R2F_EINVAL;
    r2f_lens_tca_params t{};
    t.model = tca->model;
    for (int i = 0; i < tca->n_coef; ++i) {
        if (!fits_float(tca->red[i]) || !fits_float(tca->blue[i])) return R2F_EINVAL;
        t.red[i] = (float)tca->red[i], t.blue[i] = (float)tca->blue[i];
    }
    *out_tca = t;
    return R2F_OK;
}

}  // namespace

extern "C" {

int r2f_lens_plan(const r2f_lens_profile* p, int H, int W, r2f_lens_params* out) { return plan(p, nullptr, nullptr, H, W, out); }

int r2f_lens_plan_tca(const r2f_lens_profile* p, const r2f_lens_tca* tca, int H, int W, r2f_lens_params* out, r2f_lens_tca_params* out_tca) {
    if (!tca || !out || !out_tca) return R2F_EINVAL;
    r2f_lens_tca_params t;
    int rc = plan_tca_record(tca, &t);
    if (rc != R2F_OK) return rc;
    r2f_lens_params r;
    rc = plan(p, nullptr, tca, H, W, &r);
    if (rc != R2F_OK) return rc;
    *out = r, *out_tca = t;
    return R2F_OK;
}

int r2f_lens_plan_projected(const r2f_lens_profile* p, const r2f_lens_projection* proj, const r2f_lens_tca* tca, int H, int W,
                            r2f_lens_params* out, r2f_lens_projection_params* out_proj, r2f_lens_tca_params* out_tca) {
    if (!proj || !out || !out_proj || (tca != nullptr) != (out_tca != nullptr)) return R2F_EINVAL;
    if (proj->type < R2F_PROJ_FISHEYE || proj->type > R2F_PROJ_ORTHOGRAPHIC) return R2F_EINVAL;
    if (!(std::isfinite(proj->focal) && proj->focal > 0) || !fits_float(1.0 / proj->focal)) return R2F_EINVAL;
    r2f_lens_tca_params t{};
    int rc = tca ? plan_tca_record(tca, &t) : R2F_OK;
    if (rc != R2F_OK) return rc;
    r2f_lens_params r;
    rc = plan(p, proj, tca, H, W, &r);
    if (rc != R2F_OK) return rc;
    *out = r;
    out_proj->type = proj->type, out_proj->inv_focal = (float)(1.0 / proj->focal);
    if (out_tca) *out_tca = t;
    return R2F_OK;
}

int r2f_lens_phase_table(float* table_32x8) {
    if (!table_32x8) return R2F_EINVAL;
    for (int ph = 0; ph < 32; ++ph) r2f::plan::lanczos4_coeffs((float)ph / 32.f, table_32x8 + 8 * ph);
    return R2F_OK;
}

}  // extern "C"
