// r2f_denoise_plan.cpp -- host planner of the wavelet denoise of a Bayer mosaic (include/r2f.h: r2f_mosaic_denoise_plan, step 1 and
// the checks) and its workspace size.  No HIP in this file: hipcc compiles it into the library, g++ -fsanitize=address,undefined into
// tests/denoise_check.cpp's program.  The comparisons are written so that a NaN fails them, and nothing is converted before it has
// passed.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // (the library's build reads this file as HIP: r2f_mosaic_math.h's macro set then takes its qualifiers)
#endif
#include <cmath>

#include "../../include/r2f.h"
#include "r2f_denoise_math.h"

extern "C" {

int r2f_mosaic_denoise_plan(double threshold, int maximum, const double* black, int H, int W, r2f_denoise_params* out) {
    using namespace r2f::denoise;
    if (!black || !out || !side_ok(H) || !side_ok(W) || maximum < 1 || maximum > 65535) return R2F_EINVAL;
    if (!(threshold > 0.0 && threshold <= (double)kMaxThreshold)) return R2F_EINVAL;
    r2f_denoise_params p{};
    for (int k = 0; k < 4; ++k) {
        const double b = black[k];
        if (!(b >= 0.0 && b <= 65535.0) || b != std::floor(b)) return R2F_EINVAL;
        p.black[k] = (int32_t)b;
    }
    p.shift = shift_of(maximum);
    p.threshold = (float)threshold;
    if (!params_ok(p.black, p.shift, p.threshold)) return R2F_EINVAL;  // (a threshold that rounds to 0 as a float)
    *out = p;
    return R2F_OK;
}

size_t r2f_mosaic_denoise_workspace_bytes(int H, int W) {
    using namespace r2f::denoise;
    if (!side_ok(H) || !side_ok(W)) return 0;
    return (size_t)12 * (size_t)H * (size_t)W;
}

}  // extern "C"
