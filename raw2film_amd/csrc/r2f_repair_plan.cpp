// r2f_repair_plan.cpp -- host planner of the hot-pixel repair of a mosaic (include/r2f.h: r2f_mosaic_repair_plan): the checks, the
// levels widened to one 6 x 6 table and the neighbour table of step N.  No HIP in this file: hipcc compiles it into the library, g++
// -fsanitize=address,undefined into tests/repair_check.cpp's program.  Nothing is converted before it has passed its check, and *out
// is written once, behind the last of them.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // (the library's build reads this file as HIP: r2f_mosaic_math.h's macro set then takes its qualifiers)
#endif
#include <cmath>

#include "../../include/r2f.h"
#include "r2f_repair_math.h"

extern "C" {

int r2f_mosaic_repair_plan(int period, const int32_t* cfa, const double* black, int threshold, int q, int min_neighbours, int H, int W,
                           r2f_repair_params* out) {
    using namespace r2f::repair;
    if (!black || !out || (period != 2 && period != kPeriod) || (period == kPeriod && !cfa)) return R2F_EINVAL;
    if (H < kMinSide || W < kMinSide || !numbers_ok(threshold, q, min_neighbours)) return R2F_EINVAL;
    r2f_repair_params p{};
    p.period = period, p.threshold = threshold, p.q = q, p.min_neighbours = min_neighbours;
    for (int i = 0; i < period * period; ++i) {
        const double b = black[i];
        if (!(b >= 0.0 && b <= 65535.0) || b != std::floor(b)) return R2F_EINVAL;
    }
    if (period == kPeriod)
        for (int i = 0; i < kPhases; ++i)
            if (cfa[i] < 0 || cfa[i] > 2) return R2F_EINVAL;
    for (int py = 0; py < kPeriod; ++py)
        for (int px = 0; px < kPeriod; ++px) {
            const int ph = py * kPeriod + px;
            p.black[ph] = (int32_t)black[(py % period) * period + px % period];
            for (int d = 0; d < 4; ++d) {
                int dy = bayer_dy(d), dx = bayer_dx(d);
                if (period == kPeriod && !xtrans_neighbour(cfa, py, px, d, dy, dx)) return R2F_EINVAL;
                p.offset[ph][d][0] = (int8_t)dy, p.offset[ph][d][1] = (int8_t)dx;
            }
        }
    *out = p;
    return R2F_OK;
}

}  // extern "C"
