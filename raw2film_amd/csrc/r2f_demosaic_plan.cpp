// r2f_demosaic_plan.cpp -- host planner of the Bayer demosaic (include/r2f.h: r2f_demosaic_plan).  No HIP in this file: hipcc
// compiles it into the library, g++ -fsanitize=address,undefined,float-cast-overflow into tests/demosaic_check.cpp's program.
#include "../../include/r2f.h"
#include "r2f_mosaic_plan.h"

namespace {

// colour id (0 R, 1 G, 2 B) of site k = (y & 1) * 2 + (x & 1), per pattern
constexpr int kCfa[4][4] = {
    {0, 1, 1, 2},  // RGGB
    {2, 1, 1, 0},  // BGGR
    {1, 0, 2, 1},  // GRBG
    {1, 2, 0, 1},  // GBRG
};

}  // namespace

extern "C" {

int r2f_demosaic_plan(const r2f_raw_profile* p, int H, int W, r2f_demosaic_params* out) {
    if (!p || !out || H < 2 || W < 2) return R2F_EINVAL;
    if (p->pattern < R2F_CFA_RGGB || p->pattern > R2F_CFA_GBRG) return R2F_EINVAL;
    const bool half = p->half_size != 0;
    if (half && ((H | W) & 1)) return R2F_EINVAL;
    r2f_demosaic_params r{};
    if (!r2f::mosaic_plan::black_levels(p->black, r.black) || !r2f::mosaic_plan::multipliers(p->mul, r.mul) ||
        !r2f::mosaic_plan::matrix(p->matrix, r.M))
        return R2F_EINVAL;
    for (int k = 0; k < 4; ++k) r.cfa[k] = kCfa[p->pattern][k];
    r.half_size = half ? 1 : 0;
    r.out_h = half ? H / 2 : H;
    r.out_w = half ? W / 2 : W;
    *out = r;
    return R2F_OK;
}

}  // extern "C"
