// r2f_xtrans_plan.cpp -- host planner of the X-Trans demosaic (include/r2f.h: r2f_xtrans_plan).  No HIP in this file: hipcc
// compiles it into the library, g++ -fsanitize=address,undefined,float-cast-overflow into tests/xtrans_check.cpp's program.
#include <cstring>

#include "../../include/r2f.h"
#include "r2f_mosaic_plan.h"

namespace r2f {

namespace xtrans {
constexpr int kRed = 0, kGreen = 1, kBlue = 2;  // (r2f_xtrans_math.h's; that header is device text and is not included here)
}
bool xtrans_tables(const uint8_t (&cfa)[36], bool reduced, r2f_xtrans_params* out);  // (declared for its callers in r2f_xtrans_math.h)

// The tables are functions of the 6 x 6 pattern taken cyclically: a frame site's neighbours within 3 samples have the phases
// this walks, wherever the site lies.
bool xtrans_tables(const uint8_t (&cfa)[36], bool reduced, r2f_xtrans_params* out) {
    int present[3] = {0, 0, 0};
    for (int i = 0; i < 36; ++i) {
        if (cfa[i] > 2) return false;
        ++present[cfa[i]];
    }
    if (!present[0] || !present[1] || !present[2]) return false;
    auto at = [&](int y, int x) { return (int)cfa[((y % 6 + 6) % 6) * 6 + (x % 6 + 6) % 6]; };
    r2f_xtrans_params& r = *out;
    memset(r.gap, 0, sizeof r.gap), memset(r.taps, 0, sizeof r.taps), memset(r.wsum, 0, sizeof r.wsum);
    memset(r.recip, 0, sizeof r.recip), memset(r.cell_count, 0, sizeof r.cell_count);
    for (int y = 0; y < 6; ++y)
        for (int x = 0; x < 6; ++x) {
            const int ph = y * 6 + x, c0 = at(y, x);
            if (c0 != xtrans::kGreen) {  // B1: the nearest green on each side along h, then along v
                const int dir[4][2] = {{0, -1}, {0, 1}, {-1, 0}, {1, 0}};
                for (int k = 0; k < 4; ++k) {
                    int d = 1;
                    while (d <= 2 && at(y + d * dir[k][0], x + d * dir[k][1]) != xtrans::kGreen) ++d;
                    if (d > 2) return false;
                    r.gap[ph][k] = (uint8_t)d;
                }
            }
            for (int slot = 0; slot < 2; ++slot) {  // B2: the sites of red (slot 0) and blue (slot 1) in the centred 3 x 3
                const int c = slot ? xtrans::kBlue : xtrans::kRed;
                if (c == c0) continue;
                int mask = 0, w = 0;
                for (int k = 0; k < 9; ++k)
                    if (k != 4 && at(y + k / 3 - 1, x + k % 3 - 1) == c) mask |= 1 << k, w += (k & 1) ? 2 : 1;
                if (!w) return false;
                r.taps[ph][slot] = (uint16_t)mask;
                r.wsum[ph][slot] = (uint8_t)w;
                r.recip[ph][slot] = w > 1 ? (uint32_t)(0x100000000ull / (unsigned)w) + 1u : 0u;
            }
            if (c0 != xtrans::kGreen) {  // the centred 3 x 3 holds green too (B1's gaps may both be 2: that alone does not say so)
                bool green = false;
                for (int k = 0; k < 9; ++k) green = green || (k != 4 && at(y + k / 3 - 1, x + k % 3 - 1) == xtrans::kGreen);
                if (!green) return false;
            }
        }
    for (int cell = 0; cell < 4; ++cell) {
        for (int k = 0; k < 9; ++k) ++r.cell_count[cell][at(3 * (cell >> 1) + k / 3, 3 * (cell & 1) + k % 3)];
        if (reduced && !(r.cell_count[cell][0] && r.cell_count[cell][1] && r.cell_count[cell][2])) return false;
    }
    return true;
}

}  // namespace r2f

extern "C" {

int r2f_xtrans_plan(const r2f_xtrans_profile* p, int H, int W, r2f_xtrans_params* out) {
    if (!p || !out || H < 6 || W < 6) return R2F_EINVAL;
    r2f_xtrans_params r;
    memset(&r, 0, sizeof r);
    for (int i = 0; i < 36; ++i) {
        if (p->pattern[i] < 0 || p->pattern[i] > 2) return R2F_EINVAL;
        r.cfa[i] = (uint8_t)p->pattern[i];
    }
    const bool reduced = p->reduced != 0;
    if (!r2f::mosaic_plan::black_levels(p->black, r.black) || !r2f::xtrans_tables(r.cfa, reduced, &r) ||
        !r2f::mosaic_plan::multipliers(p->mul, r.mul) || !r2f::mosaic_plan::matrix(p->matrix, r.M))
        return R2F_EINVAL;
    r.reduced = reduced ? 1 : 0;
    r.out_h = reduced ? H / 3 : H;
    r.out_w = reduced ? W / 3 : W;
    *out = r;
    return R2F_OK;
}

}  // extern "C"
