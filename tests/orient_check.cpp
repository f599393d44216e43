// orient_check.cpp -- the index map of the oriented demosaic (raw2film_amd/csrc/r2f_mosaic_math.h, namespace orient: the text the
// entry points' checks and the device kernels compile) as a stand-alone program; tests/test_orientation_host.py builds it with
// g++ -fsanitize=address,undefined and runs it.  For all 8 orientations and frames with sides 1 .. 9 plus a few ragged larger ones:
//   * to_frame is a bijection of O onto D and equals the NumPy statement of include/r2f.h, carried out here on arrays of pixel
//     numbers (mirror the rows, mirror the columns, transpose -- no index arithmetic shared with the header); from_frame inverts it
//   * for every [y0, y1) (the larger frames: every pair of a set of cuts) rect_of's rectangle of D holds exactly the pixels of those
//     rows of O
//   * source_rows names the mosaic rows of the contract: those of the rectangle's rows of D by the upright rule (written out here),
//     every row with the axes swapped
// Prints "orient_check: N cases ok"; any failure prints what differed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../raw2film_amd/csrc/r2f_mosaic_math.h"

using namespace r2f;

namespace {

[[noreturn]] void die(const char* what, int o, int h, int w, int a, int b) {
    fprintf(stderr, "orient_check: %s (orientation %d, frame %d x %d, %d, %d)\n", what, o, h, w, a, b);
    exit(1);
}

// E of the NumPy statement, as the pixel numbers y * w + x of D: E = D; if o & 2: E = E[::-1]; if o & 1: E = E[:, ::-1];
// if o & 4: E = E.transpose(1, 0, 2).  Returns E row-major and sets its shape.
std::vector<int> numpy_statement(int o, int h, int w, int& eh, int& ew) {
    std::vector<int> e((size_t)h * w);
    for (int i = 0; i < h * w; ++i) e[i] = i;
    if (o & 2)
        for (int y = 0; y < h / 2; ++y)
            for (int x = 0; x < w; ++x) std::swap(e[(size_t)y * w + x], e[(size_t)(h - 1 - y) * w + x]);
    if (o & 1)
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w / 2; ++x) std::swap(e[(size_t)y * w + x], e[(size_t)y * w + w - 1 - x]);
    eh = h, ew = w;
    if (o & 4) {
        std::vector<int> t((size_t)h * w);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) t[(size_t)x * h + y] = e[(size_t)y * w + x];
        e.swap(t);
        eh = w, ew = h;
    }
    return e;
}

long check_frame(int o, int h, int w, const std::vector<int>& cuts) {
    long cases = 0;
    int eh, ew;
    const std::vector<int> e = numpy_statement(o, h, w, eh, ew);
    if (orient::rows(o, h, w) != eh || orient::cols(o, h, w) != ew) die("the shape of O", o, h, w, eh, ew);
    std::vector<int> row_of((size_t)h * w, -1);  // the row of O a pixel of D lands in
    std::vector<char> seen((size_t)h * w, 0);
    for (int r = 0; r < eh; ++r)
        for (int c = 0; c < ew; ++c) {
            int dy = -1, dx = -1;
            orient::to_frame(o, h, w, r, c, dy, dx);
            if (dy < 0 || dy >= h || dx < 0 || dx >= w) die("to_frame leaves D", o, h, w, r, c);
            if (dy * w + dx != e.at((size_t)r * ew + c)) die("to_frame is not the NumPy statement", o, h, w, r, c);
            if (seen[(size_t)dy * w + dx]++) die("to_frame meets a pixel twice", o, h, w, r, c);
            row_of[(size_t)dy * w + dx] = r;
            int r2 = -1, c2 = -1;
            orient::from_frame(o, h, w, dy, dx, r2, c2);
            if (r2 != r || c2 != c) die("from_frame does not invert to_frame", o, h, w, r, c);
            ++cases;
        }
    for (size_t i = 0; i < cuts.size(); ++i)
        for (size_t j = i; j < cuts.size(); ++j) {
            const int y0 = cuts[i], y1 = cuts[j];
            const orient::Rect d = orient::rect_of(o, h, w, y0, y1);
            if (d.y0 < 0 || d.y1 > h || d.x0 < 0 || d.x1 > w || d.y0 > d.y1 || d.x0 > d.x1) die("rect_of leaves D", o, h, w, y0, y1);
            if ((long)(d.y1 - d.y0) * (d.x1 - d.x0) != (long)(y1 - y0) * ew && y1 > y0) die("rect_of's area", o, h, w, y0, y1);
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) {
                    const bool in_rect = y >= d.y0 && y < d.y1 && x >= d.x0 && x < d.x1;
                    const int r = row_of[(size_t)y * w + x];
                    if (in_rect != (r >= y0 && r < y1)) die("rect_of is not the pixels of those rows of O", o, h, w, y0, y1);
                }
            if (y1 == y0) continue;
            // the contract's mosaic rows: Bayer (reach 4, halves) and X-Trans (reach 3, thirds), full size and reduced, the reduced
            // mosaic with a tail that fills no cell
            for (int k = 2; k <= 3; ++k) {
                const int reach = k == 2 ? 4 : 3;
                for (int reduced = 0; reduced < 2; ++reduced) {
                    const int H = reduced ? k * h + (k - 1) : h;
                    int want_lo, want_hi;
                    if (o & 4) {
                        want_lo = 0, want_hi = H;
                    } else {
                        const int a = o & 2 ? h - y1 : y0, b = o & 2 ? h - y0 : y1;  // the rows of D
                        if (a != d.y0 || b != d.y1 || d.x0 != 0 || d.x1 != w) die("rect_of's rows of D", o, h, w, y0, y1);
                        want_lo = reduced ? k * a : (a - reach > 0 ? a - reach : 0);
                        want_hi = reduced ? k * b : (b + reach < H ? b + reach : H);
                    }
                    int lo = -1, hi = -1;
                    orient::source_rows(o, d, H, reach, reduced ? k : 0, lo, hi);
                    if (lo != want_lo || hi != want_hi) die("source_rows is not the contract's", o, h, w, y0, y1);
                    if (lo < 0 || hi > H || lo >= hi) die("source_rows leaves the mosaic", o, h, w, lo, hi);
                    ++cases;
                }
            }
            if ((o & 4) && (d.y0 != 0 || d.y1 != h)) die("a turned call takes whole columns of D", o, h, w, y0, y1);
        }
    return cases;
}

}  // namespace

int main() {
    long cases = 0;
    for (int o = -2; o <= 9; ++o)
        if (orient::valid(o) != (o >= 0 && o <= 7)) die("valid", o, 0, 0, 0, 0);
    const int ragged[][2] = {{33, 65}, {70, 134}, {134, 70}, {23, 45}, {71, 137}};
    for (int o = 0; o < 8; ++o) {
        for (int h = 1; h <= 9; ++h)
            for (int w = 1; w <= 9; ++w) {
                std::vector<int> cuts;
                for (int y = 0; y <= orient::rows(o, h, w); ++y) cuts.push_back(y);  // every [y0, y1)
                cases += check_frame(o, h, w, cuts);
            }
        for (const auto& s : ragged) {
            const int n = orient::rows(o, s[0], s[1]);
            std::vector<int> cuts;
            for (int y : {0, 1, 5, 31, 32, 33, 64, 65, n - 1, n})
                if (y >= 0 && y <= n && (cuts.empty() || y > cuts.back())) cuts.push_back(y);
            cases += check_frame(o, s[0], s[1], cuts);
        }
    }
    printf("orient_check: %ld cases ok\n", cases);
    return 0;
}
