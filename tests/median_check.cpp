// median_check.cpp -- the arithmetic of step M (raw2film_amd/csrc/r2f_median_math.h: median::median9 and median::pass_pixel) in a
// stand-alone program, built by tests/test_median_host.py with g++ -fsanitize=address,undefined.
//   median_check network        median9 on all 512 inputs of zeros and ones.  A network of exchanges that selects the median of
//                               every zero-one input selects it of every input (the zero-one principle: an exchange commutes with
//                               any monotone map of the values).  Prints "512 ok".
//   median_check random SEED N  N inputs of nine ints with ties (values from a range of 1, 3, 17 or 131071 around a random centre
//                               in [-65535, 65535]): median9 against std::nth_element.  Prints "N ok".
//   median_check clamp          pass_pixel on constant planes: a difference that takes the sum below 0 or above 65535 is clamped
//                               there, the ends themselves pass, and red and blue are filtered independently.  Prints "clamp ok".
//   median_check planes H W SEED N   N passes over random H x W planes (one of five levels per sample, as the GPU tests' clamp
//                               fixture); prints the planes of I_0 and I_N, one row of 3 W integers per line: the host test holds
//                               them to the NumPy model.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../raw2film_amd/csrc/r2f_median_math.h"

namespace {

using r2f::median::median9;
using r2f::median::pass_pixel;

int reference_median(const int (&v)[9]) {
    int w[9];
    std::copy(v, v + 9, w);
    std::nth_element(w, w + 4, w + 9);
    return w[4];
}

int network() {
    for (int bits = 0; bits < 512; ++bits) {
        int v[9], ones = 0;
        for (int i = 0; i < 9; ++i) v[i] = (bits >> i) & 1, ones += v[i];
        const int got = median9(v);
        if (got != (ones >= 5)) return std::fprintf(stderr, "input %d: median %d\n", bits, got), 1;
    }
    std::printf("512 ok\n");
    return 0;
}

int random_inputs(uint64_t seed, int n) {
    std::mt19937_64 rng(seed);
    const int spans[] = {1, 3, 17, 131071};
    for (int k = 0; k < n; ++k) {
        const int span = spans[rng() % 4], centre = (int)(rng() % 131071) - 65535;
        int v[9], w[9];
        for (int i = 0; i < 9; ++i) v[i] = w[i] = std::clamp(centre + (int)(rng() % span) - span / 2, -65535, 65535);
        const int want = reference_median(w), got = median9(v);
        if (got != want) return std::fprintf(stderr, "case %d: median %d, expected %d\n", k, got, want), 1;
    }
    std::printf("%d ok\n", n);
    return 0;
}

struct Plane {
    const int* v;
    int w;
    int operator()(int y, int x) const { return v[y * w + x]; }
};

int clamp() {
    struct Case {
        int r, g_around, b, g_centre, want_r, want_b;
    };
    // the nine differences are r - g_around (b - g_around); the centre's own green differs
    const Case cases[] = {{0, 65535, 65535, 0, 0, 0},           {65535, 0, 0, 65535, 65535, 65535}, {100, 300, 300, 100, 0, 100},
                          {65000, 100, 100, 65000, 65535, 65000}, {0, 0, 65535, 0, 0, 65535},         {65535, 65535, 0, 65535, 65535, 0},
                          {5, 5, 5, 0, 0, 0},                   {5, 5, 5, 65535, 65535, 65535}};
    for (const Case& c : cases) {
        int r[9], g[9], b[9];
        std::fill(r, r + 9, c.r), std::fill(g, g + 9, c.g_around), std::fill(b, b + 9, c.b);
        g[4] = c.g_centre;  // the centre's difference is one of nine: the median is still the surrounding eight's
        int got_r, got_b;
        pass_pixel(Plane{r, 3}, Plane{b, 3}, Plane{g, 3}, 1, 1, got_r, got_b);
        if (got_r != c.want_r || got_b != c.want_b)
            return std::fprintf(stderr, "clamp case (%d, %d, %d, %d): (%d, %d), expected (%d, %d)\n", c.r, c.g_around, c.b, c.g_centre, got_r,
                                got_b, c.want_r, c.want_b),
                   1;
    }
    std::printf("clamp ok\n");
    return 0;
}

void print_planes(const std::vector<int>& r, const std::vector<int>& g, const std::vector<int>& b, int h, int w) {
    for (int y = 0; y < h; ++y) {
        for (int x = 0; x < w; ++x) std::printf("%d %d %d ", r[y * w + x], g[y * w + x], b[y * w + x]);
        std::printf("\n");
    }
}

int planes(int h, int w, uint64_t seed, int n) {
    if (h < 1 || w < 1 || h > 512 || w > 512 || n < 0 || n > 16) return 2;
    const int levels[] = {0, 40, 30000, 65000, 65535};
    std::mt19937_64 rng(seed);
    std::vector<int> r(h * w), g(h * w), b(h * w);
    for (int i = 0; i < h * w; ++i) r[i] = levels[rng() % 5], g[i] = levels[rng() % 5], b[i] = levels[rng() % 5];
    print_planes(r, g, b, h, w);
    for (int k = 0; k < n; ++k) {
        std::vector<int> r1 = r, b1 = b;  // (a border pixel is carried over)
        for (int y = 1; y < h - 1; ++y)
            for (int x = 1; x < w - 1; ++x)
                pass_pixel(Plane{r.data(), w}, Plane{b.data(), w}, Plane{g.data(), w}, y, x, r1[y * w + x], b1[y * w + x]);
        r.swap(r1), b.swap(b1);
    }
    print_planes(r, g, b, h, w);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "network")) return network();
    if (argc == 4 && !std::strcmp(argv[1], "random")) return random_inputs(std::strtoull(argv[2], nullptr, 10), std::atoi(argv[3]));
    if (argc == 2 && !std::strcmp(argv[1], "clamp")) return clamp();
    if (argc == 6 && !std::strcmp(argv[1], "planes"))
        return planes(std::atoi(argv[2]), std::atoi(argv[3]), std::strtoull(argv[4], nullptr, 10), std::atoi(argv[5]));
    std::fprintf(stderr, "usage: median_check network | random SEED N | clamp | planes H W SEED N\n");
    return 2;
}
