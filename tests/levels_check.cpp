// levels_check.cpp -- r2f_raw_scale_plan (raw2film_amd/csrc/r2f_levels_plan.cpp) in a stand-alone program, built by
// tests/test_levels_host.py with g++ -fsanitize=address,undefined,float-cast-overflow -ffp-contract=off.
//   levels_check sweep JOB   every line of JOB is a case: wb0 wb1 wb2 white_level thr d n_black black... (doubles as C99 hex
//                            floats or decimals, d and n_black as integers, white_level as an integer of any size: one outside
//                            int32 is a refusal of the caller's, printed as such).  One line out per case: "rc mul0 mul1 mul2
//                            maximum_used adjusted", the multipliers as hex floats; "rc" alone for a refusal -- after the program
//                            has checked that the refusal left *out alone.
//   levels_check fuzz SEED N N random cases, hostile values among them (NaN, infinities, huge and negative numbers): the planner
//                            answers R2F_OK or R2F_EINVAL, an OK result has multipliers of at least 1 (wb / min(wb) >= 1 and 65535 / m_eff
//                            >= 1; a huge white balance may reach infinity, which the demosaic planners refuse) and a maximum in
//                            [1, 65535], a refusal leaves *out alone.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "../include/r2f.h"

namespace {

const r2f_raw_scale kSentinel = {{-1.5, -2.5, -3.5}, -77, -88};

bool untouched(const r2f_raw_scale& s) { return std::memcmp(&s, &kSentinel, sizeof s) == 0; }

int sweep(const char* path) {
    std::ifstream in(path);
    if (!in) return std::fprintf(stderr, "cannot read %s\n", path), 2;
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        std::string tok[6];
        for (auto& t : tok) ss >> t;
        r2f_raw_levels lv{};
        for (int c = 0; c < 3; ++c) lv.white_balance[c] = std::strtod(tok[c].c_str(), nullptr);
        const long long white = std::strtoll(tok[3].c_str(), nullptr, 10);
        lv.adjust_maximum_thr = std::strtod(tok[4].c_str(), nullptr);
        const unsigned long d = std::strtoul(tok[5].c_str(), nullptr, 10);
        int n = 0;
        ss >> n;
        std::vector<double> black((size_t)(n > 0 ? n : 0));
        for (auto& b : black) {
            std::string t;
            ss >> t;
            b = std::strtod(t.c_str(), nullptr);
        }
        if (!ss) return std::fprintf(stderr, "short line: %s\n", line.c_str()), 2;
        r2f_raw_scale out = kSentinel;
        int rc = R2F_EINVAL;
        if (white >= INT32_MIN && white <= INT32_MAX) {
            lv.white_level = (int32_t)white;
            rc = r2f_raw_scale_plan(&lv, black.data(), n, (uint32_t)d, &out);
        }
        if (rc != R2F_OK) {
            if (!untouched(out)) return std::fprintf(stderr, "a refusal wrote *out: %s\n", line.c_str()), 1;
            std::printf("%d\n", rc);
        } else {
            std::printf("%d %a %a %a %d %d\n", rc, out.mul[0], out.mul[1], out.mul[2], out.maximum_used, out.adjusted);
        }
    }
    return 0;
}

int fuzz(unsigned seed, long n) {
    std::mt19937_64 rng(seed);
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double hostile[] = {nan, inf, -inf, 0.0, -0.0, -1.0, 1e300, -1e300, 1e-320, 65535.0, 65536.0, 0.5, 4294967296.0, 0.00001, 0.99999};
    auto number = [&](double lo, double hi) {
        if (rng() % 8 == 0) return hostile[rng() % (sizeof hostile / sizeof *hostile)];
        return lo + (hi - lo) * (double)(rng() % 1000001) / 1e6;
    };
    long ok = 0;
    for (long i = 0; i < n; ++i) {
        r2f_raw_levels lv{};
        for (double& w : lv.white_balance) w = number(0.1, 8.0);
        lv.white_level = rng() % 8 == 0 ? (int32_t)rng() : (int32_t)(rng() % 70000);
        lv.adjust_maximum_thr = number(0.0, 1.0);
        const int n_black = rng() % 16 == 0 ? (int)(rng() % 40) : (rng() % 2 ? 4 : 36);
        std::vector<double> black((size_t)n_black);
        const double base = std::floor(number(0.0, 4096.0));
        for (double& b : black) b = rng() % 16 == 0 ? number(0.0, 70000.0) : base + (double)(rng() % 64);
        const uint32_t d = rng() % 8 == 0 ? (uint32_t)rng() : (uint32_t)(rng() % 65536);
        r2f_raw_scale out = kSentinel;
        const int rc = r2f_raw_scale_plan(&lv, black.data(), n_black, d, &out);
        if (rc == R2F_OK) {
            ++ok;
            for (double m : out.mul)
                if (!(m >= 1.0)) return std::fprintf(stderr, "case %ld: multiplier %g\n", i, m), 1;
            if (out.maximum_used < 1 || out.maximum_used > 65535 || (out.adjusted != 0 && out.adjusted != 1) ||
                (out.adjusted && (uint32_t)out.maximum_used != d))
                return std::fprintf(stderr, "case %ld: maximum %d, adjusted %d\n", i, out.maximum_used, out.adjusted), 1;
        } else if (rc != R2F_EINVAL || !untouched(out)) {
            return std::fprintf(stderr, "case %ld: rc %d, *out %s\n", i, rc, untouched(out) ? "untouched" : "written"), 1;
        }
    }
    if (r2f_raw_scale_plan(nullptr, nullptr, 4, 0, nullptr) != R2F_EINVAL) return std::fprintf(stderr, "null pointers were taken\n"), 1;
    std::printf("%ld cases ok (%ld planned)\n", n, ok);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 3 && !std::strcmp(argv[1], "sweep")) return sweep(argv[2]);
    if (argc == 4 && !std::strcmp(argv[1], "fuzz")) return fuzz((unsigned)std::strtoul(argv[2], nullptr, 10), std::strtol(argv[3], nullptr, 10));
    std::fprintf(stderr, "usage: levels_check sweep JOB | fuzz SEED N\n");
    return 2;
}
