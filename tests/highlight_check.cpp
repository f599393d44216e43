// highlight_check.cpp -- r2f_raw_scale_plan_highlight (raw2film_amd/csrc/r2f_levels_plan.cpp) and mosaic::blend_pixel
// (raw2film_amd/csrc/r2f_mosaic_math.h) in a stand-alone program, built by tests/test_highlight_host.py with g++
// -fsanitize=address,undefined,float-cast-overflow -ffp-contract=off.
//   highlight_check plan JOB     every line of JOB is a case: wb0 wb1 wb2 white_level thr d mode n_black black... (doubles as C99 hex
//                                floats or decimals, the rest integers).  One line out per case: "rc mul0 mul1 mul2 maximum_used
//                                adjusted mode clip", the multipliers as hex floats; "rc" alone for a refusal -- after the program has
//                                checked that the refusal left *out and *hl alone.  A mode-0 case is also held to r2f_raw_scale_plan's
//                                bytes.
//   highlight_check fuzz SEED N  N random cases, hostile values and every mode from -2 to 11 among them: R2F_OK or R2F_EINVAL; an OK
//                                result of modes 1 and 2 has its largest multiplier equal to 65535 / maximum_used and none above it,
//                                mode 2 a clip in [1, 65535] and the others 0; mode 0 is r2f_raw_scale_plan's bytes; a mode outside
//                                {0, 1, 2} is refused; a refusal leaves both outputs alone.
//   highlight_check blend        blend_pixel over the check set (below): per clip level "clip count changed digest".
//   highlight_check blend CLIP   the same set for one level, one line "v0 v1 v2 o0 o1 o2" per triple.
// The check set, which tests/test_highlight_host.py regenerates: for each clip level, every triple over its edge values (0, 1, clip - 1,
// clip, clip + 1, clip + 2, clip + clip / 2, 2 clip, 32768, 65534, 65535, clamped to [0, 65535], sorted, without repeats), then
// 20000 triples from a 64-bit LCG (x = x * 6364136223846793005 + 1442695040888963407, seeded with the clip level; a value is
// (x >> 33) % 65536; every fourth triple repeats its first value in all channels).  The digest is the sum over the set, modulo 2^64, of
// (o0 + 65536 o1 + 65536^2 o2 + 1) * (2 i + 1), i the triple's index.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "../include/r2f.h"
#include "../raw2film_amd/csrc/r2f_mosaic_math.h"

namespace {

const r2f_raw_scale kSentinel = {{-1.5, -2.5, -3.5}, -77, -88};
const r2f_highlight kHlSentinel = {-55, -66};
const int kClips[] = {1, 2, 255, 4096, 31207, 40000, 65534, 65535};

bool untouched(const r2f_raw_scale& s, const r2f_highlight& h) {
    return std::memcmp(&s, &kSentinel, sizeof s) == 0 && std::memcmp(&h, &kHlSentinel, sizeof h) == 0;
}

// mode 0 against the plain planner: the same answer, the same bytes
bool same_as_plain(const r2f_raw_levels& lv, const double* black, int n, uint32_t d, int rc, const r2f_raw_scale& out, const r2f_highlight& hl) {
    r2f_raw_scale plain = kSentinel;
    const int rc_plain = r2f_raw_scale_plan(&lv, black, n, d, &plain);
    if (rc != rc_plain) return false;
    return rc != R2F_OK || (std::memcmp(&plain, &out, sizeof out) == 0 && hl.mode == 0 && hl.clip == 0);
}

int plan(const char* path) {
    std::ifstream in(path);
    if (!in) return std::fprintf(stderr, "cannot read %s\n", path), 2;
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        std::string tok[7];
        for (auto& t : tok) ss >> t;
        r2f_raw_levels lv{};
        for (int c = 0; c < 3; ++c) lv.white_balance[c] = std::strtod(tok[c].c_str(), nullptr);
        lv.white_level = (int32_t)std::strtol(tok[3].c_str(), nullptr, 10);
        lv.adjust_maximum_thr = std::strtod(tok[4].c_str(), nullptr);
        const unsigned long d = std::strtoul(tok[5].c_str(), nullptr, 10);
        const int mode = (int)std::strtol(tok[6].c_str(), nullptr, 10);
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
        r2f_highlight hl = kHlSentinel;
        const int rc = r2f_raw_scale_plan_highlight(&lv, black.data(), n, (uint32_t)d, mode, &out, &hl);
        if (mode == 0 && !same_as_plain(lv, black.data(), n, (uint32_t)d, rc, out, hl))
            return std::fprintf(stderr, "mode 0 is not r2f_raw_scale_plan: %s\n", line.c_str()), 1;
        if (rc != R2F_OK) {
            if (!untouched(out, hl)) return std::fprintf(stderr, "a refusal wrote an output: %s\n", line.c_str()), 1;
            std::printf("%d\n", rc);
        } else {
            std::printf("%d %a %a %a %d %d %d %d\n", rc, out.mul[0], out.mul[1], out.mul[2], out.maximum_used, out.adjusted, hl.mode, hl.clip);
        }
    }
    return 0;
}

int fuzz(unsigned seed, long n) {
    std::mt19937_64 rng(seed);
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double hostile[] = {nan, inf, -inf, 0.0, -0.0, -1.0, 1e300, -1e300, 1e-320, 1e-6, 65535.0, 65536.0, 0.5, 1024.0, 70000.0};
    auto number = [&](double lo, double hi) {
        if (rng() % 8 == 0) return hostile[rng() % (sizeof hostile / sizeof *hostile)];
        return lo + (hi - lo) * (double)(rng() % 1000001) / 1e6;
    };
    long ok = 0, blends = 0;
    for (long i = 0; i < n; ++i) {
        r2f_raw_levels lv{};
        for (double& w : lv.white_balance) w = number(0.1, 8.0);
        if (rng() % 8 == 0) lv.white_balance[1] = lv.white_balance[2] = lv.white_balance[0];  // equal in all channels
        lv.white_level = rng() % 8 == 0 ? (int32_t)rng() : (int32_t)(rng() % 70000);
        lv.adjust_maximum_thr = number(0.0, 1.0);
        const int n_black = rng() % 16 == 0 ? (int)(rng() % 40) : (rng() % 2 ? 4 : 36);
        std::vector<double> black((size_t)n_black);
        const double base = std::floor(number(0.0, 4096.0));
        for (double& b : black) b = rng() % 16 == 0 ? number(0.0, 70000.0) : base + (double)(rng() % 64);
        const uint32_t d = rng() % 8 == 0 ? (uint32_t)rng() : (uint32_t)(rng() % 65536);
        const int mode = rng() % 16 == 0 ? (int)rng() : (int)(rng() % 14) - 2;
        r2f_raw_scale out = kSentinel;
        r2f_highlight hl = kHlSentinel;
        const int rc = r2f_raw_scale_plan_highlight(&lv, black.data(), n_black, d, mode, &out, &hl);
        if (mode == 0 && !same_as_plain(lv, black.data(), n_black, d, rc, out, hl))
            return std::fprintf(stderr, "case %ld: mode 0 is not r2f_raw_scale_plan\n", i), 1;
        if (rc == R2F_OK) {
            ++ok;
            if (mode < 0 || mode > 2 || hl.mode != mode) return std::fprintf(stderr, "case %ld: mode %d planned as %d\n", i, mode, hl.mode), 1;
            if (out.maximum_used < 1 || out.maximum_used > 65535 || (out.adjusted != 0 && out.adjusted != 1) ||
                (out.adjusted && (uint32_t)out.maximum_used != d))
                return std::fprintf(stderr, "case %ld: maximum %d, adjusted %d\n", i, out.maximum_used, out.adjusted), 1;
            if (mode != 0) {
                const double top = 65535.0 / (double)out.maximum_used;  // (w / w is exactly 1 for a finite w > 0)
                double largest = 0.0;
                for (double m : out.mul) {
                    if (!(m >= 0.0 && m <= top)) return std::fprintf(stderr, "case %ld: multiplier %g above %g\n", i, m, top), 1;
                    largest = m > largest ? m : largest;
                }
                if (largest != top) return std::fprintf(stderr, "case %ld: the largest multiplier is %g, not %g\n", i, largest, top), 1;
            }
            if (mode == 2 ? (hl.clip < 1 || hl.clip > 65535) : hl.clip != 0) return std::fprintf(stderr, "case %ld: clip %d\n", i, hl.clip), 1;
            blends += mode == 2;
        } else if (rc != R2F_EINVAL || !untouched(out, hl)) {
            return std::fprintf(stderr, "case %ld: rc %d, outputs %s\n", i, rc, untouched(out, hl) ? "untouched" : "written"), 1;
        }
    }
    r2f_raw_levels lv{{2.0, 1.0, 1.5}, 16383, 0.75};
    const double black[4] = {512, 512, 512, 512};
    r2f_raw_scale out = kSentinel;
    r2f_highlight hl = kHlSentinel;
    if (r2f_raw_scale_plan_highlight(&lv, black, 4, 0, 2, nullptr, &hl) != R2F_EINVAL || r2f_raw_scale_plan_highlight(&lv, black, 4, 0, 2, &out, nullptr) != R2F_EINVAL ||
        r2f_raw_scale_plan_highlight(nullptr, black, 4, 0, 2, &out, &hl) != R2F_EINVAL || !untouched(out, hl))
        return std::fprintf(stderr, "null pointers were taken\n"), 1;
    std::printf("%ld cases ok (%ld planned, %ld with a clip level)\n", n, ok, blends);
    return 0;
}

std::vector<int> check_set(int clip) {  // v0 v1 v2 of every triple, one after the other
    std::vector<int> edge;
    for (long long v : {0LL, 1LL, clip - 1LL, (long long)clip, clip + 1LL, clip + 2LL, clip + clip / 2LL, 2LL * clip, 32768LL, 65534LL, 65535LL})
        edge.push_back((int)std::min(std::max(v, 0LL), 65535LL));
    std::sort(edge.begin(), edge.end());
    edge.erase(std::unique(edge.begin(), edge.end()), edge.end());
    std::vector<int> set;
    for (int a : edge)
        for (int b : edge)
            for (int c : edge) set.insert(set.end(), {a, b, c});
    uint64_t x = (uint64_t)clip;
    auto next = [&] {
        x = x * 6364136223846793005ULL + 1442695040888963407ULL;
        return (int)((x >> 33) % 65536);
    };
    for (int i = 0; i < 20000; ++i) {
        const int a = next(), b = next(), c = next();
        if (i % 4 == 3)
            set.insert(set.end(), {a, a, a});
        else
            set.insert(set.end(), {a, b, c});
    }
    return set;
}

int blend(int only) {
    for (int clip : kClips) {
        if (only && clip != only) continue;
        const std::vector<int> set = check_set(clip);
        uint64_t digest = 0;
        long changed = 0;
        for (size_t i = 0; i < set.size() / 3; ++i) {
            int v[3] = {set[3 * i], set[3 * i + 1], set[3 * i + 2]};
            r2f::mosaic::blend_pixel(v, clip);
            for (int c = 0; c < 3; ++c)
                if (v[c] < 0 || v[c] > 65535) return std::fprintf(stderr, "clip %d triple %zu: channel %d left as %d\n", clip, i, c, v[c]), 1;
            const bool above = set[3 * i] > clip || set[3 * i + 1] > clip || set[3 * i + 2] > clip;
            const bool moved = v[0] != set[3 * i] || v[1] != set[3 * i + 1] || v[2] != set[3 * i + 2];
            if (!above && moved) return std::fprintf(stderr, "clip %d triple %zu: a pixel with no channel above clip changed\n", clip, i), 1;
            changed += moved;
            if (only) std::printf("%d %d %d %d %d %d\n", set[3 * i], set[3 * i + 1], set[3 * i + 2], v[0], v[1], v[2]);
            digest += ((uint64_t)v[0] + 65536ULL * (uint64_t)v[1] + 65536ULL * 65536ULL * (uint64_t)v[2] + 1ULL) * (2ULL * i + 1ULL);
        }
        if (!only) std::printf("%d %zu %ld %llu\n", clip, set.size() / 3, changed, (unsigned long long)digest);
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 3 && !std::strcmp(argv[1], "plan")) return plan(argv[2]);
    if (argc == 4 && !std::strcmp(argv[1], "fuzz")) return fuzz((unsigned)std::strtoul(argv[2], nullptr, 10), std::strtol(argv[3], nullptr, 10));
    if (argc == 2 && !std::strcmp(argv[1], "blend")) return blend(0);
    if (argc == 3 && !std::strcmp(argv[1], "blend")) return blend((int)std::strtol(argv[2], nullptr, 10));
    std::fprintf(stderr, "usage: highlight_check plan JOB | fuzz SEED N | blend [CLIP]\n");
    return 2;
}
