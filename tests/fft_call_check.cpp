// fft_call_check -- plan::fft_call (raw2film_amd/csrc/r2f_plan.cpp) walked over the cases of tests/fft_call_model.py, one line per
// case in the model's format (its `cases` and `line`): tests/test_fft_call_host.py builds this with the sanitizers and holds every
// line equal to the model's.  Test infrastructure: nothing in the product links this file.
#include <cinttypes>
#include <cstdint>
#include <cstdio>

#include "../raw2film_amd/csrc/r2f_plan.h"

using namespace r2f::plan;

static void print_case(const char* label, const FftCallIn& in) {
    const FftCall c = fft_call(in);
    if (!c.ok) {
        printf("%s : no window\n", label);
        return;
    }
    const FftBatches& b = c.b;
    uint64_t h = 0;
    for (int i = 0; i < b.launches; ++i) {
        const FftBatch t = c.batch(i);
        h = (h * 1000003u + (uint64_t)t.pair0 * 31 + (uint64_t)t.npairs * 7 + (uint64_t)t.lane * 3 + t.scratch_offset) % (1ull << 40);
    }
    const FftBatch first = c.batch(0), last = c.batch(b.launches - 1);
    printf("%s : %d %d %d %d k %d %d %d e %d %d %d t %d %d %d %d s %d %d %d %zu %zu p %.17g %.17g %.17g w %d %d %d %d %zu / %d %d %d %zu / %" PRIu64 "\n",
           label, b.ny, b.nx, b.vy, b.vx, c.kreal, c.oy, c.ox, c.element, c.elem_bytes, c.timing_offset, b.gx, b.ntiles, b.ppc, b.pairs,
           b.nstreams, b.batch, b.launches, b.img_bytes, b.scratch_bytes, c.pass_bytes[0], c.pass_bytes[1], c.pass_bytes[2], b.launches,
           first.pair0, first.npairs, first.lane, first.scratch_offset, last.pair0, last.npairs, last.lane, last.scratch_offset, h);
}

int main() {
    const Options defaults;
    char label[128];
    // 1: the facts and switches (the model's order: the last of its 13 bits runs fastest)
    const int boxes_a[2][2] = {{31, 31}, {201, 25}};
    for (const auto& box : boxes_a)
        for (int bits = 0; bits < (1 << 13); ++bits) {
            int v[13];
            for (int i = 0; i < 13; ++i) v[i] = (bits >> (12 - i)) & 1;
            const int which = v[4];
            auto mask = [&](int bit) { return (bit << which) | ((1 - bit) << (1 - which)); };
            FftCallIn in;
            in.take_options(defaults);
            in.bh = box[0], in.bw = box[1], in.ay = box[0] / 2, in.ax = box[1] / 2;
            in.nch = 2, in.which = which, in.W = 520, in.y0 = 0, in.y1 = 300;
            in.fft_s32 = mask(v[0]), in.fft_s96 = mask(v[1]);
            in.any_mixed_sign = v[2], in.fft_mixed_sign = v[3];
            in.epilogue = v[5], in.dyn = v[6], in.fft_s96_auto = v[7];
            in.symmetric = v[8], in.fft_real = v[9];
            in.all_unit_gain = v[10], in.fft_cols_walk = v[11], in.curve_set = v[12];
            int n = snprintf(label, sizeof label, "A %d %d ", box[0], box[1]);
            for (int i = 0; i < 13; ++i) label[n++] = (char)('0' + v[i]);
            label[n] = 0;
            print_case(label, in);
        }
    // 2: the geometries
    const int boxes[5][2] = {{31, 31}, {85, 85}, {35, 35}, {201, 25}, {25, 301}}, frames[2][2] = {{300, 520}, {12288, 8192}};
    const int mibs[2] = {1, 192}, streams[3] = {1, 2, 4};
    for (const auto& box : boxes)
        for (const auto& frame : frames)
            for (int rows = 0; rows < 3; ++rows)
                for (int mib : mibs)
                    for (int ns : streams)
                        for (int even = 0; even < 2; ++even)
                            for (int which = 0; which < 2; ++which) {
                                const int ranges[3][2] = {{0, frame[0]}, {40, 200}, {1058, 2116}};
                                FftCallIn in;
                                in.take_options(defaults);
                                in.fo.batch_mib = mib, in.fo.streams = ns, in.fo.even = even;
                                in.bh = box[0], in.bw = box[1], in.ay = box[0] / 2, in.ax = box[1] / 2;
                                in.nch = 3 - which, in.which = which, in.W = frame[1], in.y0 = ranges[rows][0], in.y1 = ranges[rows][1];
                                in.all_unit_gain = in.symmetric = in.dyn = in.curve_set = true;
                                in.epilogue = 1;
                                snprintf(label, sizeof label, "B %d %d %d %d %d %d %d %d %d %d", box[0], box[1], in.W, in.y0, in.y1, mib, ns, even,
                                         which, in.nch);
                                print_case(label, in);
                            }
    return 0;
}
