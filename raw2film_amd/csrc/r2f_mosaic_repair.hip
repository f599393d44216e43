// r2f_mosaic_repair.hip -- the repair of hot pixels of a mosaic (include/r2f.h: r2f_mosaic_repair; r2f_repair_math.h has steps N, T and
// H): one more read and write of a mosaic's 2 bytes per sample, ahead of everything else that reads it.  One kernel family (period 2
// and period 6), its arguments and its entry point.
//   The grid is mosaic_max_kernel's: resident (8 blocks of 4 waves a CU), walking groups of kRows rows, a wave per row.  A lane loads
//   kVec samples as one 16-byte word behind the source row's head and ahead of its tail, which are one 16-bit load and store a lane;
//   the word leaves as one 16-byte store where the destination row is aligned like the source row, else as eight 16-bit stores of the
//   same samples.
//   Step T and the threshold test of a word are mosaic_max_kernel's packed pairs (v_pk_sub_u16 with clamp, v_pk_max_u16) with the
//   same three registers of levels per row.  A word whose largest t does not exceed the threshold is stored as it was loaded.  Only
//   the others walk their eight samples through r2f_repair_math.h's repair_sample, which fetches the four neighbours of a candidate
//   as 16-bit loads FROM THE CACHE: rows y - 2 .. y + 2 are rows that this block's other waves and the next block stream through the
//   same L2 at the same time.  No neighbour row is staged in LDS -- the candidates are sparse wherever the step is of use, and a
//   staged row would cost every word an LDS round trip to spare a few candidates a cache hit.  By design a launch moves 2 bytes in and
//   2 bytes out per sample across the memory bus.
//   Period 2 has its offsets as compile-time constants (BayerOffsets); period 6 keeps the per-phase table in LDS.  Both keep the 36
//   levels there (a 2 x 2 table arrives widened to 6 x 6).
//   A lane keeps one vector in flight ahead of the one it works on.
//   LDS: 144 bytes of levels, 288 of offsets (period 6), 16 of wave counts.
#include "r2f_ctx.h"
#include "r2f_repair_math.h"

using namespace r2f;

namespace r2f {
namespace {

constexpr int kVec = 8, kRows = 4, kPeriod = repair::kPeriod, kPhases = repair::kPhases;
static_assert(R2F_MOSAIC_REPAIR_VEC == kVec && R2F_MOSAIC_REPAIR_ROWS == kRows, "include/r2f.h states the access width and the rows per step");
static_assert((64 * kVec) % kPeriod == 2 && kVec % 2 == 0, "a lane's next vector starts one pair of sites further along the period");

struct RepairArgs {
    const uint16_t* src;  // row src_gy0 of the mosaic
    int src_gy0;
    long long spitch;  // samples
    uint16_t* dst;     // row 0 of the repaired mosaic
    long long dpitch;
    int H, W;
    int y0, y1;  // the frame rows this call writes
    uint32_t* count;
    int threshold, q, min_neighbours;
    int32_t black[kPhases];     // per phase (y % 6) * 6 + x % 6
    int8_t off[kPhases][4][2];  // per phase and quadrant: (dy, dx)
};

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u16x2 t_pair(uint32_t word, u16x2 q) { return __builtin_elementwise_sub_sat(__builtin_bit_cast(u16x2, word), q); }

// What a sample's slow path needs of the launch, by value: the source window, the frame, the three numbers and the tables in LDS.
struct Frame {
    const uint16_t* src;
    long long spitch;
    int src_gy0, H, W, threshold, q, min_neighbours;
    const int32_t* black;
    const int8_t (*offsets)[4][2];
    __device__ __forceinline__ int operator()(int yy, int xx) const { return (int)src[(long long)(yy - src_gy0) * spitch + xx]; }
};

// the output sample at (y, x): the two call sites below are the only expansions of repair_sample in an instance
template <int P>
__device__ __forceinline__ unsigned fix(const Frame& f, int y, int x, unsigned raw, int& replaced) {
    if (P == kPeriod)
        return (unsigned)repair::repair_sample(f, repair::TableOffsets{f.offsets}, (int)raw, f.H, f.W, y, x, f.black, f.threshold, f.q,
                                               f.min_neighbours, &replaced);
    return (unsigned)repair::repair_sample(f, repair::BayerOffsets{}, (int)raw, f.H, f.W, y, x, f.black, f.threshold, f.q, f.min_neighbours,
                                           &replaced);
}

template <int P>
__global__ __launch_bounds__(64 * kRows) void mosaic_repair_kernel(const RepairArgs a) {
    __shared__ int32_t s_black[kPhases];
    __shared__ int8_t s_off[P == kPeriod ? kPhases : 1][4][2];
    __shared__ unsigned s_wave[kRows];
    const int lane = threadIdx.x, wave = threadIdx.y, tid = wave * 64 + lane;
    if (tid < kPhases) {
        s_black[tid] = a.black[tid];
        if (P == kPeriod)
            for (int d = 0; d < 4; ++d) s_off[tid][d][0] = a.off[tid][d][0], s_off[tid][d][1] = a.off[tid][d][1];
    }
    __syncthreads();
    int replaced = 0;
    const Frame f{a.src, a.spitch, a.src_gy0, a.H, a.W, a.threshold, a.q, a.min_neighbours, s_black, s_off};
    const unsigned thr = (unsigned)a.threshold;
    const int W = a.W, y0 = a.y0, y1 = a.y1;
    const int groups = (y1 - y0 + kRows - 1) / kRows;
    for (int g = blockIdx.x; g < groups; g += gridDim.x) {
        const int y = y0 + g * kRows + wave;  // (the same for all 64 lanes of a wave; the phase is the frame row's)
        if (y >= y1) continue;
        const uint16_t* row = a.src + (long long)(y - a.src_gy0) * a.spitch;
        uint16_t* drow = a.dst + (long long)y * a.dpitch;
        const int32_t* b = s_black + (y % kPeriod) * kPeriod;
        int head = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u) >> 1;
        head = head < W ? head : W;
        const int nvec = (W - head) / kVec, tail = head + nvec * kVec + lane;
#pragma unroll 1
        for (int k = 0; k < 2; ++k) {  // the head's sample of this lane, then the tail's
            const int x = k ? tail : lane;
            if (k ? tail < W : lane < head) drow[x] = (uint16_t)fix<P>(f, y, x, row[x], replaced);
        }
        const int s = (head + kVec * lane) % kPeriod;  // the phase of this lane's first vector
        u16x2 q0 = {(uint16_t)b[s], (uint16_t)b[(s + 1) % kPeriod]}, q1 = {(uint16_t)b[(s + 2) % kPeriod], (uint16_t)b[(s + 3) % kPeriod]},
              q2 = {(uint16_t)b[(s + 4) % kPeriod], (uint16_t)b[(s + 5) % kPeriod]};
        const uint4* vec = reinterpret_cast<const uint4*>(row + head);  // 16-byte aligned: vectors [0, nvec) lie inside the row
        const bool wide = (reinterpret_cast<uintptr_t>(drow + head) & 15u) == 0;
        // One vector a step, the next one loaded ahead of this one's work.  A lane's next vector starts 512 columns on, 2 modulo 6:
        // its pairs of levels are the former ones moved up by one.
        int i = lane;
        uint4 next = i < nvec ? vec[i] : make_uint4(0, 0, 0, 0);
#pragma unroll 1
        for (; i < nvec; i += 64) {
            uint4 v = next;
            if (i + 64 < nvec) next = vec[i + 64];
            // T and the threshold test on packed pairs; a vector with a candidate walks its eight samples one by one, each taken from
            // the low half of v.x while the 128 bits turn right by 16 and the result enters at the top: eight turns put them in place
            const u16x2 m = __builtin_elementwise_max(__builtin_elementwise_max(t_pair(v.x, q0), t_pair(v.y, q1)),
                                                      __builtin_elementwise_max(t_pair(v.z, q2), t_pair(v.w, q0)));
            if (m.x > thr || m.y > thr) {
                const int x0 = head + kVec * i;
#pragma unroll 1
                for (int j = 0; j < kVec; ++j) {
                    const unsigned out = fix<P>(f, y, x0 + j, v.x & 0xffffu, replaced);
                    v.x = (v.x >> 16) | (v.y << 16), v.y = (v.y >> 16) | (v.z << 16), v.z = (v.z >> 16) | (v.w << 16), v.w = (v.w >> 16) | (out << 16);
                }
            }
            uint16_t* p = drow + head + kVec * i;  // samples [head + 8 i, head + 8 i + 8) of the row: inside [0, W)
            if (wide) {
                *reinterpret_cast<uint4*>(p) = v;
            } else {  // a destination row that is not aligned like the source row: the same samples, 16 bits at a time
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) p[2 * j] = (uint16_t)(w[j] & 0xffffu), p[2 * j + 1] = (uint16_t)(w[j] >> 16);
            }
            const u16x2 t = q0;
            q0 = q1, q1 = q2, q2 = t;
        }
    }
    if (!a.count) return;  // (uniform: nothing below is reached by some lanes only)
    for (int off = 32; off > 0; off >>= 1) replaced += __shfl_xor(replaced, off, 64);
    if (lane == 0) s_wave[wave] = (unsigned)replaced;
    __syncthreads();
    if (tid == 0) {
        unsigned n = 0;
        for (int w = 0; w < kRows; ++w) n += s_wave[w];
        if (n) atomicAdd(a.count, n);  // (a block that replaced nothing leaves the word alone)
    }
}

bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + nb && b0 < a0 + na;
}

}  // namespace
}  // namespace r2f

// =============================================================================== C ABI
extern "C" {

int r2f_mosaic_repair(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W,
                      const r2f_repair_params* params, uint16_t* dst, int64_t dst_pitch, int y0, int y1, uint32_t* count, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    const char* what = "mosaic_repair";
    if (!src_rows || !params || !dst) return fail(ctx, R2F_EINVAL, "%s: the mosaic rows, the params and the destination are required", what);
    if (H < repair::kMinSide || W < repair::kMinSide || src_pitch < W || dst_pitch < W || src_gy0 < 0 || src_nrows < 0)
        return fail(ctx, R2F_EINVAL, "%s: a mosaic of at least %d x %d samples, pitches of at least W and a source window are required", what,
                    repair::kMinSide, repair::kMinSide);
    if (y0 < 0 || y1 > H || y0 > y1) return fail(ctx, R2F_EINVAL, "%s: rows [%d, %d) not inside the mosaic's [0, %d)", what, y0, y1, H);
    const int P = params->period;
    if ((P != 2 && P != kPeriod) || !repair::numbers_ok(params->threshold, params->q, params->min_neighbours))
        return fail(ctx, R2F_EINVAL, "%s: params the planner does not produce (a period of 2 or 6, a threshold in [0, 65535], q in [1, 255], 3 or 4 neighbours)", what);
    RepairArgs a{src_rows, src_gy0, (long long)src_pitch, dst, (long long)dst_pitch, H, W, y0, y1, count, params->threshold, params->q,
                 params->min_neighbours, {}, {}};
    for (int ph = 0; ph < kPhases; ++ph) {
        if (params->black[ph] < 0 || params->black[ph] > 65535) return fail(ctx, R2F_EINVAL, "%s: black level %d outside [0, 65535]", what, params->black[ph]);
        a.black[ph] = params->black[ph];
        for (int d = 0; d < 4; ++d) {
            const int dy = params->offset[ph][d][0], dx = params->offset[ph][d][1];
            if (!repair::offset_ok(dy, dx) || (P == 2 && (dy != repair::bayer_dy(d) || dx != repair::bayer_dx(d))))
                return fail(ctx, R2F_EINVAL, "%s: neighbour (%d, %d) of phase %d is not one the planner produces", what, dy, dx, ph);
            a.off[ph][d][0] = (int8_t)dy, a.off[ph][d][1] = (int8_t)dx;
        }
    }
    if (y0 == y1) return R2F_OK;
    const int r0 = y0 - repair::kReach > 0 ? y0 - repair::kReach : 0, r1 = y1 + repair::kReach < H ? y1 + repair::kReach : H;
    if (r0 < src_gy0 || (long long)r1 > (long long)src_gy0 + src_nrows)
        return fail(ctx, R2F_EINVAL, "%s: rows [%d, %d) are read, the source window holds [%d, %lld)", what, r0, r1, src_gy0,
                    (long long)src_gy0 + src_nrows);
    const size_t read_bytes = ((size_t)(r1 - r0 - 1) * (size_t)src_pitch + W) * 2, written_bytes = ((size_t)(y1 - y0 - 1) * (size_t)dst_pitch + W) * 2;
    if (ranges_overlap(src_rows + (long long)(r0 - src_gy0) * src_pitch, read_bytes, dst + (long long)y0 * dst_pitch, written_bytes))
        return fail(ctx, R2F_EINVAL, "%s: the rows read and the rows written overlap (the step is out of place)", what);
    int cus = 0;
    if (const int rc = device_cu_count(ctx, &cus)) return rc;
    const int groups = (y1 - y0 + kRows - 1) / kRows, resident = 8 * cus;
    const dim3 grid(groups < resident ? groups : resident), block(64, kRows);
    if (P == 2)
        launch_k(mosaic_repair_kernel<2>, grid, block, 0, static_cast<hipStream_t>(stream), a);
    else
        launch_k(mosaic_repair_kernel<kPeriod>, grid, block, 0, static_cast<hipStream_t>(stream), a);
    R2F_HIP(ctx, take_launch_status());
    return R2F_OK;
}

}  // extern "C"
