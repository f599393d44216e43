// r2f_mosaic_stats.hip -- the data maximum of a mosaic (include/r2f.h: r2f_mosaic_maximum): the largest black-subtracted sample of
// mosaic rows, folded into a device word, from which r2f_raw_scale_plan derives a frame's scale.  A pure read pass, 2 bytes per
// sample in and 4 bytes out, off the render path: one kernel, its arguments and its entry point.
//   The grid is resident (8 blocks of 4 waves a CU) and walks groups of kRows rows, a wave per row, so a launch's block count does
//   not grow with the frame and every row is read as one contiguous run.
//   A lane loads kVec samples as one 16-byte word behind the row's head (the up to 7 samples that lead to a 16-byte boundary) and
//   ahead of its tail (the up to 7 that trail); head and tail are one 16-bit load a lane.  Pitch and alignment move the head, nothing
//   else: the same samples either way.
//   The table has one period, 6 (the entry point widens a 2 x 2 table): a block holds its 36 levels in LDS.  A lane's vector is
//   four pairs of neighbouring sites, from whatever column s it starts at (even or odd: the head decides), with the levels of phases
//   (s, s + 1), (s + 2, s + 3), (s + 4, s + 5), (s, s + 1) modulo 6; a lane's next vector starts 512 columns on, 2 modulo 6: its pairs
//   are the former ones moved up by one.  Per row a lane therefore fetches six levels as three packed pairs (q0, q1, q2) and its vectors use
//   (q0, q1, q2, q0), (q1, q2, q0, q1), (q2, q0, q1, q2) in turn -- the loop is unrolled by three and no table is read inside it.
//   raw - black clamped at 0 and the maximum are packed 16-bit operations (v_pk_sub_u16 with clamp, v_pk_max_u16): two samples each.
//   LDS: 72 bytes of table and 16 of wave maxima.
#include "r2f_ctx.h"

using namespace r2f;

namespace r2f {
namespace {

constexpr int kVec = 8, kRows = 4, kPeriod = 6;
static_assert(R2F_MOSAIC_MAX_VEC == kVec && R2F_MOSAIC_MAX_ROWS == kRows, "include/r2f.h states the load width and the rows per step");
static_assert((64 * kVec) % kPeriod == 2 && kVec % 2 == 0, "a lane's next vector starts one pair of sites further along the period");

struct MosaicMaxArgs {
    const uint16_t* src;  // row src_gy0 of the mosaic
    int src_gy0;
    long long pitch;  // samples
    int W;
    int y0, y1;  // the frame rows this call folds
    uint32_t* dst;
    uint16_t black[kPeriod * kPeriod];  // per phase (y % 6) * 6 + x % 6
};

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

// max(m, max(pair - q, 0)) on both halves of a 32-bit word of two samples (the lower address is the lower half: q.x is its level)
__device__ __forceinline__ void fold_pair(u16x2& m, uint32_t word, u16x2 q) {
    m = __builtin_elementwise_max(m, __builtin_elementwise_sub_sat(__builtin_bit_cast(u16x2, word), q));
}
__device__ __forceinline__ void fold_vec(u16x2 (&m)[4], const uint4 v, u16x2 qa, u16x2 qb, u16x2 qc) {
    fold_pair(m[0], v.x, qa), fold_pair(m[1], v.y, qb), fold_pair(m[2], v.z, qc), fold_pair(m[3], v.w, qa);
}
__device__ __forceinline__ unsigned fold_sample(unsigned m, unsigned raw, unsigned black) {
    const unsigned d = raw > black ? raw - black : 0u;
    return d > m ? d : m;
}

__global__ __launch_bounds__(64 * kRows) void mosaic_max_kernel(const MosaicMaxArgs a) {
    __shared__ uint16_t s_black[kPeriod * kPeriod];
    __shared__ unsigned s_wave[kRows];
    const int lane = threadIdx.x, wave = threadIdx.y, tid = wave * 64 + lane;
    if (tid < kPeriod * kPeriod) s_black[tid] = a.black[tid];
    __syncthreads();
    u16x2 m[4] = {};
    unsigned ms = 0;  // the head's and the tail's
    const int groups = (a.y1 - a.y0 + kRows - 1) / kRows;
    for (int g = blockIdx.x; g < groups; g += gridDim.x) {
        const int y = a.y0 + g * kRows + wave;  // (the same for all 64 lanes of a wave; the phase is the frame row's)
        if (y >= a.y1) continue;
        const uint16_t* row = a.src + (long long)(y - a.src_gy0) * a.pitch;
        const uint16_t* b = s_black + (y % kPeriod) * kPeriod;
        int head = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u) >> 1;
        head = head < a.W ? head : a.W;
        const int nvec = (a.W - head) / kVec, tail = head + nvec * kVec + lane;
        if (lane < head) ms = fold_sample(ms, row[lane], b[lane % kPeriod]);
        if (tail < a.W) ms = fold_sample(ms, row[tail], b[tail % kPeriod]);
        const int s = (head + kVec * lane) % kPeriod;  // the phase of this lane's first vector
        const u16x2 q0 = {b[s], b[(s + 1) % kPeriod]}, q1 = {b[(s + 2) % kPeriod], b[(s + 3) % kPeriod]},
                    q2 = {b[(s + 4) % kPeriod], b[(s + 5) % kPeriod]};
        const uint4* vec = reinterpret_cast<const uint4*>(row + head);  // 16-byte aligned: vectors [0, nvec) lie inside the row
        int i = lane;
        for (; i + 128 < nvec; i += 192) {
            const uint4 v0 = vec[i], v1 = vec[i + 64], v2 = vec[i + 128];
            fold_vec(m, v0, q0, q1, q2), fold_vec(m, v1, q1, q2, q0), fold_vec(m, v2, q2, q0, q1);
        }
        if (i < nvec) fold_vec(m, vec[i], q0, q1, q2);
        if (i + 64 < nvec) fold_vec(m, vec[i + 64], q1, q2, q0);
    }
    const u16x2 mm = __builtin_elementwise_max(__builtin_elementwise_max(m[0], m[1]), __builtin_elementwise_max(m[2], m[3]));
    unsigned r = mm.x > mm.y ? mm.x : mm.y;
    r = r > ms ? r : ms;
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)r, off, 64);
        r = o > r ? o : r;
    }
    if (lane == 0) s_wave[wave] = r;
    __syncthreads();
    if (tid == 0 && (int)blockIdx.x < groups) {  // (a block that found no rows leaves the word alone)
        for (int w = 1; w < kRows; ++w) r = s_wave[w] > r ? s_wave[w] : r;
        atomicMax(a.dst, r);
    }
}

}  // namespace
}  // namespace r2f

// =============================================================================== C ABI
extern "C" {

int r2f_mosaic_maximum(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W, int period,
                       const int32_t* black, int y0, int y1, uint32_t* dst_max, void* stream) {
    if (!ctx) return R2F_EINVAL;
    R2F_GUARD(ctx);
    const char* what = "mosaic_maximum";
    if (!src_rows || !black || !dst_max) return fail(ctx, R2F_EINVAL, "%s: the mosaic rows, the black table and the destination word are required", what);
    if (period != 2 && period != kPeriod) return fail(ctx, R2F_EINVAL, "%s: period %d is neither 2 nor 6", what, period);
    if (H < period || W < period || src_pitch < W || src_gy0 < 0 || src_nrows < 0)
        return fail(ctx, R2F_EINVAL, "%s: a mosaic of at least %d x %d samples, a pitch of at least W and a source window are required", what,
                    period, period);
    if (y0 < 0 || y1 > H || y0 > y1) return fail(ctx, R2F_EINVAL, "%s: rows [%d, %d) not inside the mosaic's [0, %d)", what, y0, y1, H);
    MosaicMaxArgs a{src_rows, src_gy0, (long long)src_pitch, W, y0, y1, dst_max, {}};
    for (int py = 0; py < kPeriod; ++py)
        for (int px = 0; px < kPeriod; ++px) {  // (6 is a multiple of 2: a 2 x 2 table widened to 6 x 6 keeps every site's level)
            const int32_t v = black[(py % period) * period + px % period];
            if (v < 0 || v > 65535) return fail(ctx, R2F_EINVAL, "%s: black level %d outside [0, 65535]", what, v);
            a.black[py * kPeriod + px] = (uint16_t)v;
        }
    if (y0 == y1) return R2F_OK;
    if (y0 < src_gy0 || (long long)y1 > (long long)src_gy0 + src_nrows)
        return fail(ctx, R2F_EINVAL, "%s: rows [%d, %d) are read, the source window holds [%d, %lld)", what, y0, y1, src_gy0,
                    (long long)src_gy0 + src_nrows);
    int cus = 0;
    if (const int rc = device_cu_count(ctx, &cus)) return rc;
    const int groups = (y1 - y0 + kRows - 1) / kRows, resident = 8 * cus;
    launch_k(mosaic_max_kernel, dim3(groups < resident ? groups : resident), dim3(64, kRows), 0, static_cast<hipStream_t>(stream), a);
    R2F_HIP(ctx, take_launch_status());
    return R2F_OK;
}

}  // extern "C"
