// r2f_jpeg.hip -- baseline JPEG encoder for gfx950: a uint8 (H, W, 3) device frame -> the bytes Pillow's default JPEG save writes
// (libjpeg-turbo; host side, tables and header: r2f_jpeg_plan.cpp).  Everything is asynchronous on the caller's stream:
//   1. transform   one wave per 16 x 16 MCU: RGB -> YCbCr (jccolor.c), h2v2 downsampling (jcsample.c), edge replication, ISLOW
//                  DCT (jfdctint.c), quantisation (jcdctmgr.c), dummy blocks (jccoefct.c); coefficients stored in zigzag order, and
//                  the MCU's bits counted except for the DC differences that need the MCU before it
//   2. dc_bits     those three DC differences (one predictor per component runs across the whole frame, or its restart interval)
//   3. scan        exclusive scan of the bits per MCU, 64-bit (a worst-case 100 MP frame exceeds 2^32 bits)
//   4. zero, pack  the words the scan will occupy are cleared; one wave per MCU assembles its bits in LDS and stores them, with an
//                  atomic OR only for the first and last word, which it may share with its neighbours
//   5. stuffing    0xFF bytes counted per 4 KB chunk, scanned, and the bytes scattered with a 0x00 behind every 0xFF; the last byte
//                  is padded with 1-bits first (jchuff.c flush_bits); header, EOI and the file's length are written last
// Samplings (r2f_jpeg_encode_ex): the MCU kernels are templated on it -- 4:2:0 as above; 4:2:2 (h2v1) 16 x 8 MCUs of Y0 Y1 Cb Cr,
// chroma pairs averaged with bias 0, 1, 0, 1 (jcsample.c h2v1_downsample), a dummy Y1 when the luma blocks per row are odd;
// 4:4:4 (h1v1) 8 x 8 MCUs of Y Cb Cr at full size, no dummies.  The DC predictors run across the whole frame in each.
// optimize (one-shot only): transform stores the coefficients; a stats kernel counts their symbols as libjpeg's gather pass does
// (jchuff.c htest_one_block) into per-workgroup LDS histograms, added into 4 x 256 global counts; the host reads the counts back,
// builds the tables (jpeg_gen_optimal_table, r2f_jpeg_plan.cpp) and the header, and a bits kernel recounts each MCU's bits with
// those tables before the scan, pack and stuffing passes run as above.  The header's length is a launch argument.
// Row-wise (r2f_jpeg_rows_begin / r2f_jpeg_rows): the same passes over the MCU rows of one call, [m0, m1).  The coefficients of
// the whole frame stay in the scratch, so the first MCU's DC prediction reads the last MCU of the call before; the bit scan starts
// at the carried bit count, the words cleared start at the first one not yet touched (the last one of the call before is shared),
// and the stuffing passes take the bytes that became complete, [floor(before / 8), floor(after / 8)) -- the partial last byte
// waits for the next call, the last call pads it -- with the 0xFF count scanned from the carried one.  *out_len then counts the
// leading bytes of the file that are final.
// Restart intervals (EncodeArgs::restart MCUs each; 0 takes exactly the passes above): an MCU whose index is a multiple of the
// interval predicts its DC coefficients from 0 (dc_bits, stats, bits, pack).  The scan's positions are no plain prefix sum any
// more -- every interval starts on a byte boundary, 16 bits behind the padded end of the one before -- so after the plain scan
// three small kernels lay the intervals out (restart_* below): each interval's length with its padding and marker, the same
// 64-bit scan over the intervals, and the shift of every MCU's offset to its interval's place.  offsets[m] is then the MCU's
// bit position in a scan that holds the padding and the markers: pack, which ends an interval, writes both behind its MCU's
// bits, and the stuffing passes tell a marker's 0xFF from a data byte by looking its position up in offsets[].
#include "r2f_launch.h"
#include "r2f_jpeg.h"

#include <algorithm>

namespace r2f {

namespace {

using u64 = unsigned long long;
using jpeg::Tables;

constexpr int kWaves = 4;          // MCUs per workgroup of the transform and pack kernels (one per wave)
constexpr int kPackWords = 320;    // LDS words per wave in pack: an MCU spans at most (31 + 6 * 1660 + 31) / 32 = 313 (314 with the
                                   // 23 bits of padding and marker that end a restart interval)
constexpr int kStatsGroups = 1024; // workgroups of the stats kernel (each walks MCUs, then adds its histograms: <= 1024 atomics)

// An MCU's shape per sampling (0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0): pixels, luminance blocks, all blocks (Y.. Cb Cr)
template <int S> struct Mcu;
template <> struct Mcu<0> { static constexpr int MW = 8, MH = 8, NY = 1, NB = 3; };
template <> struct Mcu<1> { static constexpr int MW = 16, MH = 8, NY = 2, NB = 4; };
template <> struct Mcu<2> { static constexpr int MW = 16, MH = 16, NY = 4, NB = 6; };

__constant__ uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct EncodeArgs {
    const uint8_t* img;
    long long stride;  // bytes between rows
    int H, W;
    int mx_n;          // MCUs per row
    long long n_mcus;
    long long m0, m1;  // the MCUs this launch encodes (one-shot: 0, n_mcus)
    int last;          // the scan ends with this launch: its bytes run to the padded last one
    const Tables* tables;
    int16_t* coefs;    // [n_mcus][blocks per MCU][64]
    u64* offsets;      // [n_mcus + 1]
    uint32_t* words;
    u64* chunks;       // [n_chunks + 1]
    long long n_chunks;
    u64 bound_bits;
    uint8_t* out;
    u64* out_len;
    int hdr_len;       // the header's bytes (the scan starts there)
    int restart;       // MCUs per restart interval (0: none)
    u64* intervals;    // restart: [intervals of the launch + 1]
};

struct HeaderBytes {
    uint8_t b[jpeg::kHeaderBytes + jpeg::kDriBytes];
};

// The MCU before m for the DC prediction of m's coefficients `c`: none for the frame's first MCU and for the first of a restart
// interval.
__device__ inline const int16_t* prev_mcu(const EncodeArgs& a, long long m, const int16_t* c, int mcu_coefs) {
    return m && !(a.restart && (uint32_t)m % (uint32_t)a.restart == 0) ? c - mcu_coefs : nullptr;  // (MCU indices fit 32 bits)
}
// MCU m ends a restart interval (the frame's last MCU ends the last one).
__device__ inline bool ends_interval(const EncodeArgs& a, long long m) {
    return (uint32_t)(m + 1) % (uint32_t)a.restart == 0 || m + 1 == a.n_mcus;
}

__device__ inline int magnitude_bits(int v) {
    v = v < 0 ? -v : v;
    return v ? 32 - __clz(v) : 0;
}

__device__ inline u64 shfl_up_u64(u64 v, int d) {
    const int lo = __shfl_up((int)(uint32_t)v, d, 64), hi = __shfl_up((int)(uint32_t)(v >> 32), d, 64);
    return ((u64)(uint32_t)hi << 32) | (uint32_t)lo;
}

// Inclusive scan over the 64 lanes of a wave.
template <typename T>
__device__ inline T wave_inclusive(T x, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        T t;
        if constexpr (sizeof(T) == 8)
            t = (T)shfl_up_u64((u64)x, d);
        else
            t = (T)__shfl_up((int)x, d, 64);
        if (lane >= d) x += t;
    }
    return x;
}

// --------------------------------------------------------------------------------------------------------------- 1. transform
// One pass of jfdctint.c jpeg_fdct_islow over 8 samples (first = the row pass, outputs scaled by 2^PASS1_BITS).
__device__ inline void fdct8(int d[8], bool first) {
    constexpr int CB = 13, P1 = 2;
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    const int sh = first ? CB - P1 : CB + P1;
    auto desc = [](int x, int n) { return (x + (1 << (n - 1))) >> n; };
    if (first) {
        d[0] = (t10 + t11) * (1 << P1);
        d[4] = (t10 - t11) * (1 << P1);
    } else {
        d[0] = desc(t10 + t11, P1);
        d[4] = desc(t10 - t11, P1);
    }
    int z1 = (t12 + t13) * 4433;
    d[2] = desc(z1 + t13 * 6270, sh);
    d[6] = desc(z1 - t12 * 15137, sh);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373, z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7] = desc(a4 + z1 + z3, sh);
    d[5] = desc(a5 + z2 + z4, sh);
    d[3] = desc(a6 + z2 + z3, sh);
    d[1] = desc(a7 + z1 + z4, sh);
}

__device__ inline int quantize(int x, int div) {  // jcdctmgr.c: |x| / div rounded half up, sign kept
    const int q = ((x < 0 ? -x : x) + (div >> 1)) / div;
    return x < 0 ? -q : q;
}

__device__ inline int sym_len(uint32_t e) { return (int)(e & 0xFF); }

// Bits lane `lane` (= zigzag position) contributes to its block: the DC difference on lane 0, a non-zero AC coefficient with the
// ZRLs and the code in front of it, the EOB on the lane of the last non-zero coefficient.  `nz` = ballot of the non-zero AC lanes.
__device__ inline int lane_bits(const uint32_t* dc, const uint32_t* ac, int v, int dc_diff, u64 nz, int lane) {
    const u64 mask = nz | 1ull;
    const int last = 63 - __clzll(mask);
    int bits = 0;
    if (lane == 0) {
        const int n = min(magnitude_bits(dc_diff), 11);
        bits += sym_len(dc[n]) + n;
    } else if (v != 0) {
        const int prev = 63 - __clzll(mask & ((1ull << lane) - 1));
        const int run = lane - prev - 1, n = min(magnitude_bits(v), 10);
        bits += (run >> 4) * sym_len(ac[0xF0]) + sym_len(ac[((run & 15) << 4) | n]) + n;
    }
    if (lane == last && last < 63) bits += sym_len(ac[0x00]);
    return bits;
}

template <int S>
__global__ __launch_bounds__(256) void jpeg_transform_kernel(EncodeArgs a) {
    using L = Mcu<S>;
    __shared__ int blk[kWaves][L::NB][64];  // Y0 Y1 Y2 Y3 Cb Cr of each wave's MCU (4:2:2: Y0 Y1 Cb Cr, 4:4:4: Y Cb Cr)
    __shared__ uint32_t s_dc[2][16], s_ac[2][256];
    __shared__ uint16_t s_q[2][64];
    for (int i = threadIdx.x; i < 2 * 256; i += blockDim.x) (&s_ac[0][0])[i] = (&a.tables->ac[0][0])[i];
    if (threadIdx.x < 32) (&s_dc[0][0])[threadIdx.x] = (&a.tables->dc[0][0])[threadIdx.x];
    if (threadIdx.x < 128) (&s_q[0][0])[threadIdx.x] = (&a.tables->qdiv[0][0])[threadIdx.x];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long m = a.m0 + (long long)blockIdx.x * kWaves + w;
    const bool live = m < a.m1;
    const int my = (int)(m / a.mx_n), mx = (int)(m % a.mx_n);
    int(*B)[64] = blk[w];
    const int H = a.H, W = a.W;
    const int ywb = (W + 7) / 8, yhb = (H + 7) / 8, hc = (H + 1) / 2;
    const bool right_dummy = S != 0 && 2 * mx + 1 >= ywb, bottom_dummy = S == 2 && 2 * my + 1 >= yhb;
    (void)hc;
    if constexpr (S == 0) {
        if (live) {  // one pixel per lane, edges replicated (no downsampling, no dummies)
            const int cy = lane >> 3, cx = lane & 7;
            const uint8_t* p = a.img + (long long)min(my * 8 + cy, H - 1) * a.stride + (long long)min(mx * 8 + cx, W - 1) * 3;
            const int r = p[0], g = p[1], b = p[2];
            B[0][lane] = ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16) - 128;
            B[1][lane] = ((-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16) - 128;
            B[2][lane] = ((32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16) - 128;
        }
    } else if constexpr (S == 1) {
        if (live) {  // the lane's horizontal pair: two luminance samples and one chroma sample (rows past the frame repeat its last)
            const int cy = lane >> 3, cx = lane & 7;
            const int y = min(my * 8 + cy, H - 1), gx = mx * 8 + cx;
            int cb = 0, cr = 0;
            for (int dx = 0; dx < 2; ++dx) {
                const int lx = 2 * cx + dx;
                const uint8_t* p = a.img + (long long)y * a.stride + (long long)min(mx * 16 + lx, W - 1) * 3;
                const int r = p[0], g = p[1], b = p[2];
                B[lx >> 3][cy * 8 + (lx & 7)] = ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16) - 128;
                cb += (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
                cr += (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
            }
            const int bias = gx & 1;  // h2v1_downsample: 0, 1, 0, 1 ... along the row
            B[2][lane] = ((cb + bias) >> 1) - 128;
            B[3][lane] = ((cr + bias) >> 1) - 128;
        }
    } else if (live) {
        const int cy = lane >> 3, cx = lane & 7;
        auto rgb = [&](int y, int x, int& r, int& g, int& b) {
            const uint8_t* p = a.img + (long long)y * a.stride + (long long)x * 3;
            r = p[0], g = p[1], b = p[2];
        };
        // luminance of the lane's 2 x 2 quad: rows and columns past the frame repeat its last ones (expand_right_edge,
        // expand_bottom_edge); the blocks entirely past them are dummies, fixed below
        for (int dy = 0; dy < 2; ++dy)
            for (int dx = 0; dx < 2; ++dx) {
                const int ly = 2 * cy + dy, lx = 2 * cx + dx;
                int r, g, b;
                rgb(min(my * 16 + ly, H - 1), min(mx * 16 + lx, W - 1), r, g, b);
                B[(ly >> 3) * 2 + (lx >> 3)][(ly & 7) * 8 + (lx & 7)] = ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16) - 128;
            }
        // chroma sample (gy, gx): the frame's rows padded to an even count, then chroma rows past the last one repeat it
        const int gy = min(my * 8 + cy, hc - 1), gx = mx * 8 + cx;
        int cb = 0, cr = 0;
        for (int dy = 0; dy < 2; ++dy)
            for (int dx = 0; dx < 2; ++dx) {
                int r, g, b;
                rgb(min(2 * gy + dy, H - 1), min(2 * gx + dx, W - 1), r, g, b);
                cb += (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
                cr += (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
            }
        const int bias = (gx & 1) ? 2 : 1;  // h2v2_downsample: 1, 2, 1, 2 ... along the row
        B[4][lane] = ((cb + bias) >> 2) - 128;
        B[5][lane] = ((cr + bias) >> 2) - 128;
    }
    __syncthreads();
    if (live && lane < L::NB * 8) {  // rows: lane = block * 8 + row
        int* row = &B[lane >> 3][(lane & 7) * 8];
        int d[8];
        for (int i = 0; i < 8; ++i) d[i] = row[i];
        fdct8(d, true);
        for (int i = 0; i < 8; ++i) row[i] = d[i];
    }
    __syncthreads();
    if (live && lane < L::NB * 8) {  // columns, then quantisation
        const int k = lane >> 3, c = lane & 7;
        const uint16_t* q = s_q[k < L::NY ? 0 : 1];
        int d[8];
        for (int i = 0; i < 8; ++i) d[i] = B[k][i * 8 + c];
        fdct8(d, false);
        for (int i = 0; i < 8; ++i) B[k][i * 8 + c] = quantize(d[i], q[i * 8 + c]);
    }
    __syncthreads();
    // jccoefct.c compress_data: a dummy block past the right edge copies the DC of the block to its left, a row of dummy blocks
    // past the bottom the DC of the block before that row (Y1); all of their AC coefficients are zero
    if (live && right_dummy) B[1][lane] = lane ? 0 : B[0][0];
    __syncthreads();
    if constexpr (S == 2) {
        if (live && (bottom_dummy || right_dummy)) {
            const int dc = bottom_dummy ? B[1][0] : B[2][0];
            if (bottom_dummy) B[2][lane] = lane ? 0 : dc;
            B[3][lane] = lane ? 0 : dc;
        }
        __syncthreads();
    }
    if (!live) return;
    int bits = 0;
    int16_t* out = a.coefs + m * (L::NB * 64);
    for (int k = 0; k < L::NB; ++k) {
        const int t = k < L::NY ? 0 : 1;
        const int v = B[k][kZigzag[lane]];
        out[k * 64 + lane] = (int16_t)v;
        const u64 nz = __ballot(lane > 0 && v != 0);
        // (the first block of each component takes its DC difference from the MCU before: dc_bits adds that)
        const int dd = (k >= 1 && k < L::NY) ? v - B[k - 1][0] : 0;
        int lb = lane_bits(s_dc[t], s_ac[t], v, dd, nz, lane);
        if (lane == 0 && !(k >= 1 && k < L::NY)) lb -= sym_len(s_dc[t][0]);
        bits += lb;
    }
    for (int d = 32; d >= 1; d >>= 1) bits += __shfl_xor(bits, d, 64);
    if (lane == 0) a.offsets[m] = (u64)bits;
}

// --------------------------------------------------------------------------------------------------------------- 2. DC bits
__device__ inline int dc_bits(const Tables* t, int c, int diff) {
    const int n = min(magnitude_bits(diff), 11);
    return sym_len(t->dc[c][n]) + n;
}

template <int S>
__global__ __launch_bounds__(256) void jpeg_dc_bits_kernel(EncodeArgs a) {
    constexpr int NY = Mcu<S>::NY, NB = Mcu<S>::NB;
    const long long m = a.m0 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.m1) return;
    const int16_t* c = a.coefs + m * (NB * 64);
    const int16_t* p = prev_mcu(a, m, c, NB * 64);
    a.offsets[m] += (u64)(dc_bits(a.tables, 0, c[0] - (p ? p[(NY - 1) * 64] : 0)) +
                          dc_bits(a.tables, 1, c[NY * 64] - (p ? p[NY * 64] : 0)) +
                          dc_bits(a.tables, 1, c[(NY + 1) * 64] - (p ? p[(NY + 1) * 64] : 0)));
}

// The DC prediction of block k of an MCU (c) after the MCU p (nullptr: the first MCU): the block before of the same component.
template <int S>
__device__ inline int dc_pred(const int16_t* c, const int16_t* p, int k) {
    constexpr int NY = Mcu<S>::NY;
    return k >= 1 && k < NY ? c[(k - 1) * 64] : (p ? p[(k == 0 ? NY - 1 : k) * 64] : 0);
}

// ------------------------------------------------------------------------------------------------------ optimize: stats, bits
// libjpeg's gather pass (jchuff.c htest_one_block) over the stored coefficients: per block the DC difference's category, a ZRL
// per 16 zeros before a non-zero coefficient, (run << 4) | size, and the EOB when the last non-zero coefficient is before 63.
// freq[DC0, AC0, DC1, AC1][256] (zeroed before): luminance into tables 0, Cb and Cr into tables 1.  Each workgroup walks MCUs
// into LDS histograms, then adds its non-zero bins with one 64-bit atomic each (integer sums: the result is deterministic).
template <int S>
__global__ __launch_bounds__(256) void jpeg_stats_kernel(EncodeArgs a, u64* freq) {
    using L = Mcu<S>;
    __shared__ uint32_t h[4][256];
    for (int i = threadIdx.x; i < 4 * 256; i += blockDim.x) (&h[0][0])[i] = 0;
    __syncthreads();
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (long long m = a.m0 + (long long)blockIdx.x * kWaves + w; m < a.m1; m += (long long)gridDim.x * kWaves) {
        const int16_t* c = a.coefs + m * (L::NB * 64);
        const int16_t* p = prev_mcu(a, m, c, L::NB * 64);
        for (int k = 0; k < L::NB; ++k) {
            const int t = k < L::NY ? 0 : 1;
            const int v = c[k * 64 + lane];
            const u64 nz = __ballot(lane > 0 && v != 0);
            const u64 mask = nz | 1ull;
            if (lane == 0) {
                atomicAdd(&h[2 * t][min(magnitude_bits(v - dc_pred<S>(c, p, k)), 11)], 1u);
            } else if (v != 0) {
                const int prev = 63 - __clzll(mask & ((1ull << lane) - 1));
                const int run = lane - prev - 1;
                if (run >> 4) atomicAdd(&h[2 * t + 1][0xF0], (uint32_t)(run >> 4));
                atomicAdd(&h[2 * t + 1][((run & 15) << 4) | min(magnitude_bits(v), 10)], 1u);
            }
            const int last = 63 - __clzll(mask);
            if (lane == last && last < 63) atomicAdd(&h[2 * t + 1][0x00], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 4 * 256; i += blockDim.x) {
        const uint32_t n = (&h[0][0])[i];
        if (n) atomicAdd((unsigned long long*)&freq[i], (unsigned long long)n);
    }
}

// Each MCU's bits with the tables in the scratch (the optimized ones), its DC differences included: offsets[m].
template <int S>
__global__ __launch_bounds__(256) void jpeg_bits_kernel(EncodeArgs a) {
    using L = Mcu<S>;
    __shared__ uint32_t s_dc[2][16], s_ac[2][256];
    for (int i = threadIdx.x; i < 2 * 256; i += blockDim.x) (&s_ac[0][0])[i] = (&a.tables->ac[0][0])[i];
    if (threadIdx.x < 32) (&s_dc[0][0])[threadIdx.x] = (&a.tables->dc[0][0])[threadIdx.x];
    __syncthreads();
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long m = a.m0 + (long long)blockIdx.x * kWaves + w;
    if (m >= a.m1) return;
    const int16_t* c = a.coefs + m * (L::NB * 64);
    const int16_t* p = prev_mcu(a, m, c, L::NB * 64);
    int bits = 0;
    for (int k = 0; k < L::NB; ++k) {
        const int t = k < L::NY ? 0 : 1;
        const int v = c[k * 64 + lane];
        const u64 nz = __ballot(lane > 0 && v != 0);
        bits += lane_bits(s_dc[t], s_ac[t], v, v - dc_pred<S>(c, p, k), nz, lane);
    }
    for (int d = 32; d >= 1; d >>= 1) bits += __shfl_xor(bits, d, 64);
    if (lane == 0) a.offsets[m] = (u64)bits;
}

// --------------------------------------------------------------------------------------------------------------- 3. scan
// Exclusive scan, in place, of each kScanBlock elements of data[0, n); sums[block] = the block's total.  A single block also writes
// the total to data[n], and starts from *start if there is one.
__global__ __launch_bounds__(256) void scan_block_kernel(u64* data, long long n, u64* sums, const u64* start) {
    __shared__ u64 wave_tot[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long base = (long long)blockIdx.x * jpeg::kScanBlock + threadIdx.x * 4;
    u64 v[4], s = 0;
    for (int j = 0; j < 4; ++j) {
        v[j] = base + j < n ? data[base + j] : 0;
        s += v[j];
    }
    const u64 inc = wave_inclusive<u64>(s, lane);
    if (lane == 63) wave_tot[w] = inc;
    __syncthreads();
    u64 run = inc - s + (start ? *start : 0);
    for (int i = 0; i < w; ++i) run += wave_tot[i];
    for (int j = 0; j < 4; ++j) {
        if (base + j < n) data[base + j] = run;
        run += v[j];
    }
    if (threadIdx.x == 255) {
        if (sums) sums[blockIdx.x] = run;
        if (gridDim.x == 1) data[n] = run;
    }
}

// data[block * kScanBlock + i] += sums[block] (sums scanned already, sums[gridDim.x] = the total, which goes to data[n]).
__global__ __launch_bounds__(256) void scan_add_kernel(u64* data, long long n, const u64* sums) {
    const long long base = (long long)blockIdx.x * jpeg::kScanBlock;
    const u64 add = sums[blockIdx.x];
    for (int j = threadIdx.x; j < jpeg::kScanBlock; j += blockDim.x)
        if (base + j < n) data[base + j] += add;
    if (blockIdx.x == 0 && threadIdx.x == 0) data[n] = sums[gridDim.x];
}

// (base: a device word added to every element and the total, or nullptr)
void scan_u64(u64* data, long long n, u64* partial, hipStream_t s, const u64* base = nullptr) {
    const long long nb = (n + jpeg::kScanBlock - 1) / jpeg::kScanBlock;
    if (nb <= 1) {
        launch_k(scan_block_kernel, dim3(1), dim3(256), 0, s, data, n, (u64*)nullptr, base);
        return;
    }
    launch_k(scan_block_kernel, dim3((unsigned)nb), dim3(256), 0, s, data, n, partial, (const u64*)nullptr);
    scan_u64(partial, nb, partial + nb + 1, s, base);
    launch_k(scan_add_kernel, dim3((unsigned)nb), dim3(256), 0, s, data, n, (const u64*)partial);
}

// ----------------------------------------------------------------------------------------------- 3b. restart intervals
// The launch's MCUs [m0, m1) fall into the intervals j = m / restart - m0 / restart (the first may have begun in a launch before,
// the last may go on in the next).  offsets[m0 .. m1] hold the plain scan from 0.  intervals[j] = the bits interval j adds to the
// scan: its MCUs', then, if it ends in this launch, the padding to a whole byte -- counted from `*carry`, the position the launch
// starts at, for the first one, which alone may start inside a byte -- and the 16 bits of its marker unless it ends the frame.
__global__ __launch_bounds__(256) void restart_length_kernel(EncodeArgs a, long long n_int, const u64* carry) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_int) return;
    const long long k = a.m0 / a.restart + j;
    const long long first = max(k * a.restart, a.m0), end = min((k + 1) * (long long)a.restart, a.m1);
    u64 len = a.offsets[end] - a.offsets[first];
    if (end % a.restart == 0 || end == a.n_mcus) {
        const u64 at = (j == 0 && carry ? *carry : 0) + len;
        len += (0 - at) & 7;
        if (end != a.n_mcus) len += 16;
    }
    a.intervals[j] = len;
}

// intervals[] scanned (from the carried position): intervals[j] = where interval j's MCUs of this launch start.  Each becomes
// the shift of its MCUs' offsets, start - offsets[its first MCU]; intervals[n_int], the position after the launch, stays.
__global__ __launch_bounds__(256) void restart_shift_kernel(EncodeArgs a, long long n_int) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_int) return;
    a.intervals[j] -= a.offsets[max((a.m0 / a.restart + j) * a.restart, a.m0)];
}

// offsets[m] += its interval's shift; offsets[m1] = the position after the launch.  (In place: every thread touches its own
// element, the shifts were taken from the unshifted offsets by the kernel before.)
__global__ __launch_bounds__(256) void restart_place_kernel(EncodeArgs a, long long n_int) {
    const long long m = a.m0 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m < a.m1) a.offsets[m] += a.intervals[m / a.restart - a.m0 / a.restart];
    if (m == a.m1) a.offsets[m] = a.intervals[n_int];
}

// The restart-aware scan of a launch's bits per MCU: offsets[m0 .. m1] as positions in the padded scan.  Everything stays on the
// stream; the intervals take the same recursive scan as the MCUs, so their number is not bounded by one scan block.
void restart_scan(const EncodeArgs& a, u64* partial, hipStream_t s, const u64* carry) {
    const long long n = a.m1 - a.m0, n_int = (a.m1 - 1) / a.restart - a.m0 / a.restart + 1;
    scan_u64(a.offsets + a.m0, n, partial, s);
    const dim3 gi((unsigned)((n_int + 255) / 256)), b(256);
    launch_k(restart_length_kernel, gi, b, 0, s, a, n_int, carry);
    scan_u64(a.intervals, n_int, partial, s, carry);
    launch_k(restart_shift_kernel, gi, b, 0, s, a, n_int);
    launch_k(restart_place_kernel, dim3((unsigned)((n + 1 + 255) / 256)), b, 0, s, a, n_int);
}

// --------------------------------------------------------------------------------------------------------------- 4. pack
// Words [ceil(begin / 32), ceil(end / 32)) of the packed scan cleared (what pack ORs into must start at zero; the word holding bit
// `begin`, if it is not the first of its word, holds the bits of the launch before).
__global__ __launch_bounds__(256) void jpeg_zero_kernel(EncodeArgs a) {
    const u64 begin = a.offsets[a.m0], total = a.offsets[a.m1];
    if (total > a.bound_bits) return;
    const u64 w0 = (begin + 31) / 32, nw = (total + 31) / 32;
    for (u64 i = w0 + (u64)blockIdx.x * blockDim.x + threadIdx.x; i < nw; i += (u64)gridDim.x * blockDim.x) a.words[i] = 0;
}

// The low `len` (1..32) bits of `v` at bit position `pos` of a wave's LDS words, big-endian (a code and its value bits go in one
// call: the value must be masked to its own width first, or a negative one's sign bits would land on the code).
__device__ inline void put_bits(uint32_t* lds, int pos, uint32_t v, int len) {
    const u64 x = ((u64)(v & (uint32_t)((1ull << len) - 1)) << (64 - len)) >> (pos & 31);
    atomicOr(&lds[pos >> 5], (uint32_t)(x >> 32));
    if ((uint32_t)x) atomicOr(&lds[(pos >> 5) + 1], (uint32_t)x);
}

template <int S>
__global__ __launch_bounds__(256) void jpeg_pack_kernel(EncodeArgs a) {
    using L = Mcu<S>;
    __shared__ uint32_t s_words[kWaves][kPackWords];
    __shared__ uint32_t s_dc[2][16], s_ac[2][256];
    for (int i = threadIdx.x; i < 2 * 256; i += blockDim.x) (&s_ac[0][0])[i] = (&a.tables->ac[0][0])[i];
    if (threadIdx.x < 32) (&s_dc[0][0])[threadIdx.x] = (&a.tables->dc[0][0])[threadIdx.x];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long m = a.m0 + (long long)blockIdx.x * kWaves + w;
    uint32_t* lds = s_words[w];
    for (int i = lane; i < kPackWords; i += 64) lds[i] = 0;
    __syncthreads();
    const bool live = m < a.m1 && a.offsets[a.m1] <= a.bound_bits;
    const u64 start = live ? a.offsets[m] : 0, end = live ? a.offsets[m + 1] : 0;
    const int nw = live ? (int)(((start & 31) + (end - start) + 31) >> 5) : 0;
    if (live && nw <= kPackWords) {
        const int16_t* c = a.coefs + m * (L::NB * 64);
        const int16_t* p = prev_mcu(a, m, c, L::NB * 64);
        int pos = (int)(start & 31);  // bit position in the wave's words
        for (int k = 0; k < L::NB; ++k) {
            const int t = k < L::NY ? 0 : 1;
            const uint32_t* dc = s_dc[t];
            const uint32_t* ac = s_ac[t];
            const int v = c[k * 64 + lane];
            const int pred = dc_pred<S>(c, p, k);
            const u64 nz = __ballot(lane > 0 && v != 0);
            const int len = lane_bits(dc, ac, v, v - pred, nz, lane);
            const int inc = wave_inclusive<int>(len, lane);
            int at = pos + inc - len;
            if (lane == 0) {  // DC: size category, then the difference's low bits (negative: minus one, jchuff.c)
                const int diff = v - pred, n = min(magnitude_bits(diff), 11);
                const uint32_t e = dc[n];
                const int cl = sym_len(e);
                put_bits(lds, at, ((e >> 8) << n) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1)), cl + n);
                at += cl + n;
            } else if (v != 0) {
                const u64 mask = nz | 1ull;
                const int prev = 63 - __clzll(mask & ((1ull << lane) - 1));
                int run = lane - prev - 1;
                const int n = min(magnitude_bits(v), 10);
                for (; run > 15; run -= 16) {
                    put_bits(lds, at, ac[0xF0] >> 8, sym_len(ac[0xF0]));
                    at += sym_len(ac[0xF0]);
                }
                const uint32_t e = ac[(run << 4) | n];
                put_bits(lds, at, ((e >> 8) << n) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1)), sym_len(e) + n);
                at += sym_len(e) + n;
            }
            const int last = 63 - __clzll(nz | 1ull);
            if (lane == last && last < 63) put_bits(lds, at, ac[0x00] >> 8, sym_len(ac[0x00]));
            pos += __shfl(inc, 63, 64);
        }
        // the end of a restart interval: 1-bits up to the byte boundary (jchuff.c flush_bits), then RSTn unless the frame ends
        // (both inside [start, end): restart_scan counted them to this MCU, and kPackWords has room for their 23 bits)
        if (a.restart && lane == 0 && ends_interval(a, m)) {
            const int pad = -pos & 7;
            if (pad) put_bits(lds, pos, 0xFFu, pad);
            if (m + 1 != a.n_mcus) put_bits(lds, pos + pad, 0xFFD0u | (uint32_t)((m / a.restart) & 7), 16);
        }
    }
    __syncthreads();
    if (!live || nw > kPackWords) return;
    // words wholly inside this MCU's bits are its own; the first and the last may hold a neighbour's bits too
    const u64 w0 = start >> 5;
    for (int i = lane; i < nw; i += 64) {
        const bool shared = (i == 0 && (start & 31)) || (i == nw - 1 && (end & 31));
        if (shared)
            atomicOr(&a.words[w0 + i], lds[i]);
        else
            a.words[w0 + i] = lds[i];
    }
}

// --------------------------------------------------------------------------------------------------------------- 5. stuffing
// Byte i of the packed scan, the last one padded with 1-bits (flush_bits).
__device__ inline uint32_t scan_byte(const uint32_t* words, u64 i, u64 total_bits) {
    uint32_t b = (words[i >> 2] >> (24 - 8 * (i & 3))) & 0xFF;
    if (i == (total_bits - 1) / 8 && (total_bits & 7)) b |= 0xFFu >> (total_bits & 7);
    return b;
}

// The scan bytes [lo, hi) this launch stuffs: every one up to the padded last (last launch), else the complete ones, from the
// partial byte the launch before left (none if the scan broke its bound).
__device__ inline void stuff_range(const EncodeArgs& a, u64& lo, u64& hi, u64& total) {
    total = a.offsets[a.m1];
    lo = a.offsets[a.m0] / 8;
    hi = total > a.bound_bits ? lo : a.last ? (total + 7) / 8 : total / 8;
}

// Whether the 0xFF at scan byte i is the first byte of a restart marker, not data: the marker before interval k ends where the
// interval starts, at bit offsets[k restart], so byte i is one iff 8 (i + 2) is such a start.  Only a 0xFF followed by D0 .. D7
// is looked up (a binary search over the interval starts laid out so far, k <= m1 / restart; a marker's second byte lies in the
// same launch's bytes as its first).  Interval starts increase strictly: every MCU has bits.
__device__ inline bool is_marker(const EncodeArgs& a, u64 i, u64 total) {
    if (!a.restart || i + 1 >= (total + 7) / 8) return false;
    if ((scan_byte(a.words, i + 1, total) & 0xF8) != 0xD0) return false;
    const u64 want = 8 * (i + 2);
    long long lo = 1, hi = min((a.n_mcus - 1) / a.restart, a.m1 / a.restart);  // interval starts k in [lo, hi]
    while (lo < hi) {
        const long long mid = (lo + hi) / 2;
        if (a.offsets[mid * a.restart] < want)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo == hi && a.offsets[lo * a.restart] == want;
}

// Whether scan byte i gets a 0x00 behind it.
__device__ inline bool stuffed(const EncodeArgs& a, uint32_t byte, u64 i, u64 total) { return byte == 0xFF && !is_marker(a, i, total); }

// 0xFF bytes of each kStuffChunk bytes of the range (one chunk per workgroup, 16 bytes per thread); chunks past it count 0.
__global__ __launch_bounds__(256) void jpeg_ff_count_kernel(EncodeArgs a) {
    __shared__ int wave_tot[4];
    u64 lo, hi, total;
    stuff_range(a, lo, hi, total);
    const u64 b0 = lo + (u64)blockIdx.x * jpeg::kStuffChunk + threadIdx.x * 16;
    int cnt = 0;
    for (int j = 0; j < 16; ++j)
        if (b0 + j < hi) cnt += stuffed(a, scan_byte(a.words, b0 + j, total), b0 + j, total);
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
    if ((threadIdx.x & 63) == 0) wave_tot[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) a.chunks[blockIdx.x] = (u64)(wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3]);
}

// Every byte of the range to its place behind the header, a 0x00 behind each 0xFF (chunks[] scanned from the 0xFF bytes before).
__global__ __launch_bounds__(256) void jpeg_scatter_kernel(EncodeArgs a) {
    __shared__ int wave_tot[4];
    u64 lo, hi, total;
    stuff_range(a, lo, hi, total);
    const u64 b0 = lo + (u64)blockIdx.x * jpeg::kStuffChunk + threadIdx.x * 16;
    if (lo + (u64)blockIdx.x * jpeg::kStuffChunk >= hi) return;  // (the whole workgroup: no barrier is skipped by part of it)
    uint32_t bytes[16], stuff = 0;  // (stuff: bit j = a 0x00 follows byte j)
    int cnt = 0;
    for (int j = 0; j < 16; ++j) {
        bytes[j] = b0 + j < hi ? scan_byte(a.words, b0 + j, total) : 0;
        if (b0 + j < hi && stuffed(a, bytes[j], b0 + j, total)) stuff |= 1u << j, ++cnt;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int inc = wave_inclusive<int>(cnt, lane);
    if (lane == 63) wave_tot[w] = inc;
    __syncthreads();
    u64 ff = a.chunks[blockIdx.x] + (u64)(inc - cnt);
    for (int i = 0; i < w; ++i) ff += (u64)wave_tot[i];
    uint8_t* out = a.out + a.hdr_len;
    for (int j = 0; j < 16; ++j) {
        if (b0 + j >= hi) break;
        const u64 o = b0 + j + ff;
        out[o] = (uint8_t)bytes[j];
        if (stuff >> j & 1) {
            out[o + 1] = 0;
            ++ff;
        }
    }
}

// Header, EOI and the file's length (0 if the scan broke its bound, which the passes above then did not write past).
__global__ __launch_bounds__(256) void jpeg_finish_kernel(EncodeArgs a, HeaderBytes h) {
    const u64 total = a.offsets[a.m1];
    if (total > a.bound_bits) {
        if (threadIdx.x == 0) *a.out_len = 0;
        return;
    }
    for (int i = threadIdx.x; i < a.hdr_len; i += blockDim.x) a.out[i] = h.b[i];
    if (threadIdx.x == 0) {
        const u64 end = (u64)a.hdr_len + (total + 7) / 8 + a.chunks[a.n_chunks];
        a.out[end] = 0xFF;
        a.out[end + 1] = 0xD9;
        *a.out_len = end + 2;
    }
}

// Row-wise: the header, an empty carry ({bits, 0xFF bytes} so far) and *out_len = the header's length.
__global__ __launch_bounds__(256) void jpeg_rows_begin_kernel(HeaderBytes h, int hdr_len, uint8_t* out, u64* out_len, u64* carry) {
    for (int i = threadIdx.x; i < hdr_len; i += blockDim.x) out[i] = h.b[i];
    if (threadIdx.x == 0) {
        carry[0] = carry[1] = 0;
        *out_len = (u64)hdr_len;
    }
}

// Row-wise: the carry for the next launch and the final bytes so far (the last launch adds EOI).  A broken bound leaves
// *out_len = 0 and a carried bit count past the bound, so that every later launch of the encode writes nothing either.
__global__ void jpeg_rows_finish_kernel(EncodeArgs a, long long n_chunks, u64* carry) {
    const u64 total = a.offsets[a.m1];
    if (total > a.bound_bits) {
        carry[0] = a.bound_bits + 1;
        *a.out_len = 0;
        return;
    }
    const u64 ff = a.chunks[n_chunks];
    u64 end = (u64)a.hdr_len + (a.last ? (total + 7) / 8 : total / 8) + ff;
    if (a.last) {
        a.out[end] = 0xFF;
        a.out[end + 1] = 0xD9;
        end += 2;
    }
    carry[0] = total;
    carry[1] = ff;
    *a.out_len = end;
}

__global__ void jpeg_tables_kernel(Tables t, Tables* dst) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&t);
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
    for (int i = threadIdx.x; i < (int)(sizeof(Tables) / 4); i += blockDim.x) d[i] = src[i];
}

EncodeArgs encode_args(const JpegEncodeArgs& e, const jpeg::Scratch& L) {
    uint8_t* base = static_cast<uint8_t*>(e.scratch);
    EncodeArgs a;
    a.img = e.image, a.stride = e.row_stride, a.H = e.H, a.W = e.W;
    const int mw = jpeg::layout(e.sampling).mw;
    a.mx_n = (e.W + mw - 1) / mw;
    a.n_mcus = (long long)L.n_mcus;
    a.m0 = 0, a.m1 = a.n_mcus, a.last = 1;
    a.tables = reinterpret_cast<const Tables*>(base + L.tables);
    a.coefs = reinterpret_cast<int16_t*>(base + L.coefs);
    a.offsets = reinterpret_cast<u64*>(base + L.offsets);
    a.words = reinterpret_cast<uint32_t*>(base + L.words);
    a.chunks = reinterpret_cast<u64*>(base + L.chunks);
    a.n_chunks = (long long)L.stuff_chunks;
    a.bound_bits = jpeg::scan_bound_bits(e.H, e.W, e.sampling, e.restart);
    a.out = e.out, a.out_len = e.out_len;
    a.hdr_len = e.header_len;
    a.restart = e.restart;
    a.intervals = reinterpret_cast<u64*>(base + L.intervals);
    return a;
}

HeaderBytes header_bytes(const uint8_t* header, int len) {
    HeaderBytes h{};
    for (int i = 0; i < len; ++i) h.b[i] = header[i];
    return h;
}

// The MCU kernels of a sampling.
struct McuKernels {
    void (*transform)(EncodeArgs);
    void (*dc_bits)(EncodeArgs);
    void (*pack)(EncodeArgs);
    void (*stats)(EncodeArgs, u64*);
    void (*bits)(EncodeArgs);
};
template <int S>
McuKernels mcu_kernels_of() {
    return {jpeg_transform_kernel<S>, jpeg_dc_bits_kernel<S>, jpeg_pack_kernel<S>, jpeg_stats_kernel<S>, jpeg_bits_kernel<S>};
}
McuKernels mcu_kernels(int sampling) {
    return sampling == 0 ? mcu_kernels_of<0>() : sampling == 1 ? mcu_kernels_of<1>() : mcu_kernels_of<2>();
}

}  // namespace

hipError_t launch_jpeg_stats(const JpegEncodeArgs& e, unsigned long long* freq, hipStream_t s) {
    const jpeg::Scratch L = jpeg::scratch_layout(e.H, e.W, e.sampling, e.restart);
    const EncodeArgs a = encode_args(e, L);
    const McuKernels K = mcu_kernels(e.sampling);
    const unsigned mcu_groups = (unsigned)((L.n_mcus + kWaves - 1) / kWaves);
    launch_k(jpeg_tables_kernel, dim3(1), dim3(256), 0, s, e.tables, const_cast<Tables*>(a.tables));
    launch_k(K.transform, dim3(mcu_groups), dim3(256), 0, s, a);
    hipError_t err = hipMemsetAsync(freq, 0, 4 * 256 * sizeof(u64), s);
    if (err != hipSuccess) {
        (void)take_launch_status();
        return err;
    }
    launch_k(K.stats, dim3(std::min<unsigned>(mcu_groups, kStatsGroups)), dim3(256), 0, s, a, reinterpret_cast<u64*>(freq));
    return take_launch_status();
}

hipError_t launch_jpeg_transform(const JpegEncodeArgs& e, hipStream_t s) {
    const jpeg::Scratch L = jpeg::scratch_layout(e.H, e.W, e.sampling, e.restart);
    const EncodeArgs a = encode_args(e, L);
    launch_k(jpeg_tables_kernel, dim3(1), dim3(256), 0, s, e.tables, const_cast<Tables*>(a.tables));
    launch_k(mcu_kernels(e.sampling).transform, dim3((unsigned)((L.n_mcus + kWaves - 1) / kWaves)), dim3(256), 0, s, a);
    return take_launch_status();
}

void jpeg_scan_u64(unsigned long long* data, long long n, unsigned long long* partial, hipStream_t s) { scan_u64(data, n, partial, s); }

hipError_t launch_jpeg_encode(const JpegEncodeArgs& e, hipStream_t s) {
    const jpeg::Scratch L = jpeg::scratch_layout(e.H, e.W, e.sampling, e.restart);
    const EncodeArgs a = encode_args(e, L);
    u64* partial = reinterpret_cast<u64*>(static_cast<uint8_t*>(e.scratch) + L.partial);
    const HeaderBytes h = header_bytes(e.header, e.header_len);
    const McuKernels K = mcu_kernels(e.sampling);

    const unsigned mcu_groups = (unsigned)((L.n_mcus + kWaves - 1) / kWaves);
    launch_k(jpeg_tables_kernel, dim3(1), dim3(256), 0, s, e.tables, const_cast<Tables*>(a.tables));
    if (e.recount) {  // (optimize: the coefficients are in the scratch, launch_jpeg_stats made them)
        launch_k(K.bits, dim3(mcu_groups), dim3(256), 0, s, a);
    } else {
        launch_k(K.transform, dim3(mcu_groups), dim3(256), 0, s, a);
        launch_k(K.dc_bits, dim3((unsigned)((L.n_mcus + 255) / 256)), dim3(256), 0, s, a);
    }
    if (a.restart)
        restart_scan(a, partial, s, nullptr);
    else
        scan_u64(a.offsets, a.n_mcus, partial, s);
    const u64 max_words = (a.bound_bits + 31) / 32;
    launch_k(jpeg_zero_kernel, dim3((unsigned)std::min<u64>((max_words + 255) / 256, 4096)), dim3(256), 0, s, a);
    launch_k(K.pack, dim3(mcu_groups), dim3(256), 0, s, a);
    launch_k(jpeg_ff_count_kernel, dim3((unsigned)L.stuff_chunks), dim3(256), 0, s, a);
    scan_u64(a.chunks, a.n_chunks, partial, s);
    launch_k(jpeg_scatter_kernel, dim3((unsigned)L.stuff_chunks), dim3(256), 0, s, a);
    launch_k(jpeg_finish_kernel, dim3(1), dim3(256), 0, s, a, h);
    return take_launch_status();
}

hipError_t launch_jpeg_rows_begin(const JpegEncodeArgs& e, hipStream_t s) {
    const jpeg::Scratch L = jpeg::scratch_layout(e.H, e.W, e.sampling, e.restart);
    Tables* tables = reinterpret_cast<Tables*>(static_cast<uint8_t*>(e.scratch) + L.tables);
    launch_k(jpeg_tables_kernel, dim3(1), dim3(256), 0, s, e.tables, tables);
    launch_k(jpeg_rows_begin_kernel, dim3(1), dim3(256), 0, s, header_bytes(e.header, e.header_len), e.header_len, e.out, e.out_len,
             static_cast<u64*>(e.carry));
    return take_launch_status();
}

hipError_t launch_jpeg_rows(const JpegEncodeArgs& e, const jpeg::RowsGrid& g, bool last, hipStream_t s) {
    const jpeg::Scratch L = jpeg::scratch_layout(e.H, e.W, e.sampling, e.restart);
    EncodeArgs a = encode_args(e, L);
    const McuKernels K = mcu_kernels(e.sampling);
    a.m0 = (long long)g.m0, a.m1 = (long long)g.m1, a.last = last ? 1 : 0;
    a.n_chunks = (long long)g.stuff_chunks;
    u64* partial = reinterpret_cast<u64*>(static_cast<uint8_t*>(e.scratch) + L.partial);
    u64* carry = static_cast<u64*>(e.carry);

    const long long n = a.m1 - a.m0;
    const unsigned mcu_groups = (unsigned)((n + kWaves - 1) / kWaves);
    launch_k(K.transform, dim3(mcu_groups), dim3(256), 0, s, a);
    launch_k(K.dc_bits, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    // offsets[m0] = the bits before, offsets[m1] = the bits after.  With restart intervals the carry needs no new word: carry[0]
    // is the position the next MCU starts at, the padding and marker of an interval that ended with the launch included, and
    // which interval an MCU belongs to, whether it starts or ends one and the marker's number all follow from its global index.
    if (a.restart)
        restart_scan(a, partial, s, carry);
    else
        scan_u64(a.offsets + a.m0, n, partial, s, carry);
    launch_k(jpeg_zero_kernel, dim3((unsigned)std::min<u64>((g.zero_words + 255) / 256, 4096)), dim3(256), 0, s, a);
    launch_k(K.pack, dim3(mcu_groups), dim3(256), 0, s, a);
    launch_k(jpeg_ff_count_kernel, dim3((unsigned)g.stuff_chunks), dim3(256), 0, s, a);
    scan_u64(a.chunks, a.n_chunks, partial, s, carry + 1);
    launch_k(jpeg_scatter_kernel, dim3((unsigned)g.stuff_chunks), dim3(256), 0, s, a);
    launch_k(jpeg_rows_finish_kernel, dim3(1), dim3(64), 0, s, a, a.n_chunks, carry);
    return take_launch_status();
}

}  // namespace r2f
