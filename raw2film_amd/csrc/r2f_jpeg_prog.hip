// r2f_jpeg_prog.hip -- progressive JPEG encoder for gfx950: the bytes Pillow's save(..., progressive=True) writes (libjpeg-turbo
// jcphuff.c over jpeg_simple_progression's ten scans, each with its own optimized tables).  Host side: r2f_jpeg_plan.cpp.
// The coefficients come from the baseline encoder's transform pass (r2f_jpeg.hip), dummy blocks included.  Then, per scan:
//   1. flags     one thread per block: its own symbols into the scan's counts (the carried EOB run left out); for an AC scan
//                whether it codes anything, whether it ends by joining the pending run, and the correction bits it leaves buffered
//   2. runs      exclusive scans of those three, then per block the end of the run that would start there (binary searches: the
//                next coded block, EOBRUN reaching 0x7FFF, more than 937 buffered correction bits) and the next run start after
//                it; pointer doubling over that chain marks the run starts reachable from each stretch's first block (block 0 and
//                every coded block); each marked block gets its run's length and counts its EOB symbol
// The host reads the counts back (the one synchronisation before the packing), builds every scan's tables and headers, and per
// scan:
//   3. bits      one thread per block: its own bits, then (a run start) the run's EOB symbol and extra bits, then the correction
//                bits it buffered -- the order jcphuff.c emits them in, since a run's buffered bits follow its EOB symbol
//   4. pack      the exclusive scan of those, the words cleared, each block's bits ORed in (shared words atomically)
//   5. stuffing  0xFF bytes counted per chunk, scanned, and the scan's bytes scattered behind its header at the file position a
//                device word carries from scan to scan; nothing past out_cap is written (the file's length is then 0)
#include "r2f_launch.h"
#include "r2f_jpeg.h"

#include <algorithm>

namespace r2f {

namespace {

using u64 = unsigned long long;

struct ProgArgs {
    const int16_t* coefs;  // [mcus][nb][64], zigzag order
    int nb, ny, hy, vy, mx;
    int Ss, Se, Ah, Al, comp;
    long long n;  // blocks of the scan
    int bw;       // AC scans: blocks per row of the component
    u64* ecount;  // joining blocks, then their exclusive scan ([n] = total)
    u64* bcount;  // buffered correction bits at the block's end
    u64* ccount;  // coded blocks
    uint32_t* jump;  // [levels][n + 1]
    uint32_t* mark;  // [n + 1]
    uint32_t* runs;  // [n]: the EOB run a block starts
    u64* freq;       // [2][256] of this scan
    u64* extra;      // this scan's correction bits
};

__device__ inline int nbits_of(int v) {
    v = v < 0 ? -v : v;
    return v ? 32 - __clz(v) : 0;
}

__device__ inline const int16_t* block_ptr(const ProgArgs& a, long long i) {
    if (a.Ss == 0) return a.coefs + i * 64;  // the DC scans: MCU order, dummies included
    const long long by = i / a.bw, bx = i % a.bw;
    if (a.comp) return a.coefs + ((by * a.mx + bx) * a.nb + a.ny + a.comp - 1) * 64;
    const long long m = (by / a.vy) * a.mx + bx / a.hy;
    return a.coefs + (m * a.nb + (by % a.vy) * a.hy + bx % a.hy) * 64;
}

// The DC first scan's difference of block i (MCU order): the block before it of the same component, 0 for the first.
__device__ inline int dc_first_diff(const ProgArgs& a, long long i) {
    const long long m = i / a.nb;
    const int k = (int)(i % a.nb);
    const int16_t* c = a.coefs + m * a.nb * 64;
    int pred = 0;
    if (k >= 1 && k < a.ny)
        pred = c[(k - 1) * 64];
    else if (m > 0)
        pred = c[(k == 0 ? a.ny - 1 : k) * 64 - a.nb * 64];
    return (c[k * 64] >> a.Al) - (pred >> a.Al);
}

__device__ inline int dc_slot(const ProgArgs& a, long long i) { return (int)(i % a.nb) < a.ny ? 0 : 1; }

// jcphuff.c encode_mcu_AC_first / encode_mcu_AC_refine over one block, the carried EOB run left out: every symbol and raw bit
// the block emits itself goes to `sink` (sym(symbol), raw(value, n <= 32)); returns whether it coded a symbol, whether it ends
// joining the run, and the correction bits it leaves buffered (count and values, oldest first).
struct BlockTail {
    bool coded, joins;
    int br;
    u64 brv;
};

template <class Sink>
__device__ inline BlockTail walk_ac(const ProgArgs& a, const int16_t* blk, Sink& sink) {
    int16_t v[64];
    const int4* src = reinterpret_cast<const int4*>(blk);
    for (int j = 0; j < 8; ++j) *reinterpret_cast<int4*>(&v[8 * j]) = src[j];
    BlockTail t{false, false, 0, 0};
    int r = 0;
    if (a.Ah == 0) {
        for (int k = a.Ss; k <= a.Se; ++k) {
            const int c = v[k];
            const int m = (c < 0 ? -c : c) >> a.Al;
            if (m == 0) {
                ++r;
                continue;
            }
            t.coded = true;
            for (; r > 15; r -= 16) sink.sym(0xF0);
            const int n = 32 - __clz(m);
            sink.sym((r << 4) + n);
            sink.raw((uint32_t)(c < 0 ? ~m : m), n);
            r = 0;
        }
        t.joins = r > 0;
        return t;
    }
    int eob = 0;
    for (int k = a.Ss; k <= a.Se; ++k)
        if (((v[k] < 0 ? -v[k] : v[k]) >> a.Al) == 1) eob = k;
    for (int k = a.Ss; k <= a.Se; ++k) {
        const int c = v[k];
        const int m = (c < 0 ? -c : c) >> a.Al;
        if (m == 0) {
            ++r;
            continue;
        }
        while (r > 15 && k <= eob) {
            t.coded = true;
            sink.sym(0xF0);
            r -= 16;
            sink.bits64(t.brv, t.br);
            t.br = 0, t.brv = 0;
        }
        if (m > 1) {
            t.brv = (t.brv << 1) | (u64)(m & 1);
            ++t.br;
            sink.correction();
            continue;
        }
        t.coded = true;
        sink.sym((r << 4) + 1);
        sink.raw(c < 0 ? 0u : 1u, 1);
        sink.bits64(t.brv, t.br);
        t.br = 0, t.brv = 0, r = 0;
    }
    t.joins = r > 0 || t.br > 0;
    return t;
}

// ------------------------------------------------------------------------------------------------------------------- 1. flags
struct CountSink {
    uint32_t* hist;  // LDS [256] of the slot
    uint32_t corr = 0;
    __device__ void sym(int s) { atomicAdd(&hist[s], 1u); }
    __device__ void raw(uint32_t, int) {}
    __device__ void bits64(u64, int) {}
    __device__ void correction() { ++corr; }
};

__global__ __launch_bounds__(256) void prog_flags_kernel(ProgArgs a) {
    __shared__ uint32_t h[2][256];
    __shared__ uint32_t s_corr;
    for (int j = threadIdx.x; j < 512; j += blockDim.x) (&h[0][0])[j] = 0;
    if (threadIdx.x == 0) s_corr = 0;
    __syncthreads();
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n) {
        if (a.Ss == 0) {
            if (a.Ah == 0) atomicAdd(&h[dc_slot(a, i)][min(nbits_of(dc_first_diff(a, i)), 15)], 1u);
        } else {
            CountSink sink{h[0]};
            const BlockTail t = walk_ac(a, block_ptr(a, i), sink);
            a.ecount[i] = t.joins ? 1 : 0;
            a.bcount[i] = (u64)t.br;
            a.ccount[i] = t.coded ? 1 : 0;
            if (sink.corr) atomicAdd(&s_corr, sink.corr);
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < 512; j += blockDim.x) {
        const uint32_t c = (&h[0][0])[j];
        if (c) atomicAdd(&a.freq[j], (u64)c);
    }
    if (threadIdx.x == 0 && s_corr) atomicAdd(a.extra, (u64)s_corr);
}

// -------------------------------------------------------------------------------------------------------------------- 2. runs
// The first t in [lo, hi] with p[t] >= target (p non-decreasing), or hi + 1.
__device__ inline long long lower_bound_u64(const u64* p, long long lo, long long hi, u64 target) {
    long long l = lo, h = hi + 1;
    while (l < h) {
        const long long mid = l + ((h - l) >> 1);
        if (p[mid] >= target)
            h = mid;
        else
            l = mid + 1;
    }
    return l;
}

// Per block i: the run that would start at i ends at the first cap (EOBRUN reaching 0x7FFF, more than 937 buffered bits) before
// the next coded block, whose first symbol flushes it otherwise; jump[0][i] = the next run start after a cap inside the stretch,
// else n.  runs[i] = the run's length (kept by finalize for the marked starts only), mark[i] = i starts a stretch.
__global__ __launch_bounds__(256) void prog_next_kernel(ProgArgs a) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long n = a.n;
    if (i > n) return;
    if (i == n) {
        a.jump[n] = (uint32_t)n;
        a.mark[n] = 0;
        return;
    }
    const u64* E = a.ecount;
    const u64* B = a.bcount;
    const u64* C = a.ccount;
    const bool coded = C[i + 1] > C[i];
    const long long t_c = lower_bound_u64(C, i + 2, n, C[i + 1] + 1);
    const long long se = t_c <= n ? t_c - 1 : n;  // the next coded block (n: none)
    const long long t_e = lower_bound_u64(E, i + 1, n, E[i] + jpeg::kProgEobrunMax);
    const long long t_b = lower_bound_u64(B, i + 1, n, B[i] + jpeg::kProgMaxBE + 1);
    const long long cap = std::min(t_e, t_b) - 1;  // (n when neither cap is reached)
    long long end, nxt = n;
    if (cap < se) {
        end = cap;
        if (cap + 1 < se) nxt = cap + 1;
    } else {
        end = se - 1;
    }
    a.jump[i] = (uint32_t)nxt;
    a.runs[i] = (uint32_t)(E[end + 1] - E[i]);
    a.mark[i] = (i == 0 || coded) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void prog_double_kernel(const uint32_t* prev, uint32_t* next, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) next[i] = prev[prev[i]];
}

// Level k of the marking, from the top level down: every marked start marks the start 2^k links after it.  (A start marked
// during this launch may mark its own successor 2^k links on; that one is a start of the same chain, so the result is the same.)
__global__ __launch_bounds__(256) void prog_mark_kernel(const uint32_t* jump, uint32_t* mark, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && mark[i]) mark[jump[i]] = 1u;
}

__global__ __launch_bounds__(256) void prog_finalize_kernel(ProgArgs a) {
    __shared__ uint32_t h[16];
    if (threadIdx.x < 16) h[threadIdx.x] = 0;
    __syncthreads();
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n) {
        if (!a.mark[i])
            a.runs[i] = 0;
        else if (a.runs[i])
            atomicAdd(&h[31 - __clz((int)a.runs[i])], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 16 && h[threadIdx.x]) atomicAdd(&a.freq[threadIdx.x << 4], (u64)h[threadIdx.x]);
}

// ------------------------------------------------------------------------------------------------------------ 3. bits, 4. pack
struct Codes {
    uint32_t c[2][256];
};

struct LenSink {
    const uint32_t* code;  // the slot's (code << 8) | length
    u64 bits = 0;
    __device__ void sym(int s) { bits += code[s] & 0xFF; }
    __device__ void raw(uint32_t, int n) { bits += (u64)n; }
    __device__ void bits64(u64, int n) { bits += (u64)n; }
    __device__ void correction() {}
};

// Big-endian bits from bit `pos` of the packed scan: whole words this block owns are stored, the first and last (which it may
// share with its neighbours) ORed in.
struct PackSink {
    const uint32_t* code;
    uint32_t* words;
    u64 w, first_w;  // the word being filled; the first one (shared when the block starts inside it)
    bool shared_first;
    int fill;        // bits of word w taken (the neighbour's included)
    u64 buf;         // word w and the next, top-aligned
    __device__ PackSink(const uint32_t* c, uint32_t* wd, u64 pos)
        : code(c), words(wd), w(pos >> 5), first_w(pos >> 5), shared_first((pos & 31) != 0), fill((int)(pos & 31)), buf(0) {}
    __device__ void store_word() {
        const uint32_t x = (uint32_t)(buf >> 32);
        if (w == first_w && shared_first)
            atomicOr(&words[w], x);
        else
            words[w] = x;
        ++w;
        buf <<= 32;
        fill -= 32;
    }
    __device__ void raw(uint32_t v, int n) {  // n in 0..32
        if (n == 0) return;
        buf |= ((u64)(v & (uint32_t)((1ull << n) - 1)) << (64 - n)) >> fill;
        fill += n;
        if (fill >= 32) store_word();
    }
    __device__ void sym(int s) {
        const uint32_t e = code[s];
        raw(e >> 8, (int)(e & 0xFF));
    }
    __device__ void bits64(u64 v, int n) {  // n in 0..63, oldest bit highest
        if (n > 32) {
            raw((uint32_t)(v >> 32), n - 32);
            n = 32;
        }
        raw((uint32_t)v, n);
    }
    __device__ void correction() {}
    __device__ void finish() {
        if (fill > 0) atomicOr(&words[w], (uint32_t)(buf >> 32));
    }
};

// Everything block i emits in the scan, into `sink` (one of the two above).
template <class Sink>
__device__ inline void emit_block(const ProgArgs& a, long long i, Sink& sink, const uint32_t (*codes)[256]) {
    if (a.Ss == 0) {
        if (a.Ah) {
            sink.raw((uint32_t)((block_ptr(a, i)[0] >> a.Al) & 1), 1);
            return;
        }
        const int d = dc_first_diff(a, i), n = nbits_of(d);
        sink.code = codes[dc_slot(a, i)];
        sink.sym(n);
        sink.raw((uint32_t)(d < 0 ? d - 1 : d), n);
        return;
    }
    const BlockTail t = walk_ac(a, block_ptr(a, i), sink);
    const uint32_t run = a.runs[i];
    if (run) {
        const int nb = 31 - __clz((int)run);
        sink.sym(nb << 4);
        sink.raw(run, nb);
    }
    sink.bits64(t.brv, t.br);
}

__global__ __launch_bounds__(256) void prog_bits_kernel(ProgArgs a, Codes codes, u64* offsets) {
    __shared__ uint32_t s_c[2][256];
    for (int j = threadIdx.x; j < 512; j += blockDim.x) (&s_c[0][0])[j] = (&codes.c[0][0])[j];
    __syncthreads();
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    LenSink sink{s_c[0]};
    emit_block(a, i, sink, s_c);
    offsets[i] = sink.bits;
}

__global__ __launch_bounds__(256) void prog_zero_kernel(uint32_t* words, const u64* offsets, long long n, u64 max_words) {
    const u64 nw = std::min<u64>((offsets[n] + 31) / 32, max_words);
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < nw; j += (u64)gridDim.x * blockDim.x) words[j] = 0;
}

__global__ __launch_bounds__(256) void prog_pack_kernel(ProgArgs a, Codes codes, const u64* offsets, uint32_t* words, u64 bound_bits) {
    __shared__ uint32_t s_c[2][256];
    for (int j = threadIdx.x; j < 512; j += blockDim.x) (&s_c[0][0])[j] = (&codes.c[0][0])[j];
    __syncthreads();
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n || offsets[a.n] > bound_bits) return;  // (the host checked the exact bits against the words' bound)
    PackSink sink(s_c[0], words, offsets[i]);
    emit_block(a, i, sink, s_c);
    sink.finish();
}

// ---------------------------------------------------------------------------------------------------------------- 5. stuffing
struct ScanHeader {
    uint8_t b[jpeg::kProgScanHeaderMax];
};
struct FrameHeader {
    uint8_t b[jpeg::kProgFrameHeaderBytes];
};

// state[0] = the file position, state[1] = overflow
__device__ inline uint32_t scan_byte(const uint32_t* words, u64 j, u64 total_bits) {
    uint32_t b = (words[j >> 2] >> (24 - 8 * (j & 3))) & 0xFF;
    if (j == (total_bits - 1) / 8 && (total_bits & 7)) b |= 0xFFu >> (total_bits & 7);
    return b;
}

__global__ __launch_bounds__(256) void prog_ff_count_kernel(const uint32_t* words, const u64* offsets, long long n, u64* chunks,
                                                            u64 bound_bits) {
    __shared__ int wave_tot[4];
    const u64 total = offsets[n], hi = total > bound_bits ? 0 : (total + 7) / 8;
    const u64 b0 = (u64)blockIdx.x * jpeg::kStuffChunk + threadIdx.x * 16;
    int cnt = 0;
    for (int j = 0; j < 16; ++j)
        if (b0 + j < hi) cnt += scan_byte(words, b0 + j, total) == 0xFF;
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
    if ((threadIdx.x & 63) == 0) wave_tot[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) chunks[blockIdx.x] = (u64)(wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3]);
}

// Where the scan's data goes and whether it fits: [pos + header, end), EOI after the last scan included.
// (A scan past the words' bound -- which the host's exact count rules out -- counts as not fitting.)
__device__ inline bool scan_fits(const u64* offsets, long long n, const u64* chunks, long long n_chunks, const u64* state, int hdr_len,
                                 u64 out_cap, u64 bound_bits, u64& base, u64& end) {
    base = state[0] + (u64)hdr_len;
    end = base + (offsets[n] + 7) / 8 + chunks[n_chunks];
    return !state[1] && offsets[n] <= bound_bits && end + 2 <= out_cap;
}

__global__ __launch_bounds__(256) void prog_scatter_kernel(const uint32_t* words, const u64* offsets, long long n, const u64* chunks,
                                                           long long n_chunks, const u64* state, int hdr_len, uint8_t* out,
                                                           u64 out_cap, u64 bound_bits) {
    __shared__ int wave_tot[4];
    u64 base, end;
    if (!scan_fits(offsets, n, chunks, n_chunks, state, hdr_len, out_cap, bound_bits, base, end)) return;  // (uniform over the grid)
    const u64 total = offsets[n], hi = (total + 7) / 8;
    if ((u64)blockIdx.x * jpeg::kStuffChunk >= hi) return;  // (the whole workgroup)
    const u64 b0 = (u64)blockIdx.x * jpeg::kStuffChunk + threadIdx.x * 16;
    uint32_t bytes[16];
    int cnt = 0;
    for (int j = 0; j < 16; ++j) {
        bytes[j] = b0 + j < hi ? scan_byte(words, b0 + j, total) : 0;
        cnt += b0 + j < hi && bytes[j] == 0xFF;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = cnt;
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    if (lane == 63) wave_tot[w] = inc;
    __syncthreads();
    u64 ff = chunks[blockIdx.x] + (u64)(inc - cnt);
    for (int k = 0; k < w; ++k) ff += (u64)wave_tot[k];
    uint8_t* o = out + base;
    for (int j = 0; j < 16; ++j) {
        if (b0 + j >= hi) break;
        const u64 at = b0 + j + ff;
        o[at] = (uint8_t)bytes[j];
        if (bytes[j] == 0xFF) {
            o[at + 1] = 0;
            ++ff;
        }
    }
}

// The scan's header in front of its data and the file position moved past it; after the last scan EOI and the length.
__global__ __launch_bounds__(256) void prog_scan_finish_kernel(const u64* offsets, long long n, const u64* chunks, long long n_chunks,
                                                               u64* state, ScanHeader h, int hdr_len, uint8_t* out, u64 out_cap,
                                                               u64 bound_bits, int last, u64* out_len) {
    u64 base, end;
    const bool fits = scan_fits(offsets, n, chunks, n_chunks, state, hdr_len, out_cap, bound_bits, base, end);
    if (fits)
        for (int j = threadIdx.x; j < hdr_len; j += blockDim.x) out[state[0] + j] = h.b[j];
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (!fits) state[1] = 1;
    else state[0] = end;
    if (last) {
        if (state[1]) {
            *out_len = 0;
        } else {
            out[end] = 0xFF;
            out[end + 1] = 0xD9;
            *out_len = end + 2;
        }
    }
}

__global__ __launch_bounds__(256) void prog_begin_kernel(FrameHeader h, uint8_t* out, u64 out_cap, u64* state) {
    const bool fits = out_cap >= (u64)jpeg::kProgFrameHeaderBytes + 2;
    if (fits)
        for (int j = threadIdx.x; j < jpeg::kProgFrameHeaderBytes; j += blockDim.x) out[j] = h.b[j];
    if (threadIdx.x == 0) {
        state[0] = jpeg::kProgFrameHeaderBytes;
        state[1] = fits ? 0 : 1;
    }
}

ProgArgs prog_args(const JpegEncodeArgs& e, const jpeg::ProgScratch& P, int scan) {
    uint8_t* base = static_cast<uint8_t*>(e.scratch);
    const jpeg::Layout l = jpeg::layout(e.sampling);
    const jpeg::ProgScan& s = jpeg::prog_scan(scan);
    const jpeg::ProgGeom g = jpeg::prog_geom(e.H, e.W, e.sampling, scan);
    ProgArgs a;
    a.coefs = reinterpret_cast<const int16_t*>(base + P.coefs);
    a.nb = l.nb, a.ny = l.ny, a.hy = l.mw / 8, a.vy = l.mh / 8, a.mx = (e.W + l.mw - 1) / l.mw;
    a.Ss = s.Ss, a.Se = s.Se, a.Ah = s.Ah, a.Al = s.Al, a.comp = s.comp;
    a.n = (long long)g.n, a.bw = g.bw;
    a.ecount = reinterpret_cast<u64*>(base + P.ecount);
    a.bcount = reinterpret_cast<u64*>(base + P.bcount);
    a.ccount = reinterpret_cast<u64*>(base + P.ccount);
    a.jump = reinterpret_cast<uint32_t*>(base + P.jump);
    a.mark = reinterpret_cast<uint32_t*>(base + P.mark);
    a.runs = reinterpret_cast<uint32_t*>(base + P.runs) + P.run_at[scan];
    u64* freq = reinterpret_cast<u64*>(base + P.freq);
    a.freq = freq + (size_t)scan * 512;
    a.extra = freq + (size_t)jpeg::kProgScans * 512 + scan;
    return a;
}

inline unsigned groups(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

hipError_t launch_jpeg_prog_stats(const JpegEncodeArgs& e, hipStream_t s) {
    const jpeg::ProgScratch P = jpeg::prog_scratch_layout(e.H, e.W, e.sampling);
    hipError_t err = launch_jpeg_transform(e, s);
    if (err != hipSuccess) return err;
    uint8_t* base = static_cast<uint8_t*>(e.scratch);
    if ((err = hipMemsetAsync(base + P.freq, 0, jpeg::kProgFreqWords * sizeof(u64), s)) != hipSuccess) return err;
    u64* partial = reinterpret_cast<u64*>(base + P.partial);
    for (int scan = 0; scan < jpeg::kProgScans; ++scan) {
        const ProgArgs a = prog_args(e, P, scan);
        if (a.Ss == 0 && a.Ah) continue;  // (the DC refinement: no symbols, one bit per block)
        launch_k(prog_flags_kernel, dim3(groups(a.n)), dim3(256), 0, s, a);
        if (a.Ss == 0) continue;
        jpeg_scan_u64(a.ecount, a.n, partial, s);
        jpeg_scan_u64(a.bcount, a.n, partial, s);
        jpeg_scan_u64(a.ccount, a.n, partial, s);
        launch_k(prog_next_kernel, dim3(groups(a.n + 1)), dim3(256), 0, s, a);
        const int levels = jpeg::prog_levels((uint64_t)a.n, a.Ah != 0);
        const size_t stride = (size_t)a.n + 1;
        for (int k = 1; k < levels; ++k)
            launch_k(prog_double_kernel, dim3(groups(a.n + 1)), dim3(256), 0, s, (const uint32_t*)(a.jump + (k - 1) * stride),
                     a.jump + k * stride, a.n);
        for (int k = levels - 1; k >= 0; --k)
            launch_k(prog_mark_kernel, dim3(groups(a.n)), dim3(256), 0, s, (const uint32_t*)(a.jump + k * stride), a.mark, a.n);
        launch_k(prog_finalize_kernel, dim3(groups(a.n)), dim3(256), 0, s, a);
    }
    return take_launch_status();
}

hipError_t launch_jpeg_prog_pack(const JpegEncodeArgs& e, const uint8_t* frame_header, const ProgScanPlan* plans, uint64_t out_cap,
                                 hipStream_t s) {
    const jpeg::ProgScratch P = jpeg::prog_scratch_layout(e.H, e.W, e.sampling);
    uint8_t* base = static_cast<uint8_t*>(e.scratch);
    u64* offsets = reinterpret_cast<u64*>(base + P.offsets);
    uint32_t* words = reinterpret_cast<uint32_t*>(base + P.words);
    u64* chunks = reinterpret_cast<u64*>(base + P.chunks);
    u64* partial = reinterpret_cast<u64*>(base + P.partial);
    u64* state = reinterpret_cast<u64*>(base + P.freq) + jpeg::kProgScans * 512 + jpeg::kProgScans;
    FrameHeader fh;
    for (int j = 0; j < jpeg::kProgFrameHeaderBytes; ++j) fh.b[j] = frame_header[j];
    launch_k(prog_begin_kernel, dim3(1), dim3(256), 0, s, fh, e.out, (u64)out_cap, state);
    const u64 bound_bits = (u64)P.scan_words * 32;
    for (int scan = 0; scan < jpeg::kProgScans; ++scan) {
        const ProgArgs a = prog_args(e, P, scan);
        const ProgScanPlan& pl = plans[scan];
        Codes codes;
        for (int k = 0; k < 2; ++k)
            for (int v = 0; v < 256; ++v) codes.c[k][v] = pl.codes[k][v];
        ScanHeader h;
        for (int j = 0; j < jpeg::kProgScanHeaderMax; ++j) h.b[j] = j < pl.header_len ? pl.header[j] : 0;
        launch_k(prog_bits_kernel, dim3(groups(a.n)), dim3(256), 0, s, a, codes, offsets);
        jpeg_scan_u64(offsets, a.n, partial, s);
        launch_k(prog_zero_kernel, dim3((unsigned)std::min<u64>((P.scan_words + 255) / 256, 4096)), dim3(256), 0, s, words,
                 (const u64*)offsets, a.n, (u64)P.scan_words);
        launch_k(prog_pack_kernel, dim3(groups(a.n)), dim3(256), 0, s, a, codes, (const u64*)offsets, words, bound_bits);
        launch_k(prog_ff_count_kernel, dim3((unsigned)P.stuff_chunks), dim3(256), 0, s, (const uint32_t*)words, (const u64*)offsets, a.n,
                 chunks, bound_bits);
        jpeg_scan_u64(chunks, (long long)P.stuff_chunks, partial, s);
        launch_k(prog_scatter_kernel, dim3((unsigned)P.stuff_chunks), dim3(256), 0, s, (const uint32_t*)words, (const u64*)offsets, a.n,
                 (const u64*)chunks, (long long)P.stuff_chunks, (const u64*)state, pl.header_len, e.out, (u64)out_cap, bound_bits);
        launch_k(prog_scan_finish_kernel, dim3(1), dim3(256), 0, s, (const u64*)offsets, a.n, (const u64*)chunks,
                 (long long)P.stuff_chunks, state, h, pl.header_len, e.out, (u64)out_cap, bound_bits, scan == jpeg::kProgScans - 1 ? 1 : 0,
                 e.out_len);
    }
    return take_launch_status();
}

}  // namespace r2f
