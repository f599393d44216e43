/*
 * r2f.h -- C ABI of libr2f_hip.so: the MI355X (gfx950) film-emulation render path.
 *
 * This is the drop-in boundary under raw2film's processor objects.  The reference has no
 * FFI for this path (it is Python + WGSL); each entry point below names the reference
 * interface it stands in for (paths relative to /root/reference/src/raw2film/).
 *
 * Conventions
 *   - every function returns 0 on success, a negative R2F_E* code on failure;
 *     r2f_last_error(ctx) gives the message (thread-compatible: one ctx, one thread at a time,
 *     like the reference's processor objects -- gui.py:2119-2129).
 *   - `const float* host_*` arguments are HOST pointers (LUTs / stencils, copied to the device);
 *     image buffers are DEVICE pointers owned by the caller (torch tensors on the Python side).
 *   - all launches are asynchronous on `stream` (a hipStream_t passed as void*; NULL = default).
 *   - images are fp32.  Frame = H_global x W pixels; a call may address a row shard of it.
 *
 * No torch / C++ types cross this boundary.
 */
#ifndef R2F_H
#define R2F_H

#include <stddef.h>
#include <stdint.h>

/* The library is built with -fvisibility=hidden: the entry points below are its ONLY dynamic symbols (tests/test_lib_symbols.py
 * compares `nm -D --defined-only` with this header), so two builds of it can live in one process without interposing each other. */
#if defined(__GNUC__) || defined(__clang__)
#define R2F_API __attribute__((visibility("default")))
#else
#define R2F_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct r2f_ctx r2f_ctx;

enum {
    R2F_OK = 0,
    R2F_EINVAL = -1,   /* bad argument / missing LUT or stencil for an enabled stage */
    R2F_EHIP = -2,     /* a HIP runtime call failed */
    R2F_ETOOLARGE = -3 /* stencil does not fit the LDS tile configurations */
};

/* in_layout of r2f_render / r2f_stage_front */
enum {
    R2F_LAYOUT_HWC3 = 0, /* (H, W, 3) interleaved -- cpu_processor.py:136 `tex_input`            */
    R2F_LAYOUT_HWC4 = 1, /* (H, W, 4), alpha ignored -- gpu_processor.py:765 `image_array`        */
    R2F_LAYOUT_CHW = 2   /* 3 planes of (H, W) -- the device-native layout                         */
};

/* `which` of r2f_set_kernel */
enum { R2F_KERNEL_HALATION = 0, R2F_KERNEL_MTF = 1, R2F_KERNEL_GRAIN = 2 };

/* r2f_params.flags: stage gates, same conditions as cpu_processor.py:368,382,387 */
enum {
    R2F_F_MATRIX = 1u << 0,   /* S0: apply the 3x3 set by r2f_set_matrix3x3 (off = input already XYZ) */
    R2F_F_HALATION = 1u << 1, /* S2 */
    R2F_F_MTF = 1u << 2,      /* S5 */
    R2F_F_GRAIN = 1u << 3,    /* S6 (+ the clip of cpu_processor.py:397) */
    R2F_F_GRAIN_MONO = 1u << 4, /* grain == 1: noise_bw.wgsl */
    R2F_F_BURN = 1u << 5,       /* S7 highlight burn (effects.py:396-418), needs burn_* below */
    R2F_F_IDENTITY_DONE = 1u << 6, /* r2f_stage_halation only: the channels whose halation stencil is a single tap at the anchor
                                     (the blue layer of a colour stock, effects.py:248-263) were already finished into the
                                     density planes by r2f_stage_front_split for rows [y0, y1) -- skip them */
    R2F_F_FRAME_RESIDENT = 1u << 7, /* stage entry points: do NOT write p->seed into the context's device-side frame block first;
                                     the kernels read what r2f_write_frame_params last wrote there (in stream order).  For callers
                                     that replay captured launches: the write stays outside the capture, the launches inside */
    R2F_F_TRACK_RANGE = 1u << 8,   /* r2f_stage_front (upto = EXPOSURE) / r2f_stage_front_split: merge min and max |.| of the exposure
                                     samples this call writes for the halation's FFT channels into the context's exposure-range record
                                     -- a grid of 64 x 256-pixel tiles over the GLOBAL frame, reset by r2f_write_frame_params -- which is
                                     what r2f_render's front kernel does for a whole frame.  A call whose kernel cannot record (the
                                     generic pointwise kernel: an input view that is not 16-byte aligned, destination planes that do
                                     not allow float4 stores, option front_fast = 0) marks the frame's record unusable: if any
                                     tracked call of the frame could not record, every window of the frame's halation call keeps
                                     complex128 (its rows may share a 64-row tile with rows another call recorded) */
    R2F_F_RANGE_VALID = 1u << 9    /* r2f_stage_halation: the caller has kept the record for the rows the `exposure` buffer holds for the
                                     FFT channels (own rows by R2F_F_TRACK_RANGE front calls, rows received from neighbours by
                                     r2f_stage_exposure_range): the passes may then choose the 12-byte scratch element on the device,
                                     window pair by window pair, exactly like r2f_render's (below).  A tile nobody recorded reads as
                                     "unknown" and keeps complex128 for the windows that touch it; what the flag vouches for is that
                                     recorded tiles describe THIS frame's samples (the record was reset at the start of the frame) */
};

/* `upto` of r2f_stage_front */
enum { R2F_UPTO_EXPOSURE = 0, R2F_UPTO_DENSITY = 1, R2F_UPTO_OUTPUT = 2 };

typedef struct r2f_params {
    uint32_t flags;
    uint32_t seed;      /* grain seed; upstream: random per render (gpu_processor.py:586-592).  Never a launch argument: it is
                           written to a device-side block the grain kernels read (r2f_write_frame_params) */
    float log_eps;      /* lut_1d.wgsl:24 -> 1e-6 */
    float lut3d_scale;  /* cpu_processor.py:405 -> 0.25 */
    int32_t lut3d_mode; /* 0 tetrahedral (utils.py:247, the parity target), 1 trilinear (lut_3d.wgsl) */
    int32_t burn_cell;  /* S7: ceil(min(H, W) / burn_scale), the shrink factor of effects.down_up_blur (effects.py:365) */
    float burn_strength; /* S7: highlight_burn */
    float burn_d_ref;    /* S7: negative_film.d_ref[1] (or [0]), effects.py:406 */
} r2f_params;

/* Three fp32 planes holding global rows [gy0, gy0+rows) of a frame, W floats per row. */
typedef struct r2f_planes {
    float* data;          /* device pointer to plane 0, row gy0 */
    int64_t plane_stride; /* floats between consecutive channel planes (>= rows*W) */
    int32_t gy0;
    int32_t rows;
} r2f_planes;

/* --- lifetime: GpuProcessor.__init__ / device + pipeline creation, gpu_processor.py:73-257 --- */
R2F_API int r2f_create(int device, r2f_ctx** out);
R2F_API void r2f_destroy(r2f_ctx* ctx);
R2F_API const char* r2f_last_error(const r2f_ctx* ctx);
/* "gfx950" build id + ABI version, for the loader's sanity check */
R2F_API const char* r2f_version(void);

/* --- resource upload: the _ensure_* methods, gpu_processor.py:307-611 --- */
/* S0 matrix, row-major 3x3 (data.py:128-135 for linear Rec.709 input). */
R2F_API int r2f_set_matrix3x3(r2f_ctx* ctx, const float* host_m9);
/* S1 (n, n, 3) input LUT = negative_film.get_input_lut(...)   -- _ensure_lut_2d :349-376 */
R2F_API int r2f_set_lut2d(r2f_ctx* ctx, const float* host_lut, int n);
/* S4 (4, m) density curve: row 0 xp, rows 1..3 fp              -- _ensure_lut_1d :307-347 */
R2F_API int r2f_set_curve1d(r2f_ctx* ctx, const float* host_lut4xm, int m);
/* S8 (n, n, n, 3) output LUT = create_lut(..., linear_scaling=4) -- _ensure_lut_3d :378-409 */
R2F_API int r2f_set_lut3d(r2f_ctx* ctx, const float* host_lut, int n);
/* S6c (4, m) grain LUT indexed by density                      -- _ensure_grain_lut :565-611 */
R2F_API int r2f_set_grain_lut(r2f_ctx* ctx, const float* host_lut4xm, int m);
/* S2/S5/S6b stencil, (kh, kw, kc) row-major, kc in {1, 3}; correlation, anchor (kh/2, kw/2)
 *   -- _ensure_halation_kernel :498-545, _ensure_mtf_kernel :411-451, _ensure_grain_kernel :453-496 */
R2F_API int r2f_set_kernel(r2f_ctx* ctx, int which, const float* host_khwc, int kh, int kw, int kc);

/* --- whole-frame render: CpuProcessor.process hot loop cpu_processor.py:363-407,
 *     GpuProcessor._execute_gpu_pipeline gpu_processor.py:1756-1877 ---
 * in: device image (in_layout), H x W.  out_f32_hwc / out_u8_hwc: device (H, W, 3), either may be NULL.
 * workspace: device scratch of at least r2f_workspace_bytes(...) bytes (caller-owned, 16-byte aligned): the plane sets between the
 * stages; nothing past workspace_bytes is touched.
 * Stencils of >= 400 taps run as fp64 overlap-save FFTs (like cv.filter2D's own DFT branch above 11 x 11 taps, which the
 * reference's CPU path takes for both of them); their pass scratch (1 MiB per window pair in flight, 192 by default) and
 * the kernels' spectra (1 MiB per stencil channel) belong to the context, allocated on first use.
 * Scratch element of the halation's passes: complex128, or -- chosen on the device, frame by frame and WINDOW PAIR by window pair -- a
 * 12-byte element (each component a double rounded to 48 bits) when the range of the exposure samples the pair's two windows hold
 * allows it (the range comes from a grid of 64 x 256-pixel tiles the front kernel fills as it writes the exposure planes; a window
 * takes the extremes of the tiles it touches): max |x| <= bound x max(min x, first breakpoint of the density curve), the bound derived from the curve's steepest
 * cell and the element's worst error (two roundings at 2^-37 of max / shadow, x 1.5: a searched constant, tests/test_gpu_fft.py) so
 * that the element costs a density at most three fp32 ulps -- the MTF's complex64 scratch is allowed the same -- (option
 * stencil_fft_scratch96_auto, default 1; with the stand-in Portra curve windows up to max / shadow = 6.2e4 take it, wider ones
 * keep complex128 -- the headline's noise frame spans 1.4e5 as a whole and ~2e4 per window: 99 % of its window pairs take it).  The stage entry points make the same choice when their caller keeps the
 * record (R2F_F_TRACK_RANGE, r2f_stage_exposure_range, R2F_F_RANGE_VALID) and use complex128 otherwise; a row shard's windows are
 * anchored at ITS first row, so a whole-frame render and a row-sharded one agree to that element's rounding, not bit for bit.
 * Non-finite samples: in the direct form a NaN / infinity in a stencil's input comes out as NaN in every output whose tap box
 * (plus up to three zero-weight padding rows / columns) covers it, like the per-tap loop of the reference's convolution.wgsl; the FFT form takes such a sample as 0 instead (a NaN
 * handed to the transforms would come back in every output of its 256 x 512 window) -- the outputs inside the tap box are then
 * those of the frame with that sample zeroed, everything further away is untouched in both forms.  The same stencil therefore
 * treats a bad sample differently depending on which form its size selects (r2f_stencil_stats); through r2f_render both end
 * finite, because S3's max(x, log_eps) replaces a NaN (tests/test_gpu_hostile.py pins both behaviours).
 *
 * One submit per frame, like the reference's single command encoder (gpu_processor.py:1760 create_command_encoder ...
 * :1877 queue.submit): the second time a frame arrives with the same buffers, shape and parameters (the seed excepted) its
 * launches are captured into a HIP graph on a stream of the context's own and, from then on, a frame costs one write of the
 * frame block (the seed: the reference re-creates its uniform buffer `buffer_params_grain` per render, gpu_processor.py:585-597) plus one graph
 * launch on `stream`.  Any table / stencil / option change (r2f_generation) drops the graphs.  Results are the eager
 * launches', bit for bit.  r2f_set_option(ctx, "render_graph", 0) turns the replay off (A/B). */
R2F_API size_t r2f_workspace_bytes(const r2f_params* p, int H, int W);
R2F_API int r2f_render(r2f_ctx* ctx, const r2f_params* p, const void* in, int in_layout, float* out_f32_hwc,
               uint8_t* out_u8_hwc, int H, int W, void* workspace, size_t workspace_bytes, void* stream);
/* r2f_render with a 16-bit result: out_u16_hwc, device (H, W, 3) uint16, 2-byte aligned, = clip(x * 65535.0f, 0, 65535) truncated in
 * fp32 -- cpu_processor.py:407's `(image * 255).astype(uint8)` with 2 ** 16 - 1 -- of the very float out_f32_hwc receives (which may
 * be NULL).  Shares r2f_render's graph cache: which output a frame writes is part of its key, so r2f_render and r2f_render16 may
 * alternate on the same input and workspace. */
R2F_API int r2f_render16(r2f_ctx* ctx, const r2f_params* p, const void* in, int in_layout, float* out_f32_hwc, uint16_t* out_u16_hwc,
                 int H, int W, void* workspace, size_t workspace_bytes, void* stream);
/* Counters of r2f_render since r2f_create: out[0] frames replayed from a graph, out[1] graphs captured, out[2] frames launched
 * kernel by kernel, out[3] graphs dropped (context changes, evictions, failed captures). */
R2F_API int r2f_render_stats(const r2f_ctx* ctx, uint64_t* out4);

/* Introspection for the measurement harness (synchronises the device): what the front kernel of the last whole-frame render (or
 * the front / range calls of a row shard's last frame: R2F_F_TRACK_RANGE, r2f_stage_exposure_range) recorded about the exposure
 * planes the halation's FFT passes read, and what they made of it.  out4 = {min x, max |x| (the extremes over the record's tiles,
 * reduced on the host: the FRAME's range, which decides nothing by itself), bound, floor}; *armed = 1 when that render's halation
 * launches carried the rule (stencil_fft_scratch96_auto, 256-row windows, real spectrum: r2f_render above), *packed = 1 when EVERY
 * window pair then took the 12-byte scratch element (r2f_frame_scratch_choice has the counts).
 * Valid until the next write of the frame block (the next render).  Nothing upstream corresponds to it. */
R2F_API int r2f_frame_exposure_range(r2f_ctx* ctx, float* out4, int* armed, int* packed);
/* The choice itself, which is made PER WINDOW PAIR since round 6 (a pair's two windows' own range, from a grid of 64 x 256-pixel tiles
 * the front kernel fills beside the frame-level extremes): of the *pairs window pairs per channel of the last halation call that chose
 * on the device, *packed_pairs took the 12-byte element (r2f_frame_exposure_range's *packed = all of them).  0 / 0 when the last call
 * did not choose.  Synchronises the device; introspection for the measurement harness and the tests. */
R2F_API int r2f_frame_scratch_choice(r2f_ctx* ctx, int* pairs, int* packed_pairs);
/* The same choice pair by pair: flags[i] = 1 when window pair i (per channel; its windows are 2 i and 2 i + 1 in row-major order over the
 * call's grid of windows, r2f_plan_fft) took the 12-byte element.  At most `capacity` flags are written; *count = pairs per channel
 * (0 when the last halation call did not choose).  Synchronises the device.  What tools/scratch_choice_model.py checks against a host
 * model of the samples each pair's windows hold: a pair may take the element only if ITS samples allow it. */
R2F_API int r2f_frame_scratch_flags(r2f_ctx* ctx, int32_t* flags, int capacity, int* count);

/* The per-render uniform write: p->seed -> the context's device-side frame block, asynchronously on `stream`
 * (gpu_processor.py:585-597: the uniform buffer `buffer_params_grain` with a fresh random seed, made ahead of the dispatches;
 * noise.wgsl:1-6 reads it).  r2f_render and, unless R2F_F_FRAME_RESIDENT is set, every stage entry point that makes grain does this itself.
 * ONE STREAM IN FLIGHT PER CONTEXT: the frame block, like the context's FFT scratch, internal streams and capture stream, exists once
 * per context.  Frames (or stage calls) of one context must be ordered on one stream (or by events): issued on two streams at once,
 * the write for frame B may land before frame A's grain kernels have read the seed, and both would share the scratch.  The
 * reference's processors are entered by one thread at a time for the same reason (mutable caches; gui.py:2119-2129); callers that
 * want frames in flight side by side use one context each (BatchSharder does). */
R2F_API int r2f_write_frame_params(r2f_ctx* ctx, const r2f_params* p, void* stream);

/* --- stage entry points (row-shard aware): one per compute pass of
 *     gpu_processor.py:1763-1862; used by the multi-GPU row tiler and by the parity tests.
 * A call computes global rows [y0, y1) of an H_global x W frame.  Source rows outside
 * [0, H_global) are reflected (BORDER_REFLECT_101, as cv.filter2D does on the CPU path);
 * every reflected source row must lie inside the source buffer's [gy0, gy0+rows).
 * The stencil stages (r2f_stage_halation, r2f_stage_mtf, r2f_stage_stencil, r2f_stage_chroma_nr_v) are OUT OF PLACE: a
 * destination plane that shares bytes with a source plane is refused with R2F_EINVAL (tiles and FFT batches read halo rows
 * that others would already have overwritten).  r2f_stage_grain is pointwise on the density and may run exactly in place
 * (same base, stride and first row); any other overlap is refused.
 * A call writes rows [y0, y1) of its destination -- every sample of them -- and nothing else: not the destination's other rows, not
 * the pad between its planes, not a byte in front of or behind it, and nothing of its source (tests/test_gpu_write_bounds.py).
 * Every entry point binds the context's device for the duration of the call and restores the caller's current device on
 * return, so several contexts (one per GPU) can be driven from one thread. --- */

/* S0+S1 (+S3+S4 (+S8)) pointwise.  `in` holds global rows [in_gy0, in_gy0+in_rows).
 * upto=EXPOSURE/DENSITY writes planes `dst`; upto=OUTPUT writes out_* (rows indexed from out_gy0). */
R2F_API int r2f_stage_front(r2f_ctx* ctx, const r2f_params* p, const void* in, int in_layout, int in_gy0, int in_rows,
                    int upto, const r2f_planes* dst, float* out_f32_hwc, uint8_t* out_u8_hwc, int out_gy0, int y0,
                    int y1, int W, int H_global, void* stream);
/* r2f_stage_front(upto = OUTPUT) with the 16-bit output of r2f_render16 (rows indexed from out_gy0; either output may be NULL).
 * It runs the generic pointwise kernel: the LDS-staged front kernel of the 8-bit and float outputs has no uint16 store. */
R2F_API int r2f_stage_front16(r2f_ctx* ctx, const r2f_params* p, const void* in, int in_layout, int in_gy0, int in_rows, float* out_f32_hwc,
                      uint16_t* out_u16_hwc, int out_gy0, int y0, int y1, int W, int H_global, void* stream);
/* r2f_stage_front(upto = EXPOSURE) for a frame that goes on to r2f_stage_halation, split by what the halation does to each
 * channel: a channel with a real stencil gets its exposure written to `exposure`; a channel whose halation stencil is ONE tap
 * at the anchor (f_c = 0: the blue layer of a colour stock) needs no neighbours, so its tap weight, S3 and S4 are applied here
 * and the result goes straight to `density` -- its exposure plane is not written at all.  Saves that plane's round trip and
 * the pointwise pass over it.  *finished_mask receives the channels handled that way (bit c); when it is non-zero call
 * r2f_stage_halation with R2F_F_IDENTITY_DONE.  Whole-frame use only: a row shard's neighbours need the exposure rows of
 * every channel.  Falls back to plain r2f_stage_front (mask 0) when no channel qualifies or the fast kernel does not apply. */
R2F_API int r2f_stage_front_split(r2f_ctx* ctx, const r2f_params* p, const void* in, int in_layout, int in_gy0, int in_rows,
                          const r2f_planes* exposure, const r2f_planes* density, int y0, int y1, int W, int H_global,
                          int* finished_mask, void* stream);
/* A row shard's half of r2f_render's exposure-range record: min and max |.| of rows [y0, y1) and [y2, y3) of `exposure` (the
 * channels whose halation stencil takes the FFT form) merged into the context's record (its tiles), in stream order -- for the halo rows a
 * rank received from its neighbours above and below, in one launch (an empty range is skipped; its own rows are recorded by the
 * front kernel, R2F_F_TRACK_RANGE).  Nothing upstream corresponds to it. */
R2F_API int r2f_stage_exposure_range(r2f_ctx* ctx, const r2f_planes* exposure, int y0, int y1, int y2, int y3, int W, void* stream);
/* S2 halation stencil on exposure + S3 log + S4 curve -> density planes.  With R2F_F_RANGE_VALID the FFT passes choose their
 * scratch element on the device, per window pair, from the exposure-range record (see r2f_render); without it they keep complex128. */
R2F_API int r2f_stage_halation(r2f_ctx* ctx, const r2f_params* p, const r2f_planes* exposure, const r2f_planes* density,
                       int y0, int y1, int W, int H_global, void* stream);
/* S5 MTF stencil on density -> density planes. */
R2F_API int r2f_stage_mtf(r2f_ctx* ctx, const r2f_params* p, const r2f_planes* density_in, const r2f_planes* density_out,
                  int y0, int y1, int W, int H_global, void* stream);
/* [S6 grain + clip] + [S7 burn subtract + clip, when burn_map != NULL] + S8 3-D LUT (+ S9 uint8 truncation)
 * -> interleaved output.  With a burn map the grain (if any) must already have been applied by r2f_stage_grain. */
R2F_API int r2f_stage_tail(r2f_ctx* ctx, const r2f_params* p, const r2f_planes* density, const float* burn_map,
                   float* out_f32_hwc, uint8_t* out_u8_hwc, int out_gy0, int y0, int y1, int W, int H_global,
                   void* stream);
/* The grain in two halves, so that the first can run on another stream while the stencils run: r2f_stage_grain_field writes
 * the grain field G = K_g * N (noise.wgsl + the convolution of grain.wgsl:63-75; a function of the seed and the pixel
 * coordinates only) for rows [y0, y1) to `field` planes; r2f_stage_tail_field is r2f_stage_tail with that field applied
 * pointwise (out = D + G * lut(D), clip, 3-D LUT) instead of being generated in the same kernel.  Same arithmetic, same
 * results as r2f_stage_tail.  Not combinable with a burn map (use r2f_stage_grain there). */
R2F_API int r2f_stage_grain_field(r2f_ctx* ctx, const r2f_params* p, const r2f_planes* field, int y0, int y1, int W, int H_global,
                          void* stream);
R2F_API int r2f_stage_tail_field(r2f_ctx* ctx, const r2f_params* p, const r2f_planes* density, const r2f_planes* field, float* out_f32,
                         uint8_t* out_u8, int out_gy0, int y0, int y1, int W, int H_global, void* stream);

/* r2f_stage_tail / r2f_stage_tail_field with a third output form beside float and uint8: out_u16_hwc, uint16 (rows, W, 3) indexed
 * from out_gy0 like the others, 2-byte aligned (a row is 6 W bytes: with an odd W no row but the first starts on more than that).
 * S9 with 16 bits: clip(x * 65535.0f, 0, 65535) truncated, cpu_processor.py:407's rule with 2 ** 16 - 1, from the same float
 * out_f32_hwc receives.  Any of the three may be NULL, not all of them; out_f32_hwc and out_u8_hwc receive exactly what
 * r2f_stage_tail writes. */
R2F_API int r2f_stage_tail16(r2f_ctx* ctx, const r2f_params* p, const r2f_planes* density, const float* burn_map, float* out_f32_hwc,
                     uint8_t* out_u8_hwc, uint16_t* out_u16_hwc, int out_gy0, int y0, int y1, int W, int H_global, void* stream);
R2F_API int r2f_stage_tail_field16(r2f_ctx* ctx, const r2f_params* p, const r2f_planes* density, const r2f_planes* field, float* out_f32,
                           uint8_t* out_u8, uint16_t* out_u16, int out_gy0, int y0, int y1, int W, int H_global, void* stream);

/* S6 grain + clip alone, density planes -> density planes (the first half of the tail when S7 is on: the burn map
 * is a function of the WHOLE grained frame, so the frame has to exist before any pixel can be finished). */
R2F_API int r2f_stage_grain(r2f_ctx* ctx, const r2f_params* p, const r2f_planes* density_in, const r2f_planes* density_out,
                    int y0, int y1, int W, int H_global, void* stream);
/* S7 part 1: area-weighted (cv.resize INTER_AREA) partial sums of the green density over rows [y0, y1) into
 * cell_sums[(H_global / burn_cell) * (W / burn_cell)] (device).  Row shards add their arrays (all-reduce SUM). */
R2F_API int r2f_stage_burn_sums(r2f_ctx* ctx, const r2f_params* p, const r2f_planes* density, float* cell_sums, int y0, int y1,
                        int W, int H_global, void* stream);
/* S7 part 2: clip(x - d_ref, 0) and gaussian_filter(sigma=3, truncate=2) on the low-res map (device -> device).
 * `scratch` holds 2 x the map size. */
R2F_API int r2f_stage_burn_map(r2f_ctx* ctx, const r2f_params* p, const float* cell_sums, float* burn_map, float* scratch, int W,
                       int H_global, void* stream);
/* Pre-path chroma noise reduction, effects.chroma_nr_filter (effects.py:547-561): XYZ -> xyY, a separable
 * (2*size+1)-tap Gaussian on the two chromaticity planes only (coordinates clamped to the frame), back to XYZ.
 * Pass 1 (rows independent): `in` -> planes {x blurred horizontally, y blurred horizontally, Y}.
 * Pass 2 (needs size rows above/below, clamped at the global edges): those planes -> XYZ planes, which
 * r2f_stage_front / r2f_render accept as R2F_LAYOUT_CHW input. */
R2F_API int r2f_stage_chroma_nr_h(r2f_ctx* ctx, const void* in, int in_layout, int in_gy0, int in_rows, const r2f_planes* dst,
                          int size, int y0, int y1, int W, void* stream);
R2F_API int r2f_stage_chroma_nr_v(r2f_ctx* ctx, const r2f_planes* src, const r2f_planes* dst, int size, int y0, int y1, int W,
                          int H_global, void* stream);

/* Pre-path down-scale to the preview / pipeline resolution: cv.resize(..., interpolation=cv.INTER_AREA) as
 * utils.resolution_scaling applies it when the target is smaller than the frame (utils.py:226-236, called at
 * cpu_processor.py:134).  `in` is a whole H x W frame (any in_layout); `dst` receives out_h x out_w planes. */
R2F_API int r2f_resize_area(r2f_ctx* ctx, const void* in, int in_layout, int H, int W, const r2f_planes* dst, int out_h, int out_w,
                    void* stream);

/* Pre-path free rotation: cv.warpAffine(rgb, rot_mat, same size, flags=cv.INTER_LINEAR) of effects.rotate (effects.py:46-52;
 * constant border 0), restricted to the window [oy, oy + out_h) x [ox, ox + out_w) that rotate()'s centred crop keeps
 * (effects.py:54-74).  m_dst_to_src: the INVERSE of cv.getRotationMatrix2D(...), 2 x 3 row-major doubles (host memory).
 * `in` is a whole H x W frame (any in_layout); `dst` receives out_h x out_w planes. */
R2F_API int r2f_warp_affine(r2f_ctx* ctx, const void* in, int in_layout, int H, int W, const double* m_dst_to_src, const r2f_planes* dst,
                    int out_h, int out_w, int oy, int ox, void* stream);

/* Pre-path lens correction from numbers the caller supplies: what effects.lens_correction (effects.py:22-43) does with the values
 * lensfun looked up -- a radial coordinate map (Modifier.apply_geometry_distortion), an 8 x 8 LANCZOS4 gather through it
 * (lensfunpy.util.remap -> cv2.remap(..., INTER_LANCZOS4), constant border 0), a clamp at 0 and a radial vignetting gain
 * (apply_color_modification).  Transverse chromatic aberration is an entry point of its own, r2f_lens_correct_tca below.  The
 * database lookup itself and an adapter from lensfunpy objects are not here.
 *
 * The definition.  Take output pixel (X, Y) of the corrected full frame.
 *   - The host rounds these constants from double: cx, cy, q = 1/(norm_radius_px*scale), inv_scale = 1/scale, c0,
 *     qv = 1/norm_radius_px.
 *   - dx = X - cx, dy = Y - cy.
 *   - u = dx*q, v = dy*q.
 *   - r2 = u*u + v*v.
 *   - The model factor f:
 *       poly3:  f = c0 + k1*r2, with c0 = 1 - k1.
 *       poly5:  f = 1 + r2*(k1 + k2*r2).
 *       ptlens: r = sqrt(r2), f = c0 + r*(c + r*(b + r*a)), with c0 = 1 - a - b - c.
 *       none:   f = 1.
 *   - g = f*inv_scale.
 *   - sx = cx + dx*g, sy = cy + dy*g.
 * Every operation is one correctly rounded fp32 operation, with no contraction.
 * Sampling restates cv2.remap(..., INTER_LANCZOS4) with constant border 0 (OpenCV's imgwarp.cpp, INTER_BITS = 5):
 *   - qx = rint(sx*32), ix = qx >> 5, fx = qx & 31.  The same for y.
 *   - Taps are rows iy-3 .. iy+4 and columns ix-3 .. ix+4.
 *   - Tap weight is fl(wy[fy][k] * wx[fx][j]).  The table is 32 x 8 float: interpolateLanczos4(p/32) (r2f_lens_phase_table).
 *   - A tap outside the frame contributes 0 (its product with the sample 0.0f is added like any other).
 *   - The sum runs per row left to right, and rows top to bottom, each starting from the first product.
 *   - Then o = max(sum, 0), evaluated as (sum < 0 ? 0 : sum).
 * With vignetting:
 *   - rv2 = (dx*qv)^2 + (dy*qv)^2.
 *   - o = o / (1 + rv2*(v1 + rv2*(v2 + rv2*v3))), an IEEE division.
 * Edge cases:
 *   - A coordinate that is NaN, infinite, or beyond the frame by more than the tap reach yields 0 without indexing anything; that
 *     decision is made in floats (on rint(sx*32), rint(sy*32)), before any conversion to int.
 *   - One coordinate serves all three channels here; r2f_lens_correct_tca gives red and blue coordinates of their own.
 *   - A fourth input channel is ignored.
 * cx = (W - 1)/2 + center_x*norm_radius_px, cy = (H - 1)/2 + center_y*norm_radius_px.
 * Parity with real OpenCV / lensfun is UNPINNED: neither is installed on any machine this project sees; what the tests pin is this
 * definition (tests/lens_model.py restates it in NumPy). */
enum { R2F_LENS_NONE = 0, R2F_LENS_POLY3 = 1, R2F_LENS_POLY5 = 2, R2F_LENS_PTLENS = 3 };
/* What the caller knows of a lens (raw2film_amd.lens.LensProfile): n_coef coefficients of `model` (0; k1; k1, k2; a, b, c), lensfun's
 * "pa" vignetting terms when has_vignetting, the optical centre's offset in units of r, a scale > 0 (or auto_scale != 0), and the
 * pixel distance at which r = 1 (0: half the diagonal, hypot(W - 1, H - 1)/2; 1 for a 1 x 1 frame). */
typedef struct r2f_lens_profile {
    int32_t model, n_coef;
    double coef[3];
    int32_t has_vignetting, auto_scale;
    double vignetting[3];
    double center[2];
    double scale;
    double norm_radius_px;
} r2f_lens_profile;
/* The fp32 constants of the definition above for one frame size; `scale` is the scale they were made for (the resolved one with
 * auto_scale), in double. */
typedef struct r2f_lens_params {
    int32_t model, vignetting;
    float cx, cy, q, inv_scale, c0;
    float k[3];  /* poly3: k1; poly5: k1, k2; ptlens: a, b, c */
    float qv;
    float v[3];
    double scale;
} r2f_lens_params;
/* Host planner (raw2film_amd/csrc/r2f_lens_plan.cpp; no GPU, no context): profile + (H, W) -> params.  R2F_EINVAL for an unknown
 * model, a coefficient count that is not the model's, a non-finite number, scale <= 0, a negative norm_radius_px, a frame size
 * below 1 x 1, or constants that do not fit a finite float.  auto_scale: the scale at which the furthest-reaching of eight probes
 * -- the four corners and the four edge midpoints of the output frame -- lands exactly on the frame boundary [0, W - 1] x
 * [0, H - 1], found by bisection in double over [1/16, 16] and rounded to the side on which every probe is inside; R2F_EINVAL when
 * that range holds no such scale.  A frame none of whose probes can leave (1 x 1) takes scale 1. */
R2F_API int r2f_lens_plan(const r2f_lens_profile* profile, int H, int W, r2f_lens_params* out);
/* The 32 x 8 phase table of the sampling: row p = interpolateLanczos4(p/32).  No GPU, no context. */
R2F_API int r2f_lens_phase_table(float* table_32x8);
/* The correction itself.  `in` is the whole H x W frame (any in_layout); `dst` receives the window [oy, oy + out_h) x
 * [ox, ox + out_w) of the corrected frame as out_h x out_w planes -- the shape of r2f_warp_affine.  The window may reach past the
 * frame: out there the map is evaluated like anywhere else.  Lanes along x, one per output pixel of a row; the phase table sits in
 * LDS, and so does the box of source texels a block's taps touch when it fits (a block whose box does not fit gathers from global
 * memory, with the same sums in the same order: results do not depend on it). */
R2F_API int r2f_lens_correct(r2f_ctx* ctx, const void* in, int in_layout, int H, int W, const r2f_lens_params* params,
                     const r2f_planes* dst, int out_h, int out_w, int oy, int ox, void* stream);

/* The lens correction with transverse chromatic aberration (TCA): red and blue sample at coordinates of their own.  This follows
 * lensfun's order: the sub-pixel callbacks (apply_subpixel_distortion) act on the coordinates the geometry callbacks produced.
 *
 * The definition.  Everything of r2f_lens_correct's up to g = f*inv_scale is unchanged.  Then:
 *   - ox = dx*g, oy = dy*g.
 *   - Green: sx = cx + ox, sy = cy + oy -- r2f_lens_correct's values, bit for bit.
 *   - Red and blue each have three constants (v, c, b) and a factor t:
 *       linear: t = v (lensfun's kr / kb).
 *       poly3:  a = ox*qv, e = oy*qv, r2 = a*a + e*e, r = sqrt(r2); t0 = r*b, t1 = c + t0, t2 = r*t1, t = v + t2
 *               (lensfun's Rd = Ru (b Ru^2 + c Ru + v)).
 *     sx_c = cx + ox*t, sy_c = cy + oy*t.
 *   - qv = 1/norm_radius_px is the one r2f_lens_params carries, filled whether or not vignetting is on.
 * Every operation is one correctly rounded fp32 operation, with no contraction.
 * Each channel runs the phase split on its own coordinate and its own 64-tap sum over its own plane only: weights fl(wy*wx) from
 * its own phases, in the same sum order.  Then the clamp at 0 and the vignetting gain of the output pixel's (dx, dy), the same
 * for all three channels.  A channel whose coordinate is outside yields 0 for that channel alone.
 * Two consequences hold bit for bit:
 *   - the green plane equals r2f_lens_correct's green plane for the same r2f_lens_params;
 *   - a record whose factors are exactly 1 -- linear (1, 1), or poly3 with v = 1, c = b = 0 -- gives r2f_lens_correct's result on
 *     all three planes.
 * Parity with lensfun is UNPINNED, like the rest of this section (tests/lens_tca_model.py restates the definition in NumPy).
 * Lensfun's other TCA variants are not here. */
enum { R2F_TCA_NONE = 0, R2F_TCA_LINEAR = 1, R2F_TCA_POLY3 = 2 };
/* What the caller knows of a lens's TCA: n_coef constants per channel of `model` -- 1 for linear (v), 3 for poly3 (v, c, b) --
 * for red and for blue.  Constants past n_coef are not read. */
typedef struct r2f_lens_tca {
    int32_t model, n_coef;
    double red[3], blue[3]; /* (v, c, b) */
} r2f_lens_tca;
/* The fp32 constants of the TCA step: the doubles rounded to float; c = b = 0 for linear. */
typedef struct r2f_lens_tca_params {
    int32_t model;
    float red[3], blue[3]; /* (v, c, b) */
} r2f_lens_tca_params;
/* r2f_lens_plan for a profile with a TCA record: r2f_lens_plan's checks, and R2F_EINVAL for an unknown TCA model (R2F_TCA_NONE
 * included: such a profile is r2f_lens_plan's), a count that is not the model's, a non-finite constant or one that does not fit a
 * float.  auto_scale: the eight probes are evaluated for all three channels -- the map in double with the TCA factor in double
 * on top -- and the furthest reach of any channel decides, so that no channel shows a border; a record whose factors are exactly 1
 * resolves to r2f_lens_plan's scale to the last bit.  Without auto_scale *out is r2f_lens_plan's, byte for byte. */
R2F_API int r2f_lens_plan_tca(const r2f_lens_profile* profile, const r2f_lens_tca* tca, int H, int W, r2f_lens_params* out,
                      r2f_lens_tca_params* out_tca);
/* The correction with TCA: r2f_lens_correct's contract for the window, the layouts and the rows of `dst`.  tca_params->model
 * R2F_TCA_NONE is refused with R2F_EINVAL (that case is r2f_lens_correct's), and so is an unknown one.  The box a block stages in
 * LDS is the union of its three channels' tap extents; results do not depend on whether a block staged. */
R2F_API int r2f_lens_correct_tca(r2f_ctx* ctx, const void* in, int in_layout, int H, int W, const r2f_lens_params* params,
                         const r2f_lens_tca_params* tca_params, const r2f_planes* dst, int out_h, int out_w, int oy, int ox,
                         void* stream);

/* The lens correction of a lens whose own projection is not rectilinear: a fisheye frame is straightened.  This is lensfun's
 * geometry conversion from the target projection (rectilinear, the only target here) to the lens's, the step
 * Modifier.apply_geometry_distortion runs between the scale and the distortion polynomial.
 *
 * The definition.  Everything of r2f_lens_correct's up to r2 = u*u + v*v is unchanged.  Then:
 *   - r = sqrt(r2), t = r*inv_focal.  inv_focal is the float rounded from 1/focal; focal is the lens's focal length in units of
 *     the normalisation radius (of r = 1).  t is the tangent of the angle theta between the ray and the axis.
 *   - The projection factor P(t): the lens's image radius over the rectilinear radius tan(theta).  With tt = t*t, s1 = 1 + tt,
 *     s = sqrt(s1):
 *       orthographic:  P = 1/s                                      (sin(theta)/t)
 *       stereographic: d = 1 + s, P = 2/d                           (2 tan(theta/2)/t)
 *       equisolid:     n = s + 1, m = 2*s, h = n/m, e = sqrt(h), b = s*e, P = 1/b     (2 sin(theta/2)/t)
 *       fisheye (equidistant): P = atan(t)/t, evaluated without a library call from the odd polynomial atan(x) ~ x*p(x*x):
 *         t <= 1:  P = p(tt)
 *         t >  1:  w = 1/t, ww = w*w, a = w*p(ww), b = pi_2 - a, P = b*w     (atan(t) = pi/2 - atan(1/t))
 *         pi_2 = 0x1.921fb6p+0f.  p(x) = c0 + x*(c1 + x*(c2 + ... + x*c9)) by Horner from c9 down -- acc = c9; then for k = 8 .. 0:
 *         acc = acc*x, acc = c_k + acc -- with
 *           c0 = 0x1p+0f          c1 = -0x1.55554p-2f   c2 = 0x1.999278p-3f   c3 = -0x1.242702p-3f  c4 = 0x1.c0d2e2p-4f
 *           c5 = -0x1.58dd68p-4f  c6 = 0x1.dd11b4p-5f   c7 = -0x1.01b21p-5f   c8 = 0x1.6a946ap-7f   c9 = -0x1.df068p-10f
 *         Measured against atan in double over every float32 t (tests/lens_projection_check.cpp, mode `atan`), in units of the
 *         last place of the exact atan(t)/t:
 *           largest error of P for t in [2^-13, 1]: 1.16 ulp
 *           largest error of P for t in (1, 64]: 2.65 ulp
 *         (below 2^-13 p(tt) is exactly 1, within half a unit of atan(t)/t.)
 *   - u' = u*P, v' = v*P, r2' = u'*u' + v'*v'.  The model factor f comes from r2' exactly as r2f_lens_correct's does from r2
 *     (ptlens takes sqrt(r2')).
 *   - g0 = f*P, g = g0*inv_scale, ox = dx*g, oy = dy*g.
 *   - From there on nothing changes: sx = cx + ox, sy = cy + oy -- or, with a TCA record, r2f_lens_correct_tca's step on
 *     (ox, oy) -- the phase split, the 64-tap sums, the clamp, and the vignetting gain of the output pixel's (dx, dy).
 * Every operation is one correctly rounded fp32 operation (the divisions and square roots included), with no contraction.
 * One consequence holds bit for bit: when focal is so large that 1 + tt rounds to 1 everywhere in the window (and, for fisheye,
 * p(tt) to 1: tt below 2^-25 does both), P is exactly 1, and the result equals r2f_lens_correct's on all three planes -- with a
 * TCA record r2f_lens_correct_tca's.
 * Not here: lensfun's thoby, panoramic and equirectangular lens types, and any target projection other than rectilinear.
 * Parity with lensfun is UNPINNED, like the rest of this section (tests/lens_projection_model.py restates the definition). */
enum {
    R2F_PROJ_NONE = 0,
    R2F_PROJ_FISHEYE = 1,
    R2F_PROJ_STEREOGRAPHIC = 2,
    R2F_PROJ_EQUISOLID = 3,
    R2F_PROJ_ORTHOGRAPHIC = 4
};
/* What the caller knows of the lens's projection: its type and its focal length in units of the normalisation radius. */
typedef struct r2f_lens_projection {
    int32_t type;
    double focal;
} r2f_lens_projection;
/* The fp32 constant of the projection step. */
typedef struct r2f_lens_projection_params {
    int32_t type;
    float inv_focal;
} r2f_lens_projection_params;
/* r2f_lens_plan (with tca == NULL and out_tca == NULL) or r2f_lens_plan_tca (with both) for a profile with a projection: their
 * checks, and R2F_EINVAL for an unknown type, R2F_PROJ_NONE (that case is the other planners'), a focal that is not finite and
 * positive, or one whose reciprocal does not fit a finite float.  Without auto_scale *out is r2f_lens_plan's, byte for byte.
 * auto_scale: the same eight probes and the same bisection over [1/16, 16]; each probe goes through the projected map in double
 * (P from std::sqrt / std::atan, then rounded to float: the precision at which the kernel applies it, so that a projection the
 * kernel cannot resolve leaves the scale r2f_lens_plan's to the last bit), with the TCA factor on top when there is a record.
 * R2F_EINVAL when the range holds no fitting scale -- a circular fisheye whose whole image circle lies inside the frame never
 * puts a probe on the boundary. */
R2F_API int r2f_lens_plan_projected(const r2f_lens_profile* profile, const r2f_lens_projection* projection, const r2f_lens_tca* tca,
                                    int H, int W, r2f_lens_params* out, r2f_lens_projection_params* out_projection,
                                    r2f_lens_tca_params* out_tca);
/* The projected correction: r2f_lens_correct's contract for the window, the layouts and the rows of `dst`.  tca_params may be
 * NULL; a record whose model is R2F_TCA_NONE or unknown is refused with R2F_EINVAL, and so is a projection of type
 * R2F_PROJ_NONE (that case is r2f_lens_correct's or r2f_lens_correct_tca's) or of an unknown type.  A block makes a 64 x 16 tile
 * and stages the box of source texels its taps touch in LDS; where a magnifying scale makes that box too large it works in two
 * halves of 64 x 8 with a box each, and only a half whose box does not fit either gathers from global memory.  The sums are the
 * same over either source in the same order: results do not depend on the route a block took. */
R2F_API int r2f_lens_correct_projected(r2f_ctx* ctx, const void* in, int in_layout, int H, int W, const r2f_lens_params* params,
                                       const r2f_lens_projection_params* projection_params,
                                       const r2f_lens_tca_params* tca_params, const r2f_planes* dst, int out_h, int out_w, int oy,
                                       int ox, void* stream);

/* Post-path up-scale of the rendered uint8 frame: utils.resolution_scaling's cv.resize(image, dsize,
 * interpolation=cv.INTER_LANCZOS4) branch (utils.py:237-242), the way back from the `max_scale` pipeline resolution to the
 * requested one (cpu_processor.py:128-134, 411-412).  src/dst: uint8 (H, W, 3) / (out_h, out_w, 3) on the device.
 * r2f_lanczos4_table is the host-side table cv::resize derives per destination index (source index of tap 3, eight weights
 * in 11-bit fixed point); exported so the tests can pin it without a GPU. */
R2F_API int r2f_resize_lanczos4_u8(r2f_ctx* ctx, const uint8_t* src_hwc, int H, int W, uint8_t* dst_hwc, int out_h, int out_w, void* stream);
R2F_API int r2f_lanczos4_table(int ssize, int dsize, int* ofs, short* coef);

/* Pre-path up-scale to a preview LARGER than the frame: utils.resolution_scaling's cv.resize(float32 frame, dsize,
 * interpolation=cv.INTER_LANCZOS4) (utils.py:237-242, called at cpu_processor.py:134).  `in`: a whole H x W float32 frame (any
 * in_layout); `dst` receives out_h x out_w planes.  r2f_lanczos4_table_f32: the host-side per-destination tables (source index
 * of tap 3, eight float weights), exported for the tests. */
R2F_API int r2f_resize_lanczos4_f32(r2f_ctx* ctx, const void* in, int in_layout, int H, int W, const r2f_planes* dst, int out_h, int out_w,
                            void* stream);
R2F_API int r2f_lanczos4_table_f32(int ssize, int dsize, int* ofs, float* coef);

/* Caller-side RGB histogram of the rendered bitmap: the counting loop of utils.generate_histogram (utils.py:160-165; GPU twin
 * histogram.wgsl pass1_accumulate, dispatched at gpu_processor.py:1149).  image_hwc: uint8 (H, W, 3) on the device, 16-byte
 * aligned; counts: 3 x 256 uint32 on the device (R bins, G bins, B bins), overwritten.  The 768-value post-processing
 * (log1p, 3-bin smoothing, bar image) is host work: raw2film_amd/histogram.py. */
R2F_API int r2f_histogram_u8(r2f_ctx* ctx, const uint8_t* image_hwc, int H, int W, uint32_t* counts, void* stream);

/* The CPU processor's last step (cpu_processor.py:411-412 -> utils.resolution_scaling, utils.py:226-236): cv.resize(uint8 frame,
 * INTER_AREA) when the rendered (and canvas-framed) frame is larger than the requested resolution.  src / dst: uint8
 * (H, W, 3) / (out_h, out_w, 3) on the device, out_h <= H, out_w <= W. */
R2F_API int r2f_resize_area_u8(r2f_ctx* ctx, const uint8_t* src_hwc, int H, int W, uint8_t* dst_hwc, int out_h, int out_w, void* stream);

/* The two post-path resamplers on a 16-bit result (r2f_render16): utils.resolution_scaling (utils.py:226-244) as
 * cpu_processor.py:411-412 applies it, on uint16 (H, W, 3) device frames, 2-byte aligned.
 *   r2f_resize_lanczos4_u16  cv.resize(uint16, INTER_LANCZOS4): OpenCV's float-weight path (the tables of r2f_lanczos4_table_f32),
 *                            the horizontal pass then the vertical one in float, saturate_cast<ushort> (round half to even, clamp
 *                            to [0, 65535]) at the end.
 *   r2f_resize_area_u16      cv.resize(uint16, INTER_AREA), out_h <= H, out_w <= W: exact 2 x 2 as (a + b + c + d + 2) >> 2, every
 *                            other ratio as the float area sum with the same rounding and clamp. */
R2F_API int r2f_resize_lanczos4_u16(r2f_ctx* ctx, const uint16_t* src_hwc, int H, int W, uint16_t* dst_hwc, int out_h, int out_w, void* stream);
R2F_API int r2f_resize_area_u16(r2f_ctx* ctx, const uint16_t* src_hwc, int H, int W, uint16_t* dst_hwc, int out_h, int out_w, void* stream);

/* Demosaic of a Bayer frame on the device from numbers the caller supplies: what raw_to_linear (raw_conversion.py:33-53) has LibRaw
 * do behind the file parser -- black / scale, demosaic (PPG, or none with half_size), camera matrix, 16-bit clip -- so that a frame
 * crosses PCIe as the sensor's 2 bytes per pixel.  The parser stays outside; its result is an r2f_raw_profile.
 * Parity with LibRaw's bytes is UNPINNED: rawpy is on no machine this project sees.  The arithmetic follows dcraw / LibRaw's
 * published scale_colors, border_interpolate(3), ppg_interpolate, the half-size green mix and convert_to_rgb; what the tests pin is
 * THIS definition (tests/demosaic_model.py restates it in NumPy).
 *
 * Inputs.  The mosaic is uint16 (H, W), H, W >= 2.  The 2 x 2 pattern gives each site its colour col(y, x) in {R, G, B} = {0, 1, 2}.
 * black[4] (int32) and mul[4] (float) are per site, indexed by k = (y & 1) * 2 + (x & 1).  M is a float 3 x 3 matrix.
 * A. Scale.  t = (int)raw - black[k]; S = clamp(trunc(fl((float)t * mul[k])), 0, 65535): one fp32 multiply, truncation toward zero.
 * B. Full size.  S is the scaled mosaic; G, R, B are the planes being filled; a site's native plane is S and is never rewritten.
 *    floor(a / 2^n) is an arithmetic shift of a signed int.
 *    B0, border ring: every pixel with y < 3, y >= H - 3, x < 3 or x >= W - 3.  Each non-native colour c is floor(sum / count) of S
 *        over the sites of colour c in the 3 x 3 neighbourhood clipped to the frame; 0 when count is 0.
 *    B1, green at the non-green sites with 3 <= y < H - 3 and 3 <= x < W - 3.  Directions h = (0, 1), v = (1, 0); P(k) is the site
 *        displaced by k steps; every G here is a native green sample.
 *          guess = 2 (G(-1) + S(0) + G(1)) - S(-2) - S(2)
 *          diff  = 3 (|S(-2) - S(0)| + |S(2) - S(0)| + |G(-1) - G(1)|) + 2 (|G(3) - G(1)| + |G(-3) - G(-1)|)
 *        v iff diff_h > diff_v, otherwise h; G = clamp(floor(guess / 4), min(G(-1), G(1)), max(G(-1), G(1))) along that direction.
 *    B2, red and blue at the green sites with 1 <= y < H - 1 and 1 <= x < W - 1, for h and for v; c is the colour of the two
 *        neighbours along the direction: C = clamp(floor((S(-1) + S(1) + 2 G(0) - G(-1) - G(1)) / 2), 0, 65535); G(+-1) from B0 or B1.
 *    B3, the opposite colour at the red and blue sites of the same range; diagonals d1 = (1, 1), d2 = (1, -1):
 *          diff_i  = |S(-d) - S(d)| + |G(-d) - G(0)| + |G(d) - G(0)|
 *          guess_i = S(-d) + S(d) + 2 G(0) - G(-d) - G(d)
 *        diff_1 != diff_2: clamp(floor(guess of the smaller diff / 2), 0, 65535); else clamp(floor((guess_1 + guess_2) / 4), 0, 65535).
 *    B2 and B3 overwrite B0's red and blue in rings 1 and 2; ring 0 keeps B0; green in rings 0 .. 2 stays B0's.  No pass reads what
 *    the same pass writes, so every output pixel is a function of S within 4 samples of it.
 * B'. Half size (upstream's default half_size=True): H and W even, output (H / 2, W / 2); pixel (y, x) comes from the quad at
 *    (2 y, 2 x): R and B are S at their sites, G = (S(g1) + S(g2)) >> 1.
 * C. Colour.  Output channel k: acc = fl(r M[k][0]); acc = fl(acc + fl(g M[k][1])); acc = fl(acc + fl(b M[k][2])): every operation
 *    one correctly rounded fp32 operation, no contraction; out = clamp(trunc(acc), 0, 65535).
 * The destination is uint16 (H_out, W_out, 3), contiguous: r2f_decode_u16's channels = 3 input. */
enum { R2F_CFA_RGGB = 0, R2F_CFA_BGGR = 1, R2F_CFA_GRBG = 2, R2F_CFA_GBRG = 3 };
/* What the caller knows of a RAW frame (raw2film_amd.raw.RawProfile): the pattern, black level and multiplier per site of the
 * 2 x 2 quad (k = (y & 1) * 2 + (x & 1)), the camera matrix row-major, and whether to take the half-size form. */
typedef struct r2f_raw_profile {
    int32_t pattern, half_size;
    double black[4];
    double mul[4];
    double matrix[9];
} r2f_raw_profile;
/* The constants of the definition above for one frame size: cfa[k] the colour id of site k, and the output's size. */
typedef struct r2f_demosaic_params {
    int32_t cfa[4];
    int32_t black[4];
    float mul[4];
    float M[9];
    int32_t half_size, out_h, out_w;
} r2f_demosaic_params;
/* Host planner (raw2film_amd/csrc/r2f_demosaic_plan.cpp; no GPU, no context): profile + (H, W) -> params.  R2F_EINVAL for an unknown
 * pattern, H or W below 2, an odd H or W with half_size, a non-finite number, a black level outside [0, 65535] or not integral, a
 * multiplier outside (0, 1024] (as a float too) and |M| above 64.  The last two bounds keep every trunc inside int32: step A's
 * product is at most 65535 * 1024 < 2^27 in magnitude, step C's sum at most 3 * 64 * 65535 < 2^24. */
R2F_API int r2f_demosaic_plan(const r2f_raw_profile* profile, int H, int W, r2f_demosaic_params* out);
/* The demosaic itself.  src_rows: uint16 mosaic rows [src_gy0, src_gy0 + src_nrows) of the H x W frame on the device, src_pitch
 * samples apart (>= W).  Writes output rows [y0, y1) of dst (uint16 (out_h, out_w, 3), row 0 at dst) and nothing else.  Full size
 * reads mosaic rows [y0 - 4, y1 + 4) clipped to [0, H), half size [2 y0, 2 y1); those rows must lie inside the source window, else
 * R2F_EINVAL before any launch.  A band's bytes are those of the same rows of a whole-frame call, whatever the cut, the pitch or
 * the source's alignment (which only select between 32-bit and 16-bit loads of the same samples).
 * Full size is one launch: a block stages its 64 x 32 tile of scaled samples with a 4-sample apron in LDS (step A once per
 * sample), derives the green plane of the tile plus a 1-sample apron there, then B2 / B3 / C per output pixel; a wave's 64 pixels
 * of a row leave through an LDS transpose as one contiguous 384-byte segment.  Half size is a lane per output pixel. */
R2F_API int r2f_demosaic_u16(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W,
                     const r2f_demosaic_params* params, uint16_t* dst_u16_hwc3, int y0, int y1, void* stream);
/* r2f_demosaic_u16's tile (test shapes are derived from it). */
enum { R2F_DEMOSAIC_TILE_W = 64, R2F_DEMOSAIC_TILE_H = 32 };
/* The demosaic fused with the hand-off below, for a mosaic that streams in row bands: with D the uint16 (out_h, out_w, 3) frame of
 * r2f_demosaic_u16's definition (full or half size) and (row0, col0, rows, cols) a non-empty window inside D,
 *   dst[y, x, c] = fminf((float)D[row0 + y, col0 + x, c] / divisor * factor, 65504.0f)
 * -- r2f_decode_u16's expression, the same two correctly rounded fp32 operations: bit-identical to r2f_decode_u16 of that window of
 * r2f_demosaic_u16's frame, without the uint16 frame in between (12 bytes per pixel of traffic and one launch less).  dst: float32
 * (rows, cols, 3), contiguous.  Writes window rows [y0, y1) of dst and nothing else.  Full size reads mosaic rows
 * [row0 + y0 - 4, row0 + y1 + 4) clipped to [0, H), half size [2 (row0 + y0), 2 (row0 + y1)); those rows must lie inside the source
 * window, else R2F_EINVAL before any launch.  The bytes depend on neither the cut, the pitch, the source's alignment nor the window's
 * origin.  Refused: everything r2f_demosaic_u16 refuses, a window that is empty or not inside D, y0 > y1, y0 < 0, y1 > rows,
 * divisor <= 0.  The kernels are r2f_demosaic_u16's with a second epilogue: the full-size tile grid stays anchored to the frame's
 * columns (an odd col0 masks lanes, it does not move the tiles), and a wave's row segment leaves as contiguous float32 (768 bytes for
 * a full tile) in 16-byte stores behind the floats that lead to a 16-byte boundary.
 * What streams with it (raw2film_amd: HipProcessor): a mosaic whose exposure is given in stops, without quarter turns, a lens step
 * or a device pre-path; exposure measured on the device (the statistic is the whole demosaiced frame's), turns and the lens step
 * keep the one-piece path r2f_demosaic_u16 -> r2f_decode_u16. */
R2F_API int r2f_demosaic_f32(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W,
                     const r2f_demosaic_params* params, int row0, int col0, int rows, int cols, float divisor, float factor,
                     float* dst_f32_hwc3, int y0, int y1, void* stream);

/* Demosaic of a mosaic with a 6 x 6 colour filter array (Fujifilm's X-Trans) on the device: the same share of raw_to_linear as the
 * Bayer path above, next to it.  LibRaw switches to its own X-Trans interpolation (Markesteijn's) for these files; THIS IS NOT
 * THAT ALGORITHM.  It is the project's own interpolation -- directional green, colour-difference red and blue -- defined here in
 * integers, and parity with LibRaw's bytes is UNPINNED: rawpy is on no machine this project sees.  What the tests pin is THIS
 * definition (tests/xtrans_model.py restates it in NumPy).  Nothing is special-cased to Fujifilm's layout: every admissible
 * pattern (below) is handled, among them the canonical GBGGRG / RGRBGB / GBGGRG / GRGGBG / BGBRGR / GRGGBG and its 36 cyclic shifts.
 *
 * Inputs.  The mosaic is uint16 (H, W), H, W >= 6.  col(y, x) = pattern[y % 6][x % 6] in {R, G, B} = {0, 1, 2}.  black[36] (int32)
 * is indexed by the site's phase (y % 6) * 6 + x % 6, mul[3] (float) by its colour.  M is a float 3 x 3 matrix.  floor(a / n) is
 * the floor division of a signed int (toward minus infinity).
 * A. Scale, as in the Bayer definition: t = (int)raw - black[phase]; S = clamp(trunc(fl((float)t * mul[col])), 0, 65535).
 * B. Full size.
 *    B0, border ring: every pixel with y < 3, y >= H - 3, x < 3 or x >= W - 3.  Each non-native colour c is floor(sum / count) of S
 *        over the sites of colour c in the 3 x 3 neighbourhood clipped to the frame; 0 when count is 0.  The native colour is S.
 *    B1, green, defined wherever B2 reads it: at the sites with 2 <= y < H - 2 and 2 <= x < W - 2.  Green at a green site is S.  At a
 *        non-green site, for the directions h = (0, 1) and v = (1, 0): a >= 1 is the distance to the nearest green site on the
 *        negative side, b >= 1 that on the positive side (an admissible pattern has a, b <= 2), S(-a) and S(+b) those two samples;
 *          est  = floor((b S(-a) + a S(+b) + floor((a + b) / 2)) / (a + b))
 *          diff = |S(-a) - S(+b)|,  span = a + b
 *        v iff diff_h span_v > diff_v span_h, otherwise h; G is that direction's est.
 *    B2, red and blue at the interior pixels 3 <= y < H - 3, 3 <= x < W - 3.  For each colour c that is not the site's own, Q is the
 *        set of sites of colour c in the centred 3 x 3; w = 2 for the four edge neighbours, 1 for the four diagonal ones:
 *          C = clamp(G(0) + floor(sum_Q w(q) (S(q) - G(q)) / sum_Q w(q)), 0, 65535),  G from B1
 *        (for c = green at a non-green site every term is 0: the green of an interior pixel is B1's).  An admissible pattern has Q
 *        non-empty.  No pass reads what the same pass writes: every output pixel is a function of S within 3 samples of it.
 * B'. Reduced size (upstream's half_size=True; for a 6 x 6 array it yields A THIRD, not a half): the output is (H / 3, W / 3),
 *    rounded down; pixel (y, x) comes from the 3 x 3 cell at (3 y, 3 x), each channel floor(sum / count) of S over the cell's sites of
 *    that colour.  Trailing rows and columns that do not fill a cell are dropped.
 * C. Colour: step C of the Bayer definition, unchanged.
 * Every intermediate stays well inside int32: B1's numerator is at most 4 * 65535 + 2, B2's at most 12 * 65535 in magnitude.
 *
 * Admissible patterns (r2f_xtrans_plan returns R2F_EINVAL otherwise): 36 colour ids in {0, 1, 2}, each colour present; every
 * non-green site has a green site within 2 on both sides along h and along v, the pattern taken cyclically; every centred 3 x 3,
 * taken cyclically, holds both colours other than its centre's; for the reduced size each of the four aligned 3 x 3 cells holds all
 * three colours (the planner checks it then, but the rule before it already says so: an aligned cell is the centred 3 x 3 of its
 * middle site, so no pattern is admissible at full size only).  The numeric bounds are r2f_demosaic_plan's: black integral in [0, 65535], multipliers in (0, 1024]
 * as floats too, |M| <= 64, every number finite.  H or W below 6 is refused. */
typedef struct r2f_xtrans_profile {
    int32_t pattern[36]; /* colour id per phase, reading order */
    int32_t reduced;
    double black[36];
    double mul[3];
    double matrix[9];
} r2f_xtrans_profile;
/* The constants of the definition for one frame size, and the per-phase tables with which no lane searches for a neighbour:
 * gap[phase] = {a_h, b_h, a_v, b_v} of B1 (0 at a green site); for slot 0 = red and slot 1 = blue, taps[phase][slot] the 3 x 3 mask
 * of Q (bit (dy + 1) * 3 + dx + 1; 0 for the site's own colour), wsum its weight sum and recip = floor(2^32 / wsum) + 1 (0 where
 * wsum <= 1), the multiplier of the floor division (r2f_xtrans_math.h has the proof of range); cell_count[(cy, cx)][c] the sites of
 * colour c in the aligned cell at phase (3 cy, 3 cx). */
typedef struct r2f_xtrans_params {
    uint8_t cfa[36];
    uint8_t gap[36][4];
    uint16_t taps[36][2];
    uint8_t wsum[36][2];
    uint8_t cell_count[4][3];
    uint32_t recip[36][2];
    int32_t black[36];
    float mul[3];
    float M[9];
    int32_t reduced, out_h, out_w;
} r2f_xtrans_params;
/* Host planner (raw2film_amd/csrc/r2f_xtrans_plan.cpp; no GPU, no context): profile + (H, W) -> params, or R2F_EINVAL for what the
 * text above refuses; a refusal leaves *out alone. */
R2F_API int r2f_xtrans_plan(const r2f_xtrans_profile* profile, int H, int W, r2f_xtrans_params* out);
/* The demosaic itself, with r2f_demosaic_u16's row-range contract.  src_rows: uint16 mosaic rows [src_gy0, src_gy0 + src_nrows) of
 * the H x W frame on the device, src_pitch samples apart (>= W).  Writes output rows [y0, y1) of dst (uint16 (out_h, out_w, 3), row
 * 0 at dst) and nothing else.  Full size reads mosaic rows [y0 - 3, y1 + 3) clipped to [0, H), reduced size [3 y0, 3 y1); those rows
 * must lie inside the source window, else R2F_EINVAL before any launch.  A band's bytes are those of the same rows of a whole-frame
 * call, whatever the cut (it need not be a multiple of 6 or 3), the pitch or the source's alignment.  Params whose tables are not
 * those the planner derives from their cfa are refused.
 * Full size is one launch shaped like the Bayer one: a block stages its 64 x 32 tile of scaled samples with a 3-sample apron in LDS
 * (step A once per sample), derives the colour-difference plane S - G of the tile plus a 1-sample apron there (B1), then B2 / C per
 * output pixel; rows leave as contiguous segments through an LDS transpose.  The phase is that of the frame, never of the tile.
 * Reduced size is a lane per output pixel.  Row bands do not stream through the pipeline yet (raw2film_amd: the one-piece path). */
R2F_API int r2f_demosaic_xtrans_u16(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W,
                     const r2f_xtrans_params* params, uint16_t* dst_u16_hwc3, int y0, int y1, void* stream);
/* r2f_demosaic_xtrans_u16's tile (test shapes are derived from it): its sides are 4 and 2 modulo 6. */
enum { R2F_XTRANS_TILE_W = 64, R2F_XTRANS_TILE_H = 32 };

/* The sensor's orientation in the demosaic.  LibRaw rotates its output by the orientation the camera recorded (sizes.flip, with
 * user_flip left alone as raw_to_linear leaves it); the two entry points below write the demosaiced frame that way round, out of the
 * LDS in which the kernels hold every finished pixel, without a second frame.  Parity with LibRaw's bytes is UNPINNED like the rest
 * of the demosaic, and so is the reading of sizes.flip: rawpy is on no machine this project sees.
 * Let D be the uint16 (out_h, out_w, 3) frame of r2f_demosaic_u16 or r2f_demosaic_xtrans_u16 (full or reduced size).  orientation
 * is an integer 0 .. 7 with LibRaw's sizes.flip bits: 4 swaps the axes, 2 mirrors rows, 1 mirrors columns -- 0 is upright, 3 is 180
 * degrees, 5 is 90 degrees counter-clockwise and 6 is 90 degrees clockwise.  The oriented frame O has shape (out_h, out_w, 3) without
 * bit 4 and (out_w, out_h, 3) with it, and O[r, c] = D[r', c'] with
 *   (a, b) = (c, r) if orientation & 4, else (r, c);  r' = out_h - 1 - a if orientation & 2, else a;  c' = out_w - 1 - b if
 *   orientation & 1, else b.
 * In NumPy: E = D; if o & 2: E = E[::-1]; if o & 1: E = E[:, ::-1]; if o & 4: E = E.transpose(1, 0, 2).
 * [y0, y1) are rows of O: the call writes those rows of dst (O, contiguous, row 0 at dst) and nothing else.  Without bit 4 they are
 * D's rows [y0, y1), or [out_h - y1, out_h - y0) with bit 2, and the call reads the mosaic rows the upright contract names for those
 * rows of D (full size: 4 rows either side for a Bayer mosaic, 3 for an X-Trans one, clipped to [0, H); reduced size: 2 or 3 mosaic
 * rows per row); those must lie in the source window, else R2F_EINVAL before any launch.  With bit 4 they are D's columns [y0, y1),
 * or [out_w - y1, out_w - y0) with bit 1: the call reads every mosaic row, and the source window must hold [0, H).  Refused:
 * everything the upright entry point refuses, and an orientation outside 0 .. 7.  orientation = 0 writes the bytes of the upright
 * entry point (and launches its kernel).  A band's bytes are those of the same rows of a whole-frame call, whatever the cut, the
 * pitch or the source's alignment.  Every phase is still taken from frame coordinates of D.
 * The kernels are the upright ones with another epilogue (a compile-time class; raw2film_amd/csrc/r2f_mosaic_math.h has the index
 * map).  Mirrored (bits 1 and 2 only): a wave's row of the tile is still one contiguous segment of dst; with bit 1 the lanes write
 * their pixel to the mirrored slot of the row buffer, with bit 2 the segment walks upward.  Turned (bit 4): a row of D is a column
 * of O, so the block collects its 64 x 32 tile in LDS in O's layout -- 64 rows of O, an odd number of 32-bit words apart so that a
 * wave's 64 lanes write 64 rows without a bank conflict -- and each leaves as one contiguous run of up to 192 bytes.  The reduced
 * sizes stay a lane per output pixel, stored where the map puts it. */
R2F_API int r2f_demosaic_oriented_u16(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W,
                     const r2f_demosaic_params* params, int orientation, uint16_t* dst_u16_hwc3, int y0, int y1, void* stream);
R2F_API int r2f_demosaic_xtrans_oriented_u16(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H,
                     int W, const r2f_xtrans_params* params, int orientation, uint16_t* dst_u16_hwc3, int y0, int y1, void* stream);

/* The scale of a mosaic from the sensor's levels and the frame's measured maximum, on the device.  raw_to_linear's raw.postprocess
 * (raw_conversion.py:38-48) leaves LibRaw's adjust_maximum_thr at its default of 0.75: LibRaw then scales a frame to its largest
 * black-subtracted sample (its data_maximum) in place of the nominal white level whenever that sample lies between 75 % and 100 % of
 * the nominal one.  A profile's multipliers hold the white balance AND the scale to 16 bits, so a caller who wants that scale would
 * have to pass over the whole mosaic on the host; this is that pass on the device, and the multipliers derived from it.
 * Parity with LibRaw's bytes is UNPINNED like the rest of the demosaic: rawpy is on no machine this project sees.  The arithmetic
 * follows LibRaw's published raw2image_ex, adjust_maximum and scale_colors; what the tests pin is THIS definition
 * (tests/levels_model.py restates it in NumPy).
 *
 * Data maximum.  The mosaic is uint16 (H, W); P is the array's period, 2 or 6; black[P * P] (int32, each in [0, 65535]) is indexed by
 * the site's phase (y % P) * P + x % P, as in both definitions above.
 *   d = max over all sites of max((int)raw(y, x) - black[phase], 0):
 * an integer in [0, 65535], taken over the WHOLE mosaic, whatever window of the demosaiced frame the pipeline keeps.
 * Scale.  Inputs: the white balance wb[3] (doubles, finite, > 0), white_level (an integer in [1, 65535]), thr (a double in [0, 1]),
 * the black table and d.
 *   m = white_level - min(black); refused when m < 1.
 *   The threshold follows LibRaw's rule: thr < 0.00001 means no adjustment; thr > 0.99999 means 0.75; otherwise it is thr itself.
 *   With t = (float)threshold the frame is adjusted if and only if d > 0, d < m and (float)d > fl((float)m * t): one fp32 multiply
 *   and one fp32 comparison, as in LibRaw's expression.
 *   m_eff = d when adjusted, else m.
 *   mul[c] = wb[c] / min(wb) * 65535.0 / m_eff, evaluated in double, left to right.
 * The planners above round mul[c] to float once and refuse anything outside (0, 1024]; a Bayer profile spreads the three multipliers
 * over its quad by the pattern. */
typedef struct r2f_raw_levels {
    double white_balance[3];
    int32_t white_level;
    double adjust_maximum_thr;
} r2f_raw_levels;
/* What the Scale steps yield: the multipliers, m_eff, and whether the frame was adjusted (1) or keeps the nominal scale (0). */
typedef struct r2f_raw_scale {
    double mul[3];
    int32_t maximum_used;
    int32_t adjusted;
} r2f_raw_scale;
/* Host planner (raw2film_amd/csrc/r2f_levels_plan.cpp; no GPU, no context): the Scale steps.  black: n_black = 4 or 36 levels as a
 * profile states them (doubles, integral, in [0, 65535]); data_maximum: d (0 plans the nominal scale).  R2F_EINVAL for a null
 * pointer, another n_black, a black level, white balance, white level or threshold outside its range (a NaN is outside every range),
 * data_maximum above 65535 and m < 1; a refusal leaves *out alone. */
R2F_API int r2f_raw_scale_plan(const r2f_raw_levels* levels, const double* black, int n_black, uint32_t data_maximum, r2f_raw_scale* out);

/* LibRaw's highlight modes 1 (unclip) and 2 (blend) -- rawpy's highlight_mode= of the same postprocess call.  The Scale steps above
 * are mode 0 (clip): the smallest white-balance factor becomes 1 and step A clamps at 65535, so a channel with a larger factor loses
 * the top 1 - min(wb) / wb[c] of the sensor's range.  Modes 3 .. 9 (rebuild) are a sequential spreading over a down-sampled map and
 * are NOT built: they are refused by name.  Parity with LibRaw's bytes is UNPINNED like the rest of the demosaic; the arithmetic
 * follows dcraw / LibRaw's published scale_colors and blend_highlights, and what the tests pin is THIS definition
 * (tests/highlight_model.py restates it in NumPy).
 *
 * Scale with a highlight mode.  Inputs: those of the Scale steps, and mode in {0, 1, 2}.  m, the threshold rule, d and m_eff are
 * unchanged.
 *   Mode 0: exactly the Scale steps' result.
 *   Modes 1 and 2: mul[c] = wb[c] / max(wb) * 65535.0 / m_eff, evaluated in double, left to right: the largest factor becomes 1 and
 *   nothing is cut below the sensor's own saturation.
 *   Mode 2 also yields the clip level: p[c] = (float)(wb[c] / max(wb)); clip = min over c of trunc(fl(65535.0f * p[c])) -- one fp32
 *   multiply per channel; refused when clip < 1.  As in LibRaw an adjusted maximum changes mul and does not change clip.
 *
 * Blend sits between the interpolation and step C of either demosaic: it acts on the pixel's three integers (v0, v1, v2) in
 * [0, 65535] as B / B' leave them, at full and at reduced size and for either pattern.  Its one parameter is clip in [1, 65535].
 * Every operation below is one correctly rounded fp32 operation, no contraction; trunc is toward zero.
 *   If no v[c] > clip the pixel is unchanged (a pixel exactly at clip is unchanged).  Otherwise
 *     cam0[c] = (float)v[c];  cam1[c] = min(cam0[c], (float)clip)
 *     for i in {0, 1}:  lab[i][k] = fl(fl(fl(T[k][0] cam_i[0]) + fl(T[k][1] cam_i[1])) + fl(T[k][2] cam_i[2])),  k = 0, 1, 2
 *       T = {{1, 1, 1}, {0x1.bb67aep+0f, -0x1.bb67aep+0f, 0}, {-1, -1, 2}}                       (0x1.bb67aep+0f = 1.7320508f)
 *     sum[i] = fl(fl(lab[i][1]^2) + fl(lab[i][2]^2))
 *     chratio = sqrtf(fl(sum[1] / sum[0])), correctly rounded; 1 when sum[0] == 0.  (dcraw divides 0 by 0 there: three equal
 *       channels above clip have no chroma to scale, cam1's sum is 0 as well, and the NaN of 0 / 0 would reach the integer
 *       conversion.  With chratio = 1 the pixel leaves as it came, up to the rounding of the two transforms.)
 *     lab[0][1] = fl(lab[0][1] chratio);  lab[0][2] = fl(lab[0][2] chratio)
 *     out[c] = clamp(trunc(fl(fl(fl(fl(I[c][0] lab[0][0]) + fl(I[c][1] lab[0][1])) + fl(I[c][2] lab[0][2])) / 3.0f)), 0, 65535)
 *       I = {{1, 0x1.bb67aep-1f, -0x1p-1f}, {1, -0x1.bb67aep-1f, -0x1p-1f}, {1, 0, 1}}            (0x1.bb67aep-1f = 0.8660254f)
 *   Step C then runs on out.  All magnitudes stay below 2^20 ahead of the squares and below 2^41 behind them: nothing overflows, no
 *   NaN arises (sum[0] > 0 where it divides), and the truncation stays inside int. */
enum { R2F_HIGHLIGHT_CLIP = 0, R2F_HIGHLIGHT_UNCLIP = 1, R2F_HIGHLIGHT_BLEND = 2 };
/* What the Scale steps yield beside the r2f_raw_scale: the mode, and mode 2's clip level (0 for modes 0 and 1). */
typedef struct r2f_highlight {
    int32_t mode, clip;
} r2f_highlight;
/* Host planner (raw2film_amd/csrc/r2f_levels_plan.cpp; no GPU, no context): Scale with a highlight mode.  Mode 0 yields
 * r2f_raw_scale_plan's result bit for bit and *hl = {0, 0}.  R2F_EINVAL for everything r2f_raw_scale_plan refuses, a null hl, a mode
 * outside {0, 1, 2} -- LibRaw's rebuild modes 3 .. 9 among them -- and clip < 1; a refusal leaves *out and *hl alone. */
R2F_API int r2f_raw_scale_plan_highlight(const r2f_raw_levels* levels, const double* black, int n_black, uint32_t data_maximum, int mode,
                     r2f_raw_scale* out, r2f_highlight* hl);
/* The demosaics with Blend.  Each is the entry point it is named after with one more argument, clip, and the same kernels compiled
 * with Blend between the interpolation and step C; nothing new is staged in LDS, and the branch diverges inside a wave only where
 * a tile crosses a blown area.  clip outside [1, 65535] is refused before any launch; clip = 65535 writes the bytes of the plain
 * entry point (no integer in [0, 65535] exceeds it).
 * r2f_demosaic_blend_u16 carries r2f_demosaic_oriented_u16's contract.  src_rows: uint16 mosaic rows [src_gy0, src_gy0 +
 * src_nrows) of the H x W frame on the device, src_pitch samples apart (>= W).  orientation = 0 is upright: writes output rows
 * [y0, y1) of dst (uint16 (out_h, out_w, 3), row 0 at dst) and nothing else; full size reads mosaic rows [y0 - 4, y1 + 4) clipped to
 * [0, H), half size [2 y0, 2 y1); those rows must lie inside the source window, else R2F_EINVAL before any launch.  With an
 * orientation [y0, y1) are rows of O: the call writes those rows of dst (O, contiguous, row 0 at dst) and nothing else.  Without
 * bit 4 they are D's rows [y0, y1), or [out_h - y1, out_h - y0) with bit 2, and the call reads the mosaic rows the upright contract
 * names for those rows of D; those must lie in the source window, else R2F_EINVAL before any launch.  With bit 4 they are D's columns
 * [y0, y1), or [out_w - y1, out_w - y0) with bit 1: the call reads every mosaic row, and the source window must hold [0, H).
 * Refused: everything the upright entry point refuses, and an orientation outside 0 .. 7.  A band's bytes are those of the same
 * rows of a whole-frame call, whatever the cut, the pitch or the source's alignment (which only select between 32-bit and 16-bit
 * loads of the same samples).  Every phase is still taken from frame coordinates of D.
 * r2f_demosaic_blend_f32 carries r2f_demosaic_f32's contract.  With D the uint16 frame above (upright, with Blend) and (row0,
 * col0, rows, cols) a non-empty window inside D, dst[y, x, c] = fminf((float)D[row0 + y, col0 + x, c] / divisor * factor, 65504.0f).
 * dst: float32 (rows, cols, 3), contiguous, 4-byte aligned.  Writes window rows [y0, y1) of dst and nothing else.  Full size reads
 * mosaic rows [row0 + y0 - 4, row0 + y1 + 4) clipped to [0, H), half size [2 (row0 + y0), 2 (row0 + y1)); those rows must lie inside
 * the source window, else R2F_EINVAL before any launch.  The bytes depend on neither the cut, the pitch, the source's alignment nor
 * the window's origin.  Refused: everything r2f_demosaic_u16 refuses, a window that is empty or not inside D, y0 > y1, y0 < 0, y1 >
 * rows, divisor <= 0.
 * r2f_demosaic_xtrans_blend_u16 carries r2f_demosaic_xtrans_oriented_u16's contract: the first paragraph above with full size
 * reading mosaic rows [y0 - 3, y1 + 3) clipped to [0, H) and reduced size [3 y0, 3 y1) (the cut need not be a multiple of 6 or 3);
 * params whose tables are not those the planner derives from their cfa are refused. */
R2F_API int r2f_demosaic_blend_u16(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W,
                     const r2f_demosaic_params* params, int orientation, int clip, uint16_t* dst_u16_hwc3, int y0, int y1, void* stream);
R2F_API int r2f_demosaic_blend_f32(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W,
                     const r2f_demosaic_params* params, int clip, int row0, int col0, int rows, int cols, float divisor, float factor,
                     float* dst_f32_hwc3, int y0, int y1, void* stream);
R2F_API int r2f_demosaic_xtrans_blend_u16(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H,
                     int W, const r2f_xtrans_params* params, int orientation, int clip, uint16_t* dst_u16_hwc3, int y0, int y1, void* stream);
/* Step M: the median filter of the colour differences (LibRaw's median_filter(): its med_passes, rawpy's median_filter_passes=,
 * dcraw's -m n).  Parity with LibRaw's bytes is UNPINNED, like every step around it.  M sits between B / B' and Blend of either
 * demosaic, for both patterns, at full and at reduced size.
 *   Let I_0 = (R, G, B) be the three integer planes in [0, 65535] that B (full size) or B' (reduced size) leaves.  They cover the
 *   WHOLE demosaiced frame D of out_h x out_w pixels, whatever window or row range a call takes.  For pass k = 1 .. n and for c in
 *   {R, B} independently:
 *     at an interior pixel (1 <= y < out_h - 1 and 1 <= x < out_w - 1)
 *       I_k[c](y, x) = clamp(median{ I_{k-1}[c](y + j, x + i) - G(y + j, x + i) : i, j in {-1, 0, 1} } + G(y, x), 0, 65535)
 *     at a border pixel  I_k[c] = I_{k-1}[c].
 *   G never changes.  Every pass reads only the pass before it (dcraw copies the channel aside before it writes).  The median of
 *   nine integers is unique; dcraw's 19-exchange network is one way to find it, not part of the definition.  Blend (if any) and
 *   step C then run on I_n.  A frame with a side below 3 has no interior: its result is the plain entry point's.
 *   n is in 1 .. R2F_MEDIAN_MAX_PASSES; the cap is what the kernels' LDS apron is sized for, and more passes are refused by name.
 * Reach.  Full size: an output row reads the mosaic rows within 4 + n (Bayer) or 3 + n (X-Trans) of it, clipped to the frame.
 * Reduced size: output rows [y0, y1) read the reduced rows [y0 - n, y1 + n) clipped to the frame, that is mosaic rows 2 (or 3) times
 * that range.  A window edge or a band edge that is not a frame edge is NOT a border: the median there reads pixels outside the
 * window and outside the band.
 * Each entry point below is the Blend entry point it is named after -- r2f_demosaic_blend_u16, r2f_demosaic_blend_f32,
 * r2f_demosaic_xtrans_blend_u16: their arguments, contracts and refusals -- with one more argument, passes, and two changes: clip =
 * 0 means no Blend (else [1, 65535]; Blend is a uniform branch of the same kernel and gives the Blend entry point's bytes), and the
 * mosaic rows a call reads are those of the reach above, which must lie inside the source window, else R2F_EINVAL before any launch
 * with the rows named.  passes outside [1, R2F_MEDIAN_MAX_PASSES] is refused before any launch.  A band's bytes are those of the
 * same rows of a whole-frame call.  One launch per call: a block stages its tile's samples n rows and columns further, evaluates
 * B once per pixel of the tile plus an n-pixel ring into LDS planes ((64 + 2n)(32 + 2n) / 2048 of the plain kernel's
 * interpolation), runs the passes there and leaves through the plain kernels' epilogues. */
#define R2F_MEDIAN_MAX_PASSES 4
R2F_API int r2f_demosaic_median_u16(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W,
                     const r2f_demosaic_params* params, int orientation, int clip, int passes, uint16_t* dst_u16_hwc3, int y0, int y1,
                     void* stream);
R2F_API int r2f_demosaic_median_f32(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W,
                     const r2f_demosaic_params* params, int clip, int passes, int row0, int col0, int rows, int cols, float divisor,
                     float factor, float* dst_f32_hwc3, int y0, int y1, void* stream);
R2F_API int r2f_demosaic_xtrans_median_u16(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H,
                     int W, const r2f_xtrans_params* params, int orientation, int clip, int passes, uint16_t* dst_u16_hwc3, int y0, int y1,
                     void* stream);
/* The data maximum of mosaic rows [y0, y1), folded into a device word: *dst_max = max(*dst_max, d of those rows).  The caller zeroes
 * the word before the first call; bands in any order and any cut then compose to the whole frame's value, and since an integer
 * maximum does not depend on order the result is exact and the same on every run.  src_rows: uint16 mosaic rows [src_gy0, src_gy0 +
 * src_nrows) of the H x W frame on the device, src_pitch samples apart (>= W); black: period * period levels ON THE HOST.  Reads
 * mosaic rows [y0, y1) and no others; those rows must lie inside the source window, else R2F_EINVAL before any launch.  Writes the 4
 * bytes of *dst_max and nothing else; y0 == y1 is R2F_OK with no launch.  Refused: a period other than 2 or 6, H or W below the
 * period, y0 > y1, y0 < 0 or y1 > H, src_pitch < W, a black level outside [0, 65535], null pointers.  The phase is that of the frame
 * (src_gy0, y0), never that of the buffer or the block; the source's alignment and pitch only select between wider and narrower loads
 * of the same samples (r2f_demosaic_u16's rule).
 * One launch of a resident grid: a block walks groups of R2F_MOSAIC_MAX_ROWS rows, a wave per row; a lane loads R2F_MOSAIC_MAX_VEC
 * samples at a time (16 bytes) behind the up to 7 samples that lead to a 16-byte boundary and ahead of the up to 7 that trail, and
 * subtracts and folds them as packed 16-bit pairs (subtract with clamp at 0, then max).  A 2 x 2 table is widened to 6 x 6 on the
 * host, so the kernel knows one period; a block keeps it in LDS and a lane fetches its row's six levels once per row: along a row
 * the pairs of a lane's vectors cycle through three registers.  The lanes' maxima meet across the wave, then across the block's
 * waves in LDS, and leave through one atomicMax per block; a block without rows does not touch the word. */
R2F_API int r2f_mosaic_maximum(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W,
                     int period, const int32_t* black, int y0, int y1, uint32_t* dst_max, void* stream);
/* r2f_mosaic_maximum's widest load in samples and the rows a block walks per step (test shapes are derived from them). */
enum { R2F_MOSAIC_MAX_VEC = 8, R2F_MOSAIC_MAX_ROWS = 4 };

/* The wavelet denoise of a Bayer mosaic on the device: rawpy's noise_thr=, dcraw's -n, the first half of wavelet_denoise() inside
 * LibRaw's scale_colors.  It runs where LibRaw runs it: behind the black subtraction and adjust_maximum, ahead of the scale, so it
 * sits in front of either Bayer demosaic above.  Parity with LibRaw's bytes is UNPINNED like the rest of the demosaic: rawpy is on
 * no machine this project sees.  The arithmetic follows dcraw / LibRaw's published wavelet_denoise and hat_transform; what the
 * tests pin is THIS definition (tests/denoise_model.py restates it in NumPy).
 * NOT built: the second half of dcraw's function, which pulls the two greens of a quad together; anything for X-Trans mosaics;
 * streaming in row bands (the five levels reach 31 plane rows either side, and every level is a whole-frame pass).
 *
 * Inputs.  The mosaic, uint16 (H, W), H and W even and at least 64; black[4] (int32, each in [0, 65535]) per site k = (y & 1) * 2 +
 * (x & 1); a maximum M, an integer in [1, 65535] -- the white level less the black level the frame is scaled by, maximum_used of
 * r2f_raw_scale --; a threshold T, a float in (0, 1e6].  The step knows nothing of colours: the four sites of the quad are four
 * planes, whatever the pattern.  Every operation below is one correctly rounded fp32 operation; trunc is toward zero.
 *   1. s is the largest integer >= 0 with (M << s) < 65536: 0 for M >= 32768, 15 for M = 1.
 *   2. Plane k has n_r = H / 2 rows and n_c = W / 2 columns.  With (yy, xx) = (k >> 1, k & 1):
 *        t[y, x] = max((int)raw[2 y + yy, 2 x + xx] - black[k], 0)
 *        F[y, x] = fl(256 * sqrtf((float)(t << s)))            (the shift product is below 2^31 and exact as a float)
 *   3. For lev = 0 .. 4 with c = 1 << lev; In = F at level 0, else L of the level before:
 *        hat(b, i, n) = fl(fl(2 b[i] + b[m]) + b[p]),   m = i - c if i >= c, else c - i;   p = i + c if i + c < n, else 2 n - 2 - (i + c)
 *        R[y, x] = 0.25 * hat(In[y, .], x, n_c);   L[y, x] = 0.25 * hat(R[., x], y, n_r)    (rows first, then columns; both
 *          quarterings are exact)
 *        theta = fl(T * noise[lev]),   noise = {0.8002f, 0.2735f, 0.1202f, 0.0585f, 0.0291f}
 *        d = fl(In - L);   d' = fl(d + theta) if d < -theta;  fl(d - theta) if d > theta;  0 otherwise
 *        D = d' at level 0, D = fl(D + d') afterwards
 *   4. out = clamp(trunc(fl(fl(D + L)^2) / 65536), 0, 65535) with L that of level 4, written at the sample's own site.
 * Side bound: n >= 32 keeps every m and p inside [0, n) at c = 16 (dcraw indexes outside the row below that size), which is why
 * sides below 64 are refused rather than defined.
 * Output and plug-in.  The output mosaic is black-free and in units of t << s: the demosaic that follows runs with black = 0 and
 * every multiplier times 2^-s (exact); all else in the profile is unchanged, and a blend clip level, which lives behind the scale,
 * does not move. */
typedef struct r2f_denoise_params {
    int32_t black[4];
    int32_t shift;    /* s */
    float threshold;  /* T */
} r2f_denoise_params;
/* The tile of one plane a workgroup of the denoise owns, in plane samples (test shapes are derived from them). */
enum { R2F_DENOISE_TILE_W = 64, R2F_DENOISE_TILE_H = 32 };
/* Host planner (raw2film_amd/csrc/r2f_denoise_plan.cpp; no GPU, no context): step 1 and the checks.  black: 4 levels as a profile
 * states them (doubles, integral, in [0, 65535]).  R2F_EINVAL for a null pointer, a threshold outside (0, 1e6] or one that rounds to
 * 0 as a float, a maximum outside [1, 65535], a black level outside its range (a NaN is outside every range), an odd side or a side
 * below 64; a refusal leaves *out alone. */
R2F_API int r2f_mosaic_denoise_plan(double threshold, int maximum, const double* black, int H, int W, r2f_denoise_params* out);
/* The bytes of workspace r2f_mosaic_denoise needs for an H x W mosaic: 12 per sample (D and two L buffers as planar floats); 0 for
 * sides the planner refuses.  No GPU, no context. */
R2F_API size_t r2f_mosaic_denoise_workspace_bytes(int H, int W);
/* Steps 2 to 4 of an H x W mosaic on the device.  src: uint16, rows src_pitch samples apart (>= W); dst: the same with dst_pitch;
 * dst == src is allowed (the last launch alone writes dst, the first alone reads src).  workspace: device memory, 16-byte aligned,
 * workspace_bytes >= r2f_mosaic_denoise_workspace_bytes(H, W), overlapping neither src nor dst.  Reads the H x W samples of src;
 * writes the H x W samples of dst and bytes inside the stated workspace, and nothing else.  Refused before any launch: null
 * pointers, sides the planner refuses, a pitch below W, a workspace that is too small, misaligned or overlaps a frame, and params
 * the planner would not have produced (a black level outside [0, 65535], a shift outside [0, 15], a threshold outside (0, 1e6]).
 * The alignment and pitch of src and dst only select between 32-bit and 16-bit accesses of the same samples.
 * Five launches, one per level; row pass, column pass, threshold and accumulation are fused in each.  A workgroup stages its
 * R2F_DENOISE_TILE_W x R2F_DENOISE_TILE_H tile of In with an apron of c samples on all four sides in LDS, runs the row pass over
 * the tile's rows and apron rows into a second LDS array, then the column pass and the rest per output sample.  Reflection is taken
 * in PLANE coordinates: the reflected sample of a border tile lies inside the tile's own clipped box.  Level 0 reads the uint16
 * source itself (step 2 on the fly, apron included) and writes D and L; levels 1 to 3 read one L buffer, write the other and update
 * D at their own samples; level 4 stores no L, finishes step 4 and writes the uint16 result.  No workgroup reads a plane another
 * workgroup of the same launch writes.  At levels 0 and 4 a workgroup owns the same tile of all four planes, so mosaic rows enter
 * and leave as contiguous segments; in between the planes are planar floats. */
R2F_API int r2f_mosaic_denoise(r2f_ctx* ctx, const uint16_t* src, int64_t src_pitch, int H, int W, const r2f_denoise_params* params,
                     uint16_t* dst, int64_t dst_pitch, void* workspace, size_t workspace_bytes, void* stream);
/* Measurement aid (tools/denoise_probe.py): the launch of ONE level, 0 .. 4, of r2f_mosaic_denoise with that call's arguments, checks and
 * buffers -- level 0 reads src, level 4 writes dst, every level reads and writes the workspace where the whole chain keeps D and L, so
 * the five calls in order are the chain.  A level other than 0 on a workspace the levels before it have not filled computes on
 * whatever the workspace holds; it reads and writes the same bytes either way.  R2F_EINVAL for a level outside 0 .. 4. */
R2F_API int r2f_mosaic_denoise_level(r2f_ctx* ctx, int level, const uint16_t* src, int64_t src_pitch, int H, int W,
                     const r2f_denoise_params* params, uint16_t* dst, int64_t dst_pitch, void* workspace, size_t workspace_bytes,
                     void* stream);

/* The repair of hot pixels of a mosaic on the device, ahead of everything else that reads it (the data maximum, the denoise, either
 * demosaic).  This is the project's OWN rule, as the X-Trans interpolation is: it is NOT LibRaw's bad_pixels, which takes a caller's
 * coordinate list and works sequentially and in place (not built; nor are a repair fused into the demosaic's staging, streaming for
 * the profiles that do not stream, and dark-frame subtraction).  tests/repair_model.py restates it in NumPy.
 *
 * Inputs.  The mosaic, uint16 (H, W), H and W at least 6; P its period, 2 for a Bayer array and 6 for an X-Trans array; phase(y, x) =
 * (y % P) * P + x % P; black[P * P] (int32, each in [0, 65535]), the profile's table; a threshold in [0, 65535], in black-subtracted
 * raw units; q in [1, 255], a ratio in 1/256ths; min_neighbours, 3 or 4.
 *   N. Every sample has four neighbours, each of its own colour.
 *        Bayer: (dy, dx) = (-2, 0), (0, 2), (2, 0), (0, -2): the same site of the quad, so the same black level, and the same green of
 *        the two.
 *        X-Trans: one per quadrant d = up, right, down, left.  The candidates of ring r = 1, 2 are (-r, a), (a, r), (r, -a), (-a, -r)
 *        for the four quadrants, with the lateral offset a in the order 0, 1, -1, 2 over -r < a <= r: the eight sites of ring 1 and the
 *        sixteen of ring 2 belong to exactly one quadrant each.  The neighbour is the first candidate of the sample's colour, ring 1
 *        before ring 2, with the pattern taken cyclically.  The planner tables them per phase and refuses a pattern that has a phase
 *        and quadrant without one inside ring 2 (Fujifilm's canonical pattern and its 36 cyclic shifts have four distinct neighbours
 *        at every phase).
 *   T. t(y, x) = max((int)raw(y, x) - black[phase(y, x)], 0).
 *   H. A neighbour k is BELOW its centre when q * t_centre > 256 * t_k (both products stay under 2^24).  The centre is hot when
 *      t_centre > threshold and at least min_neighbours of its four neighbours are below it; then
 *        out = clamp(max{t_k : k below} + black[phase of the centre], 0, 65535),
 *      and out = raw, untouched bit for bit, for every other sample.  A sample with any neighbour outside the frame is never hot (for
 *      Bayer that is the 2-sample ring).
 * Every output is a function of raw within 2 samples of it, and no pass reads what it writes.
 * The params hold one period, 6: a 2 x 2 table is widened by the planner (6 is a multiple of 2, every site keeps its level and its
 * neighbours). */
typedef struct r2f_repair_params {
    int32_t period;            /* 2 or 6, as the caller stated it */
    int32_t black[36];         /* per phase (y % 6) * 6 + x % 6 */
    int8_t offset[36][4][2];   /* per phase and quadrant (up, right, down, left): (dy, dx), each within 2 samples */
    int32_t threshold, q, min_neighbours;
} r2f_repair_params;
/* Host planner (raw2film_amd/csrc/r2f_repair_plan.cpp; no GPU, no context).  cfa: 36 colour ids of the 6 x 6 pattern for period 6
 * (ignored, and may be null, for period 2); black: period * period levels as a profile states them (doubles, integral, in [0, 65535]).
 * R2F_EINVAL for a null pointer, a period other than 2 or 6, a black level outside its range (a NaN is outside every range), a
 * threshold outside [0, 65535], q outside [1, 255], min_neighbours other than 3 or 4, H or W below 6, a colour id outside {0, 1, 2}
 * and a pattern with a phase and quadrant that has no neighbour inside ring 2; a refusal leaves *out alone. */
R2F_API int r2f_mosaic_repair_plan(int period, const int32_t* cfa, const double* black, int threshold, int q, int min_neighbours, int H,
                     int W, r2f_repair_params* out);
/* Steps N, T and H of mosaic rows [y0, y1) on the device, with the mosaic entry points' row-range contract.  src_rows: uint16 mosaic
 * rows [src_gy0, src_gy0 + src_nrows) of the H x W frame, src_pitch samples apart (>= W); dst: an H-row mosaic, row 0 at dst, rows
 * dst_pitch samples apart (>= W).  Writes the W samples of rows [y0, y1) of dst and nothing else; reads rows [y0 - 2, y1 + 2) clipped
 * to the frame, which must lie inside the source window, else R2F_EINVAL before any launch.  The bytes of a band are those of the same
 * rows of a whole-frame call, whatever the cut, the pitches and the source's alignment; y0 == y1 is R2F_OK with no launch.
 * count: null, or a device uint32 to which the call ADDS the number of samples it replaced in [y0, y1), with one atomic per block at
 * most (a block that replaced none does not touch it).
 * Refused: null pointers (count aside), H or W below 6, pitches below W, y0 > y1, y0 < 0, y1 > H, the rows read or the rows written of
 * src and dst sharing bytes, and params the planner would not have produced.
 * One launch of a resident grid shaped like r2f_mosaic_maximum's: a block walks groups of R2F_MOSAIC_REPAIR_ROWS rows, a wave per
 * row; a lane loads and stores R2F_MOSAIC_REPAIR_VEC samples at a time (16 bytes) behind the up to 7 samples that lead to a 16-byte
 * boundary of the SOURCE row and ahead of the up to 7 that trail (a destination row that is not aligned the same way takes narrower
 * stores of the same samples).  Step T and the threshold test run on packed 16-bit pairs; only a sample whose t exceeds the
 * threshold fetches its four neighbours, as 16-bit loads that the cache serves: the rows above and below are rows that the waves
 * next to this one stream through the same L2 at the same time, so a launch moves 2 bytes in and 2 bytes out per sample across the
 * memory bus by design, and the gathers add 8 bytes of cache traffic per candidate.  No LDS staging of rows: the candidates are
 * sparse wherever the step is of use (a threshold below the signal makes every sample a candidate, and the kernel then runs at the
 * cache's rate; the result is the same).  Two instances: period 2 with its offsets as compile-time constants, period 6 with the
 * offset table in LDS; both keep the 36 levels in LDS. */
R2F_API int r2f_mosaic_repair(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int64_t src_pitch, int H, int W,
                     const r2f_repair_params* params, uint16_t* dst, int64_t dst_pitch, int y0, int y1, uint32_t* count, void* stream);
/* r2f_mosaic_repair's widest access in samples and the rows a block walks per step (test shapes are derived from them). */
enum { R2F_MOSAIC_REPAIR_VEC = 8, R2F_MOSAIC_REPAIR_ROWS = 4 };

/* The hand-off from RAW decoding: the last two lines of raw_to_linear (raw_conversion.py:50-52) applied to LibRaw's 16-bit
 * output on the device, so that a decoded frame crosses PCIe as uint16 (6 bytes per pixel) instead of float32 (12 or 16):
 * dst = float(src) / divisor (65535, one correctly rounded fp32 division) * factor (the float32 of 2 ** calc_exposure(...),
 * color_processing.py:71-99 -- computed by the caller, raw2film_amd.decode.auto_exposure).  src: uint16 (H, W, channels) on
 * the device, channels 3 or 4 (a fourth is dropped); dst: float32 (H, W, 3), clamped at 65504 like every frame the GPU path
 * uploads (gpu_processor.py:275).  Bit-identical to the NumPy expressions. */
R2F_API int r2f_decode_u16(r2f_ctx* ctx, const uint16_t* src_hwc, int H, int W, int channels, float divisor, float factor, float* dst_f32_hwc3,
                   void* stream);

/* The auto exposure of the uint16 hand-off measured on the device: calc_exposure (color_processing.py:71-99) on the uploaded
 * frame, so that no host pass over the frame precedes the render and the device never waits for the host to learn the factor.
 * With u over frame[::2, ::2, 1] of the WHOLE decoded frame: g = (float)u / 65535 (one correctly rounded fp32 division, widened to
 * double), m = mean(pow(g, 1 / root)), stops = log2(ref_exposure / pow(m, root)), factor = the float32 of 2 ** stops -- upstream's
 * formula in fp64.  Upstream evaluates it in float32 (raw2film_amd.decode.auto_exposure does so bit for bit) and lands 2e-8 ..
 * 5e-5 stops away, so the two factors usually differ in the last bits: this is an opt-in mode, not a replacement.
 *   r2f_exposure_rows    the fp64 sums of the sampled rows (global row index even) of [y0, y1) into a per-row array the context
 *                        owns (grown when a taller frame arrives; r2f_generation stays).  src_rows: uint16 rows [src_gy0, src_gy0 +
 *                        src_nrows) of the (H, W, channels) frame on the device, channels 3 or 4.  One fixed-shape reduction per row:
 *                        a row's sum depends only on its bytes, W, channels and root, so the result is the same bits whether the
 *                        frame comes in one call, in bands of any size and order, or twice.  No floating-point atomics.
 *   r2f_exposure_finish  one workgroup adds the ceil(H / 2) row sums in a fixed order and writes stops and factor into the
 *                        context's device-side record (every sampled row of the frame must have been summed on `stream` before).
 *   r2f_decode_u16_auto  r2f_decode_u16 with the factor read from the record -- the same floats for the same factor -- and a
 *                        pitched source: W pixels of each of H rows that lie src_pitch pixels apart (a crop of the uploaded
 *                        frame is a pointer offset plus the pitch).  dst: float32 (H, W, 3), contiguous.
 *   r2f_exposure_result  waits for the last r2f_exposure_finish (not for what was queued behind it) and returns its record. */
R2F_API int r2f_exposure_rows(r2f_ctx* ctx, const uint16_t* src_rows, int src_gy0, int src_nrows, int H, int W, int channels, int y0, int y1,
                      double root, void* stream);
R2F_API int r2f_exposure_finish(r2f_ctx* ctx, int H, int W, double root, double ref_exposure, void* stream);
R2F_API int r2f_decode_u16_auto(r2f_ctx* ctx, const uint16_t* src_hwc, int H, int W, int channels, int64_t src_pitch, float divisor,
                        float* dst_f32_hwc3, void* stream);
R2F_API int r2f_exposure_result(r2f_ctx* ctx, double* stops, float* factor);

/* The GPU processor's preview blit, shaders/copy_to_int.wgsl as bound by gpu_processor.py:1416-1539: the display-referred float
 * frame (H, W, 3) sampled bilinearly (clamp to edge) into an RGBA8 destination (dst_h, dst_w, 4): inside the scaled image the
 * sample (alpha 255), elsewhere inside the canvas bounds the canvas colour, transparent outside.  The transform is the shader's
 * uniform block (raw2film_amd.geometry.blit_transform computes it like _bind_copy_to_dst).  dst_rgba: 4-byte aligned. */
typedef struct r2f_blit {
    float scale_x, scale_y;    /* 1 / rendered size of the image inside the destination, in destination pixels */
    float offset_x, offset_y;  /* its top-left corner */
    float canvas_min_x, canvas_min_y, canvas_max_x, canvas_max_y;
    float canvas_color[3];     /* 0..1 */
} r2f_blit;
R2F_API int r2f_blit_rgba8(r2f_ctx* ctx, const float* src_f32_hwc, int H, int W, uint8_t* dst_rgba, int dst_h, int dst_w, const r2f_blit* t,
                   void* stream);

/* shaders/histogram.wgsl pass2_process + pass3_render and shaders/scale_texture.wgsl (gpu_processor.py:1245-1285, 1883-1889) on
 * the counts of r2f_histogram_u8: log1p of the normalised counts, 3-bin smoothing, bar heights, the (height, 256, 4) RGBA bar
 * image coloured by mix_table_rgba (HOST, 8 x 4 bytes, index is_r * 4 + is_g * 2 + is_b) and, when target_rgba is given, its
 * nearest-neighbour copy into a (target_h, target_w, 4) widget texture.  counts / image / target are device pointers; image and
 * target 4-byte aligned. */
R2F_API int r2f_histogram_render(r2f_ctx* ctx, const uint32_t* counts, const uint8_t* mix_table_rgba, int height, uint8_t* image_rgba,
                         uint8_t* target_rgba, int target_h, int target_w, void* stream);

/* Test entry for S6a: raw PCG3D hash (3 uint32 planes) and Gaussian field (3 fp32 planes) for
 * global rows [y0, y1); either output may be NULL.  noise.wgsl:14-62 / noise_bw.wgsl. */
R2F_API int r2f_stage_noise(r2f_ctx* ctx, const r2f_params* p, uint32_t* hash_planes, float* noise_planes, int y0, int y1,
                    int W, void* stream);
/* Test entry: plain per-channel stencil (no epilogue) with the kernel set for `which`. */
R2F_API int r2f_stage_stencil(r2f_ctx* ctx, int which, const r2f_planes* src, const r2f_planes* dst, int y0, int y1, int W,
                      int H_global, void* stream);

/* Introspection for the measurement harness: what the device form of stencil `which` executes.  out: 3 channels x 8 ints
 * {entries, row steps, LDS phases, form word, cropped rows, cropped (padded) columns, rows per lane, FFT word}.
 * Form word: bit 0 = mirrored taps are paired in the entry list; the bits above = R when the channel takes the fully unrolled
 * (2 R + 1)^2 direct form instead of the entry list (bits 1-7); bit 8 = the grain stencil is u v^T to fp32 rounding and runs as two
 * 1-D passes (known after the first tail launch); bit 9 = ... and the pass along x runs in registers while the noise is hashed
 * (R <= 4; option grain_xpass_lds = 1 keeps it in LDS).  FFT word: bit 0 = the channel takes the FFT form (then the direct form's numbers before it are not what runs); the bits
 * above it = window rows * 4096 + window columns of its last launch (0 before the first); bit 30 = that launch multiplied by a REAL
 * kernel spectrum (taps centrally symmetric around an anchor at the centre of their box: option stencil_fft_real_spectrum).  One entry =
 * 32 packed FMAs per lane for 16 pixels (x2 taps when mirror-paired). */
R2F_API int r2f_stencil_stats(r2f_ctx* ctx, int which, int* out);

/* Per-launch device timing of the FFT stencil passes, for the roofline line of bench.py.  After r2f_set_option(ctx,
 * "kernel_timing", mask) every launch of a pass cls whose bit (1 << cls) is set (0 rows forward, 1 columns, 2 rows inverse) is bracketed by events on its own
 * stream; this call waits for them, returns their summed duration, the launch count and the summed algorithmic bytes
 * (scratch images and windows the pass has to move; the 1 MB kernel spectrum stays in L2), and resets the counters.
 * cls = pass (0..2) for launches on complex128 scratch (the halation), pass + 3 for launches on complex64 scratch (the MTF). */
R2F_API int r2f_kernel_timing(r2f_ctx* ctx, int cls, double* total_ms, int* launches, double* bytes);

/* Measurement aid for bench.py's `roofline.copy_ceiling` ("state the measured hipMemcpyDtoD / stream-triad
 * ceiling beside it"): a float4 streaming copy of `bytes` bytes from src to dst on the device -- 2 x bytes of HBM traffic and no
 * arithmetic.  Nothing upstream corresponds to it; bytes must be a multiple of 16 and both buffers 16-byte aligned. */
R2F_API int r2f_stream_copy(r2f_ctx* ctx, const void* src, void* dst, size_t bytes, void* stream);

/* Change counter of everything a captured HIP graph of this context's launches freezes: bumped by every table / stencil /
 * matrix upload, every option change and every re-allocation of a context-owned buffer (LUTs, stencil forms, FFT scratch and
 * spectra).  The reference re-binds its resources per dispatch (gpu_processor.py:1756-1877) and has nothing to invalidate; a
 * caller that replays captured launches must re-capture when this value moves. */
R2F_API uint64_t r2f_generation(const r2f_ctx* ctx);

/* Tuning knobs for A/B runs (every one of them bumps r2f_generation).  Round 5's, all defaulting to the faster form:
 *   stencil_fft_real_spectrum  1: centrally symmetric tap boxes (every halation disc / MTF kernel the reference builds) are laid
 *                                 out around the window origin, pass 2 multiplies by a REAL spectrum (8 B per element)
 *   stencil_fft_cols_walk      1: pass 2 of 256-row windows with a real spectrum runs as a resident grid walking the launch's
 *                                 pairs per column block (spectrum in registers); 0: one workgroup per (column block, pair)
 *   stencil_fft_scratch96_auto 1: the halation's passes take the 12-byte scratch element for the window pairs whose exposure range
 *                                 allows it (above); stencil_fft_scratch96 (mask per stencil) forces it for all
 *   stencil_fft_mixed_sign     1: channels with taps of both signs take the float64 FFT form whatever their size
 * (older ones: stencil_fft, stencil_fft_window[_rows|_max], stencil_fft_batch, stencil_fft_streams, stencil_fft_scratch32,
 *  stencil_fft_min_taps, stencil_fft_epilogue_lds, render_graph, front_fast, ... -- the table in r2f_plan.cpp, defaults in r2f_plan.h) */
R2F_API int r2f_set_option(r2f_ctx* ctx, const char* name, int value);

/* --- plan-only entry points: the host-side planners of this library (raw2film_amd/csrc/r2f_plan.cpp), callable without a GPU and
 * without a context.  Nothing upstream corresponds to them (the reference leaves these decisions to OpenCV and wgpu:
 * cv.filter2D picks its own DFT sizes, effects.py:151-153); they exist so that what the library decides on the CPU before it
 * launches anything can be pinned and fuzzed -- also under AddressSanitizer / UBSan, tests/test_plan_sanitizers.py -- on a machine
 * without a device. */
typedef struct r2f_fft_plan {
    int32_t ny, nx;          /* window rows, columns */
    int32_t vy, vx;          /* valid outputs per window */
    int32_t gx, ntiles;      /* windows per row of windows, windows per channel */
    int32_t pairs_per_channel, pairs;
    int32_t streams, batch, launches; /* internal streams, window pairs per launch triple, launch triples */
    uint64_t scratch_bytes;  /* pass scratch the context allocates for it */
} r2f_fft_plan;
/* The FFT form's plan for a bh x bw tap box on a call that covers `rows` output rows of a W-column frame with nch channels:
 * window shape (the cheapest under the stencil_fft_window / _rows / _max options, 0 = not forced), tiling and batches
 * (batch_mib MiB of scratch in flight on `streams` internal streams).  scratch_elem_bytes: 16, 8 or 12.  R2F_EINVAL when no window
 * shape fits. */
R2F_API int r2f_plan_fft(int bh, int bw, int W, int rows, int nch, int scratch_elem_bytes, int window, int window_rows, int window_max,
                 int batch_mib, int streams, r2f_fft_plan* out);
/* The direct form's device entry list for channel `channel` of a (kh, kw, kc) stencil on a TW x TH tile with Q rows per lane and
 * an LDS budget (0 = one phase): out8 = {entries, row steps, LDS phases, mirrored taps paired, cropped rows, cropped (padded)
 * columns, LDS row stride, rows of the largest phase}.  The list is checked against the taps it was built from (every tap exactly
 * once, offsets inside the phase's LDS rows): R2F_EHIP would mean a planner bug.  R2F_ETOOLARGE: a row step does not fit. */
R2F_API int r2f_plan_stencil(const float* host_khwc, int kh, int kw, int kc, int channel, int Q, int TW, int TH, int lds_budget_bytes,
                     int allow_sym, int* out8);
/* Tile order of a gx x gy grid of stencil workgroups (a permutation of 0 .. gx gy - 1; band = 0: automatic band width). */
R2F_API int r2f_plan_tile_order(int gx, int gy, int band, int* order);

/* --- JPEG export: gui.py:2338-2341 `Image.fromarray(image).save(path, "JPEG", quality=quality)` on the device.  The file is byte for
 * byte the one Pillow writes with its defaults (libjpeg-turbo baseline: JFIF 1.01 APP0, two 8-bit DQT, SOF0 4:2:0, the four
 * Annex K Huffman tables, one interleaved scan without restart markers, EOI).  quality: 0 .. 100 like the reference's slider
 * (0 writes what 1 writes).  H and W: 1 .. 65535. */
/* Worst-case file size of an H x W frame at any quality (0 for sizes JPEG cannot hold).  No GPU, no context. */
R2F_API uint64_t r2f_jpeg_bound_bytes(int H, int W);
/* The file's header, SOI up to and including SOS, into buf (cap >= 623); *len = its length.  No GPU, no context. */
R2F_API int r2f_jpeg_header(int quality, int H, int W, uint8_t* buf, size_t cap, size_t* len);
/* Encode a uint8 (H, W, 3) RGB device image whose rows are row_stride bytes apart into the device buffer `out` (out_cap >=
 * r2f_jpeg_bound_bytes(H, W)); the file's length lands in the device word *out_len (8-byte aligned).  Asynchronous on `stream`:
 * nothing is read back.  The scratch (about 3 bytes per pixel of coefficients plus the packed scan) belongs to the context and
 * only grows, so frames of alternating sizes neither re-allocate nor synchronise.  *out_len = 0 would mean an internal bound was
 * broken (nothing was written past it). */
R2F_API int r2f_jpeg_encode(r2f_ctx* ctx, const uint8_t* image, int H, int W, int64_t row_stride, int quality, uint8_t* out,
                            uint64_t out_cap, uint64_t* out_len, void* stream);
/* Row-wise encode: the same file, written while the frame's rows are still being made.  Begin opens the encode of an H x W frame
 * into `out` (out_cap >= r2f_jpeg_bound_bytes(H, W)) and writes its header; *out_len (device word, 8-byte aligned) then counts the
 * leading bytes of the file that are final -- the header and every stuffed scan byte no later rows can change -- and after the call
 * that completes the frame it is the file's length.  0 means an internal bound was broken.  The state between calls lives in the
 * context's encoder scratch and a small device carry; nothing is read back, everything is asynchronous on `stream`.  A one-shot
 * encode or a new begin ends an open row-wise encode. */
R2F_API int r2f_jpeg_rows_begin(r2f_ctx* ctx, int H, int W, int quality, uint8_t* out, uint64_t out_cap, uint64_t* out_len,
                                void* stream);
/* Encode the rows [y0, y1) of the frame whose row 0 is at `image` (uint8 RGB, rows row_stride bytes apart; only these rows are
 * read).  y0 must be the previous call's y1 (0 at first); y1 must lie past y0 and be a multiple of the open encode's MCU height
 * (16 for 4:2:0, 8 for 4:2:2 and 4:4:4), or H, which completes the file (padding bits, EOI) and ends the encode.  Anything else,
 * or no open encode: R2F_EINVAL (the open encode stays as it was). */
R2F_API int r2f_jpeg_rows(r2f_ctx* ctx, const uint8_t* image, int64_t row_stride, int y0, int y1, void* stream);

/* --- JPEG export with Pillow's options: save(..., quality=q, subsampling=s, optimize=o).  The entry points above are the
 * sampling = 2, optimize = 0 cases of these.  sampling: 0 = 4:4:4 (8 x 8 MCUs), 1 = 4:2:2 (16 x 8), 2 = 4:2:0 (16 x 16).
 * optimize: per-image Huffman tables (libjpeg's optimize_coding), generated from the frame's symbol counts.  EXIF (an APP1
 * segment after SOI + APP0) is the caller's to splice into the file: it needs no device work.  progressive: 0, or 1 for
 * save(..., progressive=True): SOF2 and libjpeg's ten-scan jpeg_simple_progression, every scan with its own optimized tables
 * (libjpeg forces optimize_coding there, so `optimize` makes no difference); one-shot only (r2f_jpeg_encode_ex).
 * restart_interval: 0, or the MCUs per restart interval, 1 .. 65535 -- Pillow's restart_marker_blocks, or restart_marker_rows
 * times the MCUs per row, clamped to 65535.  The header then carries a DRI segment (FF DD 00 04 hi lo) between the last DHT and
 * SOS; every interval codes its DC coefficients from predictors of 0 and ends padded with 1-bits to a whole byte, and RSTn
 * (FF D0 + n, n = the interval's index mod 8, never stuffed) separates it from the next.  Baseline only: with progressive it is
 * R2F_EINVAL.  x_density, y_density: both > 0 (at most 65535) make APP0 say dots per inch (Pillow's dpi, rounded); otherwise APP0
 * stays "no units, 1 : 1".  The variable-length segments (EXIF, XMP, ICC, COM) are the caller's to splice in after APP0.
 * The fields after `progressive` were appended: an initialiser of the first four leaves them 0, which is "none". */
typedef struct r2f_jpeg_opts {
    int32_t quality, sampling, optimize, progressive;
    int32_t restart_interval;
    int32_t x_density, y_density;
} r2f_jpeg_opts;
/* Worst-case file size of an H x W frame in `sampling` at any quality and either table choice (0 for sizes JPEG cannot hold or a
 * bad sampling).  Per pixel: about 9.7 bytes for 4:2:0, 13.0 for 4:2:2, 19.5 for 4:4:4.  No GPU, no context. */
R2F_API uint64_t r2f_jpeg_bound_bytes_ex(int H, int W, int sampling);
/* Worst-case file size for any options, progressive included (0 for bad options or sizes).  A progressive file's bound is
 * larger than a baseline one's: a coefficient can cost a symbol, its value bits and correction bits in several scans (about
 * 12.1 bytes per pixel for 4:2:0, 16.1 for 4:2:2, 24.1 for 4:4:4).  No GPU, no context.
 * A restart interval adds the DRI segment's 6 bytes and 4 bytes per interval (ceil(MCUs / restart_interval) of them): the
 * marker's 2, the byte the interval's padding completes, and the 0x00 stuffed behind that byte when it comes out as 0xFF.  The
 * scan's own bits are already counted at two bytes per byte. */
R2F_API uint64_t r2f_jpeg_bound_bytes_opts(const r2f_jpeg_opts* opts, int H, int W);
/* The header (SOI .. SOS) with the standard tables, APP0's density and the DRI segment of the options (cap >= 629 with a
 * restart interval); R2F_EINVAL for optimize and progressive (their tables come from the frame).  No GPU. */
R2F_API int r2f_jpeg_header_ex(const r2f_jpeg_opts* opts, int H, int W, uint8_t* buf, size_t cap, size_t* len);
/* jpeg_gen_optimal_table of libjpeg: symbol counts -> bits[0] = 0, bits[1..16] codes per length, huffval[*n] the symbols by
 * code length, then symbol.  R2F_EINVAL when every count is zero, or when counts past libjpeg's 10^9 sentinel leave a table
 * libjpeg itself would refuse.  No GPU, no context. */
R2F_API int r2f_jpeg_optimal_table(const uint64_t freq[256], uint8_t bits[17], uint8_t huffval[256], int* n);
/* r2f_jpeg_encode with options (out_cap >= r2f_jpeg_bound_bytes_ex(H, W, sampling); with a restart interval
 * r2f_jpeg_bound_bytes_opts(opts, H, W)).  Without optimize it is asynchronous like
 * r2f_jpeg_encode.  With optimize the call blocks once: the frame's coefficients and symbol counts are made on `stream`, the
 * 8 KB of counts are read back, the tables and header are built on the host, and the rest of the encode is queued on `stream`.
 * The context's scratch grows with the sampling: about 3, 4 and 6 bytes per pixel of coefficients plus the packed scan.
 * R2F_ETOOLARGE (optimize only): the optimized scan would exceed the bound, or the frame's symbol counts pass libjpeg's 10^9
 * sentinel (r2f_jpeg_optimal_table); nothing is written.
 * progressive: out_cap >= r2f_jpeg_bound_bytes_opts(opts, H, W).  The call blocks for the ten scans' symbol counts (40 KB read
 * back), builds every scan's tables and headers on the host, queues the packing of the scans one after the other and waits for
 * the file's length.  R2F_ETOOLARGE when the counts pass libjpeg's 10^9 sentinel, or -- which the bound rules out -- the exact
 * file would exceed out_cap: *out_len is then 0 and `out` holds no file. */
R2F_API int r2f_jpeg_encode_ex(r2f_ctx* ctx, const uint8_t* image, int H, int W, int64_t row_stride, const r2f_jpeg_opts* opts,
                               uint8_t* out, uint64_t out_cap, uint64_t* out_len, void* stream);
/* r2f_jpeg_rows_begin with options (out_cap >= r2f_jpeg_bound_bytes_opts(opts, H, W)); R2F_EINVAL for optimize, whose tables
 * need the whole frame before the first scan byte, and for progressive, whose every scan spans the whole frame.  A restart
 * interval may straddle calls: a marker is final, and counted in *out_len, with the call that holds its interval's last MCU. */
R2F_API int r2f_jpeg_rows_begin_ex(r2f_ctx* ctx, int H, int W, const r2f_jpeg_opts* opts, uint8_t* out, uint64_t out_cap,
                                   uint64_t* out_len, void* stream);

/* --- TIFF export: a 16-bit (or 8-bit) result on disk.  Upstream stops at gui.py:2338-2341's 8-bit JPEG; this is the same hand-off
 * for a frame of r2f_render16.  The file is baseline TIFF 6.0: little-endian, uncompressed, chunky RGB, BitsPerSample 8,8,8 or
 * 16,16,16, Orientation 1, one strip per rows_per_strip rows (about 256 KiB each), the ICC profile in tag 34675 when given.
 * Everything but the pixels is the header this call writes; the strips follow it one behind the other, so row y of the frame is
 * the row_bytes bytes at header_bytes + y * row_bytes (samples little-endian) and every offset is known before a pixel exists.
 * buf = NULL: the sizes alone (*len, *plan).  R2F_ETOOLARGE: the file would pass a classic TIFF's 4 GiB (plan->file_bytes says by
 * how much; nothing is written).  No GPU, no context. */
typedef struct r2f_tiff_plan {
    uint64_t header_bytes; /* = *len: where the first strip starts (4-byte aligned) */
    uint64_t file_bytes;
    uint64_t row_bytes;    /* W * 3 * bits / 8 */
    uint32_t rows_per_strip, strips;
} r2f_tiff_plan;
R2F_API int r2f_tiff_header(int H, int W, int bits, const uint8_t* icc, size_t icc_len, uint8_t* buf, size_t cap, size_t* len,
                    r2f_tiff_plan* plan);

#ifdef __cplusplus
}
#endif
#endif /* R2F_H */
