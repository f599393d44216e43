// r2f_graph.hip -- the whole-frame render (r2f_render): the launches of one frame, and the cache of captured HIP graphs that
// replays them.
#include <algorithm>
#include <cstring>

#include "r2f_ctx.h"

using namespace r2f;

namespace r2f {

static bool same_structure(const RenderGraph& a, const RenderGraph& b) {
    return a.in_layout == b.in_layout && a.H == b.H && a.W == b.W && !memcmp(&a.p, &b.p, sizeof a.p);
}
static bool same_entry(const RenderGraph& a, const RenderGraph& b) {
    return a.in == b.in && a.out == b.out && a.workspace == b.workspace && same_structure(a, b);
}

RenderGraphCache::~RenderGraphCache() {
    if (cap_stream) (void)hipStreamDestroy(cap_stream);
}

int RenderGraphCache::find(const RenderGraph& key) const {
    int slot = -1;
    for (size_t i = 0; i < graphs.size(); ++i)
        if (same_entry(graphs[i], key)) slot = (int)i;
    return slot;
}

void RenderGraphCache::note_eager(const RenderGraph& key) {
    warm = key, warm_valid = true;
    for (const auto& k : seen)
        if (same_entry(k, key)) return;
    if (seen.size() >= 16) seen.erase(seen.begin());
    seen.push_back(key);
}

// The first frame of a structure runs kernel by kernel (uploads and allocations synchronise and cannot be captured); once the
// context has rendered this structure at this generation, an entry is captured the second time its buffers come by (fresh buffers
// every frame -- results a caller keeps alive -- would pay ~0.9 ms per 24 MP frame for graphs never replayed).
bool RenderGraphCache::should_capture(const RenderGraph& key, int slot) const {
    if ((slot >= 0 && graphs[slot].never) || !warm_valid || !same_structure(warm, key)) return false;
    for (const auto& k : seen)
        if (same_entry(k, key)) return true;
    return false;
}

int RenderGraphCache::insert(const RenderGraph& key) {
    if (graphs.size() >= 8) {  // callers that hand in fresh buffers every frame: bounded bookkeeping, least recently used out
        size_t lru = 0;
        for (size_t i = 1; i < graphs.size(); ++i)
            if (graphs[i].last_use < graphs[lru].last_use) lru = i;
        retire(graphs[lru]);  // (a replay of it may still be running: destroyed behind its event, later)
        graphs.erase(graphs.begin() + (long)lru);
    }
    graphs.push_back(key);
    return (int)graphs.size() - 1;
}

void RenderGraphCache::retire(RenderGraph& g) {
    if (g.exec) {
        retired.push_back({g.graph, g.exec, g.done});
        ++dropped;
    } else {
        if (g.graph) (void)hipGraphDestroy(g.graph);
        if (g.done) (void)hipEventDestroy(g.done);
    }
    g.graph = nullptr, g.exec = nullptr, g.done = nullptr;
}

void RenderGraphCache::drop_all() {
    // a replay of one of them may still be running (an option changed between two asynchronous frames; table uploads and buffer
    // growth have synchronised already): an executable graph must outlive its last launch -- parked, not waited for
    for (auto& g : graphs) retire(g);
    graphs.clear();
    warm_valid = false;
    reap(false);
}

void RenderGraphCache::follow(uint64_t ctx_generation) {
    if (generation == ctx_generation) return;
    drop_all();
    generation = ctx_generation;
}

void RenderGraphCache::reap(bool wait) {
    // Graphs whose completion cannot be asked for -- no event (its creation failed at capture time), or one recorded inside a
    // caller's stream capture -- are kept; when more than a handful of entries pile up the device is synchronised once and
    // everything goes (a missing event used to read as "complete", and the list could grow without bound).
    if (!wait && retired.size() > 16) {
        (void)hipDeviceSynchronize();
        wait = true;
    }
    size_t kept = 0;
    for (auto& r : retired) {
        hipError_t e = r.done ? (wait ? hipEventSynchronize(r.done) : hipEventQuery(r.done)) : (wait ? hipSuccess : hipErrorNotReady);
        if (e == hipErrorNotReady) {
            retired[kept++] = r;
            continue;
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();  // (an event recorded inside a caller's stream capture cannot be queried: keep the graph until
            if (!wait) {              //  the list is flushed behind a device synchronisation, above or in r2f_destroy)
                retired[kept++] = r;
                continue;
            }
        }
        if (r.exec) (void)hipGraphExecDestroy(r.exec);
        if (r.graph) (void)hipGraphDestroy(r.graph);
        if (r.done) (void)hipEventDestroy(r.done);
    }
    retired.resize(kept);
}

}  // namespace r2f

// The launches of one frame, in order, on stream `stream` (a capturing stream of the context's own or the caller's).
static int render_launches(r2f_ctx* ctx, const r2f_params* p, const void* in, int in_layout, const HwcOut& out, int H, int W,
                           void* workspace, void* stream) {
    const bool hal = p->flags & R2F_F_HALATION, mtf = p->flags & R2F_F_MTF, grain = p->flags & R2F_F_GRAIN;
    const bool burn = p->flags & R2F_F_BURN;
    const size_t set_floats = plan::plane_set_floats(H, W);
    float* base = static_cast<float*>(workspace);
    r2f_planes A{base, (int64_t)(set_floats / 3), 0, H};
    r2f_planes B{base + set_floats, (int64_t)(set_floats / 3), 0, H};
    int rc, finished = 0;
    bool tracked = false;
    ctx->frame_dyn_armed = false;
    if (hal) {  // the halation's identity channels (blue on a colour stock) are finished by the front kernel, straight into B
        // kernel by kernel: the frame block (seed, exposure range reset) ahead of the front kernel.  A caller that keeps the seed
        // resident still gets the range reset -- every frame's record starts empty, whatever the flag (the union of
        // earlier frames' ranges used to decide frame N's scratch element); inside a capture the reset stays outside with the seed
        // write (r2f_render issues one or the other ahead of every replay)
        if (!(p->flags & R2F_F_FRAME_RESIDENT) || !ctx->capturing) {
            rc = write_frame_params(ctx, p, static_cast<hipStream_t>(stream), (p->flags & R2F_F_FRAME_RESIDENT) ? 2 : 1);
            if (rc) return rc;
        }
        // ... and also records the range of the exposure planes it writes (every row of them)
        rc = stage_front_impl(ctx, p, in, in_layout, 0, H, R2F_UPTO_EXPOSURE, &A, HwcOut{}, 0, H, W, H, stream, &B, &finished, &tracked);
    } else
        rc = stage_front_impl(ctx, p, in, in_layout, 0, H, R2F_UPTO_DENSITY, &A, HwcOut{}, 0, H, W, H, stream);
    if (rc) return rc;
    const r2f_planes* cur = &A;
    const r2f_planes* other = &B;
    if (hal) {
        // (r2f_stage_halation with the vouching bit: the record's tiles were filled for exactly these exposure planes)
        rc = run_stencil(ctx, R2F_KERNEL_HALATION, cur, other, 0, H, W, H, 1, p->log_eps, static_cast<hipStream_t>(stream),
                         finished != 0 || (p->flags & R2F_F_IDENTITY_DONE) != 0, tracked);
        if (rc) return rc;
        std::swap(cur, other);
    }
    if (mtf) {
        rc = r2f_stage_mtf(ctx, p, cur, other, 0, H, W, H, stream);
        if (rc) return rc;
        std::swap(cur, other);
    }
    if (!burn) return stage_tail_impl(ctx, p, cur, nullptr, out, 0, H, W, H, stream);
    // S7: the burn map depends on the whole grained frame -> grain to planes, reduce, blur, then finish
    int sets_used = (hal || mtf) ? 2 : 1;
    if (grain) {
        if (sets_used == 1) sets_used = 2;
        rc = r2f_stage_grain(ctx, p, cur, other, 0, H, W, H, stream);
        if (rc) return rc;
        std::swap(cur, other);
    }
    int h_lo, w_lo;
    if (!plan::burn_geometry(p->burn_cell, H, W, &h_lo, &w_lo)) return fail(ctx, R2F_EINVAL, "render: bad burn_cell");
    float* sums = base + (size_t)sets_used * set_floats;
    float* map = sums + (size_t)h_lo * w_lo;
    float* scratch = map + (size_t)h_lo * w_lo;
    rc = r2f_stage_burn_sums(ctx, p, cur, sums, 0, H, W, H, stream);
    if (rc) return rc;
    rc = r2f_stage_burn_map(ctx, p, sums, map, scratch, W, H, stream);
    if (rc) return rc;
    r2f_params q = *p;
    q.flags &= ~(uint32_t)R2F_F_GRAIN;
    return stage_tail_impl(ctx, &q, cur, map, out, 0, H, W, H, stream);
}

// r2f_render (out.u16 = nullptr) and r2f_render16 (out.u8 = nullptr): one graph cache, the output a frame writes in its key
static int render_impl(r2f_ctx* ctx, const r2f_params* p, const void* in, int in_layout, const HwcOut& out, bool want16, int H, int W,
                       void* workspace, size_t workspace_bytes, void* stream) {
    if (!ctx || !p) return R2F_EINVAL;
    R2F_GUARD(ctx);
    if (H <= 0 || W <= 0) return fail(ctx, R2F_EINVAL, "render: empty frame");
    if (want16 && !out.u16) return fail(ctx, R2F_EINVAL, "render16: no uint16 output buffer");
    const size_t need = r2f_workspace_bytes(p, H, W);
    if (need > workspace_bytes || (need && !workspace)) return fail(ctx, R2F_EINVAL, "render: workspace too small (%zu needed)", need);
    if (need && !aligned16(workspace)) return fail(ctx, R2F_EINVAL, "render: workspace must be 16-byte aligned");
    const bool hal = p->flags & R2F_F_HALATION, mtf = p->flags & R2F_F_MTF, grain = p->flags & R2F_F_GRAIN;
    const bool burn = p->flags & R2F_F_BURN;
    if (!(hal || mtf || grain || burn))  // config "LUTs only": one fused pointwise pass (one submit as it is)
        return stage_front_impl(ctx, p, in, in_layout, 0, H, R2F_UPTO_OUTPUT, nullptr, out, 0, H, W, H, stream);
    hipStream_t s = static_cast<hipStream_t>(stream);
    RenderGraphCache& gc = ctx->graphs;
    // per-launch event timing (bench.py's breakdowns) creates and records events per launch: kernel by kernel only
    if (!ctx->opt.render_graph || ctx->opt.timing) {
        ++gc.eager;
        return render_launches(ctx, p, in, in_layout, out, H, W, workspace, stream);
    }
    if (!gc.retired.empty()) gc.reap(false);
    gc.follow(ctx->generation);
    RenderGraph key;
    key.in = in, key.in_layout = in_layout, key.out = out, key.H = H, key.W = W, key.workspace = workspace;
    key.p = *p;
    key.p.seed = 0;
    key.p.flags &= ~(uint32_t)R2F_F_FRAME_RESIDENT;
    int slot = gc.find(key);
    auto eager = [&]() -> int {
        ++gc.eager;
        const int rc = render_launches(ctx, p, in, in_layout, out, H, W, workspace, stream);
        gc.follow(ctx->generation);  // this frame built something (a lazy table, a larger scratch): every captured pointer may dangle
        if (rc == R2F_OK) gc.note_eager(key);
        return rc;
    };
    auto replay = [&](RenderGraph& g) -> int {
        // seed + range reset; a caller that wrote the seed itself (the flag) gets the range reset alone
        int rc = write_frame_params(ctx, p, s, (p->flags & R2F_F_FRAME_RESIDENT) ? 2 : 1);
        if (rc) return rc;
        R2F_HIP(ctx, hipGraphLaunch(g.exec, s));
        if (g.done) R2F_HIP(ctx, hipEventRecord(g.done, s));
        ++gc.replays;
        return R2F_OK;
    };
    if (slot >= 0 && gc.graphs[slot].exec) {
        RenderGraph& g = gc.graphs[slot];
        g.last_use = ++gc.clock;
        ctx->frame_dyn_armed = g.dyn_armed;
        return replay(g);
    }
    if (!gc.should_capture(key, slot)) return eager();
    if (!gc.cap_stream) R2F_HIP(ctx, hipStreamCreateWithFlags(&gc.cap_stream, hipStreamNonBlocking));
    if (slot < 0) slot = gc.insert(key);
    const uint64_t gen0 = ctx->generation;
    r2f_params q = *p;
    q.flags |= R2F_F_FRAME_RESIDENT;  // the seed write stays outside the graph
    hipGraph_t graph = nullptr;
    // thread-local mode: other threads of the process (RCCL's watchdog, a producer thread) may keep calling into HIP meanwhile
    hipError_t e = hipStreamBeginCapture(gc.cap_stream, hipStreamCaptureModeThreadLocal);
    int rc = R2F_OK;
    if (e == hipSuccess) {
        ctx->capturing = true;
        rc = render_launches(ctx, &q, in, in_layout, out, H, W, workspace, gc.cap_stream);
        ctx->capturing = false;
        e = hipStreamEndCapture(gc.cap_stream, &graph);
    }
    hipGraphExec_t exec = nullptr;
    if (e == hipSuccess && rc == R2F_OK && graph && ctx->generation == gen0) e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (e != hipSuccess || rc != R2F_OK || !exec || ctx->generation != gen0) {
        // a failed capture must not cost the frame: clear the sticky error, remember not to try again, launch kernel by kernel
        (void)hipGetLastError();
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
        ++gc.dropped;
        if (ctx->generation != gen0)
            gc.follow(ctx->generation);
        else
            gc.graphs[slot].never = true;
        return eager();
    }
    RenderGraph& g = gc.graphs[slot];
    g.graph = graph;
    g.exec = exec;
    g.last_use = ++gc.clock;
    g.dyn_armed = ctx->frame_dyn_armed;  // (what the captured halation launches carry; r2f_frame_exposure_range after a replay)
    if (hipEventCreateWithFlags(&g.done, hipEventDisableTiming) != hipSuccess) g.done = nullptr, (void)hipGetLastError();
    ++gc.captures;
    return replay(g);
}

extern "C" {

int r2f_render(r2f_ctx* ctx, const r2f_params* p, const void* in, int in_layout, float* out_f32, uint8_t* out_u8, int H,
               int W, void* workspace, size_t workspace_bytes, void* stream) {
    return render_impl(ctx, p, in, in_layout, HwcOut{out_f32, out_u8, nullptr, 0}, false, H, W, workspace, workspace_bytes, stream);
}

int r2f_render16(r2f_ctx* ctx, const r2f_params* p, const void* in, int in_layout, float* out_f32, uint16_t* out_u16, int H, int W,
                 void* workspace, size_t workspace_bytes, void* stream) {
    return render_impl(ctx, p, in, in_layout, HwcOut{out_f32, nullptr, out_u16, 0}, true, H, W, workspace, workspace_bytes, stream);
}

int r2f_render_stats(const r2f_ctx* ctx, uint64_t* out4) {
    if (!ctx || !out4) return R2F_EINVAL;
    out4[0] = ctx->graphs.replays, out4[1] = ctx->graphs.captures, out4[2] = ctx->graphs.eager, out4[3] = ctx->graphs.dropped;
    return R2F_OK;
}

}  // extern "C"
