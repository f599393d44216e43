"""Multi-GPU layers over the single-GPU path (nothing like them exists upstream).

RowShardedRenderer -- ONE large frame, contiguous row shards, one process per GPU
    (torch.distributed; backend "nccl" = RCCL over xGMI on the GPU box, "gloo" in CPU tests).
    Pixels are independent except for the two stencils, so a frame costs ONE neighbour
    exchange (or two: `exchanges`, measured on the first frames when left on "auto") and no reduction:
        S0+S1 on own rows -> exposure E            exchange r_h + r_m rows of E  (both stencils' halo)
        S2+S3+S4 on own rows + r_m -> density D    [or: exchange r_m rows of D  (MTF halo)]
        S5 -> S6 (hash noise at GLOBAL coordinates, no exchange) -> S8 -> own output rows
        [S7 highlight burn, when on: one all-reduce (SUM) of the ~50 x 75 low-res cell sums between S6 and S8]
    The exchange is one send + one receive per neighbour and plane, batched (`batch_isend_irecv`, i.e.
    ncclGroupStart/End): at 100 MP that is 60 rows x 12288 px x 4 B for the two planes the halation blurs and
    17 rows for the single-tap blue plane (MTF halo only) = 6.6 MB per direction -- latency-bound, every pair
    on its own xGMI link.  S0+S1 runs on the rows the neighbours wait for
    first and on the interior rows while the halos travel.  Global top/bottom edges are
    reflected (BORDER_REFLECT_101) inside the kernels.  With the DIRECT stencils (`stencil_fft = 0`) every
    stage sums its taps in a tile-independent order and the sharded result is bit-identical to the single-GPU
    one.  The default fp64 FFT form anchors its overlap-save windows at the first row of the call, so a shard
    tiles the frame differently from the whole-frame render: the fp64 rounding noise (~1e-13) differs, and after
    the one rounding to fp32 a handful of pixels of a 100 MP frame may differ by one ulp (tests/test_gpu_fullsize.py).
    Which schedule runs -- one exchange with the halation in one call, or as interior + bands with the interior ahead of the
    exchange, or two exchanges (exposure halo, then density halo: one halation window row fewer per 1/8 shard at 100 MP) -- is
    MEASURED: the first frames render under each candidate between events on the launch stream, the ranks all-reduce (MAX)
    the times and take the one whose slowest rank was fastest (`schedule`, `tuned_ms`); graphs are captured for that one.

BatchSharder -- MANY frames (batch export, gui.py:2393-2514): frame i -> rank i mod world, no
    collectives; per rank a producer thread runs the host phase (`extract_image_data_cpu`) one
    frame ahead of the device phase (`process_preloaded`) through a depth-1 queue, and a frame
    whose host phase fails is skipped -- the semantics of GpuWorker.run_tasks (gui_objects.py:65-115).

The compute itself is behind a small backend protocol so that the exchange logic can be tested
on CPU tensors (tests/test_sharding_cpu.py); `HipStageBackend` is the product backend.

Where things are: shard_plan.py holds the integer side of the row shards without torch (`plan_shard`: rows, plane extents, halos, split,
candidate schedules; `schedule_of`; `ScheduleTuner`); here, `GraphCache` keeps the books of the captured graphs and `RowShardedRenderer`
the planes, the exchange and ONE description of a frame -- a list of steps (`_build_steps`) that the eager launches, the capture and
the replay all walk.  tools/shard_walk_digest.py logs what that walk asks of a backend, case by case, without a GPU.
"""

from __future__ import annotations

import gc
import queue
import threading
from typing import NamedTuple

from .shard_plan import ScheduleTuner, ShardPlan, plan_shard, schedule_of, shard_rows  # noqa: F401 -- (ShardPlan, shard_rows: re-exported)


class HipStageBackend:
    """Stage calls of one GPU's HipContext on (3, rows, W) float32 CUDA tensors."""

    def __init__(self, ctx, params, halation_taps=(0, 0), mtf_taps=(0, 0), halation_taps_per_channel=None, halation_box=None):
        """halation_taps_per_channel: [(above, below)] x 3 (stencils.vertical_reach_per_channel): planes whose halation stencil is a
        single tap need no halation halo.  halation_box: (rows, columns) of the halation's non-zero tap box, for `halation_band_rows`."""
        import torch

        self.torch = torch
        self.ctx = ctx
        # a copy: begin_frame() writes the seed and F_FRAME_RESIDENT into it, which must not leak into a parameter block the caller
        # goes on to hand to ctx.render() (whose own seed write that flag would switch off)
        from . import _lib

        self.params = _lib.Params.from_buffer_copy(params) if isinstance(params, _lib.Params) else params
        self.halation_taps = halation_taps  # (rows above, rows below) the stencil reaches
        self.mtf_taps = mtf_taps
        self.halation_taps_per_channel = halation_taps_per_channel
        self.halation_box = halation_box
        self.device = ctx.device

    @classmethod
    def for_stencils(cls, ctx, params, halation_kernel=None, mtf_kernel=None):
        """The backend for a context whose halation / MTF stencils are these (kh, kw, 1|3) arrays (None: stage off): their vertical
        reach, the reach of each halation plane on its own and the halation's tap box are what the row tiler plans with."""
        import numpy as np

        from . import stencils

        per, box = None, None
        if halation_kernel is not None:
            k = np.asarray(halation_kernel)
            k = k[..., None] if k.ndim == 2 else k
            per = stencils.vertical_reach_per_channel(k)
            nz = np.nonzero(np.any(k != 0, axis=2))
            if nz[0].size:
                box = (int(nz[0].max() - nz[0].min() + 1), int(nz[1].max() - nz[1].min() + 1))
        return cls(ctx, params,
                   halation_taps=stencils.vertical_reach(halation_kernel) if halation_kernel is not None else (0, 0),
                   mtf_taps=stencils.vertical_reach(mtf_kernel) if mtf_kernel is not None else (0, 0),
                   halation_taps_per_channel=per, halation_box=box)

    def halation_band_rows(self, W: int, rows: int) -> int:
        """Rows one window row of the halation's FFT form yields on a call of `rows` rows (r2f_plan_fft, default options): a boundary
        band of that height costs the frame no extra window row.  0 when unknown (direct form, no box given)."""
        import ctypes as C

        from . import _lib

        if not self.halation_box:
            return 0
        bh, bw = self.halation_box
        if bh * bw < 400 or max(bh, bw) > 400:
            return 0
        plan = _lib.FftPlan()
        if _lib.load().r2f_plan_fft(int(bh), int(bw), int(W), int(rows), 2, 16, 0, 0, 512, 192, 2, C.byref(plan)) != 0:
            return 0
        return int(plan.vy)

    def empty(self, rows, W):
        return self.torch.empty((3, rows, W), dtype=self.torch.float32, device=self.device)

    def begin_frame(self, seed=None):
        """Ahead of a frame's stage calls: the grain seed (a new one when given) goes to the context's device-side frame block
        (r2f_write_frame_params) and the stage calls are told to read it there (F_FRAME_RESIDENT) -- so a captured graph of
        those calls does not freeze the seed (the reference makes a new seed per render, gpu_processor.py:585-597)."""
        from . import _lib

        if seed is not None:
            self.params.seed = int(seed) & 0xFFFFFFFF
        self.params.flags |= _lib.F_FRAME_RESIDENT
        self.ctx.write_frame_params(self.params)

    def graph_key(self) -> bytes:
        """The parameter block as a captured graph sees it: everything but the seed."""
        from . import _lib

        p = _lib.Params.from_buffer_copy(self.params)
        p.seed = 0
        p.flags |= _lib.F_FRAME_RESIDENT
        return bytes(p)

    # The exposure-range record behind the device-side choice of the halation's FFT scratch element (r2f.h, r2f_render): the stage
    # path keeps it like a whole-frame render does -- front calls record the rows they write (track), `exposure_range` adds the rows
    # received from the neighbours, and `halation(range_valid=True)` vouches that the record covers every row of the buffer it reads.
    tracks_range = True

    def front(self, image_rows, in_gy0, upto, dst, dst_gy0, y0, y1, H, track=False):
        self.ctx.stage_front(image_rows, self.params, upto, in_gy0=in_gy0, dst=dst, dst_gy0=dst_gy0, y0=y0, y1=y1, H_global=H,
                             track_range=track)

    def front_split(self, image_rows, in_gy0, E, e_gy0, D, d_gy0, y0, y1, H, track=False):
        """front(upto = exposure) with the halation's identity channels finished straight into D; returns their mask."""
        return self.ctx.stage_front_split(image_rows, self.params, E, D, in_gy0=in_gy0, exposure_gy0=e_gy0, density_gy0=d_gy0,
                                          y0=y0, y1=y1, H_global=H, track_range=track)

    def exposure_range(self, E, e_gy0, y0, y1, y2=0, y3=0):
        self.ctx.stage_exposure_range(E, src_gy0=e_gy0, y0=y0, y1=y1, y2=y2, y3=y3)

    def halation(self, E, e_gy0, D, d_gy0, y0, y1, H, identity_done=0, range_valid=False):
        self.ctx.stage_halation(E, D, self.params, src_gy0=e_gy0, dst_gy0=d_gy0, y0=y0, y1=y1, H_global=H,
                                identity_done=identity_done, range_valid=range_valid)

    def mtf(self, D, d_gy0, D2, d2_gy0, y0, y1, H):
        self.ctx.stage_mtf(D, D2, self.params, src_gy0=d_gy0, dst_gy0=d2_gy0, y0=y0, y1=y1, H_global=H)

    def tail(self, D, d_gy0, out_f32, out_u8, out_gy0, y0, y1, H, burn_map=None):
        params = self.params
        if burn_map is not None:  # the grain has been applied by grain() already
            from . import _lib

            params = _lib.Params.from_buffer_copy(self.params)
            params.flags &= ~_lib.F_GRAIN
        self.ctx.stage_tail(D, params, src_gy0=d_gy0, out_f32=out_f32, out_u8=out_u8, out_gy0=out_gy0, y0=y0, y1=y1,
                            H_global=H, burn_map=burn_map)

    def grain_field(self, F, f_gy0, y0, y1, H):
        """K_g * N for rows [y0, y1): depends on the seed and the coordinates only, so it can run beside the stencils."""
        self.ctx.stage_grain_field(F, self.params, dst_gy0=f_gy0, y0=y0, y1=y1, H_global=H)

    def tail_field(self, D, d_gy0, F, f_gy0, out_f32, out_u8, out_gy0, y0, y1, H):
        self.ctx.stage_tail_field(D, F, self.params, src_gy0=d_gy0, field_gy0=f_gy0, out_f32=out_f32, out_u8=out_u8,
                                  out_gy0=out_gy0, y0=y0, y1=y1, H_global=H)

    def grain(self, D, d_gy0, G, g_gy0, y0, y1, H):
        self.ctx.stage_grain(D, G, self.params, src_gy0=d_gy0, dst_gy0=g_gy0, y0=y0, y1=y1, H_global=H)

    def burn_sums(self, D, d_gy0, y0, y1, H):
        return self.ctx.stage_burn_sums(D, self.params, src_gy0=d_gy0, y0=y0, y1=y1, H_global=H)

    def burn_map(self, sums, W, H):
        return self.ctx.stage_burn_map(sums, self.params, W=W, H_global=H)

    def front_to_output(self, image_rows, in_gy0, out_f32, out_u8, out_gy0, y0, y1, H):
        self.ctx.stage_front(image_rows, self.params, 2, in_gy0=in_gy0, out_f32=out_f32, out_u8=out_u8, out_gy0=out_gy0,
                             y0=y0, y1=y1, H_global=H)


class GraphCache:
    """The bookkeeping of a renderer's captured graphs -- plain Python, the graphs themselves are opaque to it.
    key -> [frames seen with this key, its graphs or None], most recently used last, at most `LIMIT` keys: callers that hand in
    fresh buffers every frame pile up neither graphs nor counters.
    A capture freezes every by-value launch argument (seed, flags, curve constants, tap weights) and every device pointer into the
    context's tables and scratch.  `state` is what the graphs were captured from: the context's change counter (table / stencil /
    option uploads and re-allocations of its internal buffers) and the parameter block.  When it moves, every graph is dropped and
    the frame at hand runs eagerly, like a first frame."""

    LIMIT = 8

    def __init__(self):
        self._slots = {}
        self.state = None

    def slot(self, key, state) -> list:
        """This frame's [frames seen, graphs or None], counted in.  1: a first frame with these buffers runs eagerly (tables,
        scratch and spectra get built there); with None from 2 on: capture."""
        if state != self.state:
            self._slots.clear()
            self.state = state
        slot = self._slots.pop(key, None) or [0, None]
        self._slots[key] = slot  # most recently used last
        while len(self._slots) > self.LIMIT:
            del self._slots[next(iter(self._slots))]
        slot[0] += 1
        return slot

    def after_eager(self, key, slot, state):
        """state: what the eager first frame left -- what it built lazily is the state the next one is captured from.  Where that
        frame moved the context (a lazy table upload, a re-allocated scratch), graphs captured for OTHER buffer keys froze the old
        pointers: they go, only this key's counter stays."""
        if state != self.state:
            self._slots = {key: slot}
        self.state = state

    def drop(self):
        self._slots.clear()

    def counts(self) -> list:
        """Per key, least recently used first: the number of captured graphs, None where nothing is captured yet."""
        return [None if graphs is None else len(graphs) for _, graphs in self._slots.values()]


class Step(NamedTuple):
    """One step of a frame (RowShardedRenderer._build_steps)."""
    name: str  # the trace word of a host step, and of the graph that ends with this step ("replay:<name>")
    run: object  # run(frame)
    capture: bool  # may be part of a captured graph
    host: bool = False  # runs on the host on every frame, noted in the trace -- also where a graph's run includes it


class _Frame:
    """What the steps of one frame share."""
    __slots__ = ("image_rows", "out_f32", "out_u8", "field_ready", "pending")

    def __init__(self, image_rows, out_f32, out_u8, field_ready=None):
        self.image_rows, self.out_f32, self.out_u8, self.field_ready = image_rows, out_f32, out_u8, field_ready
        self.pending = None  # the exposure exchange in flight


class RowShardedRenderer:
    """Render one H x W frame whose rows are sharded over the ranks of a process group.

    backend:   object with empty/front/halation/mtf/tail/front_to_output (see HipStageBackend)
    halation / mtf / grain: which stages are enabled (the stage gates of cpu_processor.py:368,382,387)
    dyn_scratch: with a backend that keeps the exposure-range record (HipStageBackend.tracks_range) the halation's FFT passes
               choose their scratch element on the device, per frame and per window pair, like a whole-frame r2f_render's (default); False: complex128
               whatever the rows hold (bit-for-bit comparisons with a render under stencil_fft_scratch96_auto = 0, A/B)
    frame_timer(candidate, render) -> ms: how a measuring frame is timed; default: two events on the launch stream around the
               frame (device backends only).  Tests of the tuning protocol itself inject a clock of their own (CPU backends, gloo).

    The geometry, the candidate schedules and the tuner's protocol are shard_plan.py's; the order of a frame is `_build_steps`.
    """

    def __init__(self, backend, H: int, W: int, *, halation: bool, mtf: bool, grain: bool = True, burn: bool = False,
                 group=None, rank=None, world=None, side_grain: bool = False, graph: bool = False, split_halation="auto",
                 exchanges="auto", tune_frames: int = 2, frame_timer=None, dyn_scratch: bool = True):
        import torch
        import torch.distributed as dist

        self.torch, self.dist = torch, dist
        self.backend, self.group = backend, group
        live = dist.is_available() and dist.is_initialized()
        if rank is None:
            rank = dist.get_rank(group) if live else 0
        if world is None:
            world = dist.get_world_size(group) if live else 1
        self.halation, self.mtf, self.grain, self.burn = halation, mtf, grain, burn
        # The halation's FFT passes choose their scratch element on the device, per frame and window pair, exactly like a whole-frame r2f_render
        # (VERDICT r5, next 3): this rank's front calls record the range of the exposure rows they write, a small kernel adds the
        # halo rows the neighbours sent, and the halation calls vouch for the record.  A rank-local record is sufficient -- the
        # choice is per window pair (tiles indexed by GLOBAL rows), and every window of this rank reads rows of this rank's buffer only.
        self._dyn = bool(dyn_scratch and halation and getattr(backend, "tracks_range", False))
        lay = self._layout = plan_shard(
            H, W, rank, world, halation=halation, mtf=mtf, halation_taps=backend.halation_taps if halation else (0, 0),
            mtf_taps=backend.mtf_taps if mtf else (0, 0), halation_taps_per_channel=getattr(backend, "halation_taps_per_channel", None),
            band_rows=getattr(backend, "halation_band_rows", lambda W, rows: 0), exchanges=exchanges, split_halation=split_halation)
        self.plan, self._candidates = lay.plan, lay.candidates
        self.e_lo, self.e_hi, self.d_lo, self.d_hi = lay.e_lo, lay.e_hi, lay.d_lo, lay.d_hi
        on_device = getattr(backend, "device", None) is not None and torch.cuda.is_available()
        self._allocate(bool(side_grain and on_device))
        # graph = True (device backends): everything after the halo exchange -- the ~130 launches of the FFT stencils and the
        # tail, on this renderer's own persistent planes -- is captured into a HIP graph the second time a frame arrives with
        # the same output buffers, and replayed from then on: one graph launch (10-16 us of host time) instead of one launch
        # per kernel, which is what a 1/8 row shard (~1 ms of device work) needs to stay device-bound.  With world == 1 there
        # is no exchange and the front kernel is part of the graph.  Results are the eager path's, bit for bit.
        self.graph = bool(graph and not burn and not self.side_grain and on_device and (halation or mtf or grain))
        self._cache = GraphCache()
        self._identity_done = 0  # channel mask front_split finished (world == 1 only)
        self.trace = None  # a list here collects (event name) in issue order: tests look at the overlap structure
        self.schedule = None
        self.tuned_ms = None  # per candidate: the measured frame time (max over ranks) the choice was made from
        self._frame_timer = frame_timer
        # nothing to choose from, tune_frames = 0 or a backend without a device to time (the CPU backends of the test-suite): the
        # first candidate -- one exchange, no split -- unless the caller fixed the schedule
        self._tuner = ScheduleTuner(lay.candidates, tune_frames, can_measure=frame_timer is not None or on_device)
        self.tune_frames = self._tuner.tune_frames
        self._check_candidates()
        self._set_schedule(self._tuner.current)

    def _allocate(self, side_grain: bool):
        """The planes of this rank, from the backend at hand (plain attributes, read at render time: callers may share them)."""
        p, be, W = self.plan, self.backend, self.plan.W
        halation, mtf = self.halation, self.mtf
        self.E = be.empty(self.e_hi - self.e_lo, W) if halation else None
        self.D = be.empty(self.d_hi - self.d_lo, W) if (halation or mtf) else None
        self.D2 = be.empty(p.rows, W) if mtf else None
        self.Dplain = be.empty(p.rows, W) if not (halation or mtf) else None
        self.G = be.empty(p.rows, W) if (self.burn and self.grain) else None  # grained density, needed whole before S7
        # The grain field does not depend on the image: with a device backend it is made on a side stream while the
        # (memory-bound) stencils run, and the tail shrinks to a pointwise pass.
        self.side_grain = bool(side_grain and self.grain and not self.burn and (halation or mtf) and hasattr(be, "grain_field"))
        self.F = be.empty(p.rows, W) if self.side_grain else None
        self.side_stream = self.torch.cuda.Stream(device=be.device) if self.side_grain else None

    # ------------------------------------------------------------------ host-side agreement
    def _can_agree(self) -> bool:
        """Is there a real process group to agree with?  (A subclass that replaces the transport has no peers to ask.)"""
        dist = self.dist
        return (self.plan.world > 1 and dist.is_available() and dist.is_initialized()
                and type(self)._exchange is RowShardedRenderer._exchange)

    def _agree_max(self, values) -> list[float]:
        """The element-wise MAX over the ranks of a short vector of floats: one all-reduce of float64, in host memory for gloo,
        on the backend's device otherwise."""
        torch, dist = self.torch, self.dist
        dev = getattr(self.backend, "device", None)
        if dev is None or dist.get_backend(self.group) == "gloo":
            dev = "cpu"
        buf = torch.tensor(list(values), dtype=torch.float64, device=dev)
        dist.all_reduce(buf, op=dist.ReduceOp.MAX, group=self.group)
        return buf.cpu().tolist()

    def _check_candidates(self):
        """The ranks walk the candidate list in lockstep (one all-reduce per decision, and the two-exchange form needs both
        neighbours to play along): a list that differs between ranks would deadlock in a collective much later -- compare a hash
        of it once, at construction, and fail on every rank at once."""
        cands, p = self._candidates, self.plan
        if not (cands and self._can_agree()):
            return
        import hashlib

        digest = hashlib.sha256(repr((cands, p.H, p.W, p.world)).encode()).digest()
        h = float(int.from_bytes(digest[:6], "big"))  # 48 bits: exact in fp64
        hi, neg_lo = self._agree_max([h, -h])
        if hi != -neg_lo:
            raise RuntimeError(f"rank {p.rank}: the ranks derived different candidate schedules {cands} for this frame "
                               "(different stencils, options or library builds across the ranks?)")

    # ------------------------------------------------------------------ schedule
    @property
    def tuning(self) -> bool:
        """True while the first frames are still measuring the candidate schedules (they render correctly, kernel by kernel)."""
        return self._tuner.measuring

    def _set_schedule(self, sched):
        """sched = (exchanges, split) or None (shard_plan.schedule_of): the halos, the split and the frame's steps follow it."""
        self.single_exchange, self.halo_e_ch, self.split, self.schedule = schedule_of(self._layout, sched)
        self._build_steps()
        self.reset_graphs()

    def _tune_frame(self, image_rows, out_f32, out_u8):
        """One frame of the measuring phase: rendered kernel by kernel under the current candidate, timed between two events on the
        launch stream (exchange included); moves on to the next candidate / to the decision when this one has its frames."""
        torch, t = self.torch, self._tuner
        if not t.next_is_timed:
            t.frame_done()
            return self._render_eager(image_rows, out_f32, out_u8)
        if self._frame_timer is not None:
            box = []
            ms = self._frame_timer(t.current, lambda: box.append(self._render_eager(image_rows, out_f32, out_u8)))
            res = box[0]
        else:
            # on the stream the launches go to: the backend's device's current stream (torch's current DEVICE may be another one)
            stream = torch.cuda.current_stream(self.backend.device)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            res = self._render_eager(image_rows, out_f32, out_u8)
            b.record(stream)
            b.synchronize()
            ms = a.elapsed_time(b)
        if t.frame_done(ms):
            if t.current is not None:
                self._set_schedule(t.current)
            else:
                self._decide()
        return res

    def _decide(self):
        """The schedule whose slowest rank was fastest (best frame of each candidate; MAX over the ranks, so every rank picks the
        same one -- the two-exchange form needs its neighbours to play along)."""
        ms = self._tuner.best()
        if self._can_agree():
            ms = self._agree_max(ms)
        sched, self.tuned_ms = self._tuner.choose(ms)
        self._set_schedule(sched)

    # ------------------------------------------------------------------ neighbour exchange
    def _exchange(self, buf, buf_gy0: int, above, below, wait: bool = True):
        """Fill the halo rows of `buf` (global rows [buf_gy0, ...)) from the neighbours' own rows.
        Rank k sends its first `below_of_prev` rows up and its last `above_of_next` rows down.  above / below: rows per plane
        (an int for all three, or one per plane).
        wait=False: the transfers are only started (RCCL runs them on its own stream, ordered after what the current
        stream holds now); hand the return value to `_exchange_finish` before the halo rows are read."""
        p, dist, torch = self.plan, self.dist, self.torch
        above = [above] * 3 if isinstance(above, int) else list(above)
        below = [below] * 3 if isinstance(below, int) else list(below)
        if p.world == 1 or (max(above) == 0 and max(below) == 0):
            return None
        ops, recvs = [], []
        own0 = p.r0 - buf_gy0  # buffer row of the first own row
        # RCCL moves device buffers directly and orders them against the current stream.  gloo (CPU tests,
        # single-GPU validation) is a host transport: stage through host memory explicitly.
        host_staging = buf.is_cuda and dist.get_backend(self.group) == "gloo"

        # A halo is `n` consecutive rows of each of the 3 planes: 3 contiguous blocks.  On RCCL they are sent
        # from / received into the plane buffer directly (no staging copies); on gloo through host tensors.
        def add_send(first_row, rows_of, peer):
            for c in range(3):
                n = rows_of[c]
                if n:
                    block = buf[c, first_row(n):first_row(n) + n, :]
                    ops.append(dist.P2POp(dist.isend, block.cpu() if host_staging else block, peer, self.group))

        def add_recv(first_row, rows_of, peer):
            for c in range(3):
                n = rows_of[c]
                if not n:
                    continue
                block = buf[c, first_row(n):first_row(n) + n, :]
                if host_staging:
                    tmp = torch.empty((n, p.W), dtype=buf.dtype, device="cpu")
                    ops.append(dist.P2POp(dist.irecv, tmp, peer, self.group))
                    recvs.append((tmp, block))
                else:
                    ops.append(dist.P2POp(dist.irecv, block, peer, self.group))

        if p.rank > 0:  # neighbour above: it needs my top `below` rows, I need its bottom `above` rows
            add_send(lambda n: own0, below, self._peer(p.rank - 1))
            add_recv(lambda n: own0 - n, above, self._peer(p.rank - 1))
        if p.rank < p.world - 1:  # neighbour below
            add_send(lambda n: own0 + p.rows - n, above, self._peer(p.rank + 1))
            add_recv(lambda n: own0 + p.rows, below, self._peer(p.rank + 1))
        reqs = dist.batch_isend_irecv(ops) if ops else []
        if not wait:
            return reqs, recvs
        self._exchange_finish((reqs, recvs))
        return None

    @staticmethod
    def _exchange_finish(pending):
        """Second half of `_exchange(..., wait=False)`: the halo rows are in place (ordered against the current stream)."""
        if pending is None:
            return
        reqs, recvs = pending
        for req in reqs:
            req.wait()
        for tmp, block in recvs:
            block.copy_(tmp)

    def _peer(self, group_rank: int) -> int:
        if self.group is None:
            return group_rank
        return self.dist.get_global_rank(self.group, group_rank)

    # ------------------------------------------------------------------ one frame
    def _build_steps(self):
        """THE order of a frame under the current schedule; the eager launches, the capture and the replay all walk this list.
        A step that may be captured becomes part of a graph, and a graph is a maximal run of such steps, named after its last one:
          world > 1: the front kernels and the exchange(s) are issued every frame.  One exchange: [`halation_interior`, replayed
            while the halos travel,] then `after_exchange`, everything downstream of the exchange.  Two exchanges (or the MTF
            alone): `density` (the halation of the own rows), then -- after the density halo exchange, issued every frame like
            the first one -- `finish`, the MTF and the tail.
          world == 1: nothing travels and every step may be captured: one graph (`after_exchange`), front included (then the
            input buffer is part of the graph's key).  The wait stays a host step all the same: it has nothing to wait for.
        The list follows the schedule, not the frame: `_set_schedule` rebuilds it (and drops the graphs)."""
        whole = self.plan.world == 1
        travels = self.mtf and not self.single_exchange  # density halo rows between the halation and the MTF
        steps = [Step("front", self._step_front, whole)]
        if self.split:
            steps.append(Step("halation_interior", lambda f: self._halation_interior(), True))
        steps.append(Step("exchange_finish", lambda f: self._exchange_finish(f.pending), whole, host=True))
        if self.halation:
            steps.append(Step("density", lambda f: self._density(), True))
        if travels:
            steps.append(Step("exchange_density", lambda f: self._exchange_density(), whole))
        steps.append(Step("finish" if travels and not whole else "after_exchange",
                          lambda f: self._finish(f.out_f32, f.out_u8, f.field_ready), True))
        self._steps = steps
        self._head = 0 if whole else 1  # the front step is launched ahead of the captures of a frame, unless it is captured itself

    def _walk(self, f, start=0, graphs=None):
        """The steps of frame `f` from `start` on.  graphs = None: every step is launched here, kernel by kernel.  Otherwise
        {index of a run's last step: its captured graph}: a captured step is left to its graph, replayed where the run ends."""
        steps = self._steps
        for i in range(start, len(steps)):
            step = steps[i]
            if graphs is None or step.host or not step.capture:
                if step.host:
                    self._note(step.name)
                step.run(f)
            if graphs is not None and i in graphs:
                self._note("replay:" + step.name)
                graphs[i].replay()
        return f.out_f32, f.out_u8

    def _capture(self, f, start):
        """One graph per maximal run of capturable steps from `start` on: {index of the run's last step: graph}."""
        torch, steps = self.torch, self._steps
        graphs, run = {}, []
        # No cycle collection while a capture is open: the steps run Python, so the collector can start in the middle of one, and a
        # dead cycle's finalizer may destroy a captured graph with its memory pool, a stream or a context (an earlier renderer is
        # such a cycle: its step closures refer to it) -- calls a capturing thread must not make; the runtime aborts the process.
        # torch.cuda.graph no longer collects before it begins, so this is done here, once per capture, outside of it.
        gc_was_on = gc.isenabled()
        gc.collect()
        gc.disable()
        try:
            for i in range(start, len(steps) + 1):
                if i < len(steps) and steps[i].capture:
                    run.append(steps[i])
                elif run:
                    g = torch.cuda.CUDAGraph()
                    # thread_local: other threads (RCCL's watchdog polls events) may keep calling into HIP during the capture
                    with torch.cuda.graph(g, capture_error_mode="thread_local"):
                        for step in run:
                            step.run(f)
                    graphs[i - 1], run = g, []
        finally:
            if gc_was_on:
                gc.enable()
        return graphs

    def render(self, image_rows, out_f32=None, out_u8=None, seed=None):
        """image_rows: this rank's own rows of the decoded frame ((rows, W, 3|4) or (3, rows, W)).
        out_*: this rank's own rows of the result, (rows, W, 3).  seed: the grain seed of this frame (every rank the same);
        None keeps the backend's.  A new seed does not cost a captured graph: it lives in a device-side block."""
        if hasattr(self.backend, "begin_frame"):
            self.backend.begin_frame(seed)
        if self._tuner.measuring:
            return self._tune_frame(image_rows, out_f32, out_u8)
        if not self.graph:
            return self._render_eager(image_rows, out_f32, out_u8)
        # world == 1: the front kernel is captured too, so the input buffer is part of the key
        key = (image_rows.data_ptr() if self.plan.world == 1 else 0, tuple(image_rows.shape),
               out_f32.data_ptr() if out_f32 is not None else 0, out_u8.data_ptr() if out_u8 is not None else 0)
        state = self._graph_state()
        slot = self._cache.slot(key, state)
        if slot[0] == 1:
            res = self._render_eager(image_rows, out_f32, out_u8)
            self._cache.after_eager(key, slot, self._graph_state())
            return res
        f, head = _Frame(image_rows, out_f32, out_u8), self._head
        for i in range(head):
            self._steps[i].run(f)
        if slot[1] is None:
            slot[1] = self._try_capture(f, head, state)
            if slot[1] is None:  # the rest of a frame whose capture did not work out, launched kernel by kernel
                return self._walk(f, head)
        return self._walk(f, head, slot[1])

    def _try_capture(self, f, head, state):
        """The graphs of frame `f`'s steps from `head` on, or None where they cannot be had on this frame."""
        try:
            graphs = self._capture(f, head)
        except Exception:  # noqa: BLE001 -- a failed capture must not cost the frame: eager launches from here on
            self.graph = False
            graphs = None
        else:
            if self._graph_state() != state:
                # the capture itself changed the context (a table built lazily on this frame: its upload synchronises and does
                # not belong in a graph) -- keep this frame's eager result semantics simple: run it again eagerly, capture later
                self._cache.state = self._graph_state()
                graphs = None
        if graphs is None:
            self._cache.drop()
            self.torch.cuda.synchronize()
        return graphs

    def _note(self, what):
        if self.trace is not None:
            self.trace.append(what)

    def _graph_state(self):
        """(context change counter, parameter block) of the backend -- what a captured graph of this renderer depends on besides
        its buffers; None for backends without a context."""
        be = self.backend
        ctx, params = getattr(be, "ctx", None), getattr(be, "params", None)
        if ctx is None or not hasattr(ctx, "generation"):
            return None
        if hasattr(be, "graph_key"):  # the seed is not part of it: it lives in the device-side frame block
            return (ctx.generation(), be.graph_key())
        return (ctx.generation(), bytes(params) if params is not None else b"")

    def reset_graphs(self):
        """Drop every captured graph (they are re-captured on the frames that follow)."""
        self._cache.drop()
        self._cache.state = None

    def graph_slots(self) -> list:
        """Per graph key, least recently used first: how many graphs it holds, None where nothing is captured yet."""
        return self._cache.counts()

    def _render_eager(self, image_rows, out_f32=None, out_u8=None):
        p, be = self.plan, self.backend
        H = p.H
        field_ready = None
        if self.side_grain:
            torch = self.torch
            main = torch.cuda.current_stream()
            self.side_stream.wait_stream(main)  # the previous frame's tail may still be reading F
            with torch.cuda.stream(self.side_stream):
                be.grain_field(self.F, p.r0, p.r0, p.r1, H)
                field_ready = self.side_stream.record_event()
        if not (self.halation or self.mtf or self.grain or self.burn):  # LUTs only: one fused pointwise pass
            be.front_to_output(image_rows, p.r0, out_f32, out_u8, p.r0, p.r0, p.r1, H)
            return out_f32, out_u8
        return self._walk(_Frame(image_rows, out_f32, out_u8, field_ready))

    def _step_front(self, f):
        f.pending = self._front_and_start_exchange(f.image_rows)

    def _front_and_start_exchange(self, image_rows):
        """S0 + S1 (+ S3 + S4 without halation) on this rank's rows; the exposure halo exchange is STARTED (the rows the neighbours
        wait for are made first, the interior rows while the halos travel).  Returns what `_exchange_finish` needs."""
        p, be = self.plan, self.backend
        H = p.H
        pending = None
        if not (self.halation or self.mtf or self.grain or self.burn):
            return pending
        if not (self.halation or self.mtf):
            be.front(image_rows, p.r0, 1, self.Dplain, p.r0, p.r0, p.r1, H)
        elif self.halation:
            above, below = [a for a, _ in self.halo_e_ch], [b for _, b in self.halo_e_ch]
            tk = {"track": True} if self._dyn else {}  # the rows this rank writes go into the exposure-range record's tiles
            if p.world > 1 and (max(above) or max(below)) and p.rows >= max(above) + max(below):
                # the rows the neighbours wait for first, then the interior while the halos travel
                lo_band = p.r0 + (max(below) if p.rank > 0 else 0)
                hi_band = p.r1 - (max(above) if p.rank < p.world - 1 else 0)
                if lo_band > p.r0:
                    be.front(image_rows, p.r0, 0, self.E, self.e_lo, p.r0, lo_band, H, **tk)
                if hi_band < p.r1:
                    be.front(image_rows, p.r0, 0, self.E, self.e_lo, hi_band, p.r1, H, **tk)
                self._note("exchange_start")
                pending = self._exchange(self.E, self.e_lo, above, below, wait=False)
                be.front(image_rows, p.r0, 0, self.E, self.e_lo, lo_band, hi_band, H, **tk)
            elif p.world == 1 and hasattr(be, "front_split"):
                # no neighbours to feed: the halation's identity channels (blue on a colour stock) skip their exposure plane
                self._identity_done = be.front_split(image_rows, p.r0, self.E, self.e_lo, self.D, self.d_lo, p.r0, p.r1, H, **tk)
            else:
                be.front(image_rows, p.r0, 0, self.E, self.e_lo, p.r0, p.r1, H, **tk)
                self._note("exchange_start")
                pending = self._exchange(self.E, self.e_lo, above, below, wait=False)
        else:
            be.front(image_rows, p.r0, 1, self.D, self.d_lo, p.r0, p.r1, H)
        return pending

    def _e_rows(self):
        """The exposure planes as the halation calls of the current schedule see them: (view, first global row).  The FFT form's
        windows read any row of the buffer they are handed (rows beyond the stencil's reach feed outputs they discard), so the
        buffer handed over is exactly the rows that are valid THIS frame: own rows plus the halo the schedule exchanges.  (The
        planes are laid out for the single-exchange halo; under two exchanges the rows beyond the narrower halo hold whatever an
        earlier frame or the allocator left there -- harmless to a discarded output, not to a range record that vouches for them.)"""
        p = self.plan
        a = max(x for x, _ in self.halo_e_ch)
        b = max(y for _, y in self.halo_e_ch)
        lo, hi = max(p.r0 - a, 0), min(p.r1 + b, p.H)
        if lo == self.e_lo and hi == self.e_hi:
            return self.E, self.e_lo
        return self.E[:, lo - self.e_lo:hi - self.e_lo, :], lo

    def _halo_range(self):
        """The received halo rows join the exposure-range record's tiles (in stream order behind the exchange)."""
        if not (self._dyn and self.halation) or self.plan.world == 1:
            return
        p, be = self.plan, self.backend
        E, lo = self._e_rows()
        hi = lo + int(E.shape[1])
        self._note("halo_range")
        if lo < p.r0 or hi > p.r1:  # the band above and the band below in one launch
            be.exposure_range(E, lo, lo, p.r0, p.r1, hi)

    def _halation_interior(self):
        """The halation of the rows whose stencil reads this rank's own exposure rows only: issued before the halo exchange is
        waited for."""
        if not self.split:
            return
        p, be = self.plan, self.backend
        lo, hi = self.split
        self._note("halation_interior")
        # (no vouching here: the windows of this call read rows of the halo region too -- for outputs they discard -- and those
        # rows are still travelling)
        be.halation(self.E, self.e_lo, self.D, self.d_lo, lo, hi, p.H)

    def _exchange_density(self):
        """The second exchange of the two-exchange schedule: the MTF's halo rows of the density planes."""
        self._note("exchange_density")
        self._exchange(self.D, self.d_lo, *self.plan.halo_d)

    def _density(self):
        """S2 + S3 + S4: the halation of the rows this schedule wants density for (nothing without halation: the front kernel
        wrote density already)."""
        p, be = self.plan, self.backend
        H = p.H
        if not self.halation:
            return
        # the halo rows that have just arrived join the exposure-range record, ahead of the launches that choose from it (part of
        # the captured graph: two small launches whose issue would otherwise sit between the exchange and the replay)
        self._halo_range()
        kw = {"identity_done": self._identity_done} if self._identity_done else {}
        if self._dyn:  # the record's tiles were filled for every row of the buffer handed over (_e_rows, _halo_range)
            kw["range_valid"] = True
        E, e_lo = self._e_rows()
        if self.split:  # the interior rows are under way (or done): the bands next to the neighbours' rows
            lo, hi = self.split
            self._note("halation_bands")
            if lo > self.d_lo:
                be.halation(E, e_lo, self.D, self.d_lo, self.d_lo, lo, H, **kw)
            if hi < self.d_hi:
                be.halation(E, e_lo, self.D, self.d_lo, hi, self.d_hi, H, **kw)
        elif self.single_exchange:  # density for the rows the MTF stencil reads, halo rows included
            be.halation(E, e_lo, self.D, self.d_lo, self.d_lo, self.d_hi, H, **kw)
        else:
            be.halation(E, e_lo, self.D, self.d_lo, p.r0, p.r1, H, **kw)

    def _finish(self, out_f32, out_u8, field_ready):
        """S5 .. S8 from the density planes (their halo rows in place)."""
        p, be = self.plan, self.backend
        H = p.H
        if not (self.halation or self.mtf):
            cur, cur_lo = self.Dplain, p.r0
        else:
            cur, cur_lo = self.D, self.d_lo
            if self.mtf:
                be.mtf(self.D, self.d_lo, self.D2, p.r0, p.r0, p.r1, H)
                cur, cur_lo = self.D2, p.r0
        if not self.burn:
            if field_ready is not None:
                self.torch.cuda.current_stream().wait_event(field_ready)
                be.tail_field(cur, cur_lo, self.F, p.r0, out_f32, out_u8, p.r0, p.r0, p.r1, H)
            else:
                be.tail(cur, cur_lo, out_f32, out_u8, p.r0, p.r0, p.r1, H)
            return out_f32, out_u8
        # S7: the highlight map is a function of the whole grained frame -> grain to planes, every rank reduces the
        # cells its rows touch, one tiny all-reduce adds the partial sums, every rank blurs the (replicated) map.
        if self.grain:
            be.grain(cur, cur_lo, self.G, p.r0, p.r0, p.r1, H)
            cur, cur_lo = self.G, p.r0
        sums = be.burn_sums(cur, cur_lo, p.r0, p.r1, H)
        if p.world > 1:
            self.dist.all_reduce(sums, op=self.dist.ReduceOp.SUM, group=self.group)
        be.tail(cur, cur_lo, out_f32, out_u8, p.r0, p.r0, p.r1, H, burn_map=be.burn_map(sums, p.W, H))
        return out_f32, out_u8


class BatchSharder:
    """Frame-per-GPU batch export without collectives.

    tasks[i] is handled by rank i % world.  `prepare(task)` is the host phase (decode / load,
    `HipProcessor.extract_image_data_cpu`), `execute(task, payload)` the device phase
    (`HipProcessor.process_preloaded` + export).  One producer thread keeps the host phase one
    frame ahead of the device phase through a `Queue(maxsize=1)`; a frame whose host phase raises
    is skipped and the batch continues (gui_objects.py:86-87,101-103); `cancel()` stops both sides.
    """

    def __init__(self, rank: int = 0, world: int = 1):
        self.rank, self.world = rank, world
        self._cancel = threading.Event()

    def my_tasks(self, tasks):
        return [(i, t) for i, t in enumerate(tasks) if i % self.world == self.rank]

    def cancel(self):
        self._cancel.set()

    def run(self, tasks, prepare, execute, progress=None, collect=None):
        """collect: when given, `execute` only SUBMITS a frame (`HipProcessor.submit_preloaded`) and returns a handle; the
        handle of frame k is collected (`collect(task, handle)`, e.g. `handle.result()` + export) after frame k + 1 has been
        submitted, so uploads, renders and downloads of consecutive frames overlap on the GPU's copy and compute streams."""
        mine = self.my_tasks(tasks)
        q: queue.Queue = queue.Queue(maxsize=1)
        results, skipped = {}, []

        stop = threading.Event()  # this run is over (consumer gone); `self._cancel` is the caller's request

        def halted():
            return self._cancel.is_set() or stop.is_set()

        def put(item) -> bool:
            # never block forever on the depth-1 queue: give up as soon as the consumer has gone away
            while not halted():
                try:
                    q.put(item, timeout=0.1)
                    return True
                except queue.Full:
                    continue
            return False

        def producer():
            for idx, task in mine:
                if halted():
                    break
                try:
                    payload = prepare(task)
                except Exception:  # noqa: BLE001 -- same "skip the frame" rule as upstream
                    payload = None
                if not put((idx, task, payload)):
                    break
            put((None, None, None))

        th = threading.Thread(target=producer, daemon=True)
        th.start()
        in_flight = None  # (index, task, handle) of the frame submitted but not yet collected

        def finish(frame):
            """Collect a submitted frame (download + export), then report it: progress counts FINISHED frames."""
            results[frame[0]] = collect(frame[1], frame[2])
            if progress is not None:
                progress(frame[0], len(mine))

        try:
            while not self._cancel.is_set():
                try:
                    idx, task, payload = q.get(timeout=0.1)
                except queue.Empty:
                    if not th.is_alive() and q.empty():
                        break
                    continue
                if idx is None:
                    break
                if payload is None:
                    skipped.append(idx)
                    continue
                if collect is None:
                    results[idx] = execute(task, payload)
                    if progress is not None:
                        progress(idx, len(mine))
                else:
                    handle = execute(task, payload)
                    previous, in_flight = in_flight, (idx, task, handle)
                    if previous is not None:
                        finish(previous)
            if in_flight is not None:
                previous, in_flight = in_flight, None
                finish(previous)
        except BaseException:
            # execute / collect raised with a frame still in flight: it did render -- try to keep its result, else list it as
            # skipped, then let the error through
            if collect is not None and in_flight is not None:
                try:
                    finish(in_flight)
                except Exception:  # noqa: BLE001
                    skipped.append(in_flight[0])
            raise
        finally:
            # whatever ended the loop (cancel, the sentinel, an exception out of execute): stop the producer and drop what
            # it still holds, so it neither decodes the rest of the batch nor sits on a ~400 MB payload
            stop.set()
            while True:
                try:
                    q.get_nowait()
                except queue.Empty:
                    break
            th.join(timeout=5.0)
        return results, skipped
