"""What does RowShardedRenderer ASK of its backend, its transport and its graphs -- call by call, frame by frame, over a matrix of
worlds, ranks, stencil reaches, band heights, stage gates and schedules?  No GPU: a recording backend logs every stage call (tensors
as (buffer name, shape, storage offset)), a subclass logs every `_exchange`, and torch.cuda's graph capture is replaced by a fake
that runs the body, keeps the calls it logged and logs them again on `replay()`.  Every case's log, trace and derived geometry are
hashed; one line per group of cases is printed.  Two trees whose output is the same issue the same calls in the same order:

    python tools/shard_walk_digest.py > new.txt
    python tools/shard_walk_digest.py --package ../parent-checkout > parent.txt && diff parent.txt new.txt
    python tools/shard_walk_digest.py --case w3.reach0.band6.g1110/s1T.rank1.graph      # one case's full log, to diff a differing group

tests/golden/shard_walk_digest.txt is the record tests/test_shard_walk_host.py holds the working tree against.
"""
import argparse
import contextlib
import functools
import hashlib
import importlib
import itertools
import os
import sys

import torch

W = 8
WORLDS = ((64, 1), (64, 2), (97, 3), (160, 4), (400, 8))  # (H, world)
# (halation reach, MTF reach, the halation's reach per plane)
REACHES = (((5, 5), (2, 2), [(5, 5), (5, 5), (0, 0)]), ((7, 4), (3, 1), None), ((0, 0), (2, 2), None))
BANDS = (0, 6, 20)
SCHEDULES = (("auto", "auto"), (1, False), (1, True), (2, False))  # (exchanges, split_halation) as requested
CLOCKS = ({(1, False): 5.0, (1, True): 3.0, (2, False): 4.0}, {(1, False): 2.0, (1, True): 3.0, (2, False): 2.0})


class Recorder:
    """A stage backend that computes nothing: every stage call goes to `log`.  No device, no context, no begin_frame, no grain_field."""

    tracks_range = True
    STAGES = ("front", "exposure_range", "halation", "mtf", "tail", "tail_field", "grain", "front_to_output")

    def __init__(self, reach, band):
        self.halation_taps, self.mtf_taps, self.halation_taps_per_channel = reach
        self.band = band
        self.log, self.names, self.count = [], {}, 0
        self.sums, self.map = self.name(torch.zeros(2, 3), "sums"), self.name(torch.zeros(2, 3), "map")

    def name(self, t, name):
        self.names[t.untyped_storage().data_ptr()] = name
        return t

    def enc(self, x):
        if type(x) in (int, bool, type(None), str):
            return x
        if isinstance(x, torch.Tensor):
            return (self.names.get(x.untyped_storage().data_ptr(), "?"), tuple(x.shape), x.storage_offset())
        if isinstance(x, (list, tuple)):
            return tuple(map(self.enc, x))
        return x

    def halation_band_rows(self, W, rows):
        return self.band

    def empty(self, rows, W):
        self.count += 1
        return self.name(torch.zeros((3, rows, W)), f"plane{self.count}")

    def call(self, stage, args, kwargs):
        self.log.append((stage, self.enc(args), tuple(sorted((k, self.enc(v)) for k, v in kwargs.items()))))

    def __getattr__(self, stage):
        if stage not in self.STAGES:
            raise AttributeError(stage)
        return lambda *args, **kwargs: self.call(stage, args, kwargs)

    def front_split(self, *args, **kwargs):
        self.call("front_split", args, kwargs)
        return 4

    def burn_sums(self, *args, **kwargs):
        self.call("burn_sums", args, kwargs)
        return self.sums

    def burn_map(self, *args, **kwargs):
        self.call("burn_map", args, kwargs)
        return self.map


class FakeDist:
    """Stands in for torch.distributed on a renderer: the burn stage's all-reduce is logged, there is no group to agree with."""

    class ReduceOp:
        SUM, MAX = "SUM", "MAX"

    def __init__(self, backend):
        self.backend = backend

    def is_available(self):
        return False

    def is_initialized(self):
        return False

    def all_reduce(self, t, op=None, group=None):
        self.backend.log.append(("all_reduce", self.backend.enc(t), op))


@contextlib.contextmanager
def fake_graphs(log_of, on_capture=None):
    """torch.cuda.CUDAGraph / graph / synchronize replaced for the duration: a capture runs its body, moves the calls the body logged
    (log_of() -> the list in use) into the graph object and logs `captured`; replay() logs `replay` with those calls.
    on_capture(), when given, runs at the end of every capture's body (tests make it raise, or move the backend's state); the
    calls of a capture that raises are dropped."""

    class Graph:
        calls = ()

        def replay(self):
            log_of().append(("replay", self.calls))

    @contextlib.contextmanager
    def graph(g, **kwargs):
        mark = len(log_of())
        try:
            yield
            if on_capture is not None:
                on_capture()
        except BaseException:  # a capture that fails launches nothing
            del log_of()[mark:]
            raise
        log = log_of()
        g.calls = tuple(log[mark:])
        del log[mark:]
        log.append(("captured", len(g.calls)))

    saved = torch.cuda.CUDAGraph, torch.cuda.graph, torch.cuda.synchronize
    torch.cuda.CUDAGraph, torch.cuda.graph, torch.cuda.synchronize = Graph, graph, lambda *a: log_of().append(("synchronize",))
    try:
        yield
    finally:
        torch.cuda.CUDAGraph, torch.cuda.graph, torch.cuda.synchronize = saved


@functools.lru_cache(maxsize=None)
def logged_renderer(sharding):
    class Logged(sharding.RowShardedRenderer):
        def _exchange(self, buf, buf_gy0, above, below, wait=True):
            be = self.backend
            be.log.append(("_exchange", be.enc(buf), buf_gy0, be.enc(above), be.enc(below), wait))
            return None

    return Logged


def build(sharding, H, world, rank, reach, band, gates, sched, **kw):
    """(renderer, backend, render one frame) of one case; the constructor's ValueError goes through."""
    be = Recorder(reach, band)
    halation, mtf, grain, burn = gates
    rr = logged_renderer(sharding)(be, H, W, halation=halation, mtf=mtf, grain=grain, burn=burn, rank=rank, world=world,
                                   exchanges=sched[0], split_halation=sched[1], **kw)
    rr.dist = FakeDist(be)
    rr.trace = []
    image = be.name(torch.zeros((rr.plan.rows, W, 3)), "image")
    out = be.name(torch.zeros((rr.plan.rows, W, 3)), "out")
    return rr, be, lambda: rr.render(image, out_f32=out)


def geometry(rr):
    return (rr.schedule, list(rr._candidates), rr.split, list(rr.halo_e_ch), rr.e_lo, rr.e_hi, rr.d_lo, rr.d_hi)


_LOG = [None]  # the log of the case at hand, for the fake graphs


def run_case(sharding, H, world, rank, reach, band, gates, sched, graph):
    """The record of one case: 4 frames with the graph path on where a device would allow it (eager, capture, two replays), or
    2 eager frames."""
    try:
        rr, be, frame = build(sharding, H, world, rank, reach, band, gates, sched, tune_frames=0)
    except ValueError as e:
        return ("ValueError", str(e))
    halation, mtf, grain, burn = gates
    rr.graph = bool(graph and (halation or mtf or grain) and not burn)
    _LOG[0] = be.log
    for k in range(4 if graph else 2):
        be.log.append(("frame", k))
        rr.trace.append(("frame", k))
        frame()
    slots = rr.graph_slots() if hasattr(rr, "graph_slots") else [None if v[1] is None else sum(g is not None for g in v[1].values())
                                                                 for v in rr._graphs.values()]
    return (be.log, rr.trace, geometry(rr), rr.graph, slots)


def run_tuning(sharding, H, world, rank, reach, band, clock):
    """The measuring phase under an injected clock: the schedule after every frame, the times and the choice at the end."""
    try:
        rr, be, frame = build(sharding, H, world, rank, reach, band, (True, True, True, False), ("auto", "auto"), tune_frames=2,
                              frame_timer=lambda cand, render: (render(), clock[cand])[1])
    except ValueError as e:
        return ("ValueError", str(e))
    walked = []
    while rr.tuning and len(walked) < 50:
        frame()
        walked.append(rr.schedule)
    frame()
    return (be.log, rr.trace, geometry(rr), walked, rr.tuned_ms, rr.tuning)


def cases(sharding):
    """(group, case name, thunk) of the whole matrix, in a fixed order."""
    for (H, world), (ri, reach), band, gates in itertools.product(WORLDS, enumerate(REACHES), BANDS, itertools.product((True, False), repeat=4)):
        group = f"w{world}.reach{ri}.band{band}.g{''.join(str(int(g)) for g in gates)}"
        for sched, rank, graph in itertools.product(SCHEDULES, range(world), (True, False)):
            name = f"s{str(sched[0])[0]}{str(sched[1])[0]}.rank{rank}.{'graph' if graph else 'eager'}"
            yield group, name, (lambda a=(sharding, H, world, rank, reach, band, gates, sched, graph): run_case(*a))
    for (H, world), (ri, reach), band in itertools.product(WORLDS[1:], enumerate(REACHES[:2]), BANDS[1:]):
        group = f"w{world}.reach{ri}.band{band}.tuning"
        for ci, rank in itertools.product(range(len(CLOCKS)), sorted({0, world // 2, world - 1})):
            yield group, f"clock{ci}.rank{rank}", (lambda a=(sharding, H, world, rank, reach, band, CLOCKS[ci]): run_tuning(*a))


def digest_lines(sharding):
    """One line per group: its name, the number of cases and distinct records in it and the hash over its cases' records."""
    groups = {}
    with fake_graphs(lambda: _LOG[0]):
        for group, name, thunk in cases(sharding):
            groups.setdefault(group, []).append(repr((name, thunk())))
    lines = [f"{g} cases={len(r)} distinct={len(set(x.split(',', 1)[1] for x in r))} {hashlib.sha256(''.join(r).encode()).hexdigest()[:24]}"
             for g, r in groups.items()]
    return lines + [f"total groups={len(groups)} cases={sum(len(r) for r in groups.values())}"]


def load_sharding(package_dir=None):
    """raw2film_amd.sharding of the tree at `package_dir` (default: the tree this file is in)."""
    root = os.path.abspath(package_dir or os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    if not os.path.isdir(os.path.join(root, "raw2film_amd")):
        raise SystemExit(f"no raw2film_amd package under {root}")
    sys.path.insert(0, root)
    return importlib.import_module("raw2film_amd.sharding")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--package", metavar="DIR", help="the tree to import raw2film_amd from (default: this one)")
    ap.add_argument("--case", metavar="GROUP/NAME", help="print this case's full record instead of the digest")
    args = ap.parse_args()
    sharding = load_sharding(args.package)
    if not args.case:
        print("\n".join(digest_lines(sharding)))
        return
    for group, name, thunk in cases(sharding):
        if f"{group}/{name}" == args.case:
            with fake_graphs(lambda: _LOG[0]):
                record = thunk()
            for part in record:
                for item in (part if isinstance(part, list) else [part]):
                    print(item)
            return
    raise SystemExit(f"no case {args.case}")


if __name__ == "__main__":
    main()
