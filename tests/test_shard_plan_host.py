"""The integer side of the row-sharded renderer on its own (raw2film_amd/shard_plan.py: geometry, candidate schedules, tuner) and
the renderer's graph bookkeeping (sharding.GraphCache; the capture fallbacks under tools/shard_walk_digest.py's fake capture)."""

import itertools
import os
import sys

import pytest

from raw2film_amd.shard_plan import ScheduleTuner, ShardPlan, plan_shard, schedule_of, shard_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (halation reach, MTF reach, per halation plane): odd and even reaches, a per-plane list with a zero plane, a stencil without reach
REACHES = (((5, 5), (2, 2), [(5, 5), (5, 5), (0, 0)]), ((7, 4), (3, 1), None), ((0, 0), (2, 2), None), ((6, 6), (0, 0), [(6, 6), (0, 0), (6, 5)]))
BANDS = (0, 3, 1000)  # unknown, small, larger than any shard here
REQUESTS = (("auto", "auto"), (1, False), (1, True), (2, False))


def _old_constructor(H, W, rank, world, halation, mtf, reach, band, exchanges, split_halation):
    """The arithmetic of RowShardedRenderer.__init__ as it stood before shard_plan.py, transcribed line by line."""
    halation_taps, mtf_taps, per_channel = reach
    r0, r1 = shard_rows(H, world)[rank]
    ha, hb = halation_taps if halation else (0, 0)
    ma, mb = mtf_taps if mtf else (0, 0)
    both = halation and mtf
    ea, eb = (ha + ma, hb + mb) if both else (ha, hb)
    per = per_channel if halation else None
    if per:
        halo_e_single = [((a + ma, b + mb) if both else (a, b)) for a, b in per]
        halo_e_two = [(a, b) for a, b in per]
    else:
        halo_e_single = [(ea, eb)] * 3
        halo_e_two = [(ha, hb)] * 3
    smallest = min(b - a for a, b in shard_rows(H, world))
    need = max(ea, eb, ma, mb)
    if world > 1 and smallest < need:
        raise ValueError(
            f"row shards of {smallest} rows are shorter than the {need}-row stencil halo; use fewer ranks for this frame"
        )
    e_lo, e_hi = max(r0 - ea, 0), min(r1 + eb, H)
    d_lo, d_hi = max(r0 - ma, 0), min(r1 + mb, H)
    split_plan = None
    if halation and both and world > 1:
        need_t, need_b = (ha + ma, hb + mb)
        top = max(need_t, band) if rank > 0 else 0
        bot = max(need_b, band) if rank < world - 1 else 0
        lo, hi = d_lo + top, d_hi - bot
        if hi - lo >= max(need_t, need_b, 1):
            split_plan = (lo, hi)
    saves_row = False
    if both and world > 1:
        base = H // world
        vy = band
        if vy > 0:
            saves_row = -(-base // vy) < -(-(base + ma + mb) // vy)
    cands = []
    if both and world > 1:
        ex_opts = [1, 2] if exchanges == "auto" else [int(exchanges)]
        if exchanges == "auto" and not saves_row:
            ex_opts = [1]
        for ex in ex_opts:
            if ex == 1:
                cands += [(1, sp) for sp in ([False, True] if split_halation == "auto" else [bool(split_halation)])]
            else:
                cands.append((2, False))
    return dict(plan=(H, W, rank, world, r0, r1, (ea, eb), (ma, mb)), extents=(e_lo, e_hi, d_lo, d_hi), single=halo_e_single,
                two=halo_e_two, split=split_plan, cands=cands, both=both)


def _old_set_schedule(old, sched):
    ex, sp = sched
    single_exchange = old["both"] and ex == 1
    halo_e_ch = old["single"] if (single_exchange or not old["both"]) else old["two"]
    split = old["split"] if (single_exchange and sp) else None
    return (single_exchange, halo_e_ch, split, (ex, bool(split)))


def _heights(world, reach):
    """From one row short of the smallest frame whose shards hold the widest halo up to a few hundred rows."""
    (ha, hb), (ma, mb), _ = reach
    fits = max(ha + ma, hb + mb, 1) * world
    return sorted({fits - 1, fits, fits + 1, fits + world - 1, 2 * fits + 3, 97, 160, 301})


def _layouts():
    for world, reach, band in itertools.product(range(1, 9), REACHES, BANDS):
        for H, (halation, mtf) in itertools.product(_heights(world, reach), itertools.product((True, False), repeat=2)):
            yield world, reach, band, H, halation, mtf


def test_plan_shard_is_the_old_constructors_arithmetic():
    W, checked, rejected = 24, 0, 0
    for world, reach, band, H, halation, mtf in _layouts():
        for rank, (ex, sp) in itertools.product(range(world), REQUESTS):
            kw = dict(halation=halation, mtf=mtf, halation_taps=reach[0], mtf_taps=reach[1], halation_taps_per_channel=reach[2],
                      band_rows=lambda W, rows: band, exchanges=ex, split_halation=sp)
            try:
                old = _old_constructor(H, W, rank, world, halation, mtf, reach, band, ex, sp)
            except ValueError as e:
                with pytest.raises(ValueError) as got:
                    plan_shard(H, W, rank, world, **kw)
                assert str(got.value) == str(e)
                rejected += 1
                continue
            lay = plan_shard(H, W, rank, world, **kw)
            p = lay.plan
            case = (world, reach, band, H, halation, mtf, rank, ex, sp)
            assert isinstance(p, ShardPlan) and p.rows == p.r1 - p.r0
            assert (p.H, p.W, p.rank, p.world, p.r0, p.r1, p.halo_e, p.halo_d) == old["plan"], case
            assert (lay.e_lo, lay.e_hi, lay.d_lo, lay.d_hi) == old["extents"], case
            assert (lay.halo_e_single, lay.halo_e_two, lay.split_plan, lay.candidates) == (old["single"], old["two"], old["split"], old["cands"]), case
            for sched in old["cands"]:
                assert tuple(schedule_of(lay, sched)) == _old_set_schedule(old, sched), (case, sched)
            # no candidates: the constructor's initial state -- the single-exchange layout, nothing split, nothing reported
            assert tuple(schedule_of(lay, None)) == (old["both"], old["single"], None, None), case
            checked += 1
    assert checked > 20000 and rejected > 500, (checked, rejected)


def test_shards_tile_the_frame_and_every_derived_row_range_stays_inside_it():
    for world, reach, band, H, halation, mtf in _layouts():
        parts = shard_rows(H, world)
        assert parts[0][0] == 0 and parts[-1][1] == H and all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
        sizes = [b - a for a, b in parts]
        assert max(sizes) - min(sizes) <= 1 and (min(sizes) >= 0)
        kw = dict(halation=halation, mtf=mtf, halation_taps=reach[0], mtf_taps=reach[1], halation_taps_per_channel=reach[2],
                  band_rows=lambda W, rows: band)
        try:
            lays = [plan_shard(H, 24, rank, world, **kw) for rank in range(world)]
        except ValueError:
            continue
        (ha, hb), (ma, mb) = (reach[0] if halation else (0, 0)), (reach[1] if mtf else (0, 0))
        for rank, lay in enumerate(lays):
            p = lay.plan
            assert (p.r0, p.r1) == parts[rank]
            assert 0 <= lay.e_lo <= p.r0 <= p.r1 <= lay.e_hi <= H and 0 <= lay.d_lo <= p.r0 <= p.r1 <= lay.d_hi <= H
            assert lay.candidates == lays[0].candidates  # the ranks walk the list in lockstep: the same on every rank of a world
            if lay.split_plan is not None:
                lo, hi = lay.split_plan
                assert lay.d_lo <= lo < hi <= lay.d_hi
                assert hi - lo >= max(ha + ma, hb + mb, 1)  # at least max(need_t, need_b, 1) interior rows
                assert (lo == lay.d_lo) if rank == 0 else (lo - lay.d_lo == max(ha + ma, band))  # rank 0 has no top band ...
                assert (hi == lay.d_hi) if rank == world - 1 else (lay.d_hi - hi == max(hb + mb, band))  # ... the last rank no bottom band
            if world == 1 or not (halation and mtf):
                assert lay.candidates == [] and lay.split_plan is None


class _Clock:
    """A scripted clock: the time of the k-th timed frame of each candidate."""

    def __init__(self, times):
        self.times, self.asked = times, []

    def __call__(self, cand):
        self.asked.append(cand)
        return self.times[cand][self.asked.count(cand) - 1]


def _run_tuner(t, clock):
    """Drive a tuner the way the renderer does; (frames rendered, the candidate each ran under)."""
    ran = []
    while t.measuring:
        cand = t.current
        ran.append(cand)
        if t.frame_done(clock(cand) if t.next_is_timed else None) and t.current is None:
            break
    return ran


@pytest.mark.parametrize("tune_frames", [1, 2, 3])
def test_the_tuner_walks_every_candidate_behind_an_untimed_frame_and_takes_the_agreed_argmin(tune_frames):
    cands = [(1, False), (1, True), (2, False)]
    clock = _Clock({(1, False): [5.0, 4.0, 6.0], (1, True): [3.5, 3.0, 9.0], (2, False): [7.0, 2.0, 2.5]})
    t = ScheduleTuner(cands, tune_frames)
    assert t.measuring and t.current == (1, False) and not t.next_is_timed
    ran = _run_tuner(t, clock)
    assert len(ran) == (1 + tune_frames) * len(cands)
    assert ran == [c for c in cands for _ in range(1 + tune_frames)]
    assert clock.asked == [c for c in cands for _ in range(tune_frames)]  # the untimed frames are not counted
    best = t.best()
    assert best == [min(clock.times[c][:tune_frames]) for c in cands]
    # the choice is made from the times the ranks AGREED on, not from this rank's own
    agreed = [max(b, other) for b, other in zip(best, [1.0, 8.0, 1.0])]
    chosen, tuned = t.choose(agreed)
    assert tuned == agreed and chosen == cands[agreed.index(min(agreed))] and not t.measuring
    assert ScheduleTuner(cands, 1).choose([2.0, 2.0, 3.0])[0] == (1, False)  # the first of equals


def test_a_tuner_with_nothing_to_measure_runs_the_first_candidate():
    cands = [(1, False), (1, True)]
    for t in (ScheduleTuner(cands, 0), ScheduleTuner(cands, 2, can_measure=False), ScheduleTuner(cands[:1], 2)):
        assert not t.measuring and t.current == (1, False)
    t = ScheduleTuner([], 2)
    assert not t.measuring and t.current is None
    with pytest.raises(ValueError, match="tune_frames must be >= 0"):
        ScheduleTuner(cands, -1)


def test_the_graph_cache_counts_keys_follows_the_state_and_stays_bounded():
    from raw2film_amd.sharding import GraphCache

    c = GraphCache()
    slot = c.slot("a", 1)
    assert slot == [1, None] and c.counts() == [None]  # a first sighting runs eagerly ...
    c.after_eager("a", slot, 1)
    slot2 = c.slot("a", 1)
    assert slot2 is slot and slot[0] == 2 and slot[1] is None  # ... the second captures
    slot[1] = {3: "g", 5: "h"}
    assert c.slot("a", 1)[1] == {3: "g", 5: "h"} and c.counts() == [2]
    c.slot("b", 1)
    assert c.counts() == [2, None]
    c.slot("a", 1)
    assert c.counts() == [None, 2]  # least recently used first
    # a moved state drops everything: the frame at hand is a first frame again
    assert c.slot("a", 2) == [1, None] and c.counts() == [None]
    # a state moved BY the eager frame drops the other keys and keeps this key's counter
    c = GraphCache()
    for key in ("a", "b"):
        s = c.slot(key, 1)
        c.after_eager(key, s, 1)
        c.slot(key, 1)[1] = {0: "g"}
    s = c.slot("c", 1)
    c.after_eager("c", s, 2)
    assert c.counts() == [None] and c.state == 2
    assert c.slot("c", 2) is s and s[0] == 2
    assert c.slot("a", 2) == [1, None]
    # fresh keys every frame: neither graphs nor counters pile up
    for k in range(20):
        c.slot(("fresh", k), 2)
    assert len(c.counts()) == GraphCache.LIMIT == 8
    c.drop()
    assert c.counts() == [] and c.state == 2


def _digest_tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import shard_walk_digest as swd
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    return swd


def _frames(log):
    """The stage calls and exchanges of each frame in issue order: a replay counts as the calls its graph holds, what else the
    fakes log (`captured`, `synchronize`) is left out."""
    frames = []
    for item in log:
        if item[0] == "frame":
            frames.append([])
        elif item[0] == "replay":
            frames[-1] += item[1]
        elif item[0] not in ("captured", "synchronize"):
            frames[-1].append(item)
    return frames


class _Context:
    gen = 0

    def generation(self):
        return self.gen


@pytest.mark.parametrize("world,rank,sched", [(1, 0, ("auto", "auto")), (2, 0, (1, True)), (3, 1, (1, True)), (3, 1, (2, False))])
def test_a_capture_that_fails_or_moves_the_context_ends_in_the_eager_rest_of_that_frame(world, rank, sched):
    pytest.importorskip("torch")
    from raw2film_amd import sharding

    swd = _digest_tool()
    H = {1: 64, 2: 64, 3: 97}[world]

    def case():
        rr, be, frame = swd.build(sharding, H, world, rank, swd.REACHES[0], 6, (True, True, True, False), sched, tune_frames=0)
        be.ctx, be.params = _Context(), b"params"
        rr.graph = True
        return rr, be, frame

    def render(be, rr, frame, n, on_capture=None):
        with swd.fake_graphs(lambda: be.log, on_capture):
            for _ in range(n):
                be.log.append(("frame",))
                frame()

    # a capture that raises: the frame ends eagerly -- every call of an eager frame, once -- and the renderer stays eager
    rr, be, frame = case()

    def fail():
        raise RuntimeError("capture failed")

    render(be, rr, frame, 1)
    assert rr.graph_slots() == [None]
    render(be, rr, frame, 2, fail)
    frames = _frames(be.log)
    assert frames[1] == frames[0] and frames[2] == frames[0] and len(frames[0]) >= 4
    assert rr.graph is False and rr.graph_slots() == []
    assert ("synchronize",) in be.log and not any(x[0] in ("captured", "replay") for x in be.log)

    # a capture during which the context moved (a table built lazily): that frame runs eagerly again, the graphs come later
    rr, be, frame = case()
    moved = []

    def move_once():
        if not moved:
            moved.append(True)
            be.ctx.gen += 1

    render(be, rr, frame, 2, move_once)
    assert rr.graph is True and rr.graph_slots() == []
    render(be, rr, frame, 1)  # (a first frame again: eager)
    assert rr.graph_slots() == [None]
    render(be, rr, frame, 2)  # capture + replay, replay
    assert rr.graph_slots() == [1 if world == 1 else 2]
    assert len([x for x in be.log if x[0] == "replay"]) == 2 * rr.graph_slots()[0]
    # every frame -- eager, captured and abandoned, eager again, captured and replayed, replayed -- issues an eager frame's calls in
    # an eager frame's order: what the graphs hold is what the steps between the host steps launch
    frames = _frames(be.log)
    assert len(frames) == 5 and all(f == frames[0] for f in frames)
