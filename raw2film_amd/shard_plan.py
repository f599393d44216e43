"""The integer side of the row-sharded renderer (sharding.py): which rows a rank owns, how wide its planes are, which schedules it
may run and how the first frames choose between them.  Pure Python -- no torch, no ctypes -- so every number here can be checked
without a backend or a tensor (tests/test_shard_plan_host.py).

With both stencils on there are two ways to feed the MTF's halo rows:
  ONE exchange: the exposure halo is widened by the MTF reach and every rank also computes the halation for the density
    rows its own MTF stencil will read (2 x 17 rows of redundant halation per shard at 100 MP) -- the same bytes on the
    wire as two exchanges, one latency instead of two;
  TWO exchanges: exposure halo for the halation only, the halation covers exactly the own rows, then r_m rows of DENSITY
    travel.  A second latency -- but the halation's FFT form works in window rows (172 rows at 100 MP), and a 1/8 shard's
    1 024 own rows are 5.95 of them where 1 058 rows are 6.15, i.e. seven: one window row in seven saved.
Buffers are laid out for the wider (single-exchange) halo; which schedule runs is decided from the candidate list (`exchanges`).
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple


def shard_rows(H: int, world: int) -> list[tuple[int, int]]:
    """Contiguous row ranges [(r0, r1)] per rank, sizes differing by at most one row."""
    base, extra = divmod(H, world)
    out, r = [], 0
    for k in range(world):
        n = base + (1 if k < extra else 0)
        out.append((r, r + n))
        r += n
    return out


@dataclass
class ShardPlan:
    H: int
    W: int
    rank: int
    world: int
    r0: int
    r1: int
    halo_e: tuple[int, int]  # (above, below) exposure halo rows needed by the halation stencil
    halo_d: tuple[int, int]  # (above, below) density halo rows needed by the MTF stencil

    @property
    def rows(self) -> int:
        return self.r1 - self.r0


@dataclass(frozen=True)
class ShardLayout:
    """What `plan_shard` derives for one rank: everything the renderer's constructor used to work out inline."""
    plan: ShardPlan
    both: bool  # halation and MTF are both on: the only case with more than one schedule
    e_lo: int  # extended planes: own rows plus the halo rows that exist inside the frame -- exposure [e_lo, e_hi) ...
    e_hi: int
    d_lo: int  # ... and density [d_lo, d_hi)
    d_hi: int
    halo_e_single: list  # per plane (above, below): the exposure halo under one exchange ...
    halo_e_two: list  # ... and under two
    split_plan: tuple | None  # (lo, hi): the halation's interior rows, where the shard has room for the split
    candidates: list  # [(exchanges, split)], the same on every rank of the world


class Schedule(NamedTuple):
    """What the renderer runs under one candidate (`schedule_of`)."""
    single_exchange: bool
    halo_e_ch: list
    split: tuple | None
    schedule: tuple | None  # (exchanges, split in effect on this rank) as reported; None where there was nothing to choose


def _exposure_halos(per, both, ha, hb, ma, mb):
    """Per plane: a channel whose halation stencil is a single tap (blue on a colour stock) needs exposure halo rows only for
    the MTF reach, not for the halation's -- 17 instead of 59 rows at 100 MP, 6.7 instead of 8.7 MB per direction."""
    if per:
        return [((a + ma, b + mb) if both else (a, b)) for a, b in per], [(a, b) for a, b in per]
    ea, eb = (ha + ma, hb + mb) if both else (ha, hb)
    return [(ea, eb)] * 3, [(ha, hb)] * 3


def _split_plan(rank, world, d_lo, d_hi, need_t, need_b, band):
    """The halation in three calls: the interior rows -- whose stencil reads own exposure rows only -- are launched BEFORE the
    halo exchange is waited for (they run while the halos travel), a band at each inner boundary after it.  A band is one
    window row of the FFT form high (172 rows at 100 MP) where that is known, so the three calls together cover the same
    number of window rows as one call would.
    Worth it only where the exchange would otherwise be exposed: three calls cost ~0.05 ms more device time than one (the
    bands are small launches: measured on one GPU, tools/shard_model.py) and the interior front kernel already covers
    part of the transfer -- so this is one of the candidate schedules the first frames MEASURE (`_candidates`);
    split_halation = True / False fixes it either way."""
    top = max(need_t, band) if rank > 0 else 0
    bot = max(need_b, band) if rank < world - 1 else 0
    lo, hi = d_lo + top, d_hi - bot
    return (lo, hi) if hi - lo >= max(need_t, need_b, 1) else None


def _candidates(H, W, world, ma, mb, band_rows, exchanges, split_halation):
    """The schedules a rank can run: (exchanges, split).  Which one is fastest depends on what nobody can know ahead of the first
    frames -- how long the exchange takes on this node's links and how much of it the interior front kernel already covers
    (round 4 decided from a MODELLED 30 us + bytes / 55 GB/s) -- so "auto" MEASURES: after the first
    frame (which builds tables) every candidate renders `tune_frames` frames between two events on the launch stream, the
    ranks agree on the schedule whose slowest rank is fastest (one all-reduce of a few floats; the two-exchange form needs
    both neighbours to send density rows, so the choice must be the same everywhere), and graphs are captured for that one.
    Every candidate renders the frame correctly (results agree to the FFT form's rounding noise), so tuning costs no frame.
    Two exchanges are a candidate only where they save a halation window row on this rank's shard.
    (the candidate list must be the same on every rank -- they walk it in lockstep and reduce one time per candidate -- so it
    is derived from the geometry of a MIDDLE rank's shard, not from this rank's own; a rank without room for the split runs
    that candidate unsplit)"""
    saves_row = False
    base = H // world
    vy = band_rows(W, base)
    if vy > 0:
        saves_row = -(-base // vy) < -(-(base + ma + mb) // vy)
    ex_opts = [1, 2] if exchanges == "auto" else [int(exchanges)]
    if exchanges == "auto" and not saves_row:
        ex_opts = [1]
    cands = []
    for ex in ex_opts:
        if ex == 1:
            cands += [(1, sp) for sp in ([False, True] if split_halation == "auto" else [bool(split_halation)])]
        else:
            cands.append((2, False))
    return cands


def plan_shard(H: int, W: int, rank: int, world: int, *, halation: bool, mtf: bool, halation_taps=(0, 0), mtf_taps=(0, 0),
               halation_taps_per_channel=None, band_rows=lambda W, rows: 0, exchanges="auto", split_halation="auto") -> ShardLayout:
    """The geometry of rank `rank` of `world` on an H x W frame.  halation_taps / mtf_taps: (rows above, rows below) the stencils
    reach; halation_taps_per_channel: the same per halation plane, or None; band_rows(W, rows) -> rows one window row of the
    halation's FFT form yields on a call of `rows` rows (0: unknown).  Raises ValueError where a shard is shorter than the halo."""
    r0, r1 = shard_rows(H, world)[rank]
    ha, hb = halation_taps if halation else (0, 0)
    ma, mb = mtf_taps if mtf else (0, 0)
    both = bool(halation and mtf)
    ea, eb = (ha + ma, hb + mb) if both else (ha, hb)
    plan = ShardPlan(H, W, rank, world, r0, r1, (ea, eb), (ma, mb))
    single, two = _exposure_halos(halation_taps_per_channel if halation else None, both, ha, hb, ma, mb)
    smallest = min(b - a for a, b in shard_rows(H, world))
    need = max(ea, eb, ma, mb)
    if world > 1 and smallest < need:
        raise ValueError(
            f"row shards of {smallest} rows are shorter than the {need}-row stencil halo; use fewer ranks for this frame"
        )
    e_lo, e_hi = max(r0 - ea, 0), min(r1 + eb, H)
    d_lo, d_hi = max(r0 - ma, 0), min(r1 + mb, H)
    split, cands = None, []
    if both and world > 1:
        split = _split_plan(rank, world, d_lo, d_hi, ha + ma, hb + mb, band_rows(W, d_hi - d_lo))
        cands = _candidates(H, W, world, ma, mb, band_rows, exchanges, split_halation)
    return ShardLayout(plan, both, e_lo, e_hi, d_lo, d_hi, single, two, split, cands)


def schedule_of(layout: ShardLayout, sched) -> Schedule:
    """sched = (exchanges, split): 1 exchange (exposure halo widened by the MTF reach) with the halation in one call or as
    interior + bands, or 2 exchanges (exposure halo for the halation, then density halo for the MTF).  None: the frame has no
    choice to make (one stencil at most, or one rank) -- the single-exchange layout, nothing reported."""
    if sched is None:
        return Schedule(layout.both, layout.halo_e_single, None, None)
    ex, sp = sched
    single = layout.both and ex == 1
    halo = layout.halo_e_single if (single or not layout.both) else layout.halo_e_two
    split = layout.split_plan if (single and sp) else None
    return Schedule(single, halo, split, (ex, bool(split)))


class ScheduleTuner:
    """The measuring phase of "auto": the candidates are walked in order, each renders one UNTIMED frame and then `tune_frames`
    timed ones, and the best frame of each counts.  The first frame of EVERY candidate is not timed: the very first builds tables,
    spectra and scratch, and a later candidate's first frame may still meet a window shape of its own (a spectrum upload, a larger
    scratch -- both synchronise), which would bias the choice towards candidate 0 whenever tune_frames is 1.
    The renderer asks `current` / `next_is_timed`, reports every frame with `frame_done`, and hands the times the ranks agreed on
    to `choose`.  measuring = False (one candidate, tune_frames = 0, nothing to time with): the first candidate runs."""

    def __init__(self, candidates, tune_frames: int, can_measure: bool = True):
        if int(tune_frames) < 0:
            raise ValueError("tune_frames must be >= 0 (0: no measuring, the first candidate runs)")
        self.candidates = list(candidates)
        self.tune_frames = int(tune_frames)
        self.measuring = len(self.candidates) > 1 and bool(can_measure) and self.tune_frames > 0
        self._i = 0  # the candidate being measured
        self._warm = False  # it has rendered its untimed frame
        self._ms = [[] for _ in self.candidates]

    @property
    def current(self):
        """The candidate the next frame renders under (None: no candidates, or every one has been measured)."""
        return self.candidates[self._i] if self._i < len(self.candidates) else None

    @property
    def next_is_timed(self) -> bool:
        return self._warm

    def frame_done(self, ms=None) -> bool:
        """A frame of the current candidate has been rendered (ms: its time, None for the untimed one).  True when that was the
        candidate's last frame: `current` has moved on -- to the next candidate, or to None when it is time to `choose`."""
        if not self._warm:
            self._warm = True
            return False
        self._ms[self._i].append(float(ms))
        if len(self._ms[self._i]) < self.tune_frames:
            return False
        self._i, self._warm = self._i + 1, False
        return True

    def best(self) -> list[float]:
        """This rank's best frame per candidate: what the ranks reduce (MAX) before `choose`."""
        return [min(m) for m in self._ms]

    def choose(self, agreed) -> tuple[tuple, list[float]]:
        """agreed: per candidate, the best time of the slowest rank.  Ends the measuring; (the fastest candidate -- the first of
        equals --, the times as `tuned_ms` reports them)."""
        tuned = [float(x) for x in agreed]
        self.measuring = False
        return self.candidates[min(range(len(tuned)), key=tuned.__getitem__)], tuned
