#!/usr/bin/env python3
"""tests/golden/prepath_pairs.json: a pairwise covering list over the axes of tests/prepath_cases.py -- every pair of values of
two different axes that the code does not refuse (prepath_cases.refusal) occurs together in at least one case.

    python tools/make_prepath_pairs.py [-o tests/golden/prepath_pairs.json]

A greedy search: each new case is the best of CANDIDATES tries, a try starts from a pair not covered yet and gives every other
axis, in a shuffled order, the value that covers the most uncovered pairs with the values chosen so far while the case stays
admissible.  A case with no active RAW-side option (prepath_cases.NEUTRAL) is never kept: every case has a sibling.  The list is
committed so that no test depends on this search, or on random.Random, behaving the same everywhere.

Each case records one sibling: itself with one active RAW-side option neutralised (median 4 -> 0, blend -> clip, denoise ->
none, orientation -> 0, adjusted levels -> numeric at the nominal scale), the option taken in turn over the case index among those
whose sibling is admissible, the least used one first among equals -- every option serves at least MIN_USES times."""

from __future__ import annotations

import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import prepath_cases as pc  # noqa: E402

CANDIDATES = 60
MIN_USES = 3


def options_of(case):
    """The options a sibling of this case may neutralise: active, and the sibling admissible."""
    return [name for name, (axis, active, neutral) in pc.NEUTRAL.items() if active(case) and pc.admissible({**case, axis: neutral})]


def _gain(case, uncovered):
    return sum(1 for p in pc.pairs_of(case) if p in uncovered)


def _candidate(rng, uncovered):
    (a, u), (b, v) = seed = rng.choice(sorted(uncovered, key=repr))
    case = {a: u, b: v}
    rest = [n for n in pc.AXES if n not in case]
    rng.shuffle(rest)
    for n in rest:
        best, best_gain = [], -1
        for value in pc.AXES[n]:
            if any(_pair(k, w, n, value) in _REFUSED for k, w in case.items()):  # (every rule of `refusal` is a pair's)
                continue
            gain = sum(1 for k, w in case.items() if _pair(k, w, n, value) in uncovered)
            if gain > best_gain:
                best, best_gain = [value], gain
            elif gain == best_gain:
                best.append(value)
        case[n] = rng.choice(best)
    case = {n: case[n] for n in pc.AXES}
    return case if pc.admissible(case) and options_of(case) and seed in pc.pairs_of(case) else None


_ORDER = {n: i for i, n in enumerate(pc.AXES)}
_REFUSED = pc.refused_pairs()


def _pair(a, u, b, v):
    return ((a, u), (b, v)) if _ORDER[a] < _ORDER[b] else ((b, v), (a, u))


def generate(seed=1):
    rng = random.Random(seed)
    uncovered = pc.all_pairs() - pc.refused_pairs()
    total, cases = len(uncovered), []
    while uncovered:
        tries = [c for c in (_candidate(rng, uncovered) for _ in range(CANDIDATES)) if c is not None]
        best = max(tries, key=lambda c: _gain(c, uncovered))
        cases.append(best)
        uncovered -= pc.pairs_of(best)
    return cases, total


def siblings(cases):
    uses = dict.fromkeys(pc.NEUTRAL, 0)
    names, out = list(pc.NEUTRAL), []
    for i, case in enumerate(cases):
        able = options_of(case)
        turn = names[i % len(names):] + names[:i % len(names)]  # (the choice rotates over the case index)
        option = min(able, key=lambda n: (uses[n], turn.index(n)))
        uses[option] += 1
        axis, _, neutral = pc.NEUTRAL[option]
        out.append({"option": option, "case": {**case, axis: neutral}})
    assert min(uses.values()) >= MIN_USES, uses
    return out, uses


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-o", "--output", default=pc.GOLDEN)
    ap.add_argument("--seeds", type=int, default=8, help="searches to run; the shortest list is kept")
    args = ap.parse_args()
    cases, total = min((generate(s) for s in range(1, args.seeds + 1)), key=lambda r: len(r[0]))
    assert len(cases) <= pc.CAP, len(cases)
    sibs, uses = siblings(cases)
    header = ("A pairwise covering list over the axes of tests/prepath_cases.py, written by tools/make_prepath_pairs.py: every "
              f"admissible pair of values of two different axes ({total} pairs) occurs in at least one case; each case records one "
              "sibling, itself with one active RAW-side option neutralised.")
    with open(args.output, "w") as f:
        json.dump({"header": header, "axes": pc.AXES, "pairs": total,
                   "cases": [{"case": c, "sibling": s} for c, s in zip(cases, sibs)]}, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {args.output}: {len(cases)} cases for {total} pairs, siblings {uses}, {os.path.getsize(args.output)} bytes")


if __name__ == "__main__":
    main()
