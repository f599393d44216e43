"""The row-sharded renderer's call log, case by case, against the committed record (tools/shard_walk_digest.py): every stage call,
every exchange, every capture and replay of ~20 000 cases (worlds 1 .. 8, every rank, three reach sets, three band heights, all
stage gates, the four schedule requests, graph path and eager, the measuring phase under a scripted clock) hashed per group.
tests/golden/shard_walk_digest.txt was written by the tool from the renderer as it was BEFORE its frame order became one step
list: a line that differs is a call made, dropped or reordered -- fix the code, not the record."""

import os
import sys

import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_call_log_of_every_case_is_the_recorded_one(golden_dir):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import shard_walk_digest as swd
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    from raw2film_amd import sharding

    saved = torch.cuda.CUDAGraph, torch.cuda.graph, torch.cuda.synchronize
    got = swd.digest_lines(sharding)
    assert (torch.cuda.CUDAGraph, torch.cuda.graph, torch.cuda.synchronize) == saved  # (the tool's fakes are gone again)
    with open(os.path.join(golden_dir, "shard_walk_digest.txt")) as f:
        want = f.read().splitlines()
    for g, w in zip(got, want):
        assert g == w, f"first differing group: {w.split()[0]} (python tools/shard_walk_digest.py --case {w.split()[0]}/<case> prints a log)"
    assert len(got) == len(want) and len(got) > 700
