#!/usr/bin/env python3
"""tests/golden/noise_extremes.json: (seed, x, y) whose PCG3D hash lands where gaussian_noise() has a special region.

    python3 -B tools/find_noise_extremes.py [--procs N] [--seeds LO HI] [--out FILE]

A random frame reaches these about once in 1e7 samples, so the suite's random seeds never do; a 100 MP export does on every
frame.  The search walks seeds LO .. HI - 1 (default 0 .. 2^22 - 1) over the window x < 256, y < 64 with oracle.stages.pcg3d
(plain NumPy, no GPU, deterministic: the same records for any --procs) and keeps the first few records of every kind:

    kind        components     condition
    zero        vx, vy, vz     hash == 0: the clamp max(u, 1e-7) is all that stands before ln 0; angle exactly 0
    clamped     vx, vz         1 <= hash <= 429: the clamp branch proper (three, and one with hash <= 3)
    just-free   vx, vz         430 <= hash <= 440: the first values the clamp must NOT take
    one         vx, vy, vz     hash >= 0xFFFFFF80: float32(hash) rounds to 2^32, u == 1.0 (r = 0; a full turn; s12 >= 1)
    below-one   vx, vz         0xFFFFFE80 <= hash <= 0xFFFFFF7F: u just below 1, where the logarithm cancels
    quarter     vy             within 32 of 0x40000000, 0x80000000, 0xC0000000: uy = 1/4, 1/2, 3/4, zeros of sin / cos
    wrap        s12            float32 u1 + uy within 2^-22 of 1.0, three on either side (`side`: below / at-or-above)
    edge        vx, vz         a clamped, zero or one sample at most one pixel from the window's border: it lies inside the
                               radius of every grain stencil, whose reads clamp there

Record: {kind, component, hash, seed, x, y}; wrap records carry the hash of vx in `hash`, that of vy in `hash_y`, and `side`;
quarter records carry `quarter` (1, 2, 3).  The whole range takes about 13 min in one process and 1 min 50 s on 8.  The tool
fails if its range yields no record for a kind and component of the table (or fewer than three for the clamp and the wrap)."""
import argparse
import json
import multiprocessing
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import stages as st  # noqa: E402

W, H = 256, 64
SEEDS = (0, 1 << 22)
OUT = os.path.join(ROOT, "tests", "golden", "noise_extremes.json")
CLAMP_LAST = 429  # float32(429) * 2^-32 < float32(1e-7) <= float32(430) * 2^-32
ONE_FIRST = 0xFFFFFF80
BELOW_ONE_FIRST = 0xFFFFFE80
JUST_FREE_LAST = 440
QUARTER_REACH = 32
WRAP_REACH = 2.0 ** -22
F32 = np.float32

# (kind, component or sub-key) -> how many records the fixture keeps; every key must be found
REQUIRED = {
    **{("zero", c): 3 for c in ("vx", "vy", "vz")},
    **{("clamped", c): 3 for c in ("vx", "vz")},
    **{("clamped<=3", c): 1 for c in ("vx", "vz")},
    **{("just-free", c): 3 for c in ("vx", "vz")},
    **{("one", c): 3 for c in ("vx", "vy", "vz")},
    **{("below-one", c): 3 for c in ("vx", "vz")},
    **{("quarter", q): 2 for q in (1, 2, 3)},
    **{("wrap", s): 3 for s in ("below", "at-or-above")},
    **{("edge", c): 2 for c in ("vx", "vz")},
}

_XS, _YS = np.arange(W)[None, :], np.arange(H)[:, None]
_INV = F32(1.0) / F32(0xFFFFFFFF)


def classify(comp: str, v: int, x: int, y: int):
    """The keys of REQUIRED that one hash component at (x, y) belongs to."""
    keys = []
    if v == 0:
        keys.append(("zero", comp))
    if v >= ONE_FIRST:
        keys.append(("one", comp))
    if comp in ("vx", "vz"):
        if 1 <= v <= CLAMP_LAST:
            keys.append(("clamped", comp))
            if v <= 3:
                keys.append(("clamped<=3", comp))
        elif CLAMP_LAST < v <= JUST_FREE_LAST:
            keys.append(("just-free", comp))
        elif BELOW_ONE_FIRST <= v < ONE_FIRST:
            keys.append(("below-one", comp))
        if (v <= CLAMP_LAST or v >= ONE_FIRST) and min(x, W - 1 - x, y, H - 1 - y) <= 1:
            keys.append(("edge", comp))
    else:
        for q in (1, 2, 3):
            if abs(v - (q << 30)) <= QUARTER_REACH:
                keys.append(("quarter", q))
    return keys


def search(seed_lo: int, seed_hi: int, caps=None):
    """Every record of seeds [seed_lo, seed_hi) in (seed, y, x) order, at most caps[key] per key: [(key, record)]."""
    caps = REQUIRED if caps is None else caps
    left = dict(caps)
    found = []

    def keep(key, rec):
        if left.get(key, 0) > 0:
            left[key] -= 1
            found.append((key, rec))

    lo_span = np.uint32(JUST_FREE_LAST + (1 << 32) - BELOW_ONE_FIRST)
    shift = np.uint32((1 << 32) - BELOW_ONE_FIRST)
    with np.errstate(over="ignore"):
        for seed in range(seed_lo, seed_hi):
            vx, vy, vz = st.pcg3d(_XS, _YS, seed)
            # hash <= 440 or >= 0xFFFFFE80 in one wrapping compare; vy near a multiple of 2^30; vx + vy near 2^32
            ext = ((vx + shift) <= lo_span) | ((vy + shift) <= lo_span) | ((vz + shift) <= lo_span)
            ext |= ((vy + np.uint32(QUARTER_REACH)) & np.uint32(0x3FFFFFFF)) <= np.uint32(2 * QUARTER_REACH)
            ext |= (vx + vy + np.uint32(2048)) <= np.uint32(4096)
            if not ext.any():
                continue
            for y, x in zip(*np.nonzero(ext)):
                y, x = int(y), int(x)
                hx, hy, hz = int(vx[y, x]), int(vy[y, x]), int(vz[y, x])
                for comp, v in (("vx", hx), ("vy", hy), ("vz", hz)):
                    for key in classify(comp, v, x, y):
                        rec = {"kind": key[0].split("<")[0], "component": comp, "hash": v, "seed": seed, "x": x, "y": y}
                        if key[0] == "quarter":
                            rec["quarter"] = key[1]
                        keep(key, rec)
                s12 = np.maximum(F32(hx) * _INV, F32(1e-7)) + F32(hy) * _INV  # float32, as gaussian_noise() forms it
                if abs(float(s12) - 1.0) <= WRAP_REACH:
                    side = "below" if s12 < F32(1.0) else "at-or-above"
                    keep(("wrap", side), {"kind": "wrap", "component": "s12", "hash": hx, "hash_y": hy, "side": side,
                                          "seed": seed, "x": x, "y": y})
    return found


def _chunk(bounds):
    return search(*bounds)


def select(found):
    """The first REQUIRED[key] records of every key over chunks merged in seed order; a record two keys chose is listed once."""
    left = dict(REQUIRED)
    out = []
    for key, rec in found:
        if left[key] > 0:
            left[key] -= 1
            if rec not in out:
                out.append(rec)
    # none at all fails; the clamp branch and the wrap must have their full three
    missing = sorted(str(k) for k, n in left.items() if n == REQUIRED[k] or (n and k[0] in ("clamped", "wrap")))
    return out, missing


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--procs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--seeds", type=int, nargs=2, default=SEEDS, metavar=("LO", "HI"))
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--chunk", type=int, default=4096, help="seeds per task")
    a = ap.parse_args()
    lo, hi = a.seeds
    tasks = [(s, min(s + a.chunk, hi)) for s in range(lo, hi, a.chunk)]
    found = []
    if a.procs > 1 and len(tasks) > 1:
        with multiprocessing.Pool(a.procs) as pool:
            for part in pool.imap(_chunk, tasks):  # in task order: the result does not depend on --procs
                found.extend(part)
    else:
        for t in tasks:
            found.extend(_chunk(t))
    records, missing = select(found)
    if missing:
        sys.exit(f"seeds [{lo}, {hi}) hold too few records for: {', '.join(missing)}")
    doc = {"window": {"W": W, "H": H}, "seeds": [lo, hi], "records": records}
    with open(a.out, "w") as f:
        f.write("{\n")
        f.write(f' "window": {json.dumps(doc["window"])},\n "seeds": {json.dumps(doc["seeds"])},\n "records": [\n')
        f.write(",\n".join("  " + json.dumps(r) for r in records))
        f.write("\n ]\n}\n")
    print(a.out, os.path.getsize(a.out), "bytes,", len(records), "records")


if __name__ == "__main__":
    main()
