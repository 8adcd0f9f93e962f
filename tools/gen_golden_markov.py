#!/usr/bin/env python3
"""Golden G24: the textbook Markov statistics of the REAL reference's own (source tile, destination tile) pairs, pooled over
sliding windows of frame pairs at a lag.

TEST INFRASTRUCTURE ONLY, CPU only; no test runs it.  It follows tools/gen_golden_windowed_transition.py: the same 8-user x
60-frame video of golden G15, the same pooled dicts — one entry per (pair, user) of pairs [r * stride, r * stride + window)
present in both frames of the pair, key ``f"{pair}:{user}"``, inserted pair-major then in user order — generalised to a lag: pair f
is (frame f, frame f + lag), so the prior dict holds the Vector at frame f and the current dict the Vector at frame f + lag.  For
every kept row and every lattice it calls the reference's ``compute_transition_entropy`` and keeps only its THIRD return value, the
(p_idx, c_idx) tile pair of every entry — the reference's own nearest tiles — and applies the textbook forms to them in plain
Python (collections.Counter, math.fsum, math.log2):

    rate        sum_p (n_p / N) sum_c (n_pc / n_p) log2(n_p / n_pc)
    stationary  sum_p (n_p / N) log2(N / n_p)
    dest        sum_c (m_c / N) log2(N / m_c)
    mutual      dest - rate
    stay        sum_p n_pp / N

then the mean over the lattices.  Arrays only are stored.

    python tools/gen_golden_markov.py [--reference /root/reference/src] [--jobs 8]

tests/golden/g24_markov.npz
    <case>__rows [m]                the rows kept (tools/gen_golden_windowed_transition.py: kept_rows)
    <case>__stats [5][m], <case>__samples [m], <case>__matrix [m][n_0][n_0]  (lattice 0's dense counts, source-major)
  case = tc<counts>_w<window>_s<stride>_l<lag>; the whole video is window = 60 - lag.  The dataset is golden G15's mu / mv.
"""
from __future__ import annotations

import argparse
import math
import os
import sys
import types
from collections import Counter
from multiprocessing import Pool
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
OUT = REPO / "tests" / "golden"
sys.path.insert(0, str(REPO / "tools"))
from gen_golden_windowed_transition import T, U, dataset, kept_rows  # noqa: E402

WINDOWS, STRIDES, LAGS = (1, 2, 20, None), (1, 7), (1, 3)          # None: the whole video, T - lag pairs
TILE_COUNTS = ([50], [50, 100, 200])

_S = {}


def _init(ref_src: str, px, py, present):
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.dont_write_bytecode = True
    sys.modules.setdefault("pyvista", types.ModuleType("pyvista"))
    sys.path.insert(0, ref_src)
    _S["px"], _S["py"], _S["present"] = px, py, present
    _S["grid"] = np.load(OUT / "g2_quantiser.npz")["vec_100x200"]      # the reference's rounded Vector of every pixel


def textbook(pairs):
    """(rate, stationary, dest, mutual, stay) of a list of (p, c) pairs; five NaN for an empty list."""
    N = len(pairs)
    if N == 0:
        return (math.nan,) * 5
    n_pc, n_p, m_c = Counter(pairs), Counter(p for p, _ in pairs), Counter(c for _, c in pairs)
    rate = math.fsum((n_p[p] / N) * math.fsum((k / n_p[p]) * math.log2(n_p[p] / k) for (p2, _), k in n_pc.items() if p2 == p)
                     for p in n_p)
    stationary = math.fsum((k / N) * math.log2(N / k) for k in n_p.values())
    dest = math.fsum((k / N) * math.log2(N / k) for k in m_c.values())
    stay = sum(k for (p, c), k in n_pc.items() if p == c) / N
    return rate, stationary, dest, dest - rate, stay


def _work(job):
    from viewport_entropy_toolkit import Vector  # the reference
    from viewport_entropy_toolkit.utilities import compute_transition_entropy, generate_fibonacci_lattice, EntropyConfig
    tcs, w, s, lag, r = job
    px, py, present, grid = _S["px"], _S["py"], _S["present"], _S["grid"]
    prior, current = {}, {}
    for f in range(r * s, r * s + w):
        for u in range(U):
            if present[f, u] and present[f + lag, u]:
                prior[f"{f}:u{u:02d}"] = Vector(*map(float, grid[py[f, u], px[f, u]]))
                current[f"{f}:u{u:02d}"] = Vector(*map(float, grid[py[f + lag, u], px[f + lag, u]]))
    stats, dense = np.zeros(5), None
    for tc in tcs:
        lattice = generate_fibonacci_lattice(tc)
        pairs = []
        if current:                                            # the reference raises on empty dicts: an empty row is NaN
            with np.errstate(all="ignore"):
                _, _, assigned = compute_transition_entropy(prior, current, lattice, EntropyConfig(), 120)
            pairs = [(int(p), int(c)) for p, c in assigned.values()]
        stats += np.array(textbook(pairs))
        if tc == tcs[0]:
            dense = np.zeros((len(lattice), len(lattice)), dtype=np.int32)
            for p, c in pairs:
                dense[p, c] += 1
    return stats / len(tcs), len(current), dense


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default="/root/reference/src")
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    if not Path(args.reference).exists():
        sys.exit(f"reference not found at {args.reference}; nothing to do")
    mu, mv = dataset()
    sys.path.insert(0, str(REPO))
    from oracle import vet_oracle as vo
    px, py, present, _ = vo.sample_directions(mu, mv, 100, 200)        # the quantiser pinned by golden G2
    cases = []
    for tcs in TILE_COUNTS:
        for lag in LAGS:
            for w in WINDOWS:
                w = T - lag if w is None else w
                for s in STRIDES:
                    cases.append((f"tc{'_'.join(map(str, tcs))}_w{w}_s{s}_l{lag}", tcs, w, s, lag, kept_rows((T - lag - w) // s + 1)))
    jobs = [(tcs, w, s, lag, int(r)) for _, tcs, w, s, lag, rows in cases for r in rows]
    with Pool(args.jobs, initializer=_init, initargs=(args.reference, px, py, present)) as pool:
        results = pool.map(_work, jobs, chunksize=1)
    out, k = {}, 0
    for tag, tcs, w, s, lag, rows in cases:
        res = results[k:k + len(rows)]
        k += len(rows)
        out[f"{tag}__rows"] = rows.astype(np.int64)
        out[f"{tag}__stats"] = np.stack([x[0] for x in res], axis=1).astype(np.float64)
        out[f"{tag}__samples"] = np.array([x[1] for x in res], dtype=np.int32)
        out[f"{tag}__matrix"] = np.stack([x[2] for x in res])
        print(tag, rows.tolist(), out[f"{tag}__stats"][0].tolist(), flush=True)
    path = OUT / "g24_markov.npz"
    np.savez_compressed(path, **out)
    print("wrote", path, path.stat().st_size, "bytes,", k, "rows")


if __name__ == "__main__":
    main()
