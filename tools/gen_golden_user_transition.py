#!/usr/bin/env python3
"""Golden G17: the REAL reference's compute_transition_entropy on each viewer's own frame pairs over a run of pairs, pooled.

TEST INFRASTRUCTURE ONLY, CPU only; no test runs it.  It imports the reference the way tools/gen_golden_windowed_transition.py
does (an empty ``pyvista`` stand-in, the reference's ``src`` on the path), takes the dataset stored in
tests/golden/g16_user_entropy.npz (8 users x 300 frames, about 10 % of the samples absent, user 3 away for frames 100..199; every
sample's Vector from golden G2's table of the reference's rounded pixel directions), and for every kept row (u, r) of a
(window, stride) pair calls the reference's ``compute_transition_entropy`` on two dicts that hold one entry per pair f of
[r * stride, r * stride + window) in which user u is present in frame f and in frame f + 1 — key ``f"{f}"``, inserted in
ascending pair order, the prior dict holding the Vector at frame f and the current dict the Vector at frame f + 1 — once per
lattice, and takes the mean over the lattices as ``TransitionEntropyAnalyzer.compute_entropy`` does.  A row without such a pair
(the reference raises) is stored as NaN with 0 samples.  Arrays only are stored; the dataset is not repeated.

    python tools/gen_golden_user_transition.py [--reference /root/reference/src] [--jobs 8]

tests/golden/g17_user_transition.npz
    <case>__rows [m]                the rows r kept, the same for every user (every row, except (2, 1): every 9th row, the rows
                                    around frames 98..101 and 198..201 where user 3 leaves and returns, and the last)
    <case>__entropy [8][m], <case>__samples [8][m], <case>__srccount [8][m][n_0]  (lattice 0's weight_per_tile, dense)
  case = tc<counts>_w<window>_s<stride>
"""
from __future__ import annotations

import argparse
import os
import sys
import types
from multiprocessing import Pool
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
OUT = REPO / "tests" / "golden"
SHAPES = ((299, 1), (20, 20), (20, 7), (64, 5), (65, 5), (2, 1))          # (window, stride), in frame pairs
TILE_COUNTS = ([50], [50, 100, 200], [20])

_S = {}


def kept_rows(R: int, window: int, stride: int) -> np.ndarray:
    if (window, stride) != (2, 1):
        return np.arange(R)
    return np.unique(np.concatenate([np.arange(0, R, 9), np.arange(95, 104), np.arange(195, 204), [R - 1]]))


def _init(ref_src: str, px, py, present):
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.dont_write_bytecode = True
    sys.modules.setdefault("pyvista", types.ModuleType("pyvista"))
    sys.path.insert(0, ref_src)
    _S["px"], _S["py"], _S["present"] = px, py, present
    _S["grid"] = np.load(OUT / "g2_quantiser.npz")["vec_100x200"]      # the reference's rounded Vector of every pixel


def _work(job):
    from viewport_entropy_toolkit import ValidationError, Vector  # the reference
    from viewport_entropy_toolkit.utilities import compute_transition_entropy, generate_fibonacci_lattice, EntropyConfig
    tcs, w, s, u, r = job
    px, py, present, grid = _S["px"], _S["py"], _S["present"], _S["grid"]
    prior, current = {}, {}
    for f in range(r * s, r * s + w):
        if present[f, u] and present[f + 1, u]:
            prior[f"{f}"] = Vector(*map(float, grid[py[f, u], px[f, u]]))
            current[f"{f}"] = Vector(*map(float, grid[py[f + 1, u], px[f + 1, u]]))
    n0 = len(generate_fibonacci_lattice(tcs[0]))
    if not current:
        try:
            compute_transition_entropy(prior, current, generate_fibonacci_lattice(tcs[0]), EntropyConfig(), 120)
        except (ValidationError, ZeroDivisionError):
            return float("nan"), 0, np.zeros(n0, dtype=np.int32)
        raise AssertionError("the reference accepted a row without a pair")
    total, dense = 0, None
    with np.errstate(all="ignore"):
        for tc in tcs:
            lattice = generate_fibonacci_lattice(tc)
            e, weights, _ = compute_transition_entropy(prior, current, lattice, EntropyConfig(), 120)
            total += e
            if tc == tcs[0]:
                idx = {v: i for i, v in enumerate(lattice)}
                dense = np.zeros(len(lattice), dtype=np.int32)
                for v, x in weights.items():
                    dense[idx[v]] = x
    return float(total / len(tcs)), len(current), dense


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default="/root/reference/src")
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    if not Path(args.reference).exists():
        sys.exit(f"reference not found at {args.reference}; nothing to do")
    g16 = np.load(OUT / "g16_user_entropy.npz")
    mu, mv = g16["mu"], g16["mv"]
    T, U = mu.shape
    sys.path.insert(0, str(REPO))
    from oracle import vet_oracle as vo
    px, py, present, _ = vo.sample_directions(mu, mv, 100, 200)        # the quantiser pinned by golden G2
    out = {}
    cases = []
    for tcs in TILE_COUNTS:
        for w, s in SHAPES:
            cases.append((f"tc{'_'.join(map(str, tcs))}_w{w}_s{s}", tcs, w, s, kept_rows((T - 1 - w) // s + 1, w, s)))
    jobs = [(tcs, w, s, u, int(r)) for _, tcs, w, s, rows in cases for u in range(U) for r in rows]
    with Pool(args.jobs, initializer=_init, initargs=(args.reference, px, py, present)) as pool:
        results = pool.map(_work, jobs, chunksize=4)
    k = 0
    for tag, tcs, w, s, rows in cases:
        m = len(rows)
        res = results[k:k + U * m]
        k += U * m
        out[f"{tag}__rows"] = rows.astype(np.int64)
        out[f"{tag}__entropy"] = np.array([x[0] for x in res], dtype=np.float64).reshape(U, m)
        out[f"{tag}__samples"] = np.array([x[1] for x in res], dtype=np.int32).reshape(U, m)
        out[f"{tag}__srccount"] = np.stack([x[2] for x in res]).reshape(U, m, -1)
        ent, n = out[f"{tag}__entropy"], out[f"{tag}__samples"]
        print(tag, m, "rows per user; empty", int((n == 0).sum()), "N=1", int((n == 1).sum()), "distinct finite",
              len(np.unique(ent[np.isfinite(ent)])), flush=True)
    np.savez_compressed(OUT / "g17_user_transition.npz", **out)
    print("wrote", OUT / "g17_user_transition.npz", (OUT / "g17_user_transition.npz").stat().st_size, "bytes,", k, "rows")


if __name__ == "__main__":
    main()
