#!/usr/bin/env python3
"""Golden G15: the REAL reference's compute_transition_entropy on the transitions of sliding windows of frame pairs, pooled.

TEST INFRASTRUCTURE ONLY, CPU only; no test runs it.  It imports the reference the way oracle/gen_golden.py does (an empty
``pyvista`` stand-in, the reference's ``src`` on the path), takes an 8-user x 60-frame random walk with a few absent samples
on the 100 x 200 pixel grid (every sample's Vector from golden G2's table of the reference's rounded pixel directions, as
oracle/gen_golden.py builds golden G8), and for every kept row r of a (window, stride) pair calls the reference's
``compute_transition_entropy`` on two dicts that hold one entry per (pair, user) of pairs [r * stride, r * stride + window)
present in both frames of the pair — key ``f"{pair}:{user}"``, inserted pair-major then in user order, the prior dict holding
the Vector at frame f and the current dict the Vector at frame f + 1 — once per lattice, and takes the mean over the lattices
as ``TransitionEntropyAnalyzer.compute_entropy`` does.  Arrays only are stored.

    python tools/gen_golden_windowed_transition.py [--reference /root/reference/src] [--jobs 8]

tests/golden/g15_windowed_transition.npz
    mu, mv [60][8]                  the dataset (NaN = absent), frame-major
    <case>__rows [m]                the rows kept (first, middle, last, and the one before the last where there are four)
    <case>__entropy [m], <case>__samples [m], <case>__srccount [m][n_0]  (lattice 0's weight_per_tile, dense)
  case = tc<counts>_w<window>_s<stride>
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
import types
from multiprocessing import Pool
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
OUT = REPO / "tests" / "golden"
U, T = 8, 60
WINDOWS, STRIDES = (1, 2, 20), (1, 7)
TILE_COUNTS = ([50], [50, 100, 200])

_S = {}


def dataset():
    sys.path.insert(0, str(REPO / "viewport-entropy-toolkit_amd"))
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(U, T, base_seed=15, p_absent=0.04)
    mu[30, :5] = np.nan                        # a frame most users miss: the pairs 29 and 30 pool three users
    mv[30, :5] = np.nan
    sys.path.pop(0)
    for m in [k for k in sys.modules if k.startswith("viewport_entropy_toolkit")]:
        del sys.modules[m]
    return mu, mv


def kept_rows(R: int) -> np.ndarray:
    return np.unique([0, R // 2, max(R - 2, 0), R - 1])


def _init(ref_src: str, px, py, present):
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.dont_write_bytecode = True
    sys.modules.setdefault("pyvista", types.ModuleType("pyvista"))
    sys.path.insert(0, ref_src)
    _S["px"], _S["py"], _S["present"] = px, py, present
    _S["grid"] = np.load(OUT / "g2_quantiser.npz")["vec_100x200"]      # the reference's rounded Vector of every pixel


def _work(job):
    from viewport_entropy_toolkit import Vector  # the reference
    from viewport_entropy_toolkit.utilities import compute_transition_entropy, generate_fibonacci_lattice, EntropyConfig
    tcs, w, s, r = job
    px, py, present, grid = _S["px"], _S["py"], _S["present"], _S["grid"]
    prior, current = {}, {}
    for f in range(r * s, r * s + w):
        for u in range(U):
            if present[f, u] and present[f + 1, u]:
                prior[f"{f}:u{u:02d}"] = Vector(*map(float, grid[py[f, u], px[f, u]]))
                current[f"{f}:u{u:02d}"] = Vector(*map(float, grid[py[f + 1, u], px[f + 1, u]]))
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
    mu, mv = dataset()
    sys.path.insert(0, str(REPO))
    from oracle import vet_oracle as vo
    px, py, present, _ = vo.sample_directions(mu, mv, 100, 200)        # the quantiser pinned by golden G2
    out = {"mu": mu, "mv": mv}
    cases = []
    for tcs in TILE_COUNTS:
        for w in WINDOWS:
            for s in STRIDES:
                cases.append((f"tc{'_'.join(map(str, tcs))}_w{w}_s{s}", tcs, w, s, kept_rows((T - 1 - w) // s + 1)))
    jobs = [(tcs, w, s, int(r)) for _, tcs, w, s, rows in cases for r in rows]
    with Pool(args.jobs, initializer=_init, initargs=(args.reference, px, py, present)) as pool:
        results = pool.map(_work, jobs, chunksize=1)
    k = 0
    for tag, tcs, w, s, rows in cases:
        res = results[k:k + len(rows)]
        k += len(rows)
        out[f"{tag}__rows"] = rows.astype(np.int64)
        out[f"{tag}__entropy"] = np.array([x[0] for x in res], dtype=np.float64)
        out[f"{tag}__samples"] = np.array([x[1] for x in res], dtype=np.int32)
        out[f"{tag}__srccount"] = np.stack([x[2] for x in res])
        print(tag, rows.tolist(), out[f"{tag}__entropy"].tolist(), flush=True)
    np.savez_compressed(OUT / "g15_windowed_transition.npz", **out)
    print("wrote", OUT / "g15_windowed_transition.npz", (OUT / "g15_windowed_transition.npz").stat().st_size, "bytes,", k, "rows")


if __name__ == "__main__":
    main()
