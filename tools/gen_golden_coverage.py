#!/usr/bin/env python3
"""Golden G23: the REAL reference behind the attention coverage (include/vet.h: vet_coverage).

TEST INFRASTRUCTURE ONLY, CPU only; no test runs it.  It imports the reference the way tools/gen_golden_window_divergence.py does
(an empty ``pyvista`` stand-in, the reference's ``src`` on the path), takes golden G14's "absent" dataset (``mu_absent`` /
``mv_absent`` of tests/golden/g14_windowed.npz: 8 viewers x 300 frames), feeds it through the reference's own ingest, and for
every row r of a (window, stride, max_lag) shape calls the reference's ``compute_spatial_entropy`` (naive case:
``compute_naive_spatial_entropy``) on ONE dict holding the present samples of frames [r * stride, r * stride + window),
frame-major then user order.  The returned histogram is densified over lattice 0's tiles (naive: over the cells
``lon index * 19 + lat index``), and the coverage is taken from it by the definition, in plain Python floats:

    order   the tiles by weight descending, equal weights by index ascending
    C       one accumulator over the weights in rank order; W = its end value
    tiles   per fraction q the smallest k with C_k >= q * W
    hit     per lag l = 0 .. max_lag the sum of row r + l's histogram over row r's first ``tiles`` tiles, over the total of row
            r + l's returned dict (its values added in dict order); NaN where r + l >= R

Only lattice 0 takes part, so the case of the plan [50, 100, 200] holds the values of [50].  Arrays only are stored.

    python tools/gen_golden_coverage.py [--reference /root/reference/src] [--jobs 8]

tests/golden/g23_coverage.npz
    fractions [4]                         0.5, 0.8, 0.95, 1.0
    <case>__rows [m]                      the rows kept: every row of (20, 20, 14); of the other shapes every 7th row and the last
                                          max_lag + 1 rows (the bands the end of the video cuts)
    <case>__weights [m][n] f64            the reference's histogram of the kept rows
    <case>__tiles [m][4] i16, <case>__order [m][n] i16, <case>__hit [m][L + 1][4] f64, <case>__samples [m] i32
  case = {w_tc50|w_tc50_100_200|u_tc50|naive_h10_w20}_w<window>_s<stride>_l<max_lag>.
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
SHAPES = ((20, 20, 14), (5, 1, 6), (1, 1, 3))                      # (window, stride, max_lag)
CASES = (("w_tc50", True, 50), ("w_tc50_100_200", True, 50), ("u_tc50", False, 50))     # lattice 0 of each plan
NAIVE = (10, 20)                                                   # tile_height, tile_width
FRACTIONS = (0.5, 0.8, 0.95, 1.0)

_S = {}


def n_rows(T: int, w: int, s: int) -> int:
    return (T - w) // s + 1


def kept_rows(T: int, w: int, s: int, L: int) -> np.ndarray:
    R = n_rows(T, w, s)
    if (w, s, L) == SHAPES[0]:
        return np.arange(R)
    return np.unique(np.concatenate([np.arange(0, R, 7), np.arange(max(0, R - 1 - L), R)]))


def dataset():
    g14 = np.load(OUT / "g14_windowed.npz")
    g4 = np.load(OUT / "g4_spatial.npz")
    return g4["time_in"], g14["mu_absent"], g14["mv_absent"]


def _init(ref_src: str):
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.dont_write_bytecode = True
    sys.modules.setdefault("pyvista", types.ModuleType("pyvista"))
    sys.path.insert(0, ref_src)
    import viewport_entropy_toolkit  # noqa: F401  (the reference)
    from viewport_entropy_toolkit import AnalyzerConfig, SpatialEntropyAnalyzer
    import pandas as pd
    times, mu, mv = dataset()
    T, U = mu.shape
    with tempfile.TemporaryDirectory() as td:
        d = Path(td) / "in"
        d.mkdir()
        for u in range(U):
            keep = ~np.isnan(mu[:, u])
            pd.DataFrame({"time": times[u][keep], "2dmu": mu[keep, u], "2dmv": mv[keep, u]}).to_csv(
                d / f"user{u:03d}.csv", index=False)
        an = SpatialEntropyAnalyzer(AnalyzerConfig(output_dir=Path(td) / "out", tile_counts=[50]))
        an.process_directory(d)
        # the reference appends a time when some user first shows it: put the frame table back into frame order
        vectors = an._data_cache["vectors"].sort_values("time", kind="stable").reset_index(drop=True)
        points = an._data_cache["points"].sort_values("time", kind="stable").reset_index(drop=True)
    assert len(vectors) == T, (len(vectors), T)
    cols = sorted(c for c in vectors.columns if c != "time")
    assert len(cols) == U
    for u, c in enumerate(cols):                                   # the ingest's view of presence is the dataset's
        assert [v is not None for v in vectors[c]] == list(~np.isnan(mu[:, u])), c
    _S["frames"] = (vectors, points, cols)


def _row_dict(df, cols, f0: int, w: int):
    out = {}
    for f in range(f0, f0 + w):                                    # frame-major, then user order
        row = df.iloc[f]
        for u, c in enumerate(cols):
            if row[c] is not None:
                out[f"{f}_{u}"] = row[c]
    return out


def _work(job):
    """One (kind, flag, tile count, window, stride, row): (dense histogram [n], total in dict order, samples of the row)."""
    from viewport_entropy_toolkit.config import EntropyConfig
    from viewport_entropy_toolkit.utilities import (compute_naive_spatial_entropy, compute_spatial_entropy,
                                                    generate_fibonacci_lattice)
    kind, flag, tc, w, s, r = job
    cfg = EntropyConfig(use_weight_distribution=flag)
    vectors, points, cols = _S["frames"]
    d = _row_dict(points if kind == "naive" else vectors, cols, r * s, w)
    if kind == "naive":
        n_lat = 180 // NAIVE[0] + 1
        dense = np.zeros((360 // NAIVE[1] + 1) * n_lat)
        weights = compute_naive_spatial_entropy(d, NAIVE[0], NAIVE[1], cfg)[1] if d else {}
        for key, x in weights.items():
            li, lj = map(int, key.split("_"))
            dense[li * n_lat + lj] = x
    else:
        lattice = generate_fibonacci_lattice(tc)
        index = {tile: t for t, tile in enumerate(lattice)}
        dense = np.zeros(len(lattice))
        weights = compute_spatial_entropy(d, lattice, cfg)[1] if d else {}
        for tile, x in weights.items():
            dense[index[tile]] = x
    total = 0.0
    for x in weights.values():
        total += x
    return dense, total, len(d)


def coverage(h, totals, L):
    """The definition in Python floats on the dense rows h[R][n]: (tiles[R][Q], order[R][n], hit[R][L + 1][Q])."""
    R, n = h.shape
    Q = len(FRACTIONS)
    tiles = np.zeros((R, Q), dtype=np.int16)
    order = np.zeros((R, n), dtype=np.int16)
    hit = np.full((R, L + 1, Q), np.nan)
    for r in range(R):
        row = [float(x) for x in h[r]]
        o = sorted(range(n), key=lambda t: (-row[t], t))
        order[r] = o
        C = [0.0]
        for t in o:
            C.append(C[-1] + row[t])
        W = C[-1]
        if W > 0:
            for i, q in enumerate(FRACTIONS):
                thr = q * W
                tiles[r, i] = next(k for k in range(n + 1) if C[k] >= thr)
    for r in range(R):
        if not h[r].any():
            continue
        for l in range(L + 1):
            if r + l >= R or not totals[r + l] > 0:
                continue
            for i in range(len(FRACTIONS)):
                acc = 0.0
                for t in sorted(order[r][:tiles[r, i]]):
                    acc += float(h[r + l][t])
                hit[r, l, i] = acc / totals[r + l]
    return tiles, order, hit


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default="/root/reference/src")
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    if not Path(args.reference).exists():
        sys.exit(f"reference not found at {args.reference}; nothing to do")
    T = dataset()[1].shape[0]
    runs = {}                                                      # (kind, flag, tc, w, s) -> jobs of every row
    for w, s, L in SHAPES:
        for _, flag, tc in CASES:
            runs.setdefault(("fib", flag, tc, w, s), None)
        runs.setdefault(("naive", True, None, w, s), None)
    jobs = [key + (r,) for key in runs for r in range(n_rows(T, key[3], key[4]))]
    jobs_sorted = sorted(range(len(jobs)), key=lambda i: -jobs[i][3])                               # the long ones first
    with Pool(args.jobs, initializer=_init, initargs=(args.reference,)) as pool:
        done = pool.map(_work, [jobs[i] for i in jobs_sorted], chunksize=4)
    results = {}
    for i, res in zip(jobs_sorted, done):
        results[jobs[i]] = res
    out = {"fractions": np.array(FRACTIONS)}
    for w, s, L in SHAPES:
        R = n_rows(T, w, s)
        rows = kept_rows(T, w, s, L)
        cases = [(f"{tag}_w{w}_s{s}_l{L}", ("fib", flag, tc, w, s)) for tag, flag, tc in CASES]
        cases.append((f"naive_h{NAIVE[0]}_w{NAIVE[1]}_w{w}_s{s}_l{L}", ("naive", True, None, w, s)))
        for tag, key in cases:
            res = [results[key + (r,)] for r in range(R)]
            h = np.stack([x[0] for x in res])
            totals = np.array([x[1] for x in res])
            tiles, order, hit = coverage(h, totals, L)
            out[f"{tag}__rows"] = rows.astype(np.int32)
            out[f"{tag}__weights"] = h[rows]
            out[f"{tag}__tiles"], out[f"{tag}__order"], out[f"{tag}__hit"] = tiles[rows], order[rows], hit[rows]
            out[f"{tag}__samples"] = np.array([x[2] for x in res], dtype=np.int32)[rows]
            print(tag, len(rows), "rows of", R, "tiles", tiles[rows].min(axis=0), "..", tiles[rows].max(axis=0), "NaN entries",
                  int(np.isnan(hit[rows]).sum()), flush=True)
    np.savez_compressed(OUT / "g23_coverage.npz", **out)
    print("wrote", OUT / "g23_coverage.npz", (OUT / "g23_coverage.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
