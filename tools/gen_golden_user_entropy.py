#!/usr/bin/env python3
"""Golden G16: the REAL reference on each viewer's own samples over a run of frames, pooled into one dict.

TEST INFRASTRUCTURE ONLY, CPU only; no test runs it.  It imports the reference the way tools/gen_windowed_golden.py does (an
empty ``pyvista`` stand-in, the reference's ``src`` on the path), takes golden G4's 8-user x 300-frame dataset (read from
tests/golden/g4_spatial.npz, so the inputs are shared), removes about 10 % of the samples from a fixed seed (never in frame 0) and user 3 for frames
100..199, feeds the rest through the reference's own ingest, and for every kept row (u, r) of a (window, stride) pair calls the
reference's ``compute_spatial_entropy`` on ONE dict that holds an entry for every present sample of user u in frames
[r * stride, r * stride + window), in ascending frame order (keys ``f"{frame}"``), once per lattice, and takes the mean over
the lattices as ``compute_entropy`` does.  A row without a sample (the reference raises ValidationError) is stored as NaN with
0 samples.  Arrays only are stored.

    python tools/gen_golden_user_entropy.py [--reference /root/reference/src] [--jobs 8]

tests/golden/g16_user_entropy.npz
    mu, mv [300][8]                 the dataset (NaN = absent), frame-major
    <case>__rows [m]                the rows r kept, the same for every user ((1, 1): about 40 rows, the ends and frames around
                                    the absent stretch included; every row otherwise)
    <case>__entropy [8][m], <case>__samples [8][m]
    <case>__weights [8][m][n_0], <case>__keys [8][m][n_0]     lattice 0's dict, dense (not for the naive cases)
  case = {w|u}_tc<counts>_w<window>_s<stride> and naive_h10_w20_w<window>_s<stride> (compute_naive_spatial_entropy, 10 x 20
  degree cells; entropy and samples only).
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
SHAPES = ((300, 1), (20, 20), (20, 7), (1, 1))          # (window, stride)
CASES = (("w", True, [50]), ("w", True, [50, 100, 200]), ("u", False, [50]))
NAIVE = (10, 20)                                       # tile_height, tile_width
ABSENT_USER, ABSENT_FRAMES = 3, (100, 200)
SEED, P_ABSENT = 16, 0.1

_S = {}


def dataset():
    g4 = np.load(OUT / "g4_spatial.npz")
    times, mu, mv = g4["time_in"], g4["mu_in"].T.copy(), g4["mv_in"].T.copy()      # [T][U]
    drop = np.random.default_rng(SEED).random(mu.shape) < P_ABSENT
    drop[0] = False                     # the reference's ingest shifts a user's clock to its first sample: everyone keeps frame 0
    drop[ABSENT_FRAMES[0]:ABSENT_FRAMES[1], ABSENT_USER] = True
    mu[drop] = np.nan
    mv[drop] = np.nan
    return times, mu, mv


def kept_rows(R: int, window: int, stride: int) -> np.ndarray:
    if (window, stride) != (1, 1):
        return np.arange(R)
    rows = np.concatenate([np.arange(0, R, 9), [98, 99, 100, 101, 198, 199, 200, 201, R - 1]])
    return np.unique(rows)


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


def _row_dict(df, col, f0: int, w: int):
    out = {}
    for f in range(f0, f0 + w):
        v = df[col].iloc[f]
        if v is not None:
            out[f"{f}"] = v
    return out


def _work(job):
    from viewport_entropy_toolkit.config import EntropyConfig
    from viewport_entropy_toolkit.utilities import (compute_naive_spatial_entropy, compute_spatial_entropy,
                                                    generate_fibonacci_lattice)
    kind, flag, tcs, w, s, u, r = job
    cfg = EntropyConfig(use_weight_distribution=flag)
    vectors, points, cols = _S["frames"]
    with np.errstate(all="ignore"):
        if kind == "naive":
            d = _row_dict(points, cols[u], r * s, w)
            if not d:
                return float("nan"), 0, None, None
            e, _, _ = compute_naive_spatial_entropy(d, NAIVE[0], NAIVE[1], cfg)
            return float(e), len(d), None, None
        d = _row_dict(vectors, cols[u], r * s, w)
        n0 = len(generate_fibonacci_lattice(tcs[0]))
        if not d:
            return float("nan"), 0, np.zeros(n0), np.zeros(n0, dtype=bool)
        total, dense, keys = 0, None, None
        for tc in tcs:
            lattice = generate_fibonacci_lattice(tc)
            e, weights, _ = compute_spatial_entropy(d, lattice, cfg)
            total += e
            if tc == tcs[0]:
                idx = {v: i for i, v in enumerate(lattice)}
                dense, keys = np.zeros(len(lattice)), np.zeros(len(lattice), dtype=bool)
                for v, x in weights.items():
                    dense[idx[v]] = x
                    keys[idx[v]] = True
        return float(total / len(tcs)), len(d), dense, keys


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default="/root/reference/src")
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    if not Path(args.reference).exists():
        sys.exit(f"reference not found at {args.reference}; nothing to do")
    _, mu, mv = dataset()
    T, U = mu.shape
    out = {"mu": mu, "mv": mv}
    cases = []
    for w, s in SHAPES:
        rows = kept_rows((T - w) // s + 1, w, s)
        for flag_tag, flag, tcs in CASES:
            cases.append((f"{flag_tag}_tc{'_'.join(map(str, tcs))}_w{w}_s{s}", "fib", flag, tcs, w, s, rows))
        cases.append((f"naive_h{NAIVE[0]}_w{NAIVE[1]}_w{w}_s{s}", "naive", True, None, w, s, rows))
    jobs = [(kind, flag, tcs, w, s, u, int(r)) for _, kind, flag, tcs, w, s, rows in cases for u in range(U) for r in rows]
    with Pool(args.jobs, initializer=_init, initargs=(args.reference,)) as pool:
        results = pool.map(_work, jobs, chunksize=8)
    k = 0
    for tag, kind, flag, tcs, w, s, rows in cases:
        m = len(rows)
        res = results[k:k + U * m]
        k += U * m
        out[f"{tag}__rows"] = rows.astype(np.int64)
        out[f"{tag}__entropy"] = np.array([x[0] for x in res], dtype=np.float64).reshape(U, m)
        out[f"{tag}__samples"] = np.array([x[1] for x in res], dtype=np.int32).reshape(U, m)
        if kind == "fib":
            out[f"{tag}__weights"] = np.stack([x[2] for x in res]).reshape(U, m, -1)
            out[f"{tag}__keys"] = np.stack([x[3] for x in res]).reshape(U, m, -1)
        print(tag, m, "rows per user, mean", float(np.nanmean(out[f"{tag}__entropy"])), "NaN rows",
              int(np.isnan(out[f"{tag}__entropy"]).sum()), flush=True)
    np.savez_compressed(OUT / "g16_user_entropy.npz", **out)
    print("wrote", OUT / "g16_user_entropy.npz", (OUT / "g16_user_entropy.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
