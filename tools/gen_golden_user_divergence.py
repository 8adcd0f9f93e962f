#!/usr/bin/env python3
"""Golden G18: the REAL reference behind the pairwise viewer divergence (include/vet.h: vet_user_divergence).

TEST INFRASTRUCTURE ONLY, CPU only; no test runs it.  It imports the reference the way tools/gen_golden_user_entropy.py does (an
empty ``pyvista`` stand-in, the reference's ``src`` on the path), takes golden G16's dataset (``mu`` / ``mv`` of
tests/golden/g16_user_entropy.npz: 8 viewers x 300 frames, viewer 3 away for frames 100..199), feeds it through the reference's
own ingest, and for every kept row r of a (window, stride) pair and every pair of viewers u <= v calls the reference's
``compute_spatial_entropy`` (naive case: ``compute_naive_spatial_entropy``) on ONE dict that holds viewer u's present samples of
frames [r * stride, r * stride + window) in ascending frame order and then — for u < v — viewer v's (keys ``f"{viewer}_{frame}"``:
unique per (viewer, frame)), once per lattice.  From the returned dict it takes the total W (the sum of the values in dict
order) and S = -sum (x / W) log2(x / W) over the values in dict order — the reference's ``entropy`` before the normaliser — and

    D_k(u, v) = S_uv - (W_u S_u + W_v S_v) / (W_u + W_v),       D = mean over the lattices of D_k

NaN where either viewer has no sample in the row (the reference raises ValidationError on the empty dict), +0.0 on the diagonal
of a present viewer.  Arrays only are stored.

    python tools/gen_golden_user_divergence.py [--reference /root/reference/src] [--jobs 8]

tests/golden/g18_user_divergence.npz
    <case>__rows [m]                      the rows r kept (a subset: the ends and the rows around viewer 3's absence)
    <case>__entropy [m][K][8][8]          the reference's RETURNED (normalised) entropy of the dict of (u, v); the diagonal: u alone
    <case>__bits [m][K][8][8]             S of that dict, <case>__total [m][K][8][8] its W
    <case>__divergence [m][8][8]          D
    <case>__samples [8][m]
  case = G16's: {w|u}_tc<counts>_w<window>_s<stride> and naive_h10_w20_w<window>_s<stride>.
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
ROWS = {(300, 1): [0], (20, 20): list(range(15)), (20, 7): [0, 5, 12, 14, 15, 20, 25, 26, 28, 33, 40],
        (1, 1): [0, 54, 98, 99, 100, 101, 153, 198, 199, 200, 201, 299]}      # each a row G16 keeps

_S = {}


def dataset():
    g16 = np.load(OUT / "g16_user_entropy.npz")
    g4 = np.load(OUT / "g4_spatial.npz")
    return g4["time_in"], g16["mu"], g16["mv"]


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


def _row_dict(df, cols, viewers, f0: int, w: int):
    out = {}
    for u in viewers:
        for f in range(f0, f0 + w):
            v = df[cols[u]].iloc[f]
            if v is not None:
                out[f"{u}_{f}"] = v
    return out


def _bits(weights: dict):
    total = 0.0
    for x in weights.values():
        total += x
    s = 0.0
    for x in weights.values():
        q = x / total
        s -= q * np.log2(q)
    return float(s), float(total)


def _work(job):
    """One (case, row): (entropy[K][U][U], bits[K][U][U], total[K][U][U], samples[U])."""
    from viewport_entropy_toolkit.config import EntropyConfig
    from viewport_entropy_toolkit.utilities import (compute_naive_spatial_entropy, compute_spatial_entropy,
                                                    generate_fibonacci_lattice)
    kind, flag, tcs, w, s, r = job
    cfg = EntropyConfig(use_weight_distribution=flag)
    vectors, points, cols = _S["frames"]
    U = len(cols)
    lattices = [None] if kind == "naive" else [generate_fibonacci_lattice(tc) for tc in tcs]
    df = points if kind == "naive" else vectors
    K = len(lattices)
    ent, bits, tot = (np.full((K, U, U), np.nan) for _ in range(3))
    own = [_row_dict(df, cols, [u], r * s, w) for u in range(U)]
    with np.errstate(all="ignore"):
        for k, L in enumerate(lattices):
            for u in range(U):
                for v in range(u, U):
                    if not own[u] or not own[v]:
                        continue
                    d = own[u] if u == v else _row_dict(df, cols, [u, v], r * s, w)
                    assert len(d) == (len(own[u]) if u == v else len(own[u]) + len(own[v]))     # keys unique per (viewer, frame)
                    e, weights, _ = (compute_naive_spatial_entropy(d, NAIVE[0], NAIVE[1], cfg) if kind == "naive" else
                                     compute_spatial_entropy(d, L, cfg))
                    ent[k, u, v] = ent[k, v, u] = float(e)
                    bits[k, u, v], tot[k, u, v] = _bits(weights)
                    bits[k, v, u], tot[k, v, u] = bits[k, u, v], tot[k, u, v]
    return ent, bits, tot, np.array([len(x) for x in own], dtype=np.int32)


def divergence(bits, tot, present):
    """D[U][U] from the three-term tables [K][U][U] (the docstring's formula)."""
    K, U, _ = bits.shape
    D = np.zeros((U, U))
    with np.errstate(all="ignore"):
        for k in range(K):
            S, W = np.diag(bits[k]), np.diag(tot[k])
            Dk = bits[k] - (W[:, None] * S[:, None] + W[None, :] * S[None, :]) / (W[:, None] + W[None, :])
            ok = present & ~np.isnan(S)
            Dk[np.flatnonzero(ok), np.flatnonzero(ok)] = 0.0
            D += Dk
    D /= K
    D[~present, :] = np.nan
    D[:, ~present] = np.nan
    return D


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default="/root/reference/src")
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    if not Path(args.reference).exists():
        sys.exit(f"reference not found at {args.reference}; nothing to do")
    cases = []
    for w, s in SHAPES:
        rows = np.array(ROWS[(w, s)], dtype=np.int64)
        for flag_tag, flag, tcs in CASES:
            cases.append((f"{flag_tag}_tc{'_'.join(map(str, tcs))}_w{w}_s{s}", "fib", flag, tcs, w, s, rows))
        cases.append((f"naive_h{NAIVE[0]}_w{NAIVE[1]}_w{w}_s{s}", "naive", True, None, w, s, rows))
    jobs = [(kind, flag, tcs, w, s, int(r)) for _, kind, flag, tcs, w, s, rows in cases for r in rows]
    jobs_sorted = sorted(range(len(jobs)), key=lambda i: -jobs[i][3] * len(jobs[i][2] or [0]))      # the long ones first
    with Pool(args.jobs, initializer=_init, initargs=(args.reference,)) as pool:
        done = pool.map(_work, [jobs[i] for i in jobs_sorted], chunksize=1)
    results = [None] * len(jobs)
    for i, res in zip(jobs_sorted, done):
        results[i] = res
    out, k = {}, 0
    for tag, kind, flag, tcs, w, s, rows in cases:
        res = results[k:k + len(rows)]
        k += len(rows)
        out[f"{tag}__rows"] = rows
        out[f"{tag}__entropy"] = np.stack([x[0] for x in res])
        out[f"{tag}__bits"] = np.stack([x[1] for x in res])
        out[f"{tag}__total"] = np.stack([x[2] for x in res])
        out[f"{tag}__samples"] = np.stack([x[3] for x in res], axis=1)
        out[f"{tag}__divergence"] = np.stack([divergence(x[1], x[2], x[3] > 0) for x in res])
        d = out[f"{tag}__divergence"]
        print(tag, len(rows), "rows, max D", float(np.nanmax(d)), "NaN entries", int(np.isnan(d).sum()), flush=True)
    np.savez_compressed(OUT / "g18_user_divergence.npz", **out)
    print("wrote", OUT / "g18_user_divergence.npz", (OUT / "g18_user_divergence.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
