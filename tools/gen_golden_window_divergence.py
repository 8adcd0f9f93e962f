#!/usr/bin/env python3
"""Golden G19: the REAL reference behind the window-to-window divergence (include/vet.h: vet_window_divergence).

TEST INFRASTRUCTURE ONLY, CPU only; no test runs it.  It imports the reference the way tools/gen_golden_user_divergence.py does
(an empty ``pyvista`` stand-in, the reference's ``src`` on the path), takes golden G14's "absent" dataset (``mu_absent`` /
``mv_absent`` of tests/golden/g14_windowed.npz: 8 viewers x 300 frames, viewer 2 away for frames 50..89 and viewer 5 for frames
200..239), feeds it through the reference's own ingest, and for every kept row r of a (window, stride, max_lag) shape and every
lag l = 1 .. max_lag with r + l < R calls the reference's ``compute_spatial_entropy`` (naive case:
``compute_naive_spatial_entropy``) on three dicts, once per lattice: the present samples of row r (frames
[r * stride, r * stride + window), frame-major then user order), those of row r + l, and both (row r's then row r + l's; keys
``f"{side}_{frame}_{viewer}"``: unique per (side, frame, viewer), so overlapping windows hold their shared frames twice).  From
each returned dict it takes the total W (the sum of the values in dict order) and S = -sum (x / W) log2(x / W) over the values in
dict order — the reference's ``entropy`` before the normaliser — and

    D_k(r, l) = S_both - (W_r S_r + W_{r+l} S_{r+l}) / (W_r + W_{r+l}),       D = mean over the lattices of D_k

NaN where r + l >= R.  Arrays only are stored.

    python tools/gen_golden_window_divergence.py [--reference /root/reference/src] [--jobs 8]

tests/golden/g19_window_divergence.npz
    <case>__rows [m]                      the rows r kept: every row of (20, 20, 14); of the other shapes every 7th row and the
                                          last max_lag + 1 rows that have a partner (R - 2 - max_lag .. R - 2: the last whole band
                                          and every band the end of the video cuts); the three-lattice case keeps the same rows
    <case>__bits [m][K][L][3]             S of the dict of (row r, row r + l, both); <case>__total [m][K][L][3] its W
    <case>__divergence [m][L]             D
    <case>__samples [m]                   present samples of row r
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
SHAPES = ((20, 20, 14), (20, 5, 8), (5, 1, 6), (1, 1, 3))          # (window, stride, max_lag)
CASES = (("w", True, [50]), ("w", True, [50, 100, 200]), ("u", False, [50]))
NAIVE = (10, 20)                                       # tile_height, tile_width

_S = {}


def n_rows(T: int, w: int, s: int) -> int:
    return (T - w) // s + 1


def kept_rows(T: int, w: int, s: int, L: int) -> np.ndarray:
    R = n_rows(T, w, s)
    if (w, s, L) == SHAPES[0]:
        return np.arange(R - 1)                                    # every row that has a partner
    return np.unique(np.concatenate([np.arange(0, R - 1, 7), np.arange(max(0, R - 2 - L), R - 1)]))


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


def _row_dict(df, cols, side: str, f0: int, w: int):
    out = {}
    for f in range(f0, f0 + w):                                    # frame-major, then user order
        row = df.iloc[f]
        for u, c in enumerate(cols):
            if row[c] is not None:
                out[f"{side}_{f}_{u}"] = row[c]
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
    """One (case, shape, row): (bits[K][L][3], total[K][L][3], samples of the row)."""
    from viewport_entropy_toolkit.config import EntropyConfig
    from viewport_entropy_toolkit.utilities import (compute_naive_spatial_entropy, compute_spatial_entropy,
                                                    generate_fibonacci_lattice)
    kind, flag, tcs, w, s, L, r = job
    cfg = EntropyConfig(use_weight_distribution=flag)
    vectors, points, cols = _S["frames"]
    R = n_rows(len(vectors), w, s)
    lattices = [None] if kind == "naive" else [generate_fibonacci_lattice(tc) for tc in tcs]
    df = points if kind == "naive" else vectors
    K = len(lattices)
    bits, tot = np.full((K, L, 3), np.nan), np.zeros((K, L, 3))

    def terms(d, lat):
        if not d:
            return np.nan, 0.0                                     # the reference raises ValidationError on the empty dict
        _, weights, _ = (compute_naive_spatial_entropy(d, NAIVE[0], NAIVE[1], cfg) if kind == "naive" else
                         compute_spatial_entropy(d, lat, cfg))
        return _bits(weights)

    a = _row_dict(df, cols, "a", r * s, w)
    with np.errstate(all="ignore"):
        for k, lat in enumerate(lattices):
            own_a = terms(a, lat)
            for l in range(1, L + 1):
                if r + l >= R:
                    break
                b = _row_dict(df, cols, "b", (r + l) * s, w)
                bits[k, l - 1, 0], tot[k, l - 1, 0] = own_a
                bits[k, l - 1, 1], tot[k, l - 1, 1] = terms(b, lat)
                if a and b:
                    both = dict(a)
                    both.update(b)
                    assert len(both) == len(a) + len(b)            # keys unique per (side, frame, viewer)
                    bits[k, l - 1, 2], tot[k, l - 1, 2] = terms(both, lat)
    return bits, tot, len(a)


def divergence(bits, tot):
    """D[L] from the three-term tables [K][L][3] (the docstring's formula)."""
    with np.errstate(all="ignore"):
        Dk = bits[..., 2] - (tot[..., 0] * bits[..., 0] + tot[..., 1] * bits[..., 1]) / (tot[..., 0] + tot[..., 1])
    return Dk.sum(axis=0) / bits.shape[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default="/root/reference/src")
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    if not Path(args.reference).exists():
        sys.exit(f"reference not found at {args.reference}; nothing to do")
    T = dataset()[1].shape[0]
    cases = []
    for w, s, L in SHAPES:
        rows = kept_rows(T, w, s, L)
        for flag_tag, flag, tcs in CASES:
            cases.append((f"{flag_tag}_tc{'_'.join(map(str, tcs))}_w{w}_s{s}_l{L}", "fib", flag, tcs, w, s, L, rows))
        cases.append((f"naive_h{NAIVE[0]}_w{NAIVE[1]}_w{w}_s{s}_l{L}", "naive", True, None, w, s, L, rows))
    jobs = [(kind, flag, tcs, w, s, L, int(r)) for _, kind, flag, tcs, w, s, L, rows in cases for r in rows]
    cost = lambda j: -j[3] * j[5] * sum(j[2] or [10])                                               # the long ones first
    jobs_sorted = sorted(range(len(jobs)), key=lambda i: cost(jobs[i]))
    with Pool(args.jobs, initializer=_init, initargs=(args.reference,)) as pool:
        done = pool.map(_work, [jobs[i] for i in jobs_sorted], chunksize=1)
    results = [None] * len(jobs)
    for i, res in zip(jobs_sorted, done):
        results[i] = res
    out, k = {}, 0
    for tag, kind, flag, tcs, w, s, L, rows in cases:
        res = results[k:k + len(rows)]
        k += len(rows)
        out[f"{tag}__rows"] = rows
        out[f"{tag}__bits"] = np.stack([x[0] for x in res])
        out[f"{tag}__total"] = np.stack([x[1] for x in res])
        out[f"{tag}__samples"] = np.array([x[2] for x in res], dtype=np.int32)
        out[f"{tag}__divergence"] = np.stack([divergence(x[0], x[1]) for x in res])
        d = out[f"{tag}__divergence"]
        print(tag, len(rows), "rows, D in", float(np.nanmin(d)), float(np.nanmax(d)), "NaN entries", int(np.isnan(d).sum()),
              flush=True)
    np.savez_compressed(OUT / "g19_window_divergence.npz", **out)
    print("wrote", OUT / "g19_window_divergence.npz", (OUT / "g19_window_divergence.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
