#!/usr/bin/env python3
"""Golden G14: the REAL reference on the samples of sliding frame windows pooled into one dict.

TEST INFRASTRUCTURE ONLY, CPU only; no test runs it.  It imports the reference the way oracle/gen_golden.py does (an empty
``pyvista`` stand-in, the reference's ``src`` on the path), feeds golden G4's 8-user x 300-frame dataset (read from
tests/golden/g4_spatial.npz, so the inputs are shared) through the reference's own ingest, and for every kept row r of a
(window, stride) pair calls the reference's ``compute_spatial_entropy`` on ONE dict that holds an entry for every present
(frame, user) sample of frames [r * stride, r * stride + window), frame-major then user order (keys ``f"{frame}:{user}"``),
once per lattice, and takes the mean over the lattices as ``compute_entropy`` does.  Arrays only are stored.

    python tools/gen_windowed_golden.py [--reference /root/reference/src] [--jobs 8]

tests/golden/g14_windowed.npz
    mu, mv [300][8]                 dataset "full" (NaN = absent), frame-major
    mu_absent, mv_absent            the same with user 2 absent in frames 50..89 and user 5 in frames 200..239
    <case>__rows [m]                the rows kept (every 7th row at stride 1, every row otherwise; the last row always)
    <case>__entropy [m], <case>__samples [m]
    <case>__weights_rows [3], <case>__weights [3][n_0], <case>__keys [3][n_0]   lattice 0's dict of three rows, dense
  case = {full|absent}_{w|u}_tc<counts>_w<window>_s<stride>, and naive_{w|u}_h10_w20_w<window>_s<stride> through
  compute_naive_spatial_entropy (10 x 20 degree cells, dataset "full"; entropy and samples only).
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
WINDOWS, STRIDES = (1, 5, 20), (1, 5)
TILE_COUNTS = ([50], [50, 100, 200])
ABSENT = ((2, 50, 90), (5, 200, 240))          # (user, first frame, end frame)
NAIVE = (10, 20)                               # tile_height, tile_width

_S = {}


def kept_rows(R: int, stride: int) -> np.ndarray:
    rows = np.arange(0, R, 7 if stride == 1 else 1)
    return np.unique(np.append(rows, R - 1))


def _init(ref_src: str):
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.dont_write_bytecode = True
    sys.modules.setdefault("pyvista", types.ModuleType("pyvista"))
    sys.path.insert(0, ref_src)
    import viewport_entropy_toolkit  # noqa: F401  (the reference)
    from viewport_entropy_toolkit import AnalyzerConfig, SpatialEntropyAnalyzer
    import pandas as pd
    g4 = np.load(OUT / "g4_spatial.npz")
    times, mus, mvs = g4["time_in"], g4["mu_in"], g4["mv_in"]        # [U][T]
    U, T = mus.shape
    frames = {}
    with tempfile.TemporaryDirectory() as td:
        for name in ("full", "absent"):
            d = Path(td) / name
            d.mkdir()
            for u in range(U):
                keep = np.ones(T, dtype=bool)
                if name == "absent":
                    for au, f0, f1 in ABSENT:
                        if au == u:
                            keep[f0:f1] = False
                pd.DataFrame({"time": times[u][keep], "2dmu": mus[u][keep], "2dmv": mvs[u][keep]}).to_csv(
                    d / f"user{u:03d}.csv", index=False)
            an = SpatialEntropyAnalyzer(AnalyzerConfig(output_dir=Path(td) / "out", tile_counts=[50]))
            an.process_directory(d)
            frames[name] = (an._data_cache["vectors"], an._data_cache["points"])
    _S["frames"] = frames


def _window_dict(df, f0: int, w: int):
    cols = sorted(c for c in df.columns if c != "time")
    out = {}
    for f in range(f0, f0 + w):
        row = df.iloc[f]
        for c in cols:
            if row[c] is not None:
                out[f"{f}:{c}"] = row[c]
    return out


def _work(job):
    from viewport_entropy_toolkit.config import EntropyConfig
    from viewport_entropy_toolkit.utilities import (compute_naive_spatial_entropy, compute_spatial_entropy,
                                                    generate_fibonacci_lattice)
    kind, data, flag, tcs, w, s, r = job
    cfg = EntropyConfig(use_weight_distribution=flag)
    vectors, points = _S["frames"][data]
    with np.errstate(all="ignore"):
        if kind == "naive":
            d = _window_dict(points, r * s, w)
            e, _, _ = compute_naive_spatial_entropy(d, NAIVE[0], NAIVE[1], cfg)
            return float(e), len(d), None, None
        d = _window_dict(vectors, r * s, w)
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
    g4 = np.load(OUT / "g4_spatial.npz")
    mu, mv = g4["mu_in"].T.copy(), g4["mv_in"].T.copy()
    T = mu.shape[0]
    mu_a, mv_a = mu.copy(), mv.copy()
    for u, f0, f1 in ABSENT:
        mu_a[f0:f1, u] = np.nan
        mv_a[f0:f1, u] = np.nan
    out = {"mu": mu, "mv": mv, "mu_absent": mu_a, "mv_absent": mv_a}
    cases = []
    for w in WINDOWS:
        for s in STRIDES:
            rows = kept_rows((T - w) // s + 1, s)
            for flag in (True, False):
                for data in ("full", "absent"):
                    for tcs in TILE_COUNTS:
                        tag = f"{data}_{'w' if flag else 'u'}_tc{'_'.join(map(str, tcs))}_w{w}_s{s}"
                        cases.append((tag, "fib", data, flag, tcs, w, s, rows))
                cases.append((f"naive_{'w' if flag else 'u'}_h{NAIVE[0]}_w{NAIVE[1]}_w{w}_s{s}", "naive", "full", flag, None, w, s, rows))
    jobs = [(kind, data, flag, tcs, w, s, int(r)) for _, kind, data, flag, tcs, w, s, rows in cases for r in rows]
    with Pool(args.jobs, initializer=_init, initargs=(args.reference,)) as pool:
        results = pool.map(_work, jobs, chunksize=4)
    k = 0
    for tag, kind, data, flag, tcs, w, s, rows in cases:
        res = results[k:k + len(rows)]
        k += len(rows)
        out[f"{tag}__rows"] = rows.astype(np.int64)
        out[f"{tag}__entropy"] = np.array([x[0] for x in res], dtype=np.float64)
        out[f"{tag}__samples"] = np.array([x[1] for x in res], dtype=np.int32)
        if kind == "fib":
            pick = [0, len(rows) // 2, len(rows) - 1]
            out[f"{tag}__weights_rows"] = rows[pick].astype(np.int64)
            out[f"{tag}__weights"] = np.stack([res[i][2] for i in pick])
            out[f"{tag}__keys"] = np.stack([res[i][3] for i in pick])
        print(tag, len(rows), "rows, mean", float(np.nanmean(out[f"{tag}__entropy"])), flush=True)
    np.savez_compressed(OUT / "g14_windowed.npz", **out)
    print("wrote", OUT / "g14_windowed.npz", (OUT / "g14_windowed.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
