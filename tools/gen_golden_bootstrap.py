#!/usr/bin/env python3
"""Golden G21: the REAL reference on resampled audiences, the samples of a run of frames pooled into one dict.

TEST INFRASTRUCTURE ONLY, CPU only; no test runs it.  It imports the reference the way tools/gen_golden_user_entropy.py does (its
``dataset`` and its ingest are reused: golden G16's dataset, G4's 8 users x 300 frames with the same absences), draws 12 resamples
of the 8 viewers from one fixed seed with a numpy implementation of include/vet.h's counter-based draw, and for every kept row r
of a (window, stride) pair and every replicate b calls the reference's ``compute_spatial_entropy`` on ONE dict that holds an entry
for every present sample of frames [r * stride, r * stride + window) of every drawn viewer — frame-major, then in draw order, keys
``f"{frame}_{draw}"``, a viewer drawn c times entered c times — once per lattice, and takes the mean over the lattices as
``compute_entropy`` does.  A replicate without a sample (the reference raises ValidationError) is stored as NaN.  Arrays only are
stored.

    python tools/gen_golden_bootstrap.py --reference <the reference's src directory> [--jobs 8]

tests/golden/g21_bootstrap.npz
    seed, counts [12][8] uint16, picks [12][8]   the draw (replicate b, draw j -> viewer)
    <case>__rows [m]                the rows r kept ((1, 1): about 40 rows, the ends and the frames around the absent stretch
                                    included; every row otherwise)
    <case>__entropy [m][12], <case>__samples [m][12] (the dict's size)
    <case>__weights [m][12][n_0], <case>__keys [m][12][n_0]     lattice 0's dict, dense — for w_tc50 and u_tc50; w_tc50_100_200's
                                    lattice 0 is w_tc50's (the generator checks that they are equal and stores them once)
  case = {w|u}_tc<counts>_w<window>_s<stride> and naive_h10_w20_w<window>_s<stride> (compute_naive_spatial_entropy, 10 x 20
  degree cells; entropy and samples only).
"""
from __future__ import annotations

import argparse
import sys
from multiprocessing import Pool
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import gen_golden_user_entropy as g16  # noqa: E402  (dataset, ingest through the reference, kept rows)

OUT = g16.OUT
SHAPES = ((1, 1), (20, 20), (20, 7), (300, 1))          # (window, stride)
CASES = g16.CASES
NAIVE = g16.NAIVE
REPLICATES, SEED = 12, 0x5EEDB007


def draw(U: int, B: int, seed: int):
    """include/vet.h's draw: (counts[B][U] uint16, picks[B][U])."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.arange(B * U, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
        picks = (((z >> np.uint64(32)) * np.uint64(U)) >> np.uint64(32)).astype(np.int64).reshape(B, U)
    counts = np.stack([np.bincount(p, minlength=U) for p in picks]).astype(np.uint16)
    return counts, picks


def _row_dict(df, cols, picks_b, f0: int, w: int):
    out = {}
    for f in range(f0, f0 + w):
        for j, u in enumerate(picks_b):
            v = df[cols[u]].iloc[f]
            if v is not None:
                out[f"{f}_{j}"] = v
    return out


def _work(job):
    from viewport_entropy_toolkit.config import EntropyConfig
    from viewport_entropy_toolkit.utilities import (compute_naive_spatial_entropy, compute_spatial_entropy,
                                                    generate_fibonacci_lattice)
    kind, flag, tcs, w, s, picks_b, r = job
    cfg = EntropyConfig(use_weight_distribution=flag)
    vectors, points, cols = g16._S["frames"]
    with np.errstate(all="ignore"):
        if kind == "naive":
            d = _row_dict(points, cols, picks_b, r * s, w)
            if not d:
                return float("nan"), 0, None, None
            e, _, _ = compute_naive_spatial_entropy(d, NAIVE[0], NAIVE[1], cfg)
            return float(e), len(d), None, None
        d = _row_dict(vectors, cols, picks_b, r * s, w)
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
    ap.add_argument("--reference", required=True, help="the reference's src directory")
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    if not Path(args.reference).exists():
        sys.exit(f"reference not found at {args.reference}; nothing to do")
    _, mu, mv = g16.dataset()
    T, U = mu.shape
    counts, picks = draw(U, REPLICATES, SEED)
    assert (counts.sum(axis=1) == U).all()
    out = {"seed": np.uint64(SEED), "counts": counts, "picks": picks}
    cases = []
    for w, s in SHAPES:
        rows = g16.kept_rows((T - w) // s + 1, w, s)
        for flag_tag, flag, tcs in CASES:
            cases.append((f"{flag_tag}_tc{'_'.join(map(str, tcs))}_w{w}_s{s}", "fib", flag, tcs, w, s, rows))
        cases.append((f"naive_h{NAIVE[0]}_w{NAIVE[1]}_w{w}_s{s}", "naive", True, None, w, s, rows))
    jobs = [(kind, flag, tcs, w, s, tuple(int(u) for u in picks[b]), int(r))
            for _, kind, flag, tcs, w, s, rows in cases for r in rows for b in range(REPLICATES)]
    with Pool(args.jobs, initializer=g16._init, initargs=(args.reference,)) as pool:
        results = pool.map(_work, jobs, chunksize=4)
    k = 0
    kept_weights = {}
    for tag, kind, flag, tcs, w, s, rows in cases:
        m = len(rows)
        res = results[k:k + m * REPLICATES]
        k += m * REPLICATES
        out[f"{tag}__rows"] = rows.astype(np.int64)
        out[f"{tag}__entropy"] = np.array([x[0] for x in res], dtype=np.float64).reshape(m, REPLICATES)
        out[f"{tag}__samples"] = np.array([x[1] for x in res], dtype=np.int32).reshape(m, REPLICATES)
        if kind == "fib":
            wts = np.stack([x[2] for x in res]).reshape(m, REPLICATES, -1)
            keys = np.stack([x[3] for x in res]).reshape(m, REPLICATES, -1)
            first = kept_weights.setdefault((flag, tcs[0], w, s), (wts, keys))
            if first[0] is wts:
                out[f"{tag}__weights"], out[f"{tag}__keys"] = wts, keys
            else:                       # the same lattice 0 on the same dicts: stored once
                assert np.array_equal(first[0], wts) and np.array_equal(first[1], keys), tag
        print(tag, m, "rows, mean", float(np.nanmean(out[f"{tag}__entropy"])), "NaN replicates",
              int(np.isnan(out[f"{tag}__entropy"]).sum()), flush=True)
    path = OUT / "g21_bootstrap.npz"
    np.savez_compressed(path, **out)
    print("wrote", path, path.stat().st_size, "bytes")
    assert path.stat().st_size < 1 << 20


if __name__ == "__main__":
    main()
