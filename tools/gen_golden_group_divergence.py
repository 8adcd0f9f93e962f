#!/usr/bin/env python3
"""Golden G22: the REAL reference on two audiences and on relabellings of them, the samples of a run of frames pooled per audience.

TEST INFRASTRUCTURE ONLY, CPU only; no test runs it.  It imports the reference the way tools/gen_golden_bootstrap.py does
(tools/gen_golden_user_entropy.py's ``dataset`` and ingest are reused: golden G16's dataset, 8 users x 300 frames with absences),
takes the groups [0, 0, 0, 1, 1, 1, 1, -1] (viewer 7 excluded), draws 11 permutations from one fixed seed with a numpy
implementation of include/vet.h's keys, and for every kept row r of a (window, stride) pair and every labelling l (0: the groups
themselves) calls the reference's ``compute_spatial_entropy`` three times per lattice: on ONE dict holding every present sample of
frames [r * stride, r * stride + window) of audience A's viewers — frame-major, then by ascending viewer, keys
``f"{side}_{frame}_{viewer}"`` —, on audience B's, and on a single dict holding both, A before B.  From each returned dict it takes
the total W (the sum of the values in dict order) and S = -sum (x / W) log2(x / W) over the values in dict order — the reference's
``entropy`` before the normaliser — and D_k = S(both) - (W_A S(A) + W_B S(B)) / (W_A + W_B); D is the mean over the lattices.  A
labelling one of whose audiences has no sample in the row (the reference raises ValidationError) is stored as NaN.  Arrays only are
stored.

    python tools/gen_golden_group_divergence.py --reference <the reference's src directory> [--jobs 8]

tests/golden/g22_group_divergence.npz
    seed, groups [8] int8, labels [12][8] uint8 (0 = A, 1 = B, 255 = excluded; row 0 the groups)
    <case>__rows [m]                the rows r kept (golden G16's)
    <case>__divergence [m][12]      D of every labelling; <case>__samples [m][12][2] the two dicts' sizes
    <case>__weights [m][2][n_0], <case>__keys [m][2][n_0]     lattice 0's dicts of the observed A and B, dense — for w_tc50 and
                                    u_tc50; w_tc50_100_200's lattice 0 is w_tc50's (checked equal, stored once)
  case = {w|u}_tc<counts>_w<window>_s<stride> and naive_h10_w20_w<window>_s<stride> (compute_naive_spatial_entropy, 10 x 20
  degree cells; divergence and samples only).
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
SHAPES = ((300, 1), (20, 20), (20, 7), (1, 1))          # (window, stride)
CASES = g16.CASES
NAIVE = g16.NAIVE
GROUPS = (0, 0, 0, 1, 1, 1, 1, -1)
PERMUTATIONS, SEED = 11, 0x6A0B5EED


def draw(groups, P: int, seed: int):
    """include/vet.h's labellings: labels[P + 1][U] uint8."""
    groups = np.asarray(groups, dtype=np.int64)
    inc = np.flatnonzero(groups >= 0)
    N, UA = len(inc), int((groups == 0).sum())
    labels = np.full((P + 1, len(groups)), 255, dtype=np.uint8)
    labels[0] = np.where(groups >= 0, groups, 255)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.arange(P * N, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
        key = ((z >> np.uint64(16)) << np.uint64(16)).reshape(P, N) | np.arange(N, dtype=np.uint64)[None, :]
    for b in range(P):
        order = np.argsort(key[b], kind="stable")
        labels[b + 1, inc[order[:UA]]] = 0
        labels[b + 1, inc[order[UA:]]] = 1
    return labels


def _row_dict(df, cols, side: str, viewers, f0: int, w: int):
    out = {}
    for f in range(f0, f0 + w):
        row = df.iloc[f]
        for u in viewers:
            v = row[cols[u]]
            if v is not None:
                out[f"{side}_{f}_{u}"] = v
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
    """One (case, shape, row, labelling): (D, (samples of A, of B), lattice 0's dense dicts of A and B with their keys)."""
    from viewport_entropy_toolkit.config import EntropyConfig
    from viewport_entropy_toolkit.utilities import (compute_naive_spatial_entropy, compute_spatial_entropy,
                                                    generate_fibonacci_lattice)
    kind, flag, tcs, w, s, label, r = job
    cfg = EntropyConfig(use_weight_distribution=flag)
    vectors, points, cols = g16._S["frames"]
    df = points if kind == "naive" else vectors
    lattices = [None] if kind == "naive" else [generate_fibonacci_lattice(tc) for tc in tcs]
    a = _row_dict(df, cols, "a", [u for u, g in enumerate(label) if g == 0], r * s, w)
    b = _row_dict(df, cols, "b", [u for u, g in enumerate(label) if g == 1], r * s, w)
    both = dict(a)
    both.update(b)
    assert len(both) == len(a) + len(b)                        # keys unique per (side, frame, viewer)
    n0 = 0 if kind == "naive" else len(lattices[0])
    dense, keys = np.zeros((2, n0)), np.zeros((2, n0), dtype=bool)
    total = 0.0
    with np.errstate(all="ignore"):
        for k, lat in enumerate(lattices):
            term = []
            for side, d in enumerate((a, b, both)):
                if not d:
                    term.append((np.nan, 0.0))                 # the reference raises ValidationError on the empty dict
                    continue
                _, weights, _ = (compute_naive_spatial_entropy(d, NAIVE[0], NAIVE[1], cfg) if kind == "naive" else
                                 compute_spatial_entropy(d, lat, cfg))
                term.append(_bits(weights))
                if k == 0 and side < 2 and kind != "naive":
                    idx = {v: i for i, v in enumerate(lat)}
                    for v, x in weights.items():
                        dense[side, idx[v]] = x
                        keys[side, idx[v]] = True
            (sa, wa), (sb, wb), (sp, _) = term
            total += sp - (wa * sa + wb * sb) / (wa + wb)
    return float(total / len(lattices)) if a and b else float("nan"), (len(a), len(b)), dense, keys


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="the reference's src directory")
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    if not Path(args.reference).exists():
        sys.exit(f"reference not found at {args.reference}; nothing to do")
    _, mu, mv = g16.dataset()
    T, U = mu.shape
    labels = draw(GROUPS, PERMUTATIONS, SEED)
    assert ((labels == 0).sum(axis=1) == 3).all() and ((labels == 1).sum(axis=1) == 4).all() and (labels[:, 7] == 255).all()
    L = len(labels)
    out = {"seed": np.uint64(SEED), "groups": np.array(GROUPS, dtype=np.int8), "labels": labels}
    cases = []
    for w, s in SHAPES:
        rows = g16.kept_rows((T - w) // s + 1, w, s)
        for flag_tag, flag, tcs in CASES:
            cases.append((f"{flag_tag}_tc{'_'.join(map(str, tcs))}_w{w}_s{s}", "fib", flag, tcs, w, s, rows))
        cases.append((f"naive_h{NAIVE[0]}_w{NAIVE[1]}_w{w}_s{s}", "naive", True, None, w, s, rows))
    jobs = [(kind, flag, tcs, w, s, tuple(int(g) for g in labels[l]), int(r))
            for _, kind, flag, tcs, w, s, rows in cases for r in rows for l in range(L)]
    with Pool(args.jobs, initializer=g16._init, initargs=(args.reference,)) as pool:
        results = pool.map(_work, jobs, chunksize=4)
    k = 0
    kept_weights = {}
    for tag, kind, flag, tcs, w, s, rows in cases:
        m = len(rows)
        res = results[k:k + m * L]
        k += m * L
        out[f"{tag}__rows"] = rows.astype(np.int64)
        out[f"{tag}__divergence"] = np.array([x[0] for x in res], dtype=np.float64).reshape(m, L)
        out[f"{tag}__samples"] = np.array([x[1] for x in res], dtype=np.int32).reshape(m, L, 2)
        if kind == "fib":
            wts = np.stack([res[i * L][2] for i in range(m)])                 # labelling 0 only
            keys = np.stack([res[i * L][3] for i in range(m)])
            first = kept_weights.setdefault((flag, tcs[0], w, s), (wts, keys))
            if first[0] is wts:
                out[f"{tag}__weights"], out[f"{tag}__keys"] = wts, keys
            else:                       # the same lattice 0 on the same dicts: stored once
                assert np.array_equal(first[0], wts) and np.array_equal(first[1], keys), tag
        print(tag, m, "rows, mean", float(np.nanmean(out[f"{tag}__divergence"])), "NaN labellings",
              int(np.isnan(out[f"{tag}__divergence"]).sum()), flush=True)
    path = OUT / "g22_group_divergence.npz"
    np.savez_compressed(path, **out)
    print("wrote", path, path.stat().st_size, "bytes")
    assert path.stat().st_size < 1 << 20


if __name__ == "__main__":
    main()
