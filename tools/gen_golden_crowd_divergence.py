#!/usr/bin/env python3
"""Golden G20: the REAL reference behind the viewer-to-crowd divergence (include/vet.h: vet_crowd_divergence).

TEST INFRASTRUCTURE ONLY, CPU only; no test runs it.  It imports the reference the way tools/gen_golden_user_divergence.py does
(an empty ``pyvista`` stand-in, the reference's ``src`` on the path), takes golden G16's dataset (``mu`` / ``mv`` of
tests/golden/g16_user_entropy.npz: 8 viewers x 300 frames, viewer 3 away for frames 100..199), feeds it through the reference's
own ingest, and for every kept row r of a (window, stride) pair calls the reference's ``compute_spatial_entropy`` (naive case:
``compute_naive_spatial_entropy``), once per lattice, on

  * the dict of viewer u alone: the viewer's present samples of frames [r * stride, r * stride + window) in ascending frame
    order, for every viewer with a sample (the dict vet_user_entropy's row stands for), and
  * the pooled dict: every present (frame, viewer) sample of those frames, frame-major then viewer order (the dict
    vet_spatial_entropy_windowed's row stands for).

From a returned weight dict h it takes the total W (the sum of the values in dict order) and S = -sum (x / W) log2(x / W) over the
values in dict order — the reference's ``entropy`` before the normaliser.  With h_u, W_u a viewer's and P, W_r the pooled dict's,

    D_k(u, r)  = sum over the keys t of h_u, in dict order, of q_t log2(q_t / p_t),   q_t = h_u[t] / W_u,  p_t = P[t] / W_r
    pooled_k   = S(P),   within_k = sum_u (W_u / W_r) S(h_u),   between_k = sum_u (W_u / W_r) D_k(u, r)      (present viewers, in order)

and D, pooled, within, between are the means over the lattices.  NaN: D where the viewer has no sample in the row (the reference
raises ValidationError on the empty dict), where S(h_u) is NaN and where S(P) is NaN; the three row series where the row has no
sample or S(P) is NaN, within and between also where a present viewer's S(h_u) is NaN.  Arrays only are stored.

    python tools/gen_golden_crowd_divergence.py [--reference /root/reference/src] [--jobs 8]

tests/golden/g20_crowd_divergence.npz
    <case>__rows [m]                      the rows r kept (golden G18's subset: the ends and the rows around viewer 3's absence)
    <case>__own_bits [m][K][8]            S(h_u), <case>__own_total [m][K][8] W_u, <case>__kl [m][K][8] D_k(u, r)
    <case>__pooled_bits [m][K]            S(P), <case>__pooled_total [m][K] W_r
    <case>__pooled_entropy [m][K]         the reference's RETURNED (normalised) entropy of the pooled dict
    <case>__divergence [8][m]             D
    <case>__series [3][m]                 pooled, within, between
    <case>__samples [8][m]
  case = G16's: {w|u}_tc<counts>_w<window>_s<stride> and naive_h10_w20_w<window>_s<stride>.
"""
from __future__ import annotations

import argparse
import sys
from multiprocessing import Pool
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import gen_golden_user_divergence as g18  # noqa: E402  (the same ingest, dataset, cases and rows)

OUT = g18.OUT
NAIVE = g18.NAIVE


def _terms(weights: dict):
    total = 0.0
    for x in weights.values():
        total += x
    s = 0.0
    for x in weights.values():
        q = x / total
        s -= q * np.log2(q)
    return float(s), float(total)


def _kl(own: dict, w_u: float, pooled: dict, w_r: float) -> float:
    d = 0.0
    for t, x in own.items():
        q = x / w_u
        d += q * np.log2(q / (pooled[t] / w_r))
    return float(d)


def _work(job):
    """One (case, row): (own_bits[K][U], own_total[K][U], kl[K][U], pooled_bits[K], pooled_total[K], pooled_entropy[K],
    samples[U])."""
    from viewport_entropy_toolkit.config import EntropyConfig
    from viewport_entropy_toolkit.utilities import (compute_naive_spatial_entropy, compute_spatial_entropy,
                                                    generate_fibonacci_lattice)
    kind, flag, tcs, w, s, r = job
    cfg = EntropyConfig(use_weight_distribution=flag)
    vectors, points, cols = g18._S["frames"]
    U = len(cols)
    lattices = [None] if kind == "naive" else [generate_fibonacci_lattice(tc) for tc in tcs]
    df = points if kind == "naive" else vectors
    K = len(lattices)
    own_bits, own_tot, kl = (np.full((K, U), np.nan) for _ in range(3))
    p_bits, p_tot, p_ent = (np.full(K, np.nan) for _ in range(3))
    own = [g18._row_dict(df, cols, [u], r * s, w) for u in range(U)]
    pooled = {}
    for f in range(r * s, r * s + w):                               # frame-major, then viewer order
        for u in range(U):
            v = df[cols[u]].iloc[f]
            if v is not None:
                pooled[f"{u}_{f}"] = v
    assert len(pooled) == sum(len(x) for x in own)

    def run(d, L):
        return compute_naive_spatial_entropy(d, NAIVE[0], NAIVE[1], cfg) if kind == "naive" else compute_spatial_entropy(d, L, cfg)

    with np.errstate(all="ignore"):
        for k, L in enumerate(lattices):
            if not pooled:
                continue
            e, P, _ = run(pooled, L)
            p_ent[k] = float(e)
            p_bits[k], p_tot[k] = _terms(P)
            for u in range(U):
                if not own[u]:
                    continue
                _, h, _ = run(own[u], L)
                own_bits[k, u], own_tot[k, u] = _terms(h)
                assert set(h) <= set(P)
                kl[k, u] = _kl(h, own_tot[k, u], P, p_tot[k])
                if np.isnan(own_bits[k, u]) or np.isnan(p_bits[k]):
                    kl[k, u] = np.nan
    return own_bits, own_tot, kl, p_bits, p_tot, p_ent, np.array([len(x) for x in own], dtype=np.int32)


def combine(own_bits, own_tot, kl, p_bits, p_tot, present):
    """(D[U], series[3]) of one row from the per-lattice terms (the docstring's formulas)."""
    K, U = kl.shape
    D, series = np.zeros(U), np.zeros(3)
    with np.errstate(all="ignore"):
        for k in range(K):
            D += kl[k]
            within = between = 0.0
            for u in np.flatnonzero(present):
                m = own_tot[k, u] / p_tot[k]
                within += m * own_bits[k, u]
                between += m * kl[k, u]
            row = np.array([p_bits[k], within, between])
            if not present.any() or np.isnan(p_bits[k]):
                row[:] = np.nan
            series += row
    D /= K
    D[~present] = np.nan
    return D, series / K


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default="/root/reference/src")
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    if not Path(args.reference).exists():
        sys.exit(f"reference not found at {args.reference}; nothing to do")
    cases = []
    for w, s in g18.SHAPES:
        rows = np.array(g18.ROWS[(w, s)], dtype=np.int64)
        for flag_tag, flag, tcs in g18.CASES:
            cases.append((f"{flag_tag}_tc{'_'.join(map(str, tcs))}_w{w}_s{s}", "fib", flag, tcs, w, s, rows))
        cases.append((f"naive_h{NAIVE[0]}_w{NAIVE[1]}_w{w}_s{s}", "naive", True, None, w, s, rows))
    jobs = [(kind, flag, tcs, w, s, int(r)) for _, kind, flag, tcs, w, s, rows in cases for r in rows]
    jobs_sorted = sorted(range(len(jobs)), key=lambda i: -jobs[i][3] * len(jobs[i][2] or [0]))      # the long ones first
    with Pool(args.jobs, initializer=g18._init, initargs=(args.reference,)) as pool:
        done = pool.map(_work, [jobs[i] for i in jobs_sorted], chunksize=1)
    results = [None] * len(jobs)
    for i, res in zip(jobs_sorted, done):
        results[i] = res
    out, k = {}, 0
    names = ("own_bits", "own_total", "kl", "pooled_bits", "pooled_total", "pooled_entropy")
    for tag, kind, flag, tcs, w, s, rows in cases:
        res = results[k:k + len(rows)]
        k += len(rows)
        out[f"{tag}__rows"] = rows
        for i, name in enumerate(names):
            out[f"{tag}__{name}"] = np.stack([x[i] for x in res])
        out[f"{tag}__samples"] = np.stack([x[6] for x in res], axis=1)
        both = [combine(x[0], x[1], x[2], x[3], x[4], x[6] > 0) for x in res]
        out[f"{tag}__divergence"] = np.stack([b[0] for b in both], axis=1)
        out[f"{tag}__series"] = np.stack([b[1] for b in both], axis=1)
        d, sr = out[f"{tag}__divergence"], out[f"{tag}__series"]
        print(tag, len(rows), "rows, max D", float(np.nanmax(d)), "NaN entries", int(np.isnan(d).sum()), "between",
              float(np.nanmin(sr[2])), "..", float(np.nanmax(sr[2])), "identity",
              float(np.nanmax(np.abs(sr[0] - sr[1] - sr[2]))), flush=True)
    np.savez_compressed(OUT / "g20_crowd_divergence.npz", **out)
    print("wrote", OUT / "g20_crowd_divergence.npz", (OUT / "g20_crowd_divergence.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
