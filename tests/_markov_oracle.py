"""numpy oracles of the windowed Markov transition statistics (include/vet.h: vet_transition_markov), built on
tests/_window_transition_oracle.tiles_of (oracle.vet_oracle's quantiser and nearest tiles) only.

A video of T frames has T - lag pairs; pair f is (frame f, frame f + lag).  Row r of (window, stride) covers pairs
[r * stride, r * stride + window); a (pair, user) is pooled when the user has a sample in both frames.  With n_pc the pooled samples
per (source tile, destination tile), n_p and m_c its row and column sums and N its total, per lattice:

    rate = H(c | p)    stationary = H(p)    dest = H(c)    mutual = dest - rate    stay = sum_p n_pp / N

then the mean over the lattices.

``literal``  the collections.Counter walk in the textbook form (sum of p log2(1 / p) terms, math.fsum) — what
             tools/gen_golden_markov.py applies to the real reference's tile pairs (golden G24).
``fast``     np.unique(keys, return_counts=True) in the form the kernels evaluate: f(k) = k log2 k on integers,
             rate = (A - B) / N with A and B over the sources of at least two distinct destinations only.
Both return (stats[5][m], samples[m], matrix[m][n_0][n_0]): lattice 0's dense counts are exact integers.  An empty row is five NaN
with N = 0 and a zero matrix.
"""
import math
from collections import Counter

import numpy as np

from oracle import vet_oracle as vo
from tests._window_transition_oracle import tiles_of  # noqa: F401  (re-exported: callers build the tiles once)

STATS = ("rate", "stationary", "dest", "mutual", "stay")


def n_rows(T, window, stride, lag):
    return (T - lag - window) // stride + 1


def pooled(near, f0, window, lag):
    """(source tiles, destination tiles) of the row's pooled samples"""
    p, c = near[f0:f0 + window], near[f0 + lag:f0 + lag + window]
    both = (p >= 0) & (c >= 0)
    return p[both], c[both]


def literal_row(p, c, n):
    N = len(p)
    if N == 0:
        return (math.nan,) * 5
    pairs = list(zip(p.tolist(), c.tolist()))
    n_pc, n_p, m_c = Counter(pairs), Counter(p.tolist()), Counter(c.tolist())
    rate = math.fsum((n_p[a] / N) * math.fsum((k / n_p[a]) * math.log2(n_p[a] / k) for (a2, _), k in n_pc.items() if a2 == a)
                     for a in n_p)
    stationary = math.fsum((k / N) * math.log2(N / k) for k in n_p.values())
    dest = math.fsum((k / N) * math.log2(N / k) for k in m_c.values())
    stay = sum(k for (a, b), k in n_pc.items() if a == b) / N
    return rate, stationary, dest, dest - rate, stay


def _f(k):
    k = np.asarray(k, dtype=np.float64)
    return k * np.log2(np.where(k > 0, k, 1.0))


def fast_row(p, c, n):
    N = len(p)
    if N == 0:
        return (math.nan,) * 5
    keys, n_pc = np.unique(p.astype(np.int64) * n + c, return_counts=True)
    a, b = keys // n, keys % n
    n_p = np.bincount(a, weights=n_pc, minlength=n)
    m_c = np.bincount(b, weights=n_pc, minlength=n)
    several = np.bincount(a, minlength=n) >= 2                 # sources with at least two distinct destinations
    A, B = _f(n_p[several]).sum(), _f(n_pc[several[a]]).sum()
    rate = (A - B) / N
    stationary = math.log2(N) - _f(n_p).sum() / N
    dest = math.log2(N) - _f(m_c).sum() / N
    return rate, stationary, dest, dest - rate, n_pc[a == b].sum() / N


def _series(row_fn, mu, mv, W, H, tile_counts, window, stride, lag, rows=None, tiles=None):
    tiles = tiles_of(mu, mv, W, H, tile_counts) if tiles is None else tiles
    window = len(mu) - lag if window is None else window
    rows = np.arange(n_rows(len(mu), window, stride, lag)) if rows is None else np.asarray(rows)
    n = [len(vo.fibonacci_lattice(int(tc))) for tc in tile_counts]          # tiles per lattice (not the nominal count)
    stats = np.zeros((5, len(rows)))
    samples = np.zeros(len(rows), dtype=np.int32)
    matrix = np.zeros((len(rows), n[0], n[0]), dtype=np.int32)
    for i, r in enumerate(rows):
        for k, near in enumerate(tiles):
            p, c = pooled(near, int(r) * stride, window, lag)
            if k == 0:
                samples[i] = len(p)
                np.add.at(matrix[i], (p, c), 1)
            stats[:, i] += row_fn(p, c, n[k])
    return stats / len(tiles), samples, matrix


def literal(mu, mv, W, H, tile_counts, window, stride, lag=1, rows=None, tiles=None):
    return _series(literal_row, mu, mv, W, H, tile_counts, window, stride, lag, rows, tiles)


def fast(mu, mv, W, H, tile_counts, window, stride, lag=1, rows=None, tiles=None):
    return _series(fast_row, mu, mv, W, H, tile_counts, window, stride, lag, rows, tiles)
