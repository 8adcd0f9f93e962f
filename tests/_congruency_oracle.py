"""numpy oracle of the viewer congruency (include/vet.h: vet_congruency), from the definition alone, on top of
tests/_saliency_oracle.py (``unit_rows``, ``cosines``, ``scale_factor``, the ``np.unique`` lists).

A row's pooled list is np.unique of its present ids with counts m; viewer u's own list is np.unique of the viewer's column with
counts a (spread over the pooled list's positions, 0 where the viewer does not hold the direction).  w = m - a in integers, N' = N - n_u.
S_i = sum_j w_j * exp(kappa * (c_ij - 1)), f_i = S_i * (C / N'); lift = 4 pi * sum a_i f_i / n_u; info_gain = sum a_i log2(4 pi f_i) /
n_u; nss = (sum a_i f_i / n_u - mu) / sqrt(v), mu = 1 / (4 pi), v = (C / N')^2 * Q_u / (4 pi) - mu^2.  Q_u is the DIRECT double sum
w . G . w here — the library walks T_i = sum_j m_j G_ij and O_i = sum_{j own} a_j G_ij and takes Q - 2 B_u + A_u, so this is an
independent check of that decomposition (``split_forms`` evaluates it in numpy for the surface test).  Plain ``np.sum`` / matrix
products throughout.

The cosines c_ij are ``cosines`` (the definition's fused dot, exact) for lists of up to ``EXACT_PAIRS`` pairs and the unfused numpy
dot beyond, as in tests/_saliency_similarity_oracle.py: two more roundings of c (<= 2 * 2**-53 absolute) change exp(kappa * (c - 1))
by at most kappa * 2.3e-16 relative — 7.3e-13 at sigma 1 degree — far inside the GPU tests' 1e-10.  Pairs are evaluated in blocks of
``BLOCK`` list entries, so the largest lists of the tests (about 7 000 directions) stay under 200 MB.
"""
import numpy as np

from tests import _saliency_oracle as so

STATS = ("lift", "info_gain", "nss")
EXACT_PAIRS = 20000
BLOCK = 1024
FOUR_PI = 4.0 * np.pi


def overlap(c, kappa):
    """G(c): the integral over the sphere of the product of two kernels whose centres have cosine c"""
    c = np.asarray(c, dtype=np.float64)
    r = np.sqrt(np.maximum(0.0, 2.0 + 2.0 * c))
    x = kappa * r
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        main = 2.0 * np.pi * np.exp(kappa * (r - 2.0)) * (-np.expm1(-2.0 * x)) / x
        small = FOUR_PI * np.exp(-2.0 * kappa) * (1.0 + x * x / 6.0)
    return np.where(x < 1e-4, small, main)


def lists(ids_row, n_dirs):
    """(uniq [n], m [n], A [U][n]) of a row's ids [frames][U]: the pooled list and every viewer's own multiplicities on it"""
    ids_row = np.asarray(ids_row)
    ok = (ids_row >= 0) & (ids_row < n_dirs)
    uniq, m = np.unique(ids_row[ok], return_counts=True)
    A = np.zeros((ids_row.shape[1], len(uniq)), dtype=np.int64)
    for u in range(ids_row.shape[1]):
        own, a = np.unique(ids_row[:, u][ok[:, u]], return_counts=True)
        A[u, np.searchsorted(uniq, own)] = a
    return uniq, m.astype(np.int64), A


def pair_blocks(unit, uniq):
    """yields (slice, c [block][n]) over the pooled list"""
    X = unit[uniq]
    exact = len(uniq) * len(uniq) <= EXACT_PAIRS
    for i0 in range(0, len(uniq), BLOCK):
        sl = slice(i0, min(i0 + BLOCK, len(uniq)))
        if exact:
            yield sl, so.cosines(X[sl], X)
        else:
            Y = X[sl]
            yield sl, Y[:, None, 2] * X[None, :, 2] + (Y[:, None, 1] * X[None, :, 1] + Y[:, None, 0] * X[None, :, 0])


def split_forms(m, A, G):
    """(Q_u by the direct sum w G w, Q_u as Q - 2 B_u + A_u) [U] from the pooled m [n], the own A [U][n] and G [n][n]"""
    m, A = m.astype(np.float64), A.astype(np.float64)
    w = m[None, :] - A
    direct = np.einsum("ui,ij,uj->u", w, G, w)
    T = G @ m                                                    # T_i = sum_j m_j G_ij
    O = A @ G.T                                                  # O_ui = sum_j a_uj G_ij
    B, Au = (A * T[None, :]).sum(axis=1), (A * O).sum(axis=1)
    Q = np.sum(m * T)
    return direct, Q - 2.0 * B + Au


class Oracle:
    def __init__(self, table):
        self.unit = so.unit_rows(table)

    def row(self, ids_row, sigma, nss=True):
        """dict(stats [3][U], counts [3][U], row [4], Q [U]) of one row from its ids [frames][U]"""
        U = np.asarray(ids_row).shape[1]
        kappa = 1.0 / (sigma * sigma)
        uniq, m, A = lists(ids_row, len(self.unit))
        N, n_u = int(m.sum()), A.sum(axis=1)
        others = N - n_u
        counts = np.stack([n_u, (A > 0).sum(axis=1), others]).astype(np.int64)
        stats = np.full((3, U), np.nan)
        scored = (n_u > 0) & (others > 0)
        Wt = (m[None, :] - A).astype(np.float64)                 # w_j per viewer
        S = np.zeros((U, len(uniq)))
        Qu = np.zeros(U)
        for sl, c in pair_blocks(self.unit, uniq):
            with np.errstate(under="ignore"):
                S[:, sl] = Wt @ np.exp(kappa * (c - 1.0)).T
            if nss:
                Qu += np.einsum("ui,ij,uj->u", Wt[:, sl], overlap(c, kappa), Wt)
        mu = 1.0 / FOUR_PI
        for u in np.flatnonzero(scored):
            own = A[u] > 0
            a = A[u, own].astype(np.float64)
            g = so.scale_factor(2, kappa, int(others[u]))
            f = S[u, own] * g
            with np.errstate(invalid="ignore", divide="ignore"):
                F = np.sum(a * f)
                stats[0, u] = FOUR_PI * F / float(n_u[u])
                stats[1, u] = np.sum(a * np.log2(FOUR_PI * f)) / float(n_u[u])
                if nss:
                    v = g * g * Qu[u] / FOUR_PI - mu * mu
                    if np.isfinite(v) and v > 0:
                        stats[2, u] = (F / float(n_u[u]) - mu) / np.sqrt(v)
        k = int(scored.sum())
        with np.errstate(invalid="ignore", divide="ignore"):
            row = np.array([float(k)] + [np.sum(stats[i, scored]) / float(k) if k else np.nan for i in range(3)])
        return dict(stats=stats, counts=counts, row=row, Q=Qu)

    def rows(self, ids, window, stride, sigma, nss=True, only=None):
        """dict(stats [3][U][R], counts [3][U][R], rows [4][R]) shaped as Plan.congruency returns them; ``only``: the row indices to
        evaluate (the others are left out of the arrays)"""
        ids = np.asarray(ids)
        T = ids.shape[0]
        window = T if window is None else window
        rs = list(range(so.n_rows(T, window, stride))) if only is None else list(only)
        got = [self.row(ids[r * stride:r * stride + window], sigma, nss) for r in rs]
        return dict(stats=np.stack([g["stats"] for g in got], axis=2), counts=np.stack([g["counts"] for g in got], axis=2),
                    rows=np.stack([g["row"] for g in got], axis=1))
