"""numpy oracle of the saliency similarity (include/vet.h: vet_saliency_similarity), from the definition alone.

Audience g of a row is the row's present samples of the viewers labelled g (0 = A, 1 = B).  Its list, N, distinct, map (scale 2) and
mass are tests/_saliency_oracle.py's ``Oracle.row`` on those samples.  The pixel sums (va, vb, cov, sim, jsd, kl_ab, kl_ba) are the
definition's expressions with plain ``np.sum``; IEEE gives +inf where an audience has weight on a cell whose other value is 0.0.
NSS by point evaluation: S_i = sum_j m_j * exp(kappa * (c_ij - 1)) over the other audience's list, v_i = m_i * (S_i * g_Y),
nss_xy = (sum_i v_i / N_X - mass_Y) / sqrt(v_Y).  The point cosines c_ij are ``cosines`` (the definition's fused dot, exact) for
lists of up to ``EXACT_PAIRS`` pairs and the unfused numpy dot beyond: the exact fma is a Python loop, and two more roundings of c
(<= 2 * 2**-53 absolute) change exp(kappa * (c - 1)) by at most kappa * 2.3e-16 relative — 7.3e-13 at sigma 1 degree — far inside the
GPU tests' 1e-10.
"""
import numpy as np

from tests import _saliency_oracle as so

STATS = ("cc", "sim", "jsd", "kl_ab", "kl_ba", "nss_ab", "nss_ba", "mass_a", "mass_b")
EXACT_PAIRS = 20000


def compare(Ma, Mb, mass_a, mass_b, a_pix):
    """(va, vb, [cc, sim, jsd, kl_ab, kl_ba]) of two maps [npix] with their masses"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        qa, qb = (Ma * a_pix) / mass_a, (Mb * a_pix) / mass_b
        da, db = Ma - mass_a, Mb - mass_b
        va, vb, cov = np.sum(a_pix * (da * da)), np.sum(a_pix * (db * db)), np.sum(a_pix * (da * db))
        m = 0.5 * (qa + qb)
        ta = np.where(qa != 0, qa * np.log2(qa / m), 0.0)
        tb = np.where(qb != 0, qb * np.log2(qb / m), 0.0)
        kl_ab = np.sum(np.where(qa != 0, qa * np.log2(qa / qb), 0.0))
        kl_ba = np.sum(np.where(qb != 0, qb * np.log2(qb / qa), 0.0))
        return va, vb, [cov / np.sqrt(va * vb), np.sum(np.fmin(qa, qb)), 0.5 * np.sum(ta + tb), kl_ab, kl_ba]


def lists(ids, n_dirs):
    ids = np.asarray(ids).reshape(-1)
    ids = ids[(ids >= 0) & (ids < n_dirs)]
    return np.unique(ids, return_counts=True)


def point_sum(unit, x, mx, y, my, kappa, g_y):
    """V = sum_i m_i * (S_i * g_Y): the density of the list (y, my) at the directions of the list (x, mx)"""
    X, Y = unit[x], unit[y]
    if len(x) * len(y) <= EXACT_PAIRS:
        c = so.cosines(X, Y)
    else:
        c = X[:, None, 2] * Y[None, :, 2] + (X[:, None, 1] * Y[None, :, 1] + X[:, None, 0] * Y[None, :, 0])
    S = np.sum(my[None, :].astype(np.float64) * np.exp(kappa * (c - 1.0)), axis=1)
    return np.sum(mx.astype(np.float64) * (S * g_y))


class Oracle:
    def __init__(self, table, W, H):
        self.o = so.Oracle(table, W, H)
        self.W, self.H = W, H

    def row(self, ids_row, code, sigma):
        """dict(maps [2][npix], stats [9], counts [4]) of one row from its ids [frames][U] and the labels [U]"""
        code = np.asarray(code)
        kappa = 1.0 / (sigma * sigma)
        aud = [self.o.row(np.asarray(ids_row)[:, code == g], sigma, 2) for g in (0, 1)]
        counts = [aud[0]["samples"], aud[1]["samples"], aud[0]["distinct"], aud[1]["distinct"]]
        mass = [a["stats"][0] for a in aud]
        stats = np.full(9, np.nan)
        stats[7:] = mass
        if counts[0] and counts[1]:
            va, vb, stats[:5] = compare(aud[0]["map"], aud[1]["map"], mass[0], mass[1], self.o.a_pix)
            ls = [lists(np.asarray(ids_row)[:, code == g], len(self.o.unit)) for g in (0, 1)]
            for k, (x, y, v_y) in enumerate(((0, 1, vb), (1, 0, va))):
                V = point_sum(self.o.unit, *ls[x], *ls[y], kappa, so.scale_factor(2, kappa, counts[y]))
                with np.errstate(invalid="ignore", divide="ignore"):
                    stats[5 + k] = (V / float(counts[x]) - mass[y]) / np.sqrt(v_y)
        return dict(maps=np.stack([aud[0]["map"], aud[1]["map"]]), stats=stats, counts=np.array(counts, dtype=np.int64))

    def rows(self, ids, code, window, stride, sigma, only=None):
        """dict(maps [2][R][H][W], stats [9][R], counts [4][R]) shaped as Plan.saliency_similarity returns them; ``only``: the row
        indices to evaluate (the others are left out of the arrays)"""
        ids = np.asarray(ids)
        T = ids.shape[0]
        window = T if window is None else window
        rs = list(range(so.n_rows(T, window, stride))) if only is None else list(only)
        got = [self.row(ids[r * stride:r * stride + window], code, sigma) for r in rs]
        return dict(maps=np.stack([g["maps"] for g in got], axis=1).reshape(2, len(rs), self.H, self.W),
                    stats=np.stack([g["stats"] for g in got], axis=1), counts=np.stack([g["counts"] for g in got], axis=1))


def masked(ids, code, g):
    """ids with every viewer not labelled g absent"""
    return np.where((np.asarray(code) == g)[None, :], np.asarray(ids), -1).astype(np.int32)
