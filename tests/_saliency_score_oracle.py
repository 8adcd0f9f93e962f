"""numpy oracle of the saliency scoring (include/vet.h: vet_saliency_score), from the definition alone.

A row's list (distinct ids ascending, multiplicities m, N) is tests/_saliency_similarity_oracle.py's ``lists``; the audience's map
(scale 2) and its mass are tests/_saliency_oracle.py's ``Oracle.row``; the pixel expressions of cc, sim, jsd and kl are
tests/_saliency_similarity_oracle.py's ``compare`` with a = the audience's map, b = the predicted map.  New here: ``sample`` (the
predicted map at a direction by bilinear interpolation on the cell-centre grid, columns wrapping, rows clamping, in the header's
a + t * (b - a) form), the location metrics with plain ``np.sum``, and the AUC written twice — ``auc_ranks`` (the definition's
per-map-row ``searchsorted`` form; the tests take this one) and ``auc_ranks_brute`` (an O(entries x pixels) comparison).

``auc_gap(v, P)`` is the guard of every AUC comparison against the GPU: the smallest |v_i - P_p| / max P over unequal pairs.  The
counts #{P < v} and #{P == v} are integers; an interpolated value within rounding of a cell's value (but not equal to it) would make
them depend on the last bit of atan2 / acos.  The tests assert ``auc_gap >= GAP_MIN`` on the oracle's own values before they compare:
a condition on the inputs, not a tolerance.
"""
import numpy as np

from tests import _saliency_oracle as so
from tests import _saliency_similarity_oracle as sso

STATS = ("auc", "nss", "info_gain", "cc", "sim", "jsd", "kl", "mass", "mass_pred")
GAP_MIN = 1e-9


def sample(P, unit):
    """v [n]: the map P [H][W] at the unit vectors [n][3]"""
    P, unit = np.asarray(P, dtype=np.float64), np.asarray(unit, dtype=np.float64).reshape(-1, 3)
    H, W = P.shape
    x, y, z = unit[:, 0], unit[:, 1], unit[:, 2]
    lon = np.where((x == 0) & (y == 0), 0.0, np.arctan2(y, x))
    fx = (lon + np.pi) / (2 * np.pi) * W - 0.5
    c0f = np.floor(fx)
    tx = fx - c0f
    c0 = c0f.astype(np.int64) % W
    c1 = (c0 + 1) % W
    fy = np.clip(np.arccos(np.clip(z, -1.0, 1.0)) / np.pi * H - 0.5, 0.0, H - 1.0)
    y0f = np.floor(fy)
    ty = fy - y0f
    y0 = y0f.astype(np.int64)
    y1 = np.minimum(y0 + 1, H - 1)
    top = P[y0, c0] + tx * (P[y0, c1] - P[y0, c0])
    bot = P[y1, c0] + tx * (P[y1, c1] - P[y1, c0])
    return top + ty * (bot - top)


def auc_ranks(v, P, a_y):
    """u [n] = L(v) + 0.5 * E(v), the definition's form: per map row the sorted values, a lower and an upper bound, integer
    counts; the y sums ascending as acc = acc + a_y * count"""
    v, P = np.asarray(v), np.asarray(P)
    L, E = np.zeros(len(v)), np.zeros(len(v))
    for y in range(P.shape[0]):
        s = np.sort(P[y])
        lo, hi = np.searchsorted(s, v, side="left"), np.searchsorted(s, v, side="right")
        L = L + a_y[y] * lo.astype(np.float64)
        E = E + a_y[y] * (hi - lo).astype(np.float64)
    return L + 0.5 * E


def auc_ranks_brute(v, P, a_y):
    """the same by comparing every entry with every pixel"""
    v, P = np.asarray(v), np.asarray(P)
    lt = (P[None, :, :] < v[:, None, None]).sum(axis=2)
    eq = (P[None, :, :] == v[:, None, None]).sum(axis=2)
    L, E = np.zeros(len(v)), np.zeros(len(v))
    for y in range(P.shape[0]):
        L = L + a_y[y] * lt[:, y].astype(np.float64)
        E = E + a_y[y] * eq[:, y].astype(np.float64)
    return L + 0.5 * E


def auc_gap(v, P):
    """the smallest |v_i - P_p| / max P over the pairs with v_i != P_p; inf without such a pair"""
    v, P = np.asarray(v).reshape(-1), np.asarray(P).reshape(-1)
    if not len(v):
        return np.inf
    s = np.sort(P)
    hi = np.searchsorted(s, v, side="right")                     # the first value above v, the last value below v
    lo = np.searchsorted(s, v, side="left") - 1
    above = np.where(hi < len(s), s[np.minimum(hi, len(s) - 1)] - v, np.inf)
    below = np.where(lo >= 0, v - s[np.maximum(lo, 0)], np.inf)
    d = float(np.minimum(above, below).min())
    return d / float(P.max()) if np.isfinite(d) else np.inf


class Oracle:
    def __init__(self, table, W, H):
        self.o = so.Oracle(table, W, H)
        self.W, self.H = W, H
        self.a_y = so.cell_area(W, H)

    def row(self, ids_row, P, sigma, distribution=True):
        """dict(map [npix] | None, stats [9], counts [2], v, gap) of one row from its ids [frames][U] and its predicted map [H][W]"""
        P = np.asarray(P, dtype=np.float64).reshape(self.H, self.W)
        a_pix, Pf = self.o.a_pix, P.reshape(-1)
        uniq, m = sso.lists(ids_row, len(self.o.unit))
        N = int(m.sum())
        stats = np.full(9, np.nan)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            mass_p = np.sum(Pf * a_pix)
            d = Pf - mass_p
            var_p = np.sum(a_pix * (d * d))
            stats[8] = mass_p
            aud = self.o.row(ids_row, sigma, 2) if distribution else None
            if N == 0:
                return dict(map=None if aud is None else aud["map"], stats=stats, counts=np.array([0, 0], dtype=np.int64),
                            v=np.zeros(0), gap=np.inf)
            v = sample(P, self.o.unit[uniq])
            u = auc_ranks(v, P, self.a_y)
            md = m.astype(np.float64)
            stats[0] = np.sum(md * u) / float(N)
            stats[1] = (np.sum(md * v) / float(N) - mass_p) / np.sqrt(var_p)
            stats[2] = np.sum(md * np.log2(v / mass_p)) / float(N)
            if distribution:
                mass = aud["stats"][0]
                _, _, five = sso.compare(aud["map"], Pf, mass, mass_p, a_pix)
                stats[3:7] = five[:4]
                stats[7] = mass
        return dict(map=None if aud is None else aud["map"], stats=stats, counts=np.array([N, len(uniq)], dtype=np.int64), v=v,
                    gap=auc_gap(v, P))

    def rows(self, ids, maps, window, stride, sigma, distribution=True, only=None):
        """dict(map [R][H][W] | None, stats [9][R], counts [2][R], gap) shaped as Plan.saliency_score returns them; ``maps`` [H][W]
        or [R][H][W]; ``only``: the row indices to evaluate (the others are left out of the arrays); gap: the smallest of the rows"""
        ids, maps = np.asarray(ids), np.asarray(maps)
        T = ids.shape[0]
        window = T if window is None else window
        rs = list(range(so.n_rows(T, window, stride))) if only is None else list(only)
        got = [self.row(ids[r * stride:r * stride + window], maps if maps.ndim == 2 else maps[r], sigma, distribution) for r in rs]
        return dict(map=np.stack([g["map"] for g in got]).reshape(len(rs), self.H, self.W) if distribution else None,
                    stats=np.stack([g["stats"] for g in got], axis=1), counts=np.stack([g["counts"] for g in got], axis=1),
                    gap=min([g["gap"] for g in got], default=np.inf))


def density_map(oracle, ids, sigma, seed, n=None):
    """The tests' predicted maps, [H][W] (n None) or [n][H][W]: the video's own whole-video density, plus a quarter of its mean,
    times 1 + 5 % uniform noise — a plausible prediction whose values are all distinct and positive"""
    dens = oracle.o.row(ids, sigma, 2)["map"].reshape(oracle.H, oracle.W)
    base = dens + 0.25 * dens.mean()
    rng = np.random.default_rng(seed)
    shape = (oracle.H, oracle.W) if n is None else (n, oracle.H, oracle.W)
    return np.ascontiguousarray(base * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, size=shape)))
