"""numpy oracle of the saliency maps (include/vet.h: vet_saliency), from the definition alone.

The map is W x H cells, equirectangular, row 0 at the top: column c at lon = (c + 0.5) / W * 360 - 180, row y at lat = 90 -
(y + 0.5) / H * 180; P is the unrounded Vector.from_spherical of the cell centre, normalised; a_y the cell's share of the sphere.
A row's LIST is np.unique of its present direction ids with their counts.  c = fma(P.z, A.z, fma(P.y, A.y, P.x * A.x)) with
tests/_motion_oracle.py's exact ``fma`` (one rounding), k = np.exp(kappa * (c - 1)), S the sequential sum of m * k over the list in
ascending id (fma(m, k, S); a plain addition where m = 1, which is the same number), M = S * g.  Statistics with plain np.sum.

``Oracle(table, W, H)`` caches the cosines per direction id, so the rows of a video evaluate each (pixel, id) once.
"""
import numpy as np

from tests._motion_oracle import fma, grid_table, ids_of  # noqa: F401  (re-exported for the tests)


def cell_centres(W, H):
    """(P [H * W][3] row-major unit vectors, lon [W], lat [H]) of the cell centres"""
    lon = (np.arange(W) + 0.5) / W * 360.0 - 180.0
    lat = 90.0 - (np.arange(H) + 0.5) / H * 180.0
    theta, phi = np.radians(lon), np.radians(90.0 - lat)
    x = np.sin(phi)[:, None] * np.cos(theta)[None, :]
    y = np.sin(phi)[:, None] * np.sin(theta)[None, :]
    z = np.broadcast_to(np.cos(phi)[:, None], (H, W))
    length = np.sqrt(x * x + y * y + z * z)
    return np.stack([x / length, y / length, z / length], axis=-1).reshape(-1, 3), lon, lat


def cell_area(W, H):
    """a_y [H]: the share of the sphere of one cell of row y; W * a.sum() is 1"""
    y = np.arange(H)
    return (np.cos(np.pi * y / H) - np.cos(np.pi * (y + 1) / H)) / (2 * W)


def unit_rows(vectors):
    v = np.asarray(vectors, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))


def cosines(P, A):
    """[len(P)][len(A)]: the definition's fused dot of unit vectors P and A"""
    P, A = np.asarray(P)[:, None, :], np.asarray(A)[None, :, :]
    return fma(P[..., 2], A[..., 2], fma(P[..., 1], A[..., 1], P[..., 0] * A[..., 0]))


def scale_factor(scale, kappa, N):
    """g_r: None at scale 0 (no multiply), 1 / N, or C / N"""
    if scale == 0:
        return None
    if scale == 1:
        return 1.0 / float(N)
    return (kappa / (2.0 * np.pi * (1.0 - np.exp(-2.0 * kappa)))) / float(N)


def n_rows(T, window, stride):
    return (T - window) // stride + 1


def row_stats(M, a_pix):
    """(mass, peak, entropy, area), peak_index of one map [npix] (a row with samples)"""
    w = M * a_pix
    wsum = np.sum(w)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = w / wsum
        t = np.where(w == 0, 0.0, q * np.log2(q / a_pix))
    ent = -np.sum(t)
    return np.array([wsum, M.max(), ent, np.exp2(ent)]), int(np.argmax(M))


class Oracle:
    def __init__(self, table, W, H):
        self.W, self.H = W, H
        self.unit = unit_rows(table)
        self.P, self.lon, self.lat = cell_centres(W, H)
        self.a_pix = np.repeat(cell_area(W, H), W)
        self._cos = {}

    def cos(self, ids):
        """[npix][len(ids)]"""
        new = [int(i) for i in ids if int(i) not in self._cos]
        if new:
            c = cosines(self.P, self.unit[new])
            for j, i in enumerate(new):
                self._cos[i] = c[:, j]
        if not len(ids):
            return np.zeros((len(self.P), 0))
        return np.stack([self._cos[int(i)] for i in ids], axis=1)

    def row(self, present_ids, sigma, scale):
        """dict(S, map, stats, peak, samples, distinct) of one row from its present ids (any order, -1 dropped)"""
        ids = np.asarray(present_ids).reshape(-1)
        ids = ids[(ids >= 0) & (ids < len(self.unit))]
        uniq, m = np.unique(ids, return_counts=True)
        kappa = 1.0 / (sigma * sigma)
        S = np.zeros(len(self.P))
        c = self.cos(uniq)
        for j in range(len(uniq)):
            k = np.exp(kappa * (c[:, j] - 1.0))
            S = S + k if m[j] == 1 else fma(float(m[j]), k, S)
        N = int(m.sum())
        if N == 0:
            return dict(S=S, map=S, stats=np.full(4, np.nan), peak=-1, samples=0, distinct=0)
        g = scale_factor(scale, kappa, N)
        M = S if g is None else S * g
        stats, peak = row_stats(M, self.a_pix)
        return dict(S=S, map=M, stats=stats, peak=peak, samples=N, distinct=len(uniq))

    def rows(self, ids, window, stride, sigma, scale, per_user=False, only=None, users=None):
        """dict(S, map, stats, peak, counts) shaped as Plan.saliency returns them; ``only``: the row indices r to evaluate,
        ``users``: the viewers of the per-viewer layout to evaluate (the others are left out of the arrays)"""
        ids = np.asarray(ids)
        T, U = ids.shape
        window = T if window is None else window
        rs = list(range(n_rows(T, window, stride))) if only is None else list(only)
        us = list(range(U)) if users is None else list(users)
        got = []
        for u in (us if per_user else [None]):
            for r in rs:
                f = slice(r * stride, r * stride + window)
                got.append(self.row(ids[f, u] if per_user else ids[f], sigma, scale))
        lead = (len(us), len(rs)) if per_user else (len(rs),)
        return dict(S=np.array([g["S"] for g in got]).reshape(*lead, self.H, self.W),
                    map=np.array([g["map"] for g in got]).reshape(*lead, self.H, self.W),
                    stats=np.moveaxis(np.array([g["stats"] for g in got]).reshape(*lead, 4), -1, 0),
                    peak=np.array([g["peak"] for g in got], dtype=np.int32).reshape(lead),
                    counts=np.moveaxis(np.array([[g["samples"], g["distinct"]] for g in got], dtype=np.int64).reshape(*lead, 2), -1, 0))


def off_centre(mu, mv):
    """golden G15's walk starts at the centre of the frame, on the equator and on lon 0: on a map of even height a sample at lat 0 lies
    on the border of two cell rows, whose centres are then equally near and hold the same value — a tie of the peak; a sample at lon 0
    likewise on a map of even width.  The saliency tests move the video by an eighth of the width and 13 % of the height (NaN stays
    NaN), between the borders of 36- and 18-column maps, which keeps its shape and its absences."""
    return np.clip(np.asarray(mu) + 0.125, 0.0, 1.0), np.clip(np.asarray(mv) + 0.13, 0.0, 1.0)


def peak_margin(maps):
    """per map [..., H, W]: (largest - second largest) / largest, NaN for an all-zero map"""
    flat = np.asarray(maps).reshape(-1, maps.shape[-2] * maps.shape[-1])
    top = np.sort(flat, axis=1)[:, -2:]
    with np.errstate(invalid="ignore", divide="ignore"):
        return ((top[:, 1] - top[:, 0]) / top[:, 1]).reshape(maps.shape[:-2])
