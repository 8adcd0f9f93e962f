"""numpy oracle of the audience dispersion (include/vet.h: vet_dispersion), from the definition alone.

A pair sample is (frame f, {u, v}), u < v, both viewers present in f; its angle is tests/_motion_oracle.py's ``vector_angles`` of
the two Vectors (the definition's fused dot in exact integer arithmetic with one rounding per fma; +0.0 where the Vectors are equal
as numbers).  Each distinct (id, id) pair is evaluated once.  Rows pool the pair samples of frames [r * stride, r * stride + window)
or hold them from one viewer's side.

``frame_angles``  [T][U][U] angles (NaN: absent, the diagonal, or a NaN angle) and the same-Vector mask, from a direction table
                  [D][3] (``Plan.read_dirs()``, or ``grid_table``) and direction ids [T][U] (-1 absent)
``rows``          per row np.sum / N, np.max, the nearest-partner mean, half-open bins, counts and the centroid
"""
import numpy as np

from tests._motion_oracle import grid_table, ids_of, vector_angles  # noqa: F401  (re-exported for the tests)


def frame_angles(table, ids):
    """([T][U][U] angles, NaN where either viewer is absent and on the diagonal; [T][U][U] same-Vector mask)"""
    ids = np.asarray(ids)
    T, U = ids.shape
    a = np.broadcast_to(ids[:, :, None], (T, U, U))
    b = np.broadcast_to(ids[:, None, :], (T, U, U))
    both = (a >= 0) & (b >= 0) & ~np.eye(U, dtype=bool)[None]
    ang, same = np.full((T, U, U), np.nan), np.zeros((T, U, U), dtype=bool)
    lo, hi = np.minimum(a[both], b[both]), np.maximum(a[both], b[both])      # a(u, v) = a(v, u): one evaluation per unordered pair
    pairs, inverse = np.unique(np.stack([lo, hi], axis=1), axis=0, return_inverse=True)
    if len(pairs):
        p_ang, p_same = vector_angles(table[pairs[:, 0]], table[pairs[:, 1]])
        ang[both], same[both] = p_ang[inverse.reshape(-1)], p_same[inverse.reshape(-1)]
    return ang, same


def unit_vectors(table, ids):
    """[T][U][3]: Vector / |Vector| of every present sample, 0 where absent (or where the unit vector is NaN)"""
    table = np.asarray(table, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = table / np.sqrt((table * table).sum(axis=-1, keepdims=True))
    ids = np.asarray(ids)
    out = np.where((ids >= 0)[..., None], unit[np.maximum(ids, 0)], 0.0)
    return np.where(np.isnan(out).any(axis=-1, keepdims=True), 0.0, out)


def n_rows(T, window, stride):
    return (T - window) // stride + 1


def _hist(vals, edges):
    e = np.asarray(edges, dtype=np.float64)
    return np.array([((vals >= e[b]) & (vals < e[b + 1])).sum() for b in range(len(e) - 1)], dtype=np.int64)


def _row(ang, present, unit, edges, upper):
    """one row from ang [w][n][U] (the angles of the row's frames from the side of n viewers), present [w][n], unit [w][n][3];
    ``upper``: pooled — each pair sample once (the entries above the diagonal), else every entry"""
    vals = ang[:, np.triu(np.ones(ang.shape[1:], dtype=bool), 1)] if upper else ang
    vals = vals[~np.isnan(vals)]
    N = len(vals)
    has = ~np.isnan(ang).all(axis=-1)                             # (frame, viewer) with a partner
    slots = int(has.sum())
    counts = np.array([N, int((vals == 0.0).sum()), slots, int(present.sum())], dtype=np.int64)
    centroid = unit[present].reshape(-1, 3).sum(axis=0) if present.any() else np.zeros(3)
    hist = None if edges is None else _hist(vals, edges)
    if N == 0:
        return np.full(3, np.nan), centroid, hist, counts
    nearest = np.nanmin(ang[has], axis=-1)
    return np.array([vals.sum() / N, vals.max(), nearest.sum() / slots]), centroid, hist, counts


def rows(ang, ids, table, window, stride, per_user=False, edges=None, only=None, users=None):
    """dict(stats, centroid, hist, counts) shaped as Plan.dispersion returns them; ``only``: the row indices r to evaluate,
    ``users``: the viewers of the per-viewer layout to evaluate (the others are left out of the arrays)"""
    ids = np.asarray(ids)
    T, U = ids.shape
    window = T if window is None else window
    R = n_rows(T, window, stride)
    rs = list(range(R)) if only is None else list(only)
    us = list(range(U)) if users is None else list(users)
    present, unit = ids >= 0, unit_vectors(table, ids)
    out = dict(stats=[], centroid=[], hist=[], counts=[])
    for u in (us if per_user else [None]):
        for r in rs:
            f = slice(r * stride, r * stride + window)
            if per_user:
                s, c, h, k = _row(ang[f, u:u + 1], present[f, u:u + 1], unit[f, u:u + 1], None, False)
            else:
                s, c, h, k = _row(ang[f], present[f], unit[f], edges, True)
            out["stats"].append(s); out["centroid"].append(c); out["hist"].append(h); out["counts"].append(k)
    lead = (len(us), len(rs)) if per_user else (len(rs),)
    return dict(stats=np.moveaxis(np.array(out["stats"]).reshape(*lead, 3), -1, 0),
                centroid=np.array(out["centroid"]).reshape(*lead, 3),
                hist=None if edges is None or per_user else np.array(out["hist"], dtype=np.int64).reshape(*lead, len(edges) - 1),
                counts=np.moveaxis(np.array(out["counts"], dtype=np.int64).reshape(*lead, 4), -1, 0))


def counts(ang, ids, window, stride, per_user=False):
    """the [4][R] (or [4][U][R]) integers of every row by running sums"""
    ids = np.asarray(ids)
    T, U = ids.shape
    window = T if window is None else window
    first = np.arange(0, T - window + 1, stride)
    ok = ~np.isnan(ang)
    per = [ok.sum(axis=-1), (ang == 0.0).sum(axis=-1), ok.any(axis=-1), ids >= 0]      # [T][U] each, from every viewer's side

    def windows(x, halve):
        c = np.concatenate([np.zeros((1, U), dtype=np.int64), np.cumsum(x.astype(np.int64), axis=0)])
        w = (c[first + window] - c[first]).T                     # [U][R]
        return w if per_user else (w.sum(axis=0) // 2 if halve else w.sum(axis=0))

    return np.stack([windows(per[0], True), windows(per[1], True), windows(per[2], False), windows(per[3], False)])
