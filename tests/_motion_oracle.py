"""numpy oracle of the head-motion statistics (include/vet.h: vet_head_motion), from the definition alone.

A video of T frames has P = T - lag pairs; pair f is (frame f, frame f + lag).  A (pair, viewer) present in both frames is a sample;
its angle is arccos(clip(c, -1, 1)), c = fma(A.z, B.z, fma(A.y, B.y, A.x * B.x)) of the two unit vectors Vector / |Vector| — the
definition's fused dot, evaluated here in exact integer arithmetic with one rounding per fma — and +0.0 where the two Vectors are
equal as numbers (-0.0 == 0.0): still.  Rows pool the samples of pairs [r * stride, r * stride + window) over all viewers, or hold one viewer's own.

``angles``   the [P][U] angles (NaN absent) and the same-Vector mask, from a direction table [D][3] (``Plan.read_dirs()``, or
             ``grid_table`` from oracle.vet_oracle's quantiser) and direction ids [T][U] (-1 absent)
``rows``     per row np.mean, np.std(ddof=1), np.max, np.sum, np.sort plus the interpolation formula, half-open bins
"""
import numpy as np

from oracle import vet_oracle as vo


def grid_table(W, H):
    """[(H + 1) * (W + 1)][3]: the Vector of every pixel, direction id = py * (W + 1) + px"""
    return vo.direction_grid(W, H).reshape(-1, 3)


def ids_of(mu, mv, W, H):
    px, py, present, _ = vo.sample_directions(mu, mv, W, H)
    return np.where(present, py * (W + 1) + px, -1).astype(np.int32)


def fma(a, b, c):
    """round(a * b + c) with ONE rounding, elementwise: the fused multiply-add the definition's dot is written with.  Exact integer
    arithmetic on the floats' (numerator, power-of-two denominator) pairs; Python's int / int is correctly rounded."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    out = np.empty(a.shape, dtype=np.float64)
    flat = out.reshape(-1)
    for i, (x, y, z) in enumerate(zip(a.reshape(-1).tolist(), b.reshape(-1).tolist(), c.reshape(-1).tolist())):
        if x != x or y != y or z != z:
            flat[i] = np.nan
            continue
        (nx, dx), (ny, dy), (nz, dz) = x.as_integer_ratio(), y.as_integer_ratio(), z.as_integer_ratio()
        flat[i] = (nx * ny * dz + nz * dx * dy) / (dx * dy * dz)
    return out


def vector_angles(a, b):
    """(angle, same) of the Vectors a and b [..., 3]: the reference's vector_angle_distance with the definition's dot
    fma(A.z, B.z, fma(A.y, B.y, A.x * B.x)) of the unit vectors, 0 where the Vectors are the same"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        ua = a / np.sqrt((a * a).sum(axis=-1, keepdims=True))
        ub = b / np.sqrt((b * b).sum(axis=-1, keepdims=True))
    c = fma(ua[..., 2], ub[..., 2], fma(ua[..., 1], ub[..., 1], ua[..., 0] * ub[..., 0]))
    raw = np.arccos(np.clip(c, -1.0, 1.0))
    same = (a == b).all(axis=-1)
    return np.where(same, 0.0, raw), same


def raw_angles(a, b):
    """the reference's value without the same-Vector rule: every a[i] against every b[j] -> [m, n]"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ua = a / np.sqrt((a * a).sum(axis=-1, keepdims=True))
    ub = b / np.sqrt((b * b).sum(axis=-1, keepdims=True))
    return np.arccos(np.clip(ua @ ub.T, -1.0, 1.0))


def angles(table, ids, lag):
    """([P][U] angles, NaN where the viewer is absent from either frame; [P][U] same-Vector mask)"""
    ids = np.asarray(ids)
    a, b = ids[:-lag], ids[lag:]
    both = (a >= 0) & (b >= 0)
    ang, same = np.full(a.shape, np.nan), np.zeros(a.shape, dtype=bool)
    pairs, inverse = np.unique(np.stack([a[both], b[both]], axis=1), axis=0, return_inverse=True)    # each (id, id) once
    if len(pairs):
        p_ang, p_same = vector_angles(table[pairs[:, 0]], table[pairs[:, 1]])
        ang[both], same[both] = p_ang[inverse.reshape(-1)], p_same[inverse.reshape(-1)]
    return ang, same


def n_rows(T, window, stride, lag):
    return (T - lag - window) // stride + 1


def quantile(x, q):
    """lerp between the order statistics of the ascending x at position q (N - 1)"""
    pos = q * (len(x) - 1)
    i = int(np.floor(pos))
    if i >= len(x) - 1:
        return x[-1]
    return x[i] + (x[i + 1] - x[i]) * (pos - i)


def row_stats(vals, fractions=(), edges=None):
    """(stats[4], quantiles[Q], hist[B] or None, still, samples) of one row's values (NaN = absent)"""
    x = np.sort(vals[~np.isnan(vals)])
    N = len(x)
    hist = None
    if edges is not None:
        e = np.asarray(edges, dtype=np.float64)
        hist = np.array([((x >= e[b]) & (x < e[b + 1])).sum() for b in range(len(e) - 1)], dtype=np.int32)
    if N == 0:
        return np.full(4, np.nan), np.full(len(fractions), np.nan), hist, 0, 0
    keep = vals[~np.isnan(vals)]                                 # position order for the sums
    with np.errstate(invalid="ignore", divide="ignore"):
        sd = np.std(keep, ddof=1) if N > 1 else np.nan
    stats = np.array([np.mean(keep), sd, x[-1], np.sum(keep)])
    return stats, np.array([quantile(x, q) for q in fractions]), hist, int((x == 0).sum()), N


def counts(ang, window, stride, per_user=False):
    """(samples, still) of every row, [R] or [U][R], by running sums — the integers of all rows at once"""
    P, U = ang.shape
    window = P if window is None else window
    first = np.arange(0, P - window + 1, stride)

    def windows(flags):
        c = np.concatenate([np.zeros((1, U), dtype=np.int64), np.cumsum(flags, axis=0)])
        per = (c[first + window] - c[first]).T                   # [U][R]
        return (per if per_user else per.sum(axis=0)).astype(np.int32)

    return windows(~np.isnan(ang)), windows(ang == 0.0)


def rows(ang, window, stride, per_user=False, fractions=(), edges=None, only=None, users=None):
    """dict(stats, quantiles, hist, still, samples) shaped as Plan.head_motion returns them; ``only``: the row indices r to
    evaluate, ``users``: the viewers of the per-viewer layout to evaluate (the others are left out of the arrays)"""
    P, U = ang.shape
    window = P if window is None else window
    R = (P - window) // stride + 1
    rs = list(range(R)) if only is None else list(only)
    us = list(range(U)) if users is None else list(users)
    views = [ang[:, u:u + 1] for u in us] if per_user else [ang]
    U = len(us)
    out = dict(stats=[], quantiles=[], hist=[], still=[], samples=[])
    for v in views:
        for r in rs:
            s, q, h, still, N = row_stats(v[r * stride:r * stride + window].reshape(-1), fractions, edges)
            out["stats"].append(s); out["quantiles"].append(q); out["hist"].append(h)
            out["still"].append(still); out["samples"].append(N)
    lead = (U, len(rs)) if per_user else (len(rs),)
    res = dict(stats=np.moveaxis(np.array(out["stats"]).reshape(*lead, 4), -1, 0),
               quantiles=np.array(out["quantiles"]).reshape(*lead, len(fractions)),
               hist=None if edges is None else np.array(out["hist"], dtype=np.int32).reshape(*lead, len(edges) - 1),
               still=np.array(out["still"], dtype=np.int32).reshape(lead),
               samples=np.array(out["samples"], dtype=np.int32).reshape(lead))
    return res
