"""Oracle of the fixation and tile-dwell events (include/vet.h: vet_fixations), from the definition alone: plain Python loops per
viewer over the direction ids.

The pair (f, f + 1) of a viewer HOLDS when the viewer is present in both frames and
  mode 0  the ids are equal, the Vectors are equal as numbers, or c = fma(A.z, B.z, fma(A.y, B.y, A.x * B.x)) >= cos_threshold for
          the unit vectors A, B — tests/_motion_oracle.py's exact ``fma`` (one rounding) and the same-Vector rule, as
          tests/_cluster_oracle.frame_near decides NEAR;
  mode 1  both samples have the same nearest tile t of lattice 0 (``Plan.read_nearest(0)``), t < n.
A RUN is a maximal interval of present frames whose pairs all hold; an EVENT a run of at least min_frames frames; it belongs to the
row that holds its START, with its full length.

``hold_angle``   ([T - 1][U] HOLD, [T - 1][U] c — NaN where the cosine decides nothing) from a direction table and ids [T][U]
``hold_tile``    [T - 1][U] HOLD from the nearest-tile table
``margin``       the smallest |c - cos_threshold| over the deciding cosines
``runs``         per viewer the list of (start, L) of every run
``result``       dict(counts, hist, labels, offsets, events, centroids) shaped as Plan.fixations returns them
"""
import numpy as np

from tests._cluster_oracle import unit_rows
from tests._motion_oracle import fma, grid_table, ids_of  # noqa: F401  (re-exported for the tests)

STATS = ("samples", "fix_frames", "events", "sum_len", "max_len")


def hold_angle(table, ids, cos_threshold):
    table = np.asarray(table, dtype=np.float64)
    ids = np.asarray(ids)
    T, U = ids.shape
    unit = unit_rows(table)
    hold, c = np.zeros((max(T - 1, 0), U), dtype=bool), np.full((max(T - 1, 0), U), np.nan)
    memo = {}
    for u in range(U):
        for f in range(T - 1):
            a, b = int(ids[f, u]), int(ids[f + 1, u])
            if a < 0 or b < 0:
                continue
            if a == b:
                hold[f, u] = True
                continue
            key = (min(a, b), max(a, b))
            if key not in memo:
                A, B = unit[key[0]], unit[key[1]]
                same_vec = bool((table[key[0]] == table[key[1]]).all())
                cc = float(fma(A[2], B[2], fma(A[1], B[1], A[0] * B[0])))
                memo[key] = (same_vec or cc >= cos_threshold, np.nan if same_vec else cc)
            hold[f, u], c[f, u] = memo[key]
    return hold, c


def hold_tile(nearest, n, ids):
    ids = np.asarray(ids)
    T, U = ids.shape
    hold = np.zeros((max(T - 1, 0), U), dtype=bool)
    for u in range(U):
        for f in range(T - 1):
            a, b = int(ids[f, u]), int(ids[f + 1, u])
            if a >= 0 and b >= 0:
                ta, tb = int(nearest[a]), int(nearest[b])
                hold[f, u] = ta == tb and ta < n
    return hold


def margin(c, cos_threshold):
    """the smallest |c - cos_threshold| over the cosines that decide a pair (NaN entries decide nothing); inf if there is none"""
    v = np.asarray(c)[~np.isnan(c)]
    return float(np.abs(v - cos_threshold).min()) if len(v) else float("inf")


def runs(ids, hold):
    """per viewer u the list of (start, L) of the runs, in frame order"""
    ids = np.asarray(ids)
    T, U = ids.shape
    out = []
    for u in range(U):
        mine, f = [], 0
        while f < T:
            if ids[f, u] < 0:
                f += 1
                continue
            s = f
            while f + 1 < T and ids[f + 1, u] >= 0 and hold[f, u]:
                f += 1
            mine.append((s, f - s + 1))
            f += 1
        out.append(mine)
    return out


def n_rows(T, window, stride):
    return (T - window) // stride + 1


def result(ids, hold, window=None, stride=1, min_frames=5, per_user=False, edges=None, table=None):
    ids = np.asarray(ids)
    T, U = ids.shape
    window = T if window is None else window
    R = n_rows(T, window, stride)
    all_runs = runs(ids, hold)
    labels = np.full((U, T), -1, dtype=np.int32)
    events, offsets = [], np.zeros(U + 1, dtype=np.int64)
    for u in range(U):
        for s, L in all_runs[u]:
            labels[u, s:s + L] = L if L >= min_frames else 0
            if L >= min_frames:
                events.append((u, s, L, int(ids[s + (L - 1) // 2, u])))
        offsets[u + 1] = len(events)
    # the rows, straight from the per-sample arrays: the label, and L at the start of every event
    start_len = np.zeros((U, T), dtype=np.int64)
    for u, s, L, _ in events:
        start_len[u, s] = L
    B = 0 if edges is None else len(edges) - 1
    per = np.zeros((5, U, R), dtype=np.int64)
    per_hist = np.zeros((U, R, B), dtype=np.int32)
    for r in range(R):
        lab, sl = labels[:, r * stride:r * stride + window], start_len[:, r * stride:r * stride + window]
        per[:, :, r] = [(lab >= 0).sum(axis=1), (lab > 0).sum(axis=1), (sl > 0).sum(axis=1), sl.sum(axis=1), sl.max(axis=1)]
        for k in range(B):
            per_hist[:, r, k] = ((sl >= edges[k]) & (sl < edges[k + 1])).sum(axis=1)
    counts = per if per_user else np.concatenate([per[:4].sum(axis=1), per[4:].max(axis=1)])
    hist = None if edges is None else per_hist if per_user else per_hist.sum(axis=0, dtype=np.int32)
    out = dict(counts=counts, hist=hist, labels=labels, offsets=offsets,
               events=np.array(events, dtype=np.int32).reshape(-1, 4), centroids=None)
    if table is not None:
        unit = unit_rows(table)
        cen = np.zeros((len(events), 3))
        for i, (u, s, L, _) in enumerate(events):
            x = y = z = 0.0
            for f in range(s, s + L):
                A = unit[ids[f, u]]
                x, y, z = x + float(A[0]), y + float(A[1]), z + float(A[2])
            cen[i] = (x, y, z)
        out["centroids"] = cen
    return out
