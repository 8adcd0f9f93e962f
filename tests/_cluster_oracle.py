"""numpy oracle of the viewer clusters (include/vet.h: vet_viewer_clusters), from the definition alone.

In a frame two present viewers are NEAR when their direction ids are equal, their Vectors are equal as numbers, or
c = fma(A.z, B.z, fma(A.y, B.y, A.x * B.x)) >= cos_threshold for the unit vectors A, B — tests/_motion_oracle.py's exact ``fma`` (one
rounding), the helper the dispersion and saliency oracles use.  In a row a pair is LINKED when co >= 1 and
float(near) >= min_share * float(co); the clusters are the connected components (a plain union-find), relabelled by their smallest
member; the rest is computed directly.

``frame_near``  [T][U][U] NEAR and the cosines c (NaN: absent, the diagonal), from a direction table [D][3] and ids [T][U] (-1 absent)
``rows``        per row labels, sizes, counts, top, stats, centroids and the link words, shaped as Plan.viewer_clusters returns them
"""
import numpy as np

from tests._motion_oracle import fma, grid_table, ids_of  # noqa: F401  (re-exported for the tests)


def unit_rows(table):
    table = np.asarray(table, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return table / np.sqrt((table * table).sum(axis=-1, keepdims=True))


def frame_near(table, ids, cos_threshold):
    """([T][U][U] NEAR, [T][U][U] c — NaN where either viewer is absent, on the diagonal, and for equal ids, which are NEAR by rule)"""
    table = np.asarray(table, dtype=np.float64)
    ids = np.asarray(ids)
    T, U = ids.shape
    unit = unit_rows(table)
    a = np.broadcast_to(ids[:, :, None], (T, U, U))
    b = np.broadcast_to(ids[:, None, :], (T, U, U))
    both = (a >= 0) & (b >= 0) & ~np.eye(U, dtype=bool)[None]
    near, c = np.zeros((T, U, U), dtype=bool), np.full((T, U, U), np.nan)
    lo, hi = np.minimum(a[both], b[both]), np.maximum(a[both], b[both])      # symmetric: one evaluation per unordered pair of ids
    keys, inverse = np.unique(lo.astype(np.int64) * len(table) + hi, return_inverse=True)
    pairs = np.stack([keys // len(table), keys % len(table)], axis=1)
    if len(pairs):
        A, B = unit[pairs[:, 0]], unit[pairs[:, 1]]
        same_id = pairs[:, 0] == pairs[:, 1]
        same_vec = (table[pairs[:, 0]] == table[pairs[:, 1]]).all(axis=-1)
        pc = np.full(len(pairs), np.nan)
        d = ~same_id
        pc[d] = fma(A[d, 2], B[d, 2], fma(A[d, 1], B[d, 1], A[d, 0] * B[d, 0]))
        with np.errstate(invalid="ignore"):
            pn = same_id | same_vec | (pc >= cos_threshold)
        inverse = inverse.reshape(-1)
        near[both], c[both] = pn[inverse], np.where(same_vec, np.nan, pc)[inverse]
    return near, c


def margin(c, cos_threshold):
    """the smallest |c - cos_threshold| over the cosines that decide a pair (NaN entries decide nothing); inf if there is none"""
    v = c[~np.isnan(c)]
    return float(np.abs(v - cos_threshold).min()) if len(v) else float("inf")


def n_rows(T, window, stride):
    return (T - window) // stride + 1


def components(linked, viewers):
    """labels [U]: the connected components of ``linked`` on the ``viewers`` mask, numbered by smallest member; -1 elsewhere"""
    U = len(viewers)
    parent = list(range(U))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for u, v in zip(*np.nonzero(np.triu(linked, 1))):
        ru, rv = find(int(u)), find(int(v))
        if ru != rv:
            parent[max(ru, rv)] = min(ru, rv)
    labels, dense = np.full(U, -1, dtype=np.int32), {}
    for u in range(U):                                           # ascending u: a root is met first at its smallest member
        if viewers[u]:
            labels[u] = dense.setdefault(find(u), len(dense))
    return labels


def link_words(linked):
    """[U][ceil(U / 64)] uint64: bit v mod 64 of word v // 64 of row u"""
    U = linked.shape[0]
    words = (U + 63) // 64
    padded = np.zeros((U, words * 64), dtype=np.uint64)
    padded[:, :U] = linked
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    return (padded.reshape(U, words, 64) * weights).sum(axis=-1, dtype=np.uint64)


def row(near, ids, unit, min_share, fractions):
    """one row from near [w][U][U], ids [w][U], the unit table"""
    present = ids >= 0
    U = ids.shape[1]
    both = present[:, :, None] & present[:, None, :] & ~np.eye(U, dtype=bool)[None]
    co, nr = both.sum(axis=0), (near & both).sum(axis=0)
    linked = (co >= 1) & (nr.astype(np.float64) >= min_share * co.astype(np.float64))
    viewers = present.any(axis=0)
    labels = components(linked, viewers)
    P, K = int(viewers.sum()), int(labels.max()) + 1 if viewers.any() else 0
    sizes = np.zeros(U, dtype=np.int32)
    sizes[:K] = np.bincount(labels[labels >= 0], minlength=K)[:K] if K else 0
    s = sizes[:K].astype(np.float64)
    order = sorted(range(K), key=lambda k: (-int(sizes[k]), k))
    running = np.cumsum([int(sizes[k]) for k in order])
    top = np.array([int(np.argmax(running.astype(np.float64) >= f * float(P))) + 1 if P else 0 for f in fractions], dtype=np.int32)
    counts = np.array([P, K, int(sizes.max(initial=0)), int((sizes == 1).sum()), int(np.triu(linked, 1).sum())], dtype=np.int64)
    if P:
        H = np.log2(float(P)) - float((s * np.log2(s)).sum()) / float(P)
        stats = np.array([H, H / np.log2(float(P)) if P > 1 else np.nan, float(counts[2]) / float(P)])
    else:
        stats = np.full(3, np.nan)
    centroids = np.zeros((U, 3))
    for k in range(K):
        members = labels == k
        vec = unit[np.maximum(ids[:, members], 0)]                       # [w][m][3]: frame-major, viewer ascending
        vec = np.where((present[:, members])[..., None] & ~np.isnan(vec).any(axis=-1, keepdims=True), vec, 0.0).reshape(-1, 3)
        centroids[k] = np.cumsum(np.concatenate([np.zeros((1, 3)), vec]), axis=0)[-1]        # a sequential sum from +0.0
    return dict(labels=labels, sizes=sizes, counts=counts, top=top, stats=stats, centroids=centroids, links=link_words(linked))


def rows(near, ids, table, window, stride, min_share=1.0, fractions=(0.5, 0.8, 0.95), only=None):
    """dict(labels [R][U], sizes [R][U], counts [5][R], top [R][Q], stats [3][R], centroids [R][U][3], links [R][U][words]);
    ``only``: the row indices to evaluate"""
    ids = np.asarray(ids)
    T, U = ids.shape
    window = T if window is None else window
    rs = list(range(n_rows(T, window, stride))) if only is None else list(only)
    unit = unit_rows(table)
    got = [row(near[r * stride:r * stride + window], ids[r * stride:r * stride + window], unit, min_share, fractions) for r in rs]
    out = {k: np.stack([g[k] for g in got]) for k in ("labels", "sizes", "top", "centroids", "links")}
    out["counts"] = np.stack([g["counts"] for g in got], axis=1)
    out["stats"] = np.stack([g["stats"] for g in got], axis=1)
    return out
