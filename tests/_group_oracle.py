"""numpy oracles of the two-audience permutation test (include/vet.h: vet_group_divergence), built on oracle.vet_oracle,
tests/_user_oracle.py, tests/_divergence_oracle.py and tests/_window_divergence_oracle.py only.

``groups[U]`` is 0 (audience A), 1 (audience B) or -1 (excluded).  Labelling 0 is ``groups``; labelling b + 1 is permutation b of
the included viewers, which keeps the two group sizes.  The same labelling serves every row and lattice.  Row r of (window,
stride) covers frames [r * stride, r * stride + window).  With A / B the pooled histograms of the two audiences' present samples
of the row, W their totals and S(h) = -sum_keys (h_t / W) log2(h_t / W),

    D_k = S(A + B) - (W_A S(A) + W_B S(B)) / (W_A + W_B),      D = mean over the lattices of D_k   (bits)

``draw``     the labellings in numpy uint64: labels[P + 1][U] uint8 (0, 1, 255 = excluded).
``literal``  the definition: per labelling three calls of ``vo.spatial_entropy_frame`` — on A's directions of the row, on B's, and
             on both (A's then B's; each frame-major, then by ascending viewer) — and S taken back with
             ``_divergence_oracle.bits_of``.  tests/test_group_divergence_surface.py pins it against golden G22 (the real
             reference's dicts).
``fast``     ``_user_oracle.fast``'s per-viewer weights masked and summed, then ``_window_divergence_oracle.band``'s arithmetic on
             the pair (A, B).  Differs from ``literal`` in the association of the FP64 sums only (checked to 1e-12).
``naive``    the same on the counts of compute_naive_spatial_entropy's lat/lon cells.
``summary``  observed, p_value, p_adjusted, null_mean, null_crit and valid from the observed series and the null distribution.
D is NaN where either audience has no sample in the row and where one of the three S is NaN (a key whose sum is 0.0 or whose
proportion underflows to 0).  Results: D[R][P + 1] (column 0 the observed labelling), samples[R][P + 1][2].
"""
import numpy as np

from oracle import vet_oracle as vo
from tests import _divergence_oracle as dvo
from tests import _user_oracle as uo
from tests import _window_divergence_oracle as wdo

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
OUT = 255


def draw(groups, P, seed):
    """labels[P + 1][U] uint8: row 0 is ``groups`` (-1 as 255), row b + 1 permutation b — a function of (seed, b, N) alone."""
    groups = np.asarray(groups, dtype=np.int64)
    inc = np.flatnonzero(groups >= 0)
    N, UA = len(inc), int((groups == 0).sum())
    labels = np.full((P + 1, len(groups)), OUT, dtype=np.uint8)
    labels[0] = np.where(groups >= 0, groups, OUT)
    with np.errstate(over="ignore"):
        i = np.arange(P * N, dtype=np.uint64) + np.uint64(1)
        z = np.uint64(seed) + i * GOLDEN
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
        key = ((z >> np.uint64(16)) << np.uint64(16)).reshape(P, N) | np.arange(N, dtype=np.uint64)[None, :]
    order = np.argsort(key, axis=1, kind="stable")                        # the keys are distinct
    for b in range(P):
        labels[b + 1, inc[order[b, :UA]]] = 0
        labels[b + 1, inc[order[b, UA:]]] = 1
    return labels


def pair(hA, kA, hB, kB):
    """D_k of one lattice from the dense histograms of A and B [..][n] and their key masks: ``band``'s arithmetic on the pair."""
    h = np.stack([hA, hB])
    keys = np.stack([kA, kB])
    return wdo.band(h, keys, 1)[0, 0]


def literal(mu, mv, W, H, tile_counts, window, stride, labels, rows=None, fov_angle=120.0, power_factor=2.0,
            use_weight_distribution=True):
    """(D[m][L], samples[m][L][2]) for ``rows`` (default: every row) and every labelling of ``labels``."""
    did, flat = uo.direction_ids(mu, mv, W, H)
    T = len(did)
    lattices = [vo.fibonacci_lattice(tc) for tc in tile_counts]
    rows = np.arange(uo.n_rows(T, window, stride)) if rows is None else np.asarray(rows)
    Lb, K = len(labels), len(lattices)
    D = np.full((len(rows), Lb), np.nan)
    samples = np.zeros((len(rows), Lb, 2), dtype=np.int32)

    def terms(ids, lat):
        _, hist, _ = vo.spatial_entropy_frame(flat[ids], lat, fov_angle, power_factor, use_weight_distribution)
        _, keys = vo.tile_weight_rows(flat[ids], lat, fov_angle, power_factor, use_weight_distribution, return_keys=True)
        return dvo.bits_of(hist, keys.any(axis=0)), float(hist.sum())

    with np.errstate(all="ignore"):
        for i, r in enumerate(rows):
            blk = did[r * stride:r * stride + window]
            for l in range(Lb):
                a = blk[:, labels[l] == 0].reshape(-1)                            # frame-major, then ascending viewer
                b = blk[:, labels[l] == 1].reshape(-1)
                a, b = a[a >= 0], b[b >= 0]
                samples[i, l] = len(a), len(b)
                if not len(a) or not len(b):
                    continue
                total = 0.0
                for lat in lattices:
                    (sa, wa), (sb, wb), (sp, _) = terms(a, lat), terms(b, lat), terms(np.concatenate([a, b]), lat)
                    total += sp - (wa * sa + wb * sb) / (wa + wb)
                D[i, l] = total / K
    return D, samples


def _from_viewers(h_u, keys_u, s_u, labels):
    """(D_k[R][L], samples[R][L][2]) of one lattice from the per-viewer histograms h_u[U][R][n], key masks and samples s_u[U][R]."""
    U, R, n = h_u.shape
    Lb = len(labels)
    D = np.full((R, Lb), np.nan)
    samples = np.zeros((R, Lb, 2), dtype=np.int32)
    for l in range(Lb):
        mA, mB = labels[l] == 0, labels[l] == 1
        hA, hB = h_u[mA].sum(axis=0), h_u[mB].sum(axis=0)                         # [R][n]
        kA, kB = keys_u[mA].any(axis=0), keys_u[mB].any(axis=0)
        samples[:, l, 0], samples[:, l, 1] = s_u[mA].sum(axis=0), s_u[mB].sum(axis=0)
        for r in range(R):
            if samples[r, l, 0] and samples[r, l, 1]:
                D[r, l] = pair(hA[r], kA[r], hB[r], kB[r])
    return D, samples


def fast(mu, mv, W, H, tile_counts, window, stride, labels, fov_angle=120.0, power_factor=2.0, use_weight_distribution=True,
         want_weights=False):
    """(D[R][L], samples[R][L][2]) for every row; ``want_weights``: also lattice 0's histograms of labelling 0, [R][2][n_0]."""
    D, samples, weights = None, None, None
    with np.errstate(all="ignore"):
        for k, tc in enumerate(tile_counts):
            _, s_u, w_u = uo.fast(mu, mv, W, H, [tc], window, stride, fov_angle, power_factor, use_weight_distribution)
            Dk, samples = _from_viewers(np.abs(w_u), uo.keys_of(w_u), s_u, labels)
            D = Dk if D is None else D + Dk
            if k == 0:
                h = np.abs(w_u)
                weights = np.stack([h[labels[0] == 0].sum(axis=0), h[labels[0] == 1].sum(axis=0)], axis=1)
    D = D / len(tile_counts)
    return (D, samples, weights) if want_weights else (D, samples)


def naive_viewer_hists(mu, mv, W, H, tile_height, tile_width, window, stride, dense_bins=False):
    """The lat/lon cell counts h[U][R][cells] of every viewer and row.  ``dense_bins``: over the bins lon cell * (lat cells) +
    lat cell of the package's naive plan instead of the cells in use."""
    px, py, present, _ = vo.sample_directions(mu, mv, W, H)
    lon_axis, lat_axis = vo.axis_tables(W, H)
    li_axis, lj_axis = vo.naive_tile_indices(lon_axis, lat_axis, tile_height, tile_width)
    n_lat = int(lj_axis.max()) + 1
    cell = np.where(present, li_axis[np.where(present, px, 0)] * n_lat + lj_axis[np.where(present, py, 0)], -1)
    T, U = cell.shape
    R = uo.n_rows(T, window, stride)
    if dense_bins:
        n, index = (int(li_axis.max()) + 1) * n_lat, lambda c: c
    else:
        cells = np.unique(cell[cell >= 0])
        n, index = max(len(cells), 1), lambda c: np.searchsorted(cells, c)
    h = np.zeros((U, R, n))
    for u in range(U):
        for r in range(R):
            c = cell[r * stride:r * stride + window, u]
            np.add.at(h[u, r], index(c[c >= 0]), 1.0)
    return h


def naive(mu, mv, W, H, tile_height, tile_width, window, stride, labels, want_weights=False):
    """(D[R][L], samples[R][L][2]) on the lat/lon cell counts of compute_naive_spatial_entropy."""
    h = naive_viewer_hists(mu, mv, W, H, tile_height, tile_width, window, stride, dense_bins=want_weights)
    with np.errstate(all="ignore"):
        D, samples = _from_viewers(h, h > 0, h.sum(axis=2).astype(np.int64), labels)
    if want_weights:
        return D, samples, np.stack([h[labels[0] == 0].sum(axis=0), h[labels[0] == 1].sum(axis=0)], axis=1)
    return D, samples


def _bits(h, keys):
    """(S[..], W[..]) over the last axis: ``band``'s statements."""
    W = h.sum(axis=-1)
    q = np.where(keys, h / W[..., None], 1.0)
    return -(q * np.log2(q)).sum(axis=-1), W


def fast_rows(mu, mv, W, H, tile_counts, window, labels, fov_angle=120.0, power_factor=2.0, use_weight_distribution=True,
              naive=None, observed=None):
    """(D[R][L], samples[R][L][2], weights[R][2][n_0]) for every row of stride 1, vectorised (sliding sums over per-frame weight
    rows, one matrix product per group, ``band``'s arithmetic as array operations): the GPU tests' reference for whole shape
    matrices.  Differs from ``fast`` in the association of the sums only; integer histograms are identical.  ``naive`` =
    (tile_height, tile_width): the lat/lon cells; ``weights`` are then over the bins of the package's naive plan.  ``weights``
    are labelling 0's, or with ``observed`` = a list of labellings theirs, [R][len(observed)][2][n_0]."""
    from numpy.lib.stride_tricks import sliding_window_view
    labels = np.asarray(labels)
    mA, mB = (labels == 0).astype(np.float64), (labels == 1).astype(np.float64)            # [L][U]
    px, py, present, grid = vo.sample_directions(mu, mv, W, H)

    def window_sum(a):
        return sliding_window_view(a, window, axis=0).sum(axis=-1)

    s = window_sum(present.astype(np.float64))                                               # [R][U]
    samples = np.stack([s @ mA.T, s @ mB.T], axis=-1).astype(np.int32)                       # [R][L][2]
    if naive is not None:
        lon_axis, lat_axis = vo.axis_tables(W, H)
        li_axis, lj_axis = vo.naive_tile_indices(lon_axis, lat_axis, *naive)
        n_lat = int(lj_axis.max()) + 1
        n = (int(li_axis.max()) + 1) * n_lat
        bins = np.where(present, li_axis[np.where(present, px, 0)] * n_lat + lj_axis[np.where(present, py, 0)], 0)
        lattices = [(np.eye(n)[bins] * present[..., None], None)]
    else:
        flat = grid.reshape(-1, 3)
        did = np.where(present, py * (W + 1) + px, 0)
        used = np.unique(did[present])
        remap = np.zeros(len(flat), dtype=np.int64)
        remap[used] = np.arange(len(used))
        lattices = []
        for tc in tile_counts:
            L = vo.fibonacci_lattice(tc)
            wrows, keys = vo.tile_weight_rows(flat[used], L, fov_angle, power_factor, use_weight_distribution, return_keys=True)
            lattices.append((wrows[remap[did]] * present[..., None], keys[remap[did]] & present[..., None]))
    D = weights = None
    with np.errstate(all="ignore"):
        for k, (Wf, Kf) in enumerate(lattices):
            h = window_sum(Wf)                                                               # [R][U][n]
            hA, hB = np.matmul(mA, h), np.matmul(mB, h)                                      # [R][L][n]
            if Kf is None:
                kA, kB = hA > 0, hB > 0
            else:
                ku = sliding_window_view(Kf, window, axis=0).any(axis=-1).astype(np.float64)
                kA, kB = np.matmul(mA, ku) > 0, np.matmul(mB, ku) > 0
            (sA, wA), (sB, wB) = _bits(hA, kA), _bits(hB, kB)
            Wp = wA + wB
            qp = np.where(kA | kB, (hA + hB) / Wp[..., None], 1.0)
            Dk = -(qp * np.log2(qp)).sum(axis=-1) - (wA * sA + wB * sB) / Wp
            Dk[(samples == 0).any(axis=-1)] = np.nan
            D = Dk if D is None else D + Dk
            if k == 0:
                weights = np.stack([hA[:, 0], hB[:, 0]], axis=1) if observed is None else \
                    np.stack([hA[:, list(observed)], hB[:, list(observed)]], axis=2)
    return D / len(lattices), samples, weights


def summary(observed, null, confidence):
    """(summary[5][R] = observed, p_value, p_adjusted, null_mean, null_crit; valid[R]) from observed[R] and null[R][P]."""
    observed = np.asarray(observed, dtype=np.float64)
    null = np.asarray(null, dtype=np.float64)
    R, P = null.shape
    out = np.full((5, R), np.nan)
    out[0] = observed
    valid = np.zeros(R, dtype=np.int32)
    finite = np.isfinite(null)
    has = finite.any(axis=0)                                                      # permutations that have a maxnull
    maxnull = np.where(finite, null, -np.inf).max(axis=0)[has]
    M = int(has.sum())
    for r in range(R):
        x = np.sort(null[r][finite[r]])
        m = valid[r] = len(x)
        if not np.isnan(observed[r]):
            out[1, r] = (1 + int((x >= observed[r]).sum())) / (1 + m)
            out[2, r] = (1 + int((maxnull >= observed[r]).sum())) / (1 + M)
        if m:
            out[3, r] = x.sum() / m
            out[4, r] = np.quantile(x, confidence, method="linear")
    return out, valid
