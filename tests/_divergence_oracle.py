"""numpy oracles of the pairwise viewer divergence (include/vet.h: vet_user_divergence), built on oracle.vet_oracle and
tests/_user_oracle.py only.

Row r of (window, stride) covers frames [r * stride, r * stride + window).  With h_u viewer u's histogram of the row (what
vet_user_entropy returns in d_weights), W_u its total and S(h) = -sum_keys (h_t / W) log2(h_t / W) — the reference's ``entropy``
before the normaliser —

    D_k(u, v) = S(h_u + h_v) - (W_u S(h_u) + W_v S(h_v)) / (W_u + W_v),      D = mean over the lattices of D_k   (bits)

``literal``  the definition: per pair three calls of ``vo.spatial_entropy_frame`` — on u's directions of the row, on v's, and on
             both (u's then v's, each in ascending frame order) — and S taken back from the returned histogram with the
             reference's -sum q log2 q over its keys.  tests/test_user_divergence_surface.py pins it against golden G18 (the real
             reference's dicts).
``fast``     the same from ``_user_oracle.fast``'s weights, lattice by lattice: the pooled histogram is h_u + h_v.  Differs from
             ``literal`` in the association of the FP64 sums only (checked to 1e-12).
``naive``    the same on the counts of compute_naive_spatial_entropy's lat/lon cells.
D(u, v) is NaN when either viewer has no sample in the row or one of the three S is NaN (a key whose sum is 0.0 or whose
proportion underflows to 0); D(u, u) is +0.0 for a present viewer whose own S is a number.  Results: divergence[R][U][U],
samples[U][R].
"""
import numpy as np

from oracle import vet_oracle as vo
from tests import _user_oracle as uo


def bits_of(h, keys):
    """S(h) in bits over the keys of one dense histogram: the reference's loop (entropy_utils.py:194-198) before the normaliser."""
    with np.errstate(all="ignore"):
        q = h[keys] / float(h.sum())
        return float(-(q * np.log2(q)).sum())


def h2(p):
    """Binary entropy in bits (the upper bound of D at the mass split p)."""
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where((p <= 0) | (p >= 1), 0.0, -(p * np.log2(p) + (1 - p) * np.log2(1 - p)))


def from_hists(h, keys):
    """D_k[U][U] of one row and lattice from the dense histograms h[U][n] (values >= 0) and their key masks keys[U][n]; a
    viewer without a key is absent."""
    U, n = h.shape
    present = keys.any(axis=1)
    with np.errstate(all="ignore"):
        W = h.sum(axis=1)
        q = np.where(keys, h / W[:, None], 1.0)
        own = -(q * np.log2(q)).sum(axis=1)                                     # [U], NaN where the viewer's own S is
        Wp = W[:, None] + W[None, :]
        ku = keys[:, None, :] | keys[None, :, :]
        qp = np.where(ku, (h[:, None, :] + h[None, :, :]) / Wp[:, :, None], 1.0)
        pooled = -(qp * np.log2(qp)).sum(axis=2)
        D = pooled - (W[:, None] * own[:, None] + W[None, :] * own[None, :]) / Wp
    D[~present, :] = np.nan
    D[:, ~present] = np.nan
    ok = present & ~np.isnan(own)
    D[np.flatnonzero(ok), np.flatnonzero(ok)] = 0.0
    return D


def literal(mu, mv, W, H, tile_counts, window, stride, rows=None, fov_angle=120.0, power_factor=2.0,
            use_weight_distribution=True, want_terms=False):
    """(divergence[m][U][U], samples[U][m]) for ``rows`` (default: every row).  ``want_terms``: also S[m][K][U][U] and
    total[m][K][U][U] of the pooled dicts (the diagonal holds the viewers' own)."""
    did, flat = uo.direction_ids(mu, mv, W, H)
    T, U = did.shape
    lattices = [vo.fibonacci_lattice(tc) for tc in tile_counts]
    rows = np.arange(uo.n_rows(T, window, stride)) if rows is None else np.asarray(rows)
    K = len(lattices)
    div = np.zeros((len(rows), U, U))
    samples = np.zeros((U, len(rows)), dtype=np.int32)
    S = np.full((len(rows), K, U, U), np.nan)
    tot = np.zeros((len(rows), K, U, U))

    def bits(dirs, L):
        _, hist, _ = vo.spatial_entropy_frame(dirs, L, fov_angle, power_factor, use_weight_distribution)
        _, keys = vo.tile_weight_rows(dirs, L, fov_angle, power_factor, use_weight_distribution, return_keys=True)
        return bits_of(hist, keys.any(axis=0)), float(hist.sum())

    with np.errstate(all="ignore"):
        for i, r in enumerate(rows):
            ids = [did[r * stride:r * stride + window, u] for u in range(U)]
            ids = [x[x >= 0] for x in ids]                                      # ascending frame order
            samples[:, i] = [len(x) for x in ids]
            for k, L in enumerate(lattices):
                for u in range(U):
                    if len(ids[u]):
                        S[i, k, u, u], tot[i, k, u, u] = bits(flat[ids[u]], L)
                for u in range(U):
                    for v in range(u + 1, U):
                        if len(ids[u]) and len(ids[v]):
                            S[i, k, u, v], tot[i, k, u, v] = bits(flat[np.concatenate([ids[u], ids[v]])], L)
                            S[i, k, v, u], tot[i, k, v, u] = S[i, k, u, v], tot[i, k, u, v]
                div[i] += combine(S[i, k], tot[i, k], samples[:, i] > 0)
    div /= K
    return (div, samples, S, tot) if want_terms else (div, samples)


def combine(S, tot, present):
    """D_k[U][U] from the three-term table of one row and lattice: S[u][v] / tot[u][v] of the pooled dict, the diagonal the
    viewers' own."""
    with np.errstate(all="ignore"):
        own, W = np.diag(S), np.diag(tot)
        D = S - (W[:, None] * own[:, None] + W[None, :] * own[None, :]) / (W[:, None] + W[None, :])
    D[~present, :] = np.nan
    D[:, ~present] = np.nan
    ok = present & ~np.isnan(own)
    D[np.flatnonzero(ok), np.flatnonzero(ok)] = 0.0
    return D


def fast(mu, mv, W, H, tile_counts, window, stride, fov_angle=120.0, power_factor=2.0, use_weight_distribution=True):
    """(divergence[R][U][U], samples[U][R]) for every row."""
    div, samples = None, None
    for tc in tile_counts:
        _, samples, weights = uo.fast(mu, mv, W, H, [tc], window, stride, fov_angle, power_factor, use_weight_distribution)
        keys = uo.keys_of(weights)
        Dk = np.stack([from_hists(np.abs(weights[:, r]), keys[:, r]) for r in range(weights.shape[1])])
        div = Dk if div is None else div + Dk
    return div / len(tile_counts), samples


def naive(mu, mv, W, H, tile_height, tile_width, window, stride):
    """(divergence[R][U][U], samples[U][R]) on the lat/lon cell counts of compute_naive_spatial_entropy."""
    px, py, present, _ = vo.sample_directions(mu, mv, W, H)
    lon_axis, lat_axis = vo.axis_tables(W, H)
    li_axis, lj_axis = vo.naive_tile_indices(lon_axis, lat_axis, tile_height, tile_width)
    cell = np.where(present, li_axis[np.where(present, px, 0)] * 100000 + lj_axis[np.where(present, py, 0)], -1)
    T, U = cell.shape
    R = uo.n_rows(T, window, stride)
    cells = np.unique(cell[cell >= 0])
    col = np.searchsorted(cells, np.maximum(cell, cells[0] if len(cells) else 0))
    div = np.zeros((R, U, U))
    samples = np.zeros((U, R), dtype=np.int32)
    for r in range(R):
        h = np.zeros((U, max(len(cells), 1)))
        for u in range(U):
            c = cell[r * stride:r * stride + window, u]
            np.add.at(h[u], col[r * stride:r * stride + window, u][c >= 0], 1.0)
        samples[:, r] = h.sum(axis=1)
        div[r] = from_hists(h, h > 0)
    return div, samples
