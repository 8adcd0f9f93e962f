"""numpy oracles of the viewer-to-crowd divergence (include/vet.h: vet_crowd_divergence), built on oracle.vet_oracle,
tests/_user_oracle.py and tests/_window_oracle.py only.

Row r of (window, stride) covers frames [r * stride, r * stride + window).  With h_u viewer u's histogram of the row (what
vet_user_entropy returns in d_weights), W_u its total, P the row's pooled histogram (what vet_spatial_entropy_windowed returns in
d_weights), W_r its total and S(h) = -sum_keys (h_t / W) log2(h_t / W) — the reference's ``entropy`` before the normaliser —

    D_k(u, r) = sum_{t in keys of h_u} q_t log2(q_t / p_t),   q_t = h_ut / W_u,   p_t = P_t / W_r                  (bits)
    pooled_k = S(P),   within_k = sum_u (W_u / W_r) S(h_u),   between_k = sum_u (W_u / W_r) D_k(u, r)   (present viewers)

and the means over the lattices.

``literal``  the definition: per row one call of ``vo.spatial_entropy_frame`` per viewer — on the viewer's directions of the row
             in ascending frame order — and one on the pooled directions, frame-major then viewer order; S and D taken from the
             returned histograms.  tests/test_crowd_divergence_surface.py pins it against golden G20 (the real reference's dicts).
``fast``     the same from ``_user_oracle.fast``'s and ``_window_oracle.fast``'s weights, lattice by lattice.  Differs from
             ``literal`` in the association of the FP64 sums only (checked to 1e-12).
``naive``    the same on the counts of compute_naive_spatial_entropy's lat/lon cells.
D(u, r) is NaN when the viewer has no sample in the row, when the viewer's own S is NaN (a key whose sum is 0.0 or whose
proportion underflows to 0) and when the row's S is; the three row series are NaN when the row has no sample or its S is NaN,
within and between also when a present viewer's own S is NaN.  Results: divergence[U][R], series[3][R] (pooled, within,
between), samples[U][R].
"""
import numpy as np

from oracle import vet_oracle as vo
from tests import _user_oracle as uo
from tests import _window_oracle as wo


def bits_of(h, keys):
    """S(h) in bits over the keys of one dense histogram: the reference's loop (entropy_utils.py:194-198) before the normaliser."""
    with np.errstate(all="ignore"):
        q = h[keys] / float(h[keys].sum())
        return float(-(q * np.log2(q)).sum())


def from_hists(h, keys, P, pkeys):
    """(D_k[U], series_k[3], W[U], W_r) of one row and lattice from the viewers' dense histograms h[U][n] (values >= 0) with
    their key masks keys[U][n] and the pooled histogram P[n] with pkeys[n]; a viewer without a key is absent."""
    U, n = h.shape
    present = keys.any(axis=1)
    D = np.full(U, np.nan)
    own = np.full(U, np.nan)
    W = np.zeros(U)
    with np.errstate(all="ignore"):
        Wr = float(P[pkeys].sum()) if pkeys.any() else 0.0
        pooled = bits_of(P, pkeys) if pkeys.any() else np.nan
        for u in np.flatnonzero(present):
            k = keys[u]
            W[u] = float(h[u][k].sum())
            q = h[u][k] / W[u]
            own[u] = float(-(q * np.log2(q)).sum())
            D[u] = float((q * np.log2(q / (P[k] / Wr))).sum())
            if np.isnan(own[u]) or np.isnan(pooled):
                D[u] = np.nan
        m = W[present] / Wr
        series = np.array([pooled, float((m * own[present]).sum()), float((m * D[present]).sum())])
    if not present.any() or np.isnan(pooled):
        series[:] = np.nan
    return D, series, W, Wr


def literal(mu, mv, W, H, tile_counts, window, stride, rows=None, fov_angle=120.0, power_factor=2.0,
            use_weight_distribution=True, want_terms=False):
    """(divergence[U][m], series[3][m], samples[U][m]) for ``rows`` (default: every row).  ``want_terms``: also kl[m][K][U],
    own_total[m][K][U] and pooled_total[m][K]."""
    did, flat = uo.direction_ids(mu, mv, W, H)
    T, U = did.shape
    lattices = [vo.fibonacci_lattice(tc) for tc in tile_counts]
    rows = np.arange(uo.n_rows(T, window, stride)) if rows is None else np.asarray(rows)
    K = len(lattices)
    div = np.zeros((U, len(rows)))
    series = np.zeros((3, len(rows)))
    samples = np.zeros((U, len(rows)), dtype=np.int32)
    kl = np.full((len(rows), K, U), np.nan)
    own_tot = np.zeros((len(rows), K, U))
    p_tot = np.zeros((len(rows), K))

    def hist(dirs, L):
        _, h, _ = vo.spatial_entropy_frame(dirs, L, fov_angle, power_factor, use_weight_distribution)
        _, keys = vo.tile_weight_rows(dirs, L, fov_angle, power_factor, use_weight_distribution, return_keys=True)
        return h, keys.any(axis=0)

    with np.errstate(all="ignore"):
        for i, r in enumerate(rows):
            block = did[r * stride:r * stride + window]
            ids = [block[:, u][block[:, u] >= 0] for u in range(U)]              # ascending frame order
            samples[:, i] = [len(x) for x in ids]
            pooled_ids = block.reshape(-1)                                      # frame-major, then viewer order
            pooled_ids = pooled_ids[pooled_ids >= 0]
            for k, L in enumerate(lattices):
                n = len(L)
                h, keys = np.zeros((U, n)), np.zeros((U, n), dtype=bool)
                for u in range(U):
                    if len(ids[u]):
                        h[u], keys[u] = hist(flat[ids[u]], L)
                P, pkeys = hist(flat[pooled_ids], L) if len(pooled_ids) else (np.zeros(n), np.zeros(n, dtype=bool))
                kl[i, k], s3, own_tot[i, k], p_tot[i, k] = from_hists(h, keys, P, pkeys)
                div[:, i] += kl[i, k]
                series[:, i] += s3
    div /= K
    series /= K
    return (div, series, samples, kl, own_tot, p_tot) if want_terms else (div, series, samples)


def fast(mu, mv, W, H, tile_counts, window, stride, fov_angle=120.0, power_factor=2.0, use_weight_distribution=True,
         want_ratio=False):
    """(divergence[U][R], series[3][R], samples[U][R]) for every row.  ``want_ratio``: also the mean over the lattices of
    log2(W_r / W_u), [U][R] (the bound of D, and what its tolerance grows with)."""
    div = series = samples = ratio = None
    for tc in tile_counts:
        _, samples, weights = uo.fast(mu, mv, W, H, [tc], window, stride, fov_angle, power_factor, use_weight_distribution)
        _, _, pw = wo.fast(mu, mv, W, H, [tc], window, stride, fov_angle, power_factor, use_weight_distribution)
        keys, pkeys = uo.keys_of(weights), wo.keys_of(pw)
        R = pw.shape[0]
        got = [from_hists(np.abs(weights[:, r]), keys[:, r], np.abs(pw[r]), pkeys[r]) for r in range(R)]
        Dk, Sk = np.stack([g[0] for g in got], axis=1), np.stack([g[1] for g in got], axis=1)
        with np.errstate(all="ignore"):
            Lk = np.stack([np.log2(g[3] / g[2]) for g in got], axis=1)
        div, series, ratio = (Dk, Sk, Lk) if div is None else (div + Dk, series + Sk, ratio + Lk)
    K = len(tile_counts)
    return (div / K, series / K, samples, ratio / K) if want_ratio else (div / K, series / K, samples)


def naive(mu, mv, W, H, tile_height, tile_width, window, stride, want_ratio=False):
    """(divergence[U][R], series[3][R], samples[U][R]) on the lat/lon cell counts of compute_naive_spatial_entropy.
    ``want_ratio``: also log2(W_r / W_u), [U][R]."""
    px, py, present, _ = vo.sample_directions(mu, mv, W, H)
    lon_axis, lat_axis = vo.axis_tables(W, H)
    li_axis, lj_axis = vo.naive_tile_indices(lon_axis, lat_axis, tile_height, tile_width)
    cell = np.where(present, li_axis[np.where(present, px, 0)] * 100000 + lj_axis[np.where(present, py, 0)], -1)
    T, U = cell.shape
    R = uo.n_rows(T, window, stride)
    cells = np.unique(cell[cell >= 0])
    col = np.searchsorted(cells, np.maximum(cell, cells[0] if len(cells) else 0))
    div = np.zeros((U, R))
    series = np.zeros((3, R))
    samples = np.zeros((U, R), dtype=np.int32)
    for r in range(R):
        h = np.zeros((U, max(len(cells), 1)))
        for u in range(U):
            c = cell[r * stride:r * stride + window, u]
            np.add.at(h[u], col[r * stride:r * stride + window, u][c >= 0], 1.0)
        samples[:, r] = h.sum(axis=1)
        P = h.sum(axis=0)
        div[:, r], series[:, r], _, _ = from_hists(h, h > 0, P, P > 0)
    if want_ratio:
        with np.errstate(all="ignore"):
            return div, series, samples, np.log2(samples.sum(axis=0)[None, :] / samples.astype(np.float64))
    return div, series, samples


def atol_div(n_max, log_ratio, w_rtol):
    """The GPU tests' absolute tolerance on D(u, r), log_ratio = log2(W_r / W_u): the cross entropy is bounded by
    log2(n_max) + log2(W_r / W_u), the own entropy by log2(n_max).  Slots without a mass (NaN, inf) get the plain bound; they
    are NaN in D and compared as such."""
    lr = np.nan_to_num(np.asarray(log_ratio, dtype=np.float64), nan=0.0, posinf=0.0, neginf=0.0)
    return 2.0 * (np.log2(n_max) + np.maximum(lr, 0.0)) * w_rtol


def atol_rows(n_max, U, w_rtol):
    """The GPU tests' absolute tolerance on pooled, within and between."""
    return 2.0 * (np.log2(n_max) + np.log2(U)) * w_rtol
