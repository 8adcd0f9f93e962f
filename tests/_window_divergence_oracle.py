"""numpy oracles of the window-to-window divergence (include/vet.h: vet_window_divergence), built on oracle.vet_oracle,
tests/_window_oracle.py and tests/_divergence_oracle.py only.

Row r of (window, stride) covers frames [r * stride, r * stride + window).  With P_r the pooled histogram of the row (what
vet_spatial_entropy_windowed returns in d_weights), W_r its total and S(h) = -sum_keys (h_t / W) log2(h_t / W) — the reference's
``entropy`` before the normaliser — for the lags l = 1 .. max_lag

    D_k(r, l) = S(P_r + P_{r+l}) - (W_r S(P_r) + W_{r+l} S(P_{r+l})) / (W_r + W_{r+l}),      D = mean over the lattices of D_k   (bits)

``literal``  the definition: per pair three calls of ``vo.spatial_entropy_frame`` — on row r's directions, on row r + l's, and on
             both (row r's then row r + l's, each frame-major then user order) — and S taken back from the returned histogram with
             the reference's -sum q log2 q over its keys.  tests/test_window_divergence_surface.py pins it against golden G19 (the
             real reference's dicts).
``fast``     ``_window_oracle.fast`` per lattice, then ``band`` — ``_divergence_oracle.from_hists``'s arithmetic on the row pairs
             (r, r + l) instead of on every pair — of ``np.abs(weights)`` and ``keys_of(weights)``.  Differs from ``literal`` in the
             association of the FP64 sums only (checked to 1e-12).
``naive``    the same on the counts of compute_naive_spatial_entropy's lat/lon cells.
D(r, l) is NaN where r + l >= R, where either row has no sample and where one of the three S is NaN (a key whose sum is 0.0 or
whose proportion underflows to 0).  Results: divergence[R][L], samples[R]; with ``want_terms`` also bits[R][K][L][3] and
total[R][K][L][3]: S and W of (row r, row r + l, both), NaN / 0 where there is no such dict.
"""
import numpy as np

from oracle import vet_oracle as vo
from tests import _divergence_oracle as dvo
from tests import _window_oracle as wo

h2 = dvo.h2


def band(h, keys, L, want_terms=False):
    """D_k[R][L] of one lattice from the dense row histograms h[R][n] (values >= 0) and their key masks keys[R][n]; a row
    without a key has no sample.  ``from_hists``'s statements on the pairs (r, r + l)."""
    R, n = h.shape
    out = np.full((R, L), np.nan)
    bits = np.full((R, L, 3), np.nan)
    tot = np.zeros((R, L, 3))
    present = keys.any(axis=1)
    with np.errstate(all="ignore"):
        W = h.sum(axis=1)
        q = np.where(keys, h / W[:, None], 1.0)
        own = -(q * np.log2(q)).sum(axis=1)                                     # [R], NaN where the row's own S is
        own[~present] = np.nan
        for l in range(1, L + 1):
            if l >= R:
                break
            a, b = slice(0, R - l), slice(l, R)
            Wp = W[a] + W[b]
            ku = keys[a] | keys[b]
            qp = np.where(ku, (h[a] + h[b]) / Wp[:, None], 1.0)
            pooled = -(qp * np.log2(qp)).sum(axis=1)
            D = pooled - (W[a] * own[a] + W[b] * own[b]) / Wp
            both = present[a] & present[b]
            D[~both] = np.nan
            out[:R - l, l - 1] = D
            bits[:R - l, l - 1, 0], bits[:R - l, l - 1, 1] = own[a], own[b]
            bits[:R - l, l - 1, 2] = np.where(both, pooled, np.nan)
            tot[:R - l, l - 1, 0], tot[:R - l, l - 1, 1] = W[a], W[b]
            tot[:R - l, l - 1, 2] = np.where(both, (h[a] + h[b]).sum(axis=1), 0.0)
    return (out, bits, tot) if want_terms else out


def combine(bits, tot):
    """D_k[..] from the three-term tables [..][3] (row r, row r + l, both): the docstring's formula; NaN where a term is missing."""
    with np.errstate(all="ignore"):
        return bits[..., 2] - (tot[..., 0] * bits[..., 0] + tot[..., 1] * bits[..., 1]) / (tot[..., 0] + tot[..., 1])


def literal(mu, mv, W, H, tile_counts, window, stride, max_lag, rows=None, fov_angle=120.0, power_factor=2.0,
            use_weight_distribution=True, want_terms=False):
    """(divergence[m][L], samples[m]) for ``rows`` (default: every row); ``want_terms``: also bits[m][K][L][3], total[m][K][L][3]."""
    did, flat = wo._ids(mu, mv, W, H)
    lattices = [vo.fibonacci_lattice(tc) for tc in tile_counts]
    R, L, K = wo.n_rows(len(mu), window, stride), int(max_lag), len(lattices)
    rows = np.arange(R) if rows is None else np.asarray(rows)
    samples = np.zeros(len(rows), dtype=np.int32)
    bits = np.full((len(rows), K, L, 3), np.nan)
    tot = np.zeros((len(rows), K, L, 3))

    def row_ids(r):
        ids = did[r * stride:r * stride + window].reshape(-1)                   # frame-major, then user order
        return ids[ids >= 0]

    def terms(ids, lat):
        _, hist, _ = vo.spatial_entropy_frame(flat[ids], lat, fov_angle, power_factor, use_weight_distribution)
        _, keys = vo.tile_weight_rows(flat[ids], lat, fov_angle, power_factor, use_weight_distribution, return_keys=True)
        return dvo.bits_of(hist, keys.any(axis=0)), float(hist.sum())

    with np.errstate(all="ignore"):
        for i, r in enumerate(rows):
            a = row_ids(r)
            samples[i] = len(a)
            for k, lat in enumerate(lattices):
                own_a = terms(a, lat) if len(a) else (np.nan, 0.0)
                for l in range(1, L + 1):
                    if r + l >= R:
                        break
                    b = row_ids(r + l)
                    bits[i, k, l - 1, 0], tot[i, k, l - 1, 0] = own_a
                    if len(b):
                        bits[i, k, l - 1, 1], tot[i, k, l - 1, 1] = terms(b, lat)
                    if len(a) and len(b):
                        bits[i, k, l - 1, 2], tot[i, k, l - 1, 2] = terms(np.concatenate([a, b]), lat)
        div = combine(bits, tot).sum(axis=1) / K
    return (div, samples, bits, tot) if want_terms else (div, samples)


def fast(mu, mv, W, H, tile_counts, window, stride, max_lag, fov_angle=120.0, power_factor=2.0, use_weight_distribution=True,
         want_terms=False):
    """(divergence[R][L], samples[R]) for every row; ``want_terms``: also bits[R][K][L][3], total[R][K][L][3]."""
    div, samples, bits, tot = None, None, [], []
    for tc in tile_counts:
        _, samples, weights = wo.fast(mu, mv, W, H, [tc], window, stride, fov_angle, power_factor, use_weight_distribution)
        Dk, b, t = band(np.abs(weights), wo.keys_of(weights), int(max_lag), want_terms=True)
        div = Dk if div is None else div + Dk
        bits.append(b)
        tot.append(t)
    div = div / len(tile_counts)
    return (div, samples, np.stack(bits, axis=1), np.stack(tot, axis=1)) if want_terms else (div, samples)


def naive_hists(mu, mv, W, H, tile_height, tile_width, window, stride):
    """The dense lat/lon cell counts h[R][cells in use] of every row."""
    px, py, present, _ = vo.sample_directions(mu, mv, W, H)
    lon_axis, lat_axis = vo.axis_tables(W, H)
    li_axis, lj_axis = vo.naive_tile_indices(lon_axis, lat_axis, tile_height, tile_width)
    cell = np.where(present, li_axis[np.where(present, px, 0)] * 100000 + lj_axis[np.where(present, py, 0)], -1)
    R = wo.n_rows(len(mu), window, stride)
    cells = np.unique(cell[cell >= 0])
    h = np.zeros((R, max(len(cells), 1)))
    for r in range(R):
        c = cell[r * stride:r * stride + window].reshape(-1)
        np.add.at(h[r], np.searchsorted(cells, c[c >= 0]), 1.0)
    return h


def naive(mu, mv, W, H, tile_height, tile_width, window, stride, max_lag, want_terms=False):
    """(divergence[R][L], samples[R]) on the lat/lon cell counts of compute_naive_spatial_entropy."""
    h = naive_hists(mu, mv, W, H, tile_height, tile_width, window, stride)
    div, bits, tot = band(h, h > 0, int(max_lag), want_terms=True)
    samples = h.sum(axis=1).astype(np.int32)
    return (div, samples, bits[:, None], tot[:, None]) if want_terms else (div, samples)
