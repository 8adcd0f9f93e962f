"""numpy oracles of the attention coverage (include/vet.h: vet_coverage), built on oracle.vet_oracle, tests/_window_oracle.py and
tests/_window_divergence_oracle.py only.

Row r of (window, stride) covers frames [r * stride, r * stride + window).  With h_r >= 0 lattice 0's pooled histogram of the row
(what vet_spatial_entropy_windowed returns in d_weights, by absolute value):

    order_r      the tiles by weight descending, equal weights by tile index ascending (a stable argsort of -h_r)
    C            np.cumsum of the weights in rank order, C_0 = 0 in front; W_r = C_n
    tiles[r][i]  the first index k with C_k >= fractions[i] * W_r (0 where W_r = 0)
    hit[r][l][i] sum of h_{r+l} over the tiles whose rank in row r is below tiles[r][i], over row r + l's total; l = 0 .. max_lag;
                 NaN where r + l >= R, where W_r = 0 and where row r + l has no mass

``from_hists`` the definition on dense row histograms; also, per (row, fraction) and relative to W_r, the boundary gap (the weight
             at rank k - 1 minus the weight at rank k, k = tiles) and the threshold margin (min_j |C_j - q W|): how far the entry is
             from changing under a rounding of the histogram.
``literal``  ``from_hists`` of ``_window_oracle.literal``'s weights (lattice 0 only: the other lattices of a plan take no part).
``fast``     ``from_hists`` of ``_window_oracle.fast``'s weights.
``naive``    the same on the counts of compute_naive_spatial_entropy's lat/lon cells, in the plan's cell numbering
             (lon index * cells per column + lat index).
Results: dict(tiles[R][Q] i32, order[R][n] i32, hit[R][L + 1][Q], samples[R] where known, gap[R][Q], margin[R][Q], mass[R]).
"""
import numpy as np

from oracle import vet_oracle as vo
from tests import _window_oracle as wo


def from_hists(h, fractions, max_lag, totals=None):
    """``h`` [R][n] >= 0; ``totals`` [R]: the rows' totals that ``hit`` divides by (default: h.sum(axis=1))."""
    h = np.asarray(h, dtype=np.float64)
    R, n = h.shape
    q = np.asarray(fractions, dtype=np.float64)
    Q, L = len(q), int(max_lag)
    totals = h.sum(axis=1) if totals is None else np.asarray(totals, dtype=np.float64)
    tiles = np.zeros((R, Q), dtype=np.int32)
    order = np.empty((R, n), dtype=np.int32)
    rank = np.empty((R, n), dtype=np.int64)
    mass = np.zeros(R)
    gap = np.full((R, Q), np.nan)
    margin = np.full((R, Q), np.nan)
    for r in range(R):
        o = np.argsort(-h[r], kind="stable")
        order[r] = o
        rank[r, o] = np.arange(n)
        w = h[r][o]
        C = np.concatenate([[0.0], np.cumsum(w)])
        mass[r] = C[-1]
        if not mass[r] > 0:
            continue
        thr = q * mass[r]
        k = np.searchsorted(C, thr, side="left")                              # C is non-decreasing: the first C_k >= thr
        tiles[r] = k
        wz = np.concatenate([w, [0.0]])
        gap[r] = np.where(k >= 1, (wz[np.maximum(k, 1) - 1] - wz[k]) / mass[r], np.nan)
        margin[r] = np.abs(C[None, :] - thr[:, None]).min(axis=1) / mass[r]
    hit = np.full((R, L + 1, Q), np.nan)
    for l in range(L + 1):
        for r in range(R - l):
            if mass[r] > 0 and totals[r + l] > 0:
                for i in range(Q):
                    hit[r, l, i] = h[r + l][rank[r] < tiles[r, i]].sum() / totals[r + l]
    return dict(tiles=tiles, order=order, hit=hit, gap=gap, margin=margin, mass=mass)


def literal(mu, mv, W, H, tile_counts, window, stride, max_lag, fractions, fov_angle=120.0, power_factor=2.0,
            use_weight_distribution=True):
    _, samples, weights = wo.literal(mu, mv, W, H, list(tile_counts)[:1], window, stride, None, fov_angle, power_factor,
                                     use_weight_distribution)
    return dict(from_hists(np.abs(weights), fractions, max_lag), samples=samples, weights=weights)


def fast(mu, mv, W, H, tile_counts, window, stride, max_lag, fractions, fov_angle=120.0, power_factor=2.0,
         use_weight_distribution=True):
    _, samples, weights = wo.fast(mu, mv, W, H, list(tile_counts)[:1], window, stride, fov_angle, power_factor,
                                  use_weight_distribution)
    return dict(from_hists(np.abs(weights), fractions, max_lag), samples=samples, weights=weights)


def naive_hists(mu, mv, W, H, tile_height, tile_width, window, stride):
    """The lat/lon cell counts h[R][n] of every row in the plan's cell numbering, n = (360 / tile_width + 1) * (180 / tile_height + 1)."""
    px, py, present, _ = vo.sample_directions(mu, mv, W, H)
    lon_axis, lat_axis = vo.axis_tables(W, H)
    li_axis, lj_axis = vo.naive_tile_indices(lon_axis, lat_axis, tile_height, tile_width)
    n_lat = 180 // tile_height + 1
    n = (360 // tile_width + 1) * n_lat
    cell = np.where(present, li_axis[np.where(present, px, 0)] * n_lat + lj_axis[np.where(present, py, 0)], -1)
    R = wo.n_rows(len(mu), window, stride)
    h = np.zeros((R, n))
    for r in range(R):
        c = cell[r * stride:r * stride + window].reshape(-1)
        np.add.at(h[r], c[c >= 0], 1.0)
    return h


def naive(mu, mv, W, H, tile_height, tile_width, window, stride, max_lag, fractions):
    h = naive_hists(mu, mv, W, H, tile_height, tile_width, window, stride)
    return dict(from_hists(h, fractions, max_lag), samples=h.sum(axis=1).astype(np.int32), weights=h)
