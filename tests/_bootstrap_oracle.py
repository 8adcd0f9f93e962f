"""numpy oracles of the bootstrap confidence bands over viewers (include/vet.h: vet_bootstrap_entropy), built on
oracle.vet_oracle and tests/_user_oracle.py only.

Replicate b resamples the U viewers with replacement: draw j = 0 .. U-1 picks ``picks[b][j]`` (the counter-based generator of
include/vet.h), ``counts[b][u]`` = how often u was picked.  The same resample serves every row and lattice.  Row r of
(window, stride) covers frames [r * stride, r * stride + window); rep[r][b] is the reference's compute_spatial_entropy on ONE dict
holding every present sample of those frames for every drawn viewer, frame-major, then in draw order (a viewer drawn c times is
entered c times), per lattice, then the mean over the lattices.

``draw``     the generator in numpy uint64.
``literal``  exactly that: ``vo.spatial_entropy_frame`` on the resampled directions (naive: the cell counts through
             ``vo.naive_entropy_from_counts``).  tests/test_bootstrap_surface.py pins it against golden G21 (the real reference).
``fast``     the form the device evaluates: per-viewer row histograms (``_user_oracle.fast``'s weights) times the counts, then
             ``vo.spatial_entropy_from_hist``; a tile is a key iff it is a key of a drawn viewer.  Differs from ``literal`` in the
             association of the FP64 sums only (checked to 1e-12).
``fast_rows`` ``fast`` for every row at stride 1 at once, vectorised (sliding sums over per-frame weight rows, one matrix product per
             row, the entropy loop as array operations): the GPU tests' reference for whole shape matrices.  Differs from ``fast``
             in the association of the sums only (checked to 1e-12); integer histograms are identical.
``summary``  mean, sd (two-pass, ddof = 1), the two quantiles (linear interpolation) and the count of the finite replicates.
A replicate whose drawn viewers have no sample in the row is NaN.  Results: rep[R][B], weights[R][B][n_0] (lattice 0's replicate
histograms, plain values: +0.0 where there is no weight).
"""
import numpy as np

from oracle import vet_oracle as vo
from tests import _user_oracle as uo

GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def draw(U, B, seed):
    """(counts[B][U] uint16, picks[B][U] int64): replicate b's draw j is a function of (seed, b * U + j) alone."""
    with np.errstate(over="ignore"):
        i = np.arange(B * U, dtype=np.uint64) + np.uint64(1)
        z = np.uint64(seed) + i * GOLDEN
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
        picks = (((z >> np.uint64(32)) * np.uint64(U)) >> np.uint64(32)).astype(np.int64).reshape(B, U)
    counts = np.zeros((B, U), dtype=np.uint16)
    for b in range(B):
        counts[b] = np.bincount(picks[b], minlength=U)
    return counts, picks


def _cells(mu, mv, W, H, tile_height, tile_width):
    px, py, present, _ = vo.sample_directions(mu, mv, W, H)
    lon_axis, lat_axis = vo.axis_tables(W, H)
    li_axis, lj_axis = vo.naive_tile_indices(lon_axis, lat_axis, tile_height, tile_width)
    return np.where(present, li_axis[np.where(present, px, 0)] * 100000 + lj_axis[np.where(present, py, 0)], -1)


def literal(mu, mv, W, H, tile_counts, window, stride, picks, rows=None, fov_angle=120.0, power_factor=2.0,
            use_weight_distribution=True, naive=None):
    """(rep[m][B], weights[m][B][n_0] or None) for ``rows`` (default: every row).  ``naive`` = (tile_height, tile_width): the
    lat/lon cells of compute_naive_spatial_entropy instead of ``tile_counts`` (no weights)."""
    B = len(picks)
    if naive is not None:
        cell = _cells(mu, mv, W, H, *naive)
        T = len(cell)
    else:
        did, flat = uo.direction_ids(mu, mv, W, H)
        T = len(did)
        lattices = [vo.fibonacci_lattice(tc) for tc in tile_counts]
    rows = np.arange(uo.n_rows(T, window, stride)) if rows is None else np.asarray(rows)
    rep = np.zeros((len(rows), B))
    weights = None if naive is not None else np.zeros((len(rows), B, len(lattices[0])))
    with np.errstate(all="ignore"):
        for i, r in enumerate(rows):
            for b in range(B):
                if naive is not None:
                    c = cell[r * stride:r * stride + window][:, picks[b]].reshape(-1)      # frame-major, then draw order
                    c = c[c >= 0]
                    if len(c) == 0:
                        rep[i, b] = np.nan
                        continue
                    _, cnt = np.unique(c, return_counts=True)
                    rep[i, b] = vo.naive_entropy_from_counts(cnt, naive[0], naive[1], use_weight_distribution)
                    continue
                ids = did[r * stride:r * stride + window][:, picks[b]].reshape(-1)
                ids = ids[ids >= 0]
                if len(ids) == 0:
                    rep[i, b] = np.nan
                    continue
                for k, L in enumerate(lattices):
                    e, hist, _ = vo.spatial_entropy_frame(flat[ids], L, fov_angle, power_factor, use_weight_distribution)
                    rep[i, b] += e
                    if k == 0:
                        weights[i, b] = hist
    return (rep if naive is not None else rep / len(lattices)), weights


def fast(mu, mv, W, H, tile_counts, window, stride, counts, fov_angle=120.0, power_factor=2.0, use_weight_distribution=True,
         naive=None):
    """(rep[R][B], weights[R][B][n_0] or None, samples[R][B]) for every row; ``samples`` is the replicate's dict size."""
    counts = np.asarray(counts, dtype=np.float64)
    B, U = counts.shape
    if naive is not None:
        cell = _cells(mu, mv, W, H, *naive)
        T = len(cell)
        R = uo.n_rows(T, window, stride)
        cells = np.unique(cell[cell >= 0])
        rep = np.full((R, B), np.nan)
        samples = np.zeros((R, B), dtype=np.int64)
        for r in range(R):
            h = np.zeros((U, max(len(cells), 1)))
            blk = cell[r * stride:r * stride + window]
            for u in range(U):
                c = blk[:, u]
                np.add.at(h[u], np.searchsorted(cells, c[c >= 0]), 1.0)
            H_b = counts @ h
            samples[r] = H_b.sum(axis=1)
            for b in range(B):
                if samples[r, b]:
                    rep[r, b] = vo.naive_entropy_from_counts(H_b[b], naive[0], naive[1], use_weight_distribution)
        return rep, None, samples
    rep = weights = samples = None
    with np.errstate(all="ignore"):
        for k, tc in enumerate(tile_counts):
            _, s_u, w_u = uo.fast(mu, mv, W, H, [tc], window, stride, fov_angle, power_factor, use_weight_distribution)
            keys_u = uo.keys_of(w_u)                                   # [U][R][n]
            h_u = np.abs(w_u)
            R, n = h_u.shape[1], h_u.shape[2]
            e = np.full((R, B), np.nan)
            wk = np.zeros((R, B, n))
            samples = (counts @ s_u.astype(np.float64)).T.astype(np.int64)            # [R][B]
            for r in range(R):
                H_b = counts @ h_u[:, r]                               # [B][n]
                K_b = (counts > 0).astype(np.float64) @ keys_u[:, r].astype(np.float64) > 0
                wk[r] = H_b
                for b in range(B):
                    if samples[r, b]:
                        e[r, b] = vo.spatial_entropy_from_hist(H_b[b], K_b[b], n, use_weight_distribution)
            rep = e if rep is None else rep + e
            if k == 0:
                weights = wk
    return rep / len(tile_counts), weights, samples


def _max_entropy(count):
    with np.errstate(all="ignore"):
        p = 1.0 / count
        return -count * p * np.log2(p)                                 # vo._max_entropy, elementwise


def fast_rows(mu, mv, W, H, tile_counts, window, counts, fov_angle=120.0, power_factor=2.0, use_weight_distribution=True,
              naive=None):
    """(rep[R][B], weights[R][B][n_0], samples[R][B]) for every row of stride 1.  ``naive`` = (tile_height, tile_width): the
    lat/lon cells; ``weights`` are then over the bins lon cell * (lat cells) + lat cell of the package's naive plan."""
    from numpy.lib.stride_tricks import sliding_window_view
    counts = np.asarray(counts, dtype=np.float64)
    drawn = (counts > 0).astype(np.float64)
    px, py, present, grid = vo.sample_directions(mu, mv, W, H)
    T, U = present.shape

    def window_sum(a):
        return sliding_window_view(a, window, axis=0).sum(axis=-1)

    samples = (window_sum(present.astype(np.float64)) @ counts.T).astype(np.int64)               # [R][B]
    if naive is not None:
        lon_axis, lat_axis = vo.axis_tables(W, H)
        li_axis, lj_axis = vo.naive_tile_indices(lon_axis, lat_axis, *naive)
        n_lat = int(lj_axis.max()) + 1
        n = (int(li_axis.max()) + 1) * n_lat
        bins = np.where(present, li_axis[np.where(present, px, 0)] * n_lat + lj_axis[np.where(present, py, 0)], 0)
        lattices = [(np.eye(n)[bins] * present[..., None], None, int(180.0 / naive[0]) * int(360.0 / naive[1]))]
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
            lattices.append((wrows[remap[did]] * present[..., None], keys[remap[did]] & present[..., None], len(L)))
    rep = weights = None
    with np.errstate(all="ignore"):
        for k, (Wf, Kf, n_norm) in enumerate(lattices):
            h = window_sum(Wf)                                         # [R][U][n]
            Hb = np.matmul(counts, h)                                  # [R][B][n]
            if Kf is None:
                Kb = Hb > 0
            else:
                Kb = np.matmul(drawn, sliding_window_view(Kf, window, axis=0).any(axis=-1).astype(np.float64)) > 0
            tot = Hb.sum(axis=-1)
            q = Hb / tot[..., None]
            ent = -np.where(Kb, q * np.log2(q), 0.0).sum(axis=-1)
            mx = _max_entropy(float(n_norm)) if use_weight_distribution else \
                np.where(tot > n_norm, _max_entropy(float(n_norm)), _max_entropy(tot))
            e = ent / mx
            e[samples == 0] = np.nan
            rep = e if rep is None else rep + e
            if k == 0:
                weights = Hb
    return rep / len(lattices), weights, samples


def summary(rep, confidence):
    """(summary[4][R] = mean, sd, lo, hi over the finite replicates of each row, valid[R])."""
    rep = np.asarray(rep, dtype=np.float64)
    R = rep.shape[0]
    out = np.full((4, R), np.nan)
    valid = np.zeros(R, dtype=np.int32)
    q_lo, q_hi = (1.0 - confidence) / 2.0, 1.0 - (1.0 - confidence) / 2.0
    for r in range(R):
        x = np.sort(rep[r][np.isfinite(rep[r])])
        m = valid[r] = len(x)
        if m == 0:
            continue
        mean = x.sum() / m
        out[0, r] = mean
        if m >= 2:
            out[1, r] = np.sqrt(((x - mean) ** 2).sum() / (m - 1))
        out[2, r], out[3, r] = np.quantile(x, [q_lo, q_hi], method="linear")
    return out, valid
