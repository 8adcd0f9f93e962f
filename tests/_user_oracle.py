"""numpy oracles of the per-viewer spatial entropy (include/vet.h: vet_user_entropy), built on oracle.vet_oracle only.

Row (u, r) of (window, stride) covers frames [r * stride, r * stride + window) of user u.  Its value is the reference's
compute_spatial_entropy on ONE dict holding user u's present samples of those frames in ascending frame order, per lattice, then
the mean over the lattices.

``literal``  exactly that: ``vo.spatial_entropy_frame`` on the row's directions, row by row.  It is what
             tests/test_user_entropy_surface.py pins against golden G16 (the real reference's output).
``fast``     the same quantity for every row of a long series: weight rows per distinct direction (as ``vo.spatial_series``
             does), the row's weight rows added in frame order, then ``vo.spatial_entropy_from_hist``.  The two differ only in
             the association of the FP64 sums (1e-15 relative); test_user_entropy_surface.py checks them against each other
             to 1e-12.
``naive``    compute_naive_spatial_entropy on the row's samples (entropy and samples only).
A row without a sample (the reference raises) is NaN in all three; weights use the dense convention of include/vet.h (-0.0 = key
whose value is 0.0, +0.0 = no key).  Results are user-major: entropy[U][R], samples[U][R], weights[U][R][n_0].
"""
import numpy as np

from oracle import vet_oracle as vo


def n_rows(T, window, stride):
    return (T - window) // stride + 1


def direction_ids(mu, mv, W, H):
    """(ids[T][U] on the pixel grid, -1 absent; the grid's directions [n_dirs][3])."""
    px, py, present, grid = vo.sample_directions(mu, mv, W, H)
    return np.where(present, py * (W + 1) + px, -1), grid.reshape(-1, 3)


def literal(mu, mv, W, H, tile_counts, window, stride, rows=None, fov_angle=120.0, power_factor=2.0,
            use_weight_distribution=True):
    """(entropy[U][m], samples[U][m], weights[U][m][n_0]) for ``rows`` (default: every row)."""
    did, flat = direction_ids(mu, mv, W, H)
    T, U = did.shape
    lattices = [vo.fibonacci_lattice(tc) for tc in tile_counts]
    rows = np.arange(n_rows(T, window, stride)) if rows is None else np.asarray(rows)
    ent = np.zeros((U, len(rows)))
    samples = np.zeros((U, len(rows)), dtype=np.int32)
    weights = np.zeros((U, len(rows), len(lattices[0])))
    with np.errstate(all="ignore"):
        for u in range(U):
            for i, r in enumerate(rows):
                ids = did[r * stride:r * stride + window, u]               # ascending frame order
                ids = ids[ids >= 0]
                samples[u, i] = len(ids)
                if len(ids) == 0:
                    ent[u, i] = np.nan
                    continue
                for k, L in enumerate(lattices):
                    e, hist, _ = vo.spatial_entropy_frame(flat[ids], L, fov_angle, power_factor, use_weight_distribution)
                    ent[u, i] += e
                    if k == 0:
                        _, keys = vo.tile_weight_rows(flat[ids], L, fov_angle, power_factor, use_weight_distribution,
                                                      return_keys=True)
                        weights[u, i] = np.where(keys.any(axis=0) & (hist == 0), -0.0, hist)
    return ent / len(lattices), samples, weights


def fast(mu, mv, W, H, tile_counts, window, stride, fov_angle=120.0, power_factor=2.0, use_weight_distribution=True):
    """(entropy[U][R], samples[U][R], weights[U][R][n_0]) for every row."""
    did, flat = direction_ids(mu, mv, W, H)
    T, U = did.shape
    R = n_rows(T, window, stride)
    used = np.unique(did[did >= 0])
    remap = np.full(len(flat) + 1, -1, dtype=np.int64)
    remap[used] = np.arange(len(used))
    ent = np.zeros((U, R))
    samples = np.zeros((U, R), dtype=np.int32)
    weights = None
    with np.errstate(all="ignore"):
        for k, tc in enumerate(tile_counts):
            L = vo.fibonacci_lattice(tc)
            n = len(L)
            wrows, keys = vo.tile_weight_rows(flat[used], L, fov_angle, power_factor, use_weight_distribution, return_keys=True)
            if k == 0:
                weights = np.zeros((U, R, n))
            for u in range(U):
                col = did[:, u]
                for r in range(R):
                    ids = col[r * stride:r * stride + window]
                    ids = remap[ids[ids >= 0]]
                    samples[u, r] = len(ids)
                    if len(ids) == 0:
                        ent[u, r] = np.nan
                        continue
                    h = np.add.reduce(wrows[ids], axis=0)                  # row after row: frame order
                    key = keys[ids].any(axis=0)
                    ent[u, r] += vo.spatial_entropy_from_hist(h, key, n, use_weight_distribution)
                    if k == 0:
                        weights[u, r] = np.where(key & (h == 0), -0.0, h)
    return ent / len(tile_counts), samples, weights


def naive(mu, mv, W, H, tile_height, tile_width, window, stride, use_weight_distribution=True):
    """(entropy[U][R], samples[U][R]) of compute_naive_spatial_entropy on the row's samples."""
    px, py, present, _ = vo.sample_directions(mu, mv, W, H)
    lon_axis, lat_axis = vo.axis_tables(W, H)
    li_axis, lj_axis = vo.naive_tile_indices(lon_axis, lat_axis, tile_height, tile_width)
    cell = np.where(present, li_axis[np.where(present, px, 0)] * 100000 + lj_axis[np.where(present, py, 0)], -1)
    T, U = cell.shape
    R = n_rows(T, window, stride)
    ent = np.zeros((U, R))
    samples = np.zeros((U, R), dtype=np.int32)
    for u in range(U):
        for r in range(R):
            c = cell[r * stride:r * stride + window, u]
            c = c[c >= 0]
            samples[u, r] = len(c)
            if len(c) == 0:
                ent[u, r] = np.nan
                continue
            _, counts = np.unique(c, return_counts=True)
            ent[u, r] = vo.naive_entropy_from_counts(counts, tile_height, tile_width, use_weight_distribution)
    return ent, samples


def keys_of(weights):
    return (weights != 0) | np.signbit(weights)
