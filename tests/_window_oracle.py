"""numpy oracles of the windowed (pooled) spatial entropy, built on oracle.vet_oracle only.

Row r of (window, stride) covers frames [r * stride, r * stride + window).  Its value is the reference's
compute_spatial_entropy on ONE dict holding every present (frame, user) sample of those frames, frame-major then user order,
per lattice, then the mean over the lattices.

``literal``  exactly that: ``vo.spatial_entropy_frame`` on the window's concatenated directions, row by row.  It is what
             tests/test_windowed_surface.py pins against golden G14 (the real reference's output).
``fast``     the same quantity for every row of a long series at sizes the literal form cannot reach: weight rows per
             distinct direction (as ``vo.spatial_series`` does), per-frame sums in user order (``frame_sums``, reusable), the window's frame sums added
             in frame order, then ``vo.spatial_entropy_from_hist``.  The two differ only in the association of the FP64 sums
             (1e-15 relative); test_windowed_surface.py checks them against each other to 1e-12.
An empty window (the reference raises) is NaN in both; weights use the dense convention of include/vet.h (-0.0 = key whose
value is 0.0, +0.0 = no key).
"""
import numpy as np

from oracle import vet_oracle as vo


def n_rows(T, window, stride):
    return (T - window) // stride + 1


def _ids(mu, mv, W, H):
    px, py, present, grid = vo.sample_directions(mu, mv, W, H)
    return np.where(present, py * (W + 1) + px, -1), grid.reshape(-1, 3)


def literal(mu, mv, W, H, tile_counts, window, stride, rows=None, fov_angle=120.0, power_factor=2.0,
            use_weight_distribution=True):
    """(entropy[m], samples[m], weights[m][n_0]) for ``rows`` (default: every row)."""
    did, flat = _ids(mu, mv, W, H)
    lattices = [vo.fibonacci_lattice(tc) for tc in tile_counts]
    rows = np.arange(n_rows(len(mu), window, stride)) if rows is None else np.asarray(rows)
    ent = np.zeros(len(rows))
    samples = np.zeros(len(rows), dtype=np.int32)
    weights = np.zeros((len(rows), len(lattices[0])))
    with np.errstate(all="ignore"):
        for i, r in enumerate(rows):
            ids = did[r * stride:r * stride + window].reshape(-1)         # frame-major, then user order
            ids = ids[ids >= 0]
            samples[i] = len(ids)
            if len(ids) == 0:
                ent[i] = np.nan
                continue
            for k, L in enumerate(lattices):
                e, hist, _ = vo.spatial_entropy_frame(flat[ids], L, fov_angle, power_factor, use_weight_distribution)
                ent[i] += e
                if k == 0:
                    _, keys = vo.tile_weight_rows(flat[ids], L, fov_angle, power_factor, use_weight_distribution, return_keys=True)
                    weights[i] = np.where(keys.any(axis=0) & (hist == 0), -0.0, hist)
    return ent / len(lattices), samples, weights


def frame_sums(mu, mv, W, H, tile_counts, fov_angle=120.0, power_factor=2.0, use_weight_distribution=True):
    """Per lattice (hist[T][n], touched[T][n]) — every frame's tile sums in user order and key set — and present[T]."""
    did, flat = _ids(mu, mv, W, H)
    T = len(mu)
    used = np.unique(did[did >= 0])
    remap = np.full(len(flat) + 1, -1, dtype=np.int64)
    remap[used] = np.arange(len(used))
    out = []
    with np.errstate(all="ignore"):
        for tc in tile_counts:
            L = vo.fibonacci_lattice(tc)
            rows, keys = vo.tile_weight_rows(flat[used], L, fov_angle, power_factor, use_weight_distribution, return_keys=True)
            hist = np.zeros((T, len(L)))
            touched = np.zeros((T, len(L)), dtype=bool)
            for t in range(T):
                ids = remap[did[t][did[t] >= 0]]
                if len(ids):
                    hist[t] = np.add.reduce(rows[ids], axis=0)            # row after row: user order
                    touched[t] = keys[ids].any(axis=0)
            out.append((hist, touched))
    return out, (did >= 0).sum(axis=1)


def fast(mu, mv, W, H, tile_counts, window, stride, fov_angle=120.0, power_factor=2.0, use_weight_distribution=True,
         frames=None):
    """(entropy[R], samples[R], weights[R][n_0]) for every row; ``frames`` = a ``frame_sums`` result of the same inputs."""
    if frames is None:
        frames = frame_sums(mu, mv, W, H, tile_counts, fov_angle, power_factor, use_weight_distribution)
    per_lattice, present = frames
    R = n_rows(len(mu), window, stride)
    ent = np.zeros(R)
    samples = np.array([present[r * stride:r * stride + window].sum() for r in range(R)], dtype=np.int32)
    weights = np.zeros((R, per_lattice[0][0].shape[1]))
    with np.errstate(all="ignore"):
        for k, (hist, touched) in enumerate(per_lattice):
            n = hist.shape[1]
            for r in range(R):
                f0 = r * stride
                h = np.add.reduce(hist[f0:f0 + window], axis=0)           # frame after frame: frame order
                key = touched[f0:f0 + window].any(axis=0)
                ent[r] += vo.spatial_entropy_from_hist(h, key, n, use_weight_distribution) if samples[r] else np.nan
                if k == 0:
                    weights[r] = np.where(key & (h == 0), -0.0, h)
    return ent / len(per_lattice), samples, weights


def naive(mu, mv, W, H, tile_height, tile_width, window, stride, use_weight_distribution=True):
    """(entropy[R], samples[R]) of compute_naive_spatial_entropy on the window's pooled samples."""
    px, py, present, _ = vo.sample_directions(mu, mv, W, H)
    lon_axis, lat_axis = vo.axis_tables(W, H)
    li_axis, lj_axis = vo.naive_tile_indices(lon_axis, lat_axis, tile_height, tile_width)
    cell = np.where(present, li_axis[np.where(present, px, 0)] * 100000 + lj_axis[np.where(present, py, 0)], -1)
    R = n_rows(len(mu), window, stride)
    ent = np.zeros(R)
    samples = np.zeros(R, dtype=np.int32)
    for r in range(R):
        c = cell[r * stride:r * stride + window].reshape(-1)
        c = c[c >= 0]
        samples[r] = len(c)
        if len(c) == 0:
            ent[r] = np.nan
            continue
        _, counts = np.unique(c, return_counts=True)
        ent[r] = vo.naive_entropy_from_counts(counts, tile_height, tile_width, use_weight_distribution)
    return ent, samples


def keys_of(weights):
    return (weights != 0) | np.signbit(weights)
