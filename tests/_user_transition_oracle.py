"""numpy oracles of the per-viewer transition entropy, built on oracle.vet_oracle only.

A video of T frames has T - 1 frame pairs; pair f is (frame f, frame f + 1).  Row (u, r) of (window, stride) covers pairs
[r * stride, r * stride + window) of user u.  Its value is the reference's compute_transition_entropy on dicts that hold one
entry per pair of the row in which user u is present in both frames, inserted in ascending pair order, per lattice, then the mean
over the lattices.

``literal``  ``vo.transition_entropy_pairs`` (the dict walk) on the row's (source tile, destination tile) sequence.  It is what
             tests/test_user_transition_surface.py pins against golden G17 (the real reference's output).
``fast``     ``vo.transition_entropy_closed_form`` (the form the kernels evaluate) on the same sequence.
Both return (entropy[U][m], samples[U][m], srccount[U][m][n_0]): N of the row and lattice 0's count per source tile, exact
integers.  A row without a common sample (the reference raises) is NaN with N = 0; N = 1 is the reference's NaN (0 / 0).
"""
import functools

import numpy as np

from oracle import vet_oracle as vo


def n_rows(T, window, stride):
    """rows per user of a video of T frames (T - 1 pairs)"""
    return (T - 1 - window) // stride + 1


@functools.lru_cache(maxsize=None)
def _nearest_table(W, H, tc):
    return vo.nearest_tile(vo.direction_grid(W, H).reshape(-1, 3), vo.fibonacci_lattice(tc))


def tiles_of(mu, mv, W, H, tile_counts):
    """per lattice: int [T][U] nearest tile of every sample, -1 absent"""
    px, py, present, _ = vo.sample_directions(mu, mv, W, H)
    did = np.where(present, py * (W + 1) + px, 0)
    return [np.where(present, _nearest_table(W, H, int(tc))[did], -1) for tc in tile_counts]


def pairs_of(near_u, f0, window):
    """(source tiles, destination tiles) of one user's common pairs of the row, ascending pair order; near_u [T]"""
    p, c = near_u[f0:f0 + window], near_u[f0 + 1:f0 + window + 1]
    both = (p >= 0) & (c >= 0)
    return p[both], c[both]


def _series(fn, mu, mv, W, H, tile_counts, window, stride, rows=None, tiles=None):
    tiles = tiles_of(mu, mv, W, H, tile_counts) if tiles is None else tiles
    T, U = mu.shape
    rows = np.arange(n_rows(T, window, stride)) if rows is None else np.asarray(rows)
    n = [len(vo.fibonacci_lattice(int(tc))) for tc in tile_counts]          # tiles per lattice (not the nominal count)
    ent = np.zeros((U, len(rows)))
    samples = np.zeros((U, len(rows)), dtype=np.int32)
    srccount = np.zeros((U, len(rows), n[0]), dtype=np.int32)
    for u in range(U):
        for i, r in enumerate(rows):
            for k, near in enumerate(tiles):
                p, c = pairs_of(near[:, u], int(r) * stride, window)
                if k == 0:
                    samples[u, i] = len(p)
                    srccount[u, i] = np.bincount(p, minlength=n[0])
                ent[u, i] += fn(p, c, n[k]) if len(p) else np.nan
    return ent / len(tiles), samples, srccount


def literal(mu, mv, W, H, tile_counts, window, stride, rows=None, tiles=None):
    return _series(vo.transition_entropy_pairs, mu, mv, W, H, tile_counts, window, stride, rows, tiles)


def fast(mu, mv, W, H, tile_counts, window, stride, rows=None, tiles=None):
    return _series(vo.transition_entropy_closed_form, mu, mv, W, H, tile_counts, window, stride, rows, tiles)


def bucket_bound(near_u, f0, window, n):
    """sum over source tiles of min(samples, n): what the hash kernel's passes are cut by"""
    p, _ = pairs_of(near_u, f0, window)
    return int(np.minimum(np.bincount(p, minlength=n), n).sum())
