"""numpy oracle of the lat/lon cell heatmaps of naive plans (include/vet.h: vet_heatmap_create_latlon,
vet_heatmap_render_binned*).

The frame, colour rule and markers are those of tests/_heatmap_oracle.py; what differs is restated here from the
reference's naive tiling (find_naive_tile_index, utilities/entropy_utils.py:362-381) and its pixel quantiser
(normalize_to_pixel, utilities/data_utils.py:243-261, through _quantiser.axis_angles), without the engine.
"""
from __future__ import annotations

import numpy as np

from tests._heatmap_oracle import colour, paint_markers


def n_lat(th: int) -> int:
    return 180 // th + 1


def n_cells(tw: int, th: int) -> int:
    """(360 / tw + 1) * (180 / th + 1): lon 180 and lat 90 open one more column and row than the grid has."""
    return (360 // tw + 1) * n_lat(th)


def cell_map(tw: int, th: int, W: int, H: int) -> np.ndarray:
    """The cell of every pixel centre, int32 [H, W]: find_naive_tile_index in FP64 with C truncation."""
    c = np.arange(W, dtype=np.float64)
    r = np.arange(H, dtype=np.float64)
    lon = (c + 0.5) / W * 360 - 180
    lat = 90 - (r + 0.5) / H * 180
    li = np.trunc((lon + 180) / tw).astype(np.int64)
    lj = np.trunc((lat + 90) / th).astype(np.int64)
    return (li[None, :] * n_lat(th) + lj[:, None]).astype(np.int32)


def direction_cells(tw: int, th: int, VW: int, VH: int) -> np.ndarray:
    """The cell of every video pixel (py, px), int64 [VH + 1, VW + 1]: the quantiser's lon / lat after its rounding and
    remap (px = 0 -> lon 0, px = VW -> lon 180, py = 0 -> lat 90), then find_naive_tile_index."""
    from viewport_entropy_toolkit import _quantiser
    lon, lat = _quantiser.axis_angles(VW, VH)
    li = np.trunc((lon + 180) / tw).astype(np.int64)
    lj = np.trunc((lat + 90) / th).astype(np.int64)
    return li[None, :] * n_lat(th) + lj[:, None]


def counts(mu, mv, tw: int, th: int, VW: int, VH: int):
    """(users per cell int64 [T, n_cells], users present int64 [T]).  NaN is absent; a sample outside [0, 1] counts in
    neither."""
    mu = np.asarray(mu, dtype=np.float64)
    mv = np.asarray(mv, dtype=np.float64)
    ok = (mu >= 0) & (mu <= 1) & (mv >= 0) & (mv <= 1)          # False for NaN
    px = np.trunc(np.where(ok, mu, 0) * VW).astype(np.int64)
    py = np.trunc(np.where(ok, mv, 0) * VH).astype(np.int64)
    cells = direction_cells(tw, th, VW, VH)[py, px]
    n = n_cells(tw, th)
    T = mu.shape[0]
    out = np.zeros((T, n), dtype=np.int64)
    for t in range(T):
        out[t] = np.bincount(cells[t][ok[t]], minlength=n)
    return out, ok.sum(axis=1).astype(np.int64)


def render(mu, mv, tw: int, th: int, W: int, H: int, VW: int, VH: int, markers: bool = True, radius: int = 2):
    """Frames uint8 [T, H, W, 3]: colour(count, present) of every pixel's cell, then the markers."""
    cnt, present = counts(mu, mv, tw, th, VW, VH)
    frames = colour(cnt, present[:, None])[:, cell_map(tw, th, W, H)]
    if markers:
        paint_markers(frames, mu, mv, VW, VH, radius)
    return np.ascontiguousarray(frames)
