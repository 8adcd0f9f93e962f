"""numpy oracle of the per-frame tile-attention heatmaps (include/vet.h, vet_heatmap_*).

The frame definition the engine renders, restated from the reference's animation
(utilities/visualization_utils.py:99-204: PlotManager.update_frame / _get_color_from_intensity)
and its pixel quantiser (normalize_to_pixel, utilities/data_utils.py:243-261).
"""
from __future__ import annotations

import numpy as np

GREY = 0.8


def colour(w, n):
    """_get_color_from_intensity(w / n) as bytes: uint8 [..., 3].  Intensity 0 where n == 0; FP64 in the reference's
    operation order; byte = floor(v * 255 + 0.5)."""
    w = np.asarray(w, dtype=np.float64)
    n = np.broadcast_to(np.asarray(n), w.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        i = np.where(n > 0, w / np.where(n > 0, n, 1).astype(np.float64), 0.0)
    i = np.clip(i, 0, 1)
    red = (i * (1 - GREY)) + GREY
    gb = GREY - (i * GREY)
    rgb = np.stack([red, gb, gb], axis=-1)
    return np.floor(rgb * 255 + 0.5).astype(np.uint8)


def pixel_dirs(W: int, H: int) -> np.ndarray:
    """Unit direction of every pixel centre, [H*W, 3]: Vector.from_spherical without its rounding, normalised."""
    c = np.arange(W, dtype=np.float64)
    r = np.arange(H, dtype=np.float64)
    lon = (c + 0.5) / W * 360 - 180
    lat = 90 - (r + 0.5) / H * 180
    theta = np.radians(np.broadcast_to(lon[None, :], (H, W)).ravel())
    phi = np.radians(90 - np.broadcast_to(lat[:, None], (H, W)).ravel())
    xyz = np.stack([np.sin(phi) * np.cos(theta), np.sin(phi) * np.sin(theta), np.cos(phi)], axis=-1)
    return xyz / np.linalg.norm(xyz, axis=1, keepdims=True)


def unit(tiles: np.ndarray) -> np.ndarray:
    tiles = np.asarray(tiles, dtype=np.float64).reshape(-1, 3)
    return tiles / np.linalg.norm(tiles, axis=1, keepdims=True)


def distances(dirs: np.ndarray, tiles: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """vector_angle_distance from each direction to tile idx[i] (unit inputs)."""
    t = unit(tiles)[idx]
    return np.arccos(np.clip(np.einsum("ij,ij->i", dirs, t), -1.0, 1.0))


def nearest_map(tiles: np.ndarray, W: int, H: int, chunk: int = 1 << 15) -> np.ndarray:
    """find_nearest_tile of every pixel centre: the FIRST minimum of arccos(clip(dot)), int32 [H, W].  arccos runs only
    on the tiles whose cosine is within 1e-12 of the best (arccos is monotone: the others are strictly farther)."""
    dirs, t = pixel_dirs(W, H), unit(tiles)
    out = np.empty(len(dirs), dtype=np.int64)
    for s in range(0, len(dirs), chunk):
        cos = dirs[s:s + chunk] @ t.T
        cand = cos >= cos.max(axis=1, keepdims=True) - 1e-12
        d = np.full(cos.shape, np.inf)
        d[cand] = np.arccos(np.clip(cos[cand], -1.0, 1.0))
        out[s:s + chunk] = np.argmin(d, axis=1)
    return out.reshape(H, W).astype(np.int32)


def near_ties(dev_map: np.ndarray, tiles: np.ndarray, W: int, H: int, ulps: int = 4):
    """(pixels where dev_map differs from the oracle, of which within `ulps` ulp of the oracle's minimum distance)."""
    ref = nearest_map(tiles, W, H)
    diff = np.flatnonzero(dev_map.ravel() != ref.ravel())
    if len(diff) == 0:
        return 0, 0
    dirs = pixel_dirs(W, H)[diff]
    d_ref = distances(dirs, tiles, ref.ravel()[diff])
    d_dev = distances(dirs, tiles, dev_map.ravel()[diff])
    ok = np.abs(d_dev - d_ref) <= ulps * np.spacing(d_ref)
    return len(diff), int(ok.sum())


def marker_centres(mu, mv, VW: int, VH: int, W: int, H: int):
    """(row, col) int64 arrays of the viewport pixel of every sample, -1 where absent (NaN) or outside [0, 1]."""
    mu = np.asarray(mu, dtype=np.float64)
    mv = np.asarray(mv, dtype=np.float64)
    ok = (mu >= 0) & (mu <= 1) & (mv >= 0) & (mv <= 1)          # False for NaN
    px = np.where(ok, np.trunc(np.where(ok, mu, 0) * VW), 0).astype(np.int64)
    py = np.where(ok, np.trunc(np.where(ok, mv, 0) * VH), 0).astype(np.int64)
    col = np.minimum(px * W // VW, W - 1)
    row = np.minimum(py * H // VH, H - 1)
    return np.where(ok, row, -1), np.where(ok, col, -1)


def paint_markers(frames: np.ndarray, mu, mv, VW: int, VH: int, radius: int) -> np.ndarray:
    """Black (2 radius + 1)^2 squares on frames [T, H, W, 3] in place: columns wrap, rows clamp."""
    T, H, W, _ = frames.shape
    row, col = marker_centres(mu, mv, VW, VH, W, H)
    for t in range(T):
        for r0, c0 in zip(row[t], col[t]):
            if r0 < 0:
                continue
            rows = np.arange(max(r0 - radius, 0), min(r0 + radius, H - 1) + 1)
            cols = np.arange(c0 - radius, c0 + radius + 1) % W
            frames[t][np.ix_(rows, cols)] = 0
    return frames


def render(tile_map: np.ndarray, weights: np.ndarray, present: np.ndarray, mu=None, mv=None, VW: int = 0, VH: int = 0,
           radius: int = 2) -> np.ndarray:
    """Frames [T, H, W, 3]: the palette of every frame gathered through ``tile_map``, then the markers."""
    pal = colour(weights, np.asarray(present)[:, None])          # [T, n, 3]
    frames = pal[:, tile_map]                                      # [T, H, W, 3]
    if mu is not None:
        paint_markers(frames, mu, mv, VW, VH, radius)
    return np.ascontiguousarray(frames)
