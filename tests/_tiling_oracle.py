"""numpy oracle of the tilings drawn on the unit sphere (include/vet.h, vet_tiling_*).

The frame definition the engine renders: arcs -> 49 chords between spherical_interpolation points (reference
utilities/data_utils.py:503-518 at np.linspace(0, 1, 50)), a parallel projection from a camera (P, U, F), line / point /
disc coverage per pixel centre and the colour rule.  FP64 throughout, in the engine's operation order.

``render_frame`` also returns an *ambiguous* mask: pixels whose outcome hangs on a comparison so close to its threshold
that a last-bit difference of the device's sin / acos from numpy's could flip it (a chord's distance within 1e-6 of 1 or
its depth within 1e-12 of 0, a centre's offset within 1e-6 of 5, the disc test within 1e-9 relative).  Device frames
equal the oracle's everywhere else.
"""
from __future__ import annotations

import math

import numpy as np

SIN15 = 0.25881904510252074          # sin(15 degrees): parallel scale of a 30-degree view angle
RED, BLACK = (255, 0, 0), (0, 0, 0)
LINE_EPS, POINT_EPS, DISC_EPS, DEPTH_EPS = 1e-6, 1e-6, 1e-9, 1e-12


def chord_points(arcs) -> np.ndarray:
    """[n, 2, 3] arcs -> [n, 50, 3] slerp points; NaN for coincident or antipodal ends (sin(theta) == 0 or a clipped
    cosine of -1: sin(pi) is not 0 in FP64)."""
    arcs = np.asarray(arcs, dtype=np.float64).reshape(-1, 2, 3)
    a, b = arcs[:, 0], arcs[:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        la = np.sqrt(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2])
        lb = np.sqrt(b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1] + b[:, 2] * b[:, 2])
        ah, bh = a / la[:, None], b / lb[:, None]
        cosine = np.clip(ah[:, 0] * bh[:, 0] + ah[:, 1] * bh[:, 1] + ah[:, 2] * bh[:, 2], -1.0, 1.0)
        theta = np.arccos(cosine)
        st = np.sin(theta)
        t = np.linspace(0, 1, 50)
        s1 = np.sin((1 - t)[None, :] * theta[:, None])[..., None]
        s2 = np.sin(t[None, :] * theta[:, None])[..., None]
        pts = (s1 * ah[:, None, :] + s2 * bh[:, None, :]) / st[:, None, None]
    pts[(st == 0.0) | (cosine == -1.0)] = np.nan
    return pts


def camera(c9, W: int, H: int):
    """(P, U, F) -> dict(F, r, u, nd, s, X0, Y0) exactly as the engine's host code computes it; ValueError if degenerate."""
    P, U, F = (tuple(float(x) for x in v) for v in np.asarray(c9, dtype=np.float64).reshape(3, 3))
    vx, vy, vz = P[0] - F[0], P[1] - F[1], P[2] - F[2]
    dist = math.sqrt(vx * vx + vy * vy + vz * vz)
    if not dist > 0:
        raise ValueError("position == focal point")
    d = ((F[0] - P[0]) / dist, (F[1] - P[1]) / dist, (F[2] - P[2]) / dist)
    x = (d[1] * U[2] - d[2] * U[1], d[2] * U[0] - d[0] * U[2], d[0] * U[1] - d[1] * U[0])
    xl = math.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])
    if not xl > 0:
        raise ValueError("view-up parallel to the view direction")
    r = (x[0] / xl, x[1] / xl, x[2] / xl)
    u = (r[1] * d[2] - r[2] * d[1], r[2] * d[0] - r[0] * d[2], r[0] * d[1] - r[1] * d[0])
    s = 2.0 * dist * SIN15 / H
    ox, oy, oz = 0.0 - F[0], 0.0 - F[1], 0.0 - F[2]
    X0 = W / 2.0 + (ox * r[0] + oy * r[1] + oz * r[2]) / s
    Y0 = H / 2.0 - (ox * u[0] + oy * u[1] + oz * u[2]) / s
    return dict(F=F, r=r, u=u, nd=(-d[0], -d[1], -d[2]), d=d, s=s, X0=X0, Y0=Y0)


def project(p: np.ndarray, c, W: int, H: int):
    vx, vy, vz = p[..., 0] - c["F"][0], p[..., 1] - c["F"][1], p[..., 2] - c["F"][2]
    r, u, s = c["r"], c["u"], c["s"]
    X = W / 2.0 + (vx * r[0] + vy * r[1] + vz * r[2]) / s
    Y = H / 2.0 - (vx * u[0] + vy * u[1] + vz * u[2]) / s
    return X, Y


def _depth(p, c):
    nd = c["nd"]
    return p[..., 0] * nd[0] + p[..., 1] * nd[1] + p[..., 2] * nd[2]


def _splat_lines(pts, c, W, H, front, back, amb):
    P0 = pts[:, :-1].reshape(-1, 3)
    P1 = pts[:, 1:].reshape(-1, 3)
    ok = np.isfinite(P0).all(1) & np.isfinite(P1).all(1)
    P0, P1 = P0[ok], P1[ok]
    Ax, Ay = project(P0, c, W, H)
    Bx, By = project(P1, c, W, H)
    ok = np.isfinite(Ax) & np.isfinite(Ay) & np.isfinite(Bx) & np.isfinite(By)
    P0, P1, Ax, Ay, Bx, By = P0[ok], P1[ok], Ax[ok], Ay[ok], Bx[ok], By[ok]
    # candidate window per chord: bounding box grown by 2 pixels, clipped to the frame
    c0 = np.clip(np.floor(np.minimum(Ax, Bx) - 2.5), -1, W).astype(np.int64)
    c1 = np.clip(np.ceil(np.maximum(Ax, Bx) + 1.5), -1, W).astype(np.int64)
    r0 = np.clip(np.floor(np.minimum(Ay, By) - 2.5), -1, H).astype(np.int64)
    r1 = np.clip(np.ceil(np.maximum(Ay, By) + 1.5), -1, H).astype(np.int64)
    keep = (c1 >= 0) & (c0 < W) & (r1 >= 0) & (r0 < H)
    P0, P1, Ax, Ay, Bx, By, c0, c1, r0, r1 = (v[keep] for v in (P0, P1, Ax, Ay, Bx, By, c0, c1, r0, r1))
    if len(Ax) == 0:
        return
    ex, ey = Bx - Ax, By - Ay
    len2 = ex * ex + ey * ey
    for oy in range(int((r1 - r0).max()) + 1):
        for ox in range(int((c1 - c0).max()) + 1):
            col, row = c0 + ox, r0 + oy
            m = (col <= c1) & (row <= r1) & (col >= 0) & (col < W) & (row >= 0) & (row < H)
            if not m.any():
                continue
            qx, qy = col[m] + 0.5, row[m] + 0.5
            ax, ay, exm, eym, l2 = Ax[m], Ay[m], ex[m], ey[m], len2[m]
            with np.errstate(divide="ignore", invalid="ignore"):
                tau = np.where(l2 > 0, ((qx - ax) * exm + (qy - ay) * eym) / np.where(l2 > 0, l2, 1.0), 0.0)
            tau = np.minimum(np.maximum(tau, 0.0), 1.0)
            dx, dy = qx - (ax + tau * exm), qy - (ay + tau * eym)
            d2 = dx * dx + dy * dy
            hit = d2 <= 1.0
            p0, p1 = P0[m], P1[m]
            p = p0 + tau[:, None] * (p1 - p0)
            depth = _depth(p, c)
            rr, cc = row[m], col[m]
            front[rr[hit & (depth > 0)], cc[hit & (depth > 0)]] = True
            back[rr[hit & ~(depth > 0)], cc[hit & ~(depth > 0)]] = True
            near = (np.abs(np.sqrt(d2) - 1.0) <= LINE_EPS) | (hit & (np.abs(depth) <= DEPTH_EPS))
            amb[rr[near], cc[near]] = True


def _splat_points(centres, c, W, H, front, back, amb):
    centres = centres[np.isfinite(centres).all(1)]
    X, Y = project(centres, c, W, H)
    ok = np.isfinite(X) & np.isfinite(Y)
    centres, X, Y = centres[ok], X[ok], Y[ok]
    depth = _depth(centres, c)
    c0 = np.clip(np.floor(X - 6.5), -1, W).astype(np.int64)
    r0 = np.clip(np.floor(Y - 6.5), -1, H).astype(np.int64)
    for oy in range(13):
        for ox in range(13):
            col, row = c0 + ox, r0 + oy
            m = (col >= 0) & (col < W) & (row >= 0) & (row < H)
            ax, ay = np.abs(X[m] - (col[m] + 0.5)), np.abs(Y[m] - (row[m] + 0.5))
            hit = (ax < 5.0) & (ay < 5.0)
            dp = depth[m]
            rr, cc = row[m], col[m]
            front[rr[hit & (dp > 0)], cc[hit & (dp > 0)]] = True
            back[rr[hit & ~(dp > 0)], cc[hit & ~(dp > 0)]] = True
            # a centre's depth takes no sin / acos (the centre as given, the host's camera): it is exact on the device too,
            # so a centre on the silhouette (depth ~1e-16, e.g. frame 90 of the vertical orbit) is not ambiguous
            near = (((np.abs(ax - 5.0) <= POINT_EPS) & (ay < 5.0 + POINT_EPS)) |
                    ((np.abs(ay - 5.0) <= POINT_EPS) & (ax < 5.0 + POINT_EPS)))
            amb[rr[near], cc[near]] = True


def blend(x) -> np.ndarray:
    """Grey 128 at opacity 0.3 over x, per channel."""
    return np.floor(0.3 * 128.0 + 0.7 * np.asarray(x, dtype=np.float64) + 0.5).astype(np.uint8)


def render_frame(pts: np.ndarray, centres, cam9, W: int, H: int, background=(255, 255, 255)):
    """One frame: (uint8 [H, W, 3], ambiguous bool [H, W], flags dict).  ``pts`` = chord_points(arcs)."""
    c = camera(cam9, W, H)
    fl, bl, fp, bp, amb = (np.zeros((H, W), dtype=bool) for _ in range(5))
    _splat_lines(pts, c, W, H, fl, bl, amb)
    if centres is not None and len(centres):
        _splat_points(np.asarray(centres, dtype=np.float64).reshape(-1, 3), c, W, H, fp, bp, amb)
    Xq = np.arange(W, dtype=np.float64)[None, :] + 0.5
    Yq = np.arange(H, dtype=np.float64)[:, None] + 0.5
    dx, dy = Xq - c["X0"], Yq - c["Y0"]
    v = (dx * dx + dy * dy) * (c["s"] * c["s"])
    disc = v <= 1.0
    amb |= np.abs(v - 1.0) <= DISC_EPS
    bg = np.asarray(background, dtype=np.uint8)
    under = np.where(bp[..., None], np.uint8(RED), np.where(bl[..., None], np.uint8(BLACK), bg)).astype(np.uint8)
    img = np.where(fp[..., None], np.uint8(RED), np.where(fl[..., None], np.uint8(BLACK),
                                                          np.where(disc[..., None], blend(under), under)))
    return img.astype(np.uint8), amb, dict(front_line=fl, back_line=bl, front_point=fp, back_point=bp, disc=disc)


def render(arcs, centres, cameras, W: int, H: int, background=(255, 255, 255)):
    """[n, 3, 3] cameras -> (uint8 [n, H, W, 3], ambiguous [n, H, W])."""
    pts = chord_points(arcs)
    cams = np.asarray(cameras, dtype=np.float64).reshape(-1, 3, 3)
    out = [render_frame(pts, centres, c9, W, H, background)[:2] for c9 in cams]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
