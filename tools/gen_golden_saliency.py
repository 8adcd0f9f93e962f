#!/usr/bin/env python3
"""Golden G27: the REAL reference's ``Vector.from_spherical`` of the cell centres of a 12 x 6 saliency map and its
``vector_angle_distance`` between them and 40 of golden G2's pixel Vectors.

TEST INFRASTRUCTURE ONLY, CPU only; no test runs it.  It follows tools/gen_golden_dispersion.py.  The map's cell (c, y) has its
centre at lon = (c + 0.5) / 12 * 360 - 180, lat = 90 - (y + 0.5) / 6 * 180 (row 0 at the top; include/vet.h: vet_saliency); the
reference's Vector there is rounded to 6 decimals, which the engine's cell direction is not.  The 40 pixel Vectors are rows of
golden G2's table of the reference's rounded pixel directions of the 100 x 200 grid: both pole rows, the seam columns and a fixed
random draw.  Arrays only are stored.

    python tools/gen_golden_saliency.py [--reference /root/reference/src]

tests/golden/g27_saliency.npz
    cells   [72][3] f64    the reference's Vector of every cell centre, row-major
    lonlat  [72][2] f64    the centre's lon, lat in degrees as passed to the reference
    pixels  [40][3] f64    the pixel Vectors (from golden G2)
    pix_id  [40] i32       their direction ids py * 101 + px
    angles  [72][40] f64   the reference's vector_angle_distance(cell, pixel) in radians
"""
from __future__ import annotations

import argparse
import os
import sys
import types
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
OUT = REPO / "tests" / "golden"
MAP_W, MAP_H, GRID_W, GRID_H = 12, 6, 100, 200


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default="/root/reference/src")
    args = ap.parse_args()
    if not Path(args.reference).exists():
        sys.exit(f"reference not found at {args.reference}; nothing to do")
    grid = np.load(OUT / "g2_quantiser.npz")["vec_100x200"]            # the reference's rounded Vector of every pixel
    rng = np.random.default_rng(27)
    fixed = [(0, 0), (50, 0), (100, 0), (0, 200), (37, 200), (100, 200), (0, 100), (100, 100), (50, 100), (25, 50), (75, 150), (1, 1)]
    drawn = [(int(x), int(y)) for x, y in zip(rng.integers(0, GRID_W + 1, 28), rng.integers(0, GRID_H + 1, 28))]
    pix = fixed + drawn
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.dont_write_bytecode = True
    sys.modules.setdefault("pyvista", types.ModuleType("pyvista"))
    sys.path.insert(0, args.reference)
    from viewport_entropy_toolkit import Vector  # the reference
    from viewport_entropy_toolkit.utilities import vector_angle_distance
    pixels = [Vector(*map(float, grid[y, x])) for x, y in pix]
    cells, lonlat = [], []
    for y in range(MAP_H):
        for c in range(MAP_W):
            lon, lat = (c + 0.5) / MAP_W * 360.0 - 180.0, 90.0 - (y + 0.5) / MAP_H * 180.0
            cells.append(Vector.from_spherical(lon, lat))
            lonlat.append((lon, lat))
    ang = np.array([[float(vector_angle_distance(a, b)) for b in pixels] for a in cells])
    path = OUT / "g27_saliency.npz"
    np.savez_compressed(path, cells=np.array([[v.x, v.y, v.z] for v in cells]), lonlat=np.array(lonlat),
                        pixels=np.array([[v.x, v.y, v.z] for v in pixels]), pix_id=np.array([y * (GRID_W + 1) + x for x, y in pix], dtype=np.int32),
                        angles=ang)
    print(f"{ang.shape} angles in [{ang.min():.6f}, {ang.max():.6f}]", flush=True)
    print("wrote", path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
