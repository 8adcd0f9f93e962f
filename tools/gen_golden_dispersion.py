#!/usr/bin/env python3
"""Golden G26: the REAL reference's ``vector_angle_distance`` between the Vectors of every two viewers present in one frame.

TEST INFRASTRUCTURE ONLY, CPU only; no test runs it.  It follows tools/gen_golden_motion.py: the same 8-user x 60-frame video of
golden G15, every sample's Vector taken from golden G2's table of the reference's rounded pixel directions.  For every frame and
every pair (u, v), u != v, both present, it calls the reference's ``vector_angle_distance`` on the two Vectors and keeps the value
as it is — also where the two Vectors coincide, where the reference returns arccos of a rounded dot (0, or 1.5e-8 rad), the one
place the engine departs from it (include/vet.h: vet_dispersion).  Arrays only are stored.

    python tools/gen_golden_dispersion.py [--reference /root/reference/src]

tests/golden/g26_dispersion.npz
    angles [60][8][8] f64   the reference's angle in radians, NaN where either user is absent and on the diagonal
    same   [60][8][8] bool  the two Vectors are equal (x, y, z as numbers)
The dataset is golden G15's mu / mv.
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
sys.path.insert(0, str(REPO / "tools"))
from gen_golden_windowed_transition import T, U, dataset  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default="/root/reference/src")
    args = ap.parse_args()
    if not Path(args.reference).exists():
        sys.exit(f"reference not found at {args.reference}; nothing to do")
    mu, mv = dataset()
    sys.path.insert(0, str(REPO))
    from oracle import vet_oracle as vo
    px, py, present, _ = vo.sample_directions(mu, mv, 100, 200)        # the quantiser pinned by golden G2
    grid = np.load(OUT / "g2_quantiser.npz")["vec_100x200"]            # the reference's rounded Vector of every pixel
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.dont_write_bytecode = True
    sys.modules.setdefault("pyvista", types.ModuleType("pyvista"))
    sys.path.insert(0, args.reference)
    from viewport_entropy_toolkit import Vector  # the reference
    from viewport_entropy_toolkit.utilities import vector_angle_distance
    ang = np.full((T, U, U), np.nan)
    same = np.zeros((T, U, U), dtype=bool)
    for f in range(T):
        vec = [Vector(*map(float, grid[py[f, u], px[f, u]])) if present[f, u] else None for u in range(U)]
        for u in range(U):
            for v in range(U):
                if u != v and vec[u] is not None and vec[v] is not None:
                    a, b = vec[u], vec[v]
                    ang[f, u, v] = float(vector_angle_distance(a, b))
                    same[f, u, v] = (a.x, a.y, a.z) == (b.x, b.y, b.z)
    print(f"{int((~np.isnan(ang)).sum()) // 2} pair samples, {int(same.sum()) // 2} with the same Vector, largest reference value "
          f"there {np.nanmax(np.where(same, ang, np.nan), initial=0.0):.3e}, smallest angle elsewhere "
          f"{np.nanmin(np.where(same, np.nan, ang)):.6f}", flush=True)
    path = OUT / "g26_dispersion.npz"
    np.savez_compressed(path, angles=ang, same=same)
    print("wrote", path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
