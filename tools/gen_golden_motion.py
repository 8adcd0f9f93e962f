#!/usr/bin/env python3
"""Golden G25: the REAL reference's ``vector_angle_distance`` between every viewer's Vectors ``lag`` frames apart.

TEST INFRASTRUCTURE ONLY, CPU only; no test runs it.  It follows tools/gen_golden_markov.py: the same 8-user x 60-frame video of
golden G15, every sample's Vector taken from golden G2's table of the reference's rounded pixel directions.  For lags 1 and 3 and
every (pair f, user u) present in frames f and f + lag it calls the reference's ``vector_angle_distance`` on the two Vectors and
keeps the value as it is — also where the two Vectors coincide, where the reference returns arccos of a rounded dot (0, or
1.5e-8 rad), the one place the engine departs from it (include/vet.h: vet_head_motion).  Arrays only are stored.

    python tools/gen_golden_motion.py [--reference /root/reference/src]

tests/golden/g25_head_motion.npz
    angles_l<lag> [60 - lag][8] f64   the reference's angle in radians, NaN where the user is absent from either frame
    same_l<lag>   [60 - lag][8] bool  the two Vectors are equal (x, y, z as numbers)
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

LAGS = (1, 3)


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
    out = {}
    for lag in LAGS:
        ang = np.full((T - lag, U), np.nan)
        same = np.zeros((T - lag, U), dtype=bool)
        for f in range(T - lag):
            for u in range(U):
                if present[f, u] and present[f + lag, u]:
                    a = Vector(*map(float, grid[py[f, u], px[f, u]]))
                    b = Vector(*map(float, grid[py[f + lag, u], px[f + lag, u]]))
                    ang[f, u] = float(vector_angle_distance(a, b))
                    same[f, u] = (a.x, a.y, a.z) == (b.x, b.y, b.z)
        out[f"angles_l{lag}"], out[f"same_l{lag}"] = ang, same
        print(f"lag {lag}: {int((~np.isnan(ang)).sum())} samples, {int(same.sum())} with the same Vector, largest reference value "
              f"there {np.nanmax(np.where(same, ang, np.nan), initial=0.0):.3e}, smallest angle elsewhere "
              f"{np.nanmin(np.where(same, np.nan, ang)):.6f}", flush=True)
    path = OUT / "g25_head_motion.npz"
    np.savez_compressed(path, **out)
    print("wrote", path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
