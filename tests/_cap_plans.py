"""The one-lattice plans whose table rows cap at one, two and three blocks, and the cap rule that picks them, recomputed
with the oracle's geometry (shared by test_row_cap_plans.py, which runs without a GPU, and test_row_cap_blocks.py).

A table row holds the tiles closer to the direction than fov / 2.  ensure_wtab (csrc/vet_plan.hip) tries cnd = 64, 128, 192
below the uncapped stride (the longest row rounded up to 64) and stops at the first cnd that at most 1/32 of the rows
exceed; it caps there if the shortest row is longer than cnd - 64 and the longest at most cnd + 64, and not at all
otherwise.  The engine counts canonical rows (mirror partners share one), this module counts all (W + 1) * (H + 1)
directions of the grid: the fractions differ slightly, which is why every plan below sits well inside the 1/32 limit and
well above zero overflow rows."""
import numpy as np

from oracle import vet_oracle as vo

W, H = 100, 200
N_DIRS = (W + 1) * (H + 1)
POWER = 2.0
ROW_BLOCK = 64
MAX_CAP_BLOCKS = 3

# (tile_count, fov) -> expected cap; [1000] at fov 103 has 1 001 tiles, the most the compact record's tile field holds
CAPPED_PLANS = {
    (250, 119.0): 64,
    (500, 82.0): 64,
    (500, 120.0): 128,          # the plan the rest of the suite uses
    (700, 125.0): 192,
    (1000, 103.0): 192,
}
# the neighbours of each plan: (tile_count, fov) that does not cap at that block count, and one whose rows all fit
NEIGHBOURS = {
    (250, 119.0): ((250, 120.0), (250, 116.0)),
    (500, 82.0): ((500, 83.0), (500, 80.0)),
    (500, 120.0): ((500, 122.0), (500, 117.0)),
    (700, 125.0): ((700, 126.0), (700, 124.0)),
    (1000, 103.0): ((1000, 103.5), (1000, 102.0)),
}


def row_lengths(tile_count, fov, chunk=4096):
    """tiles inside fov / 2 of every direction of the grid [N_DIRS]"""
    dirs = vo.direction_grid(W, H).reshape(-1, 3)
    tiles = vo.fibonacci_lattice(tile_count)
    mx = np.radians(fov / 2.0)
    out = np.empty(len(dirs), dtype=np.int64)
    for s in range(0, len(dirs), chunk):
        out[s:s + chunk] = (vo.angular_distances(dirs[s:s + chunk], tiles) < mx).sum(axis=1)
    return out


def cap_rule(lengths):
    """(cap, rows longer than cap) as ensure_wtab decides them from the rows' lengths; cap == stride: not capped"""
    lengths = np.asarray(lengths)
    longest, shortest = int(lengths.max()), int(lengths.min())
    stride = (max(longest, 1) + ROW_BLOCK - 1) // ROW_BLOCK * ROW_BLOCK
    if stride <= ROW_BLOCK or 4 * longest < 3 * ROW_BLOCK:
        return stride, 0
    for cnd in range(ROW_BLOCK, min(stride - ROW_BLOCK, MAX_CAP_BLOCKS * ROW_BLOCK) + 1, ROW_BLOCK):
        longer = int((lengths > cnd).sum())
        if longer * 32 > lengths.size:
            continue
        if shortest > cnd - ROW_BLOCK and longest <= cnd + ROW_BLOCK:
            return cnd, longer
        break
    return stride, 0
