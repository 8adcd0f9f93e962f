"""The formulation rule of fp64 plans (vet_plan_set_fp64, include/vet.h formulation 4), restated for the tests.

A lattice of n tiles runs `dtable` where the table rule asks for a table and its exact FP64 weight rows fit the LDS at the
weights pass's wave count NW (4, 2 or 1: the FP64 histograms of all waves, plus the per-wave user counts), and `precise`
otherwise.  The LDS limit is the one the engine sets on MI355X: half of the 160 KiB of a CU, so that two workgroups stay
resident (vet_context.hip).  Fibonacci lattices have an odd number of tiles, at most 6783 (the plan's LDS tile cache), and
every such size fits; a requested table still falls to `precise` where the lattice has no exact rows (VET_NO_EXACT_ROWS, or
the plan-wide cap on their memory)."""
LDS_MAX = 80 * 1024


def weights_nw(n: int) -> int:
    """Waves per workgroup of the weights pass over a lattice of n tiles (vet_spatial.hip: weights_nw)."""
    nw = 4
    while nw > 1 and nw * n * 8 > LDS_MAX:
        nw //= 2
    return nw


def dtable_fits(n: int) -> bool:
    """k_spatial_dtable's LDS for one lattice of n tiles at the weights pass's NW (vet_spatial_dtable.hpp)."""
    nw = weights_nw(n)
    return nw * n * 8 + ((nw * 4 + 7) & ~7) <= LDS_MAX


def fp64_form(n: int, table_asked: bool) -> str:
    return "dtable" if table_asked and dtable_fits(n) else "precise"
