"""Why tests/test_row_cap_blocks.py uses the plans it uses: the row lengths of each plan, recomputed with the oracle's geometry,
put through ensure_wtab's cap rule (tests/_cap_plans.py).  Runs without a GPU; fails if the oracle's lattice or grid changes under
the plans, before a GPU test quietly lands on another kernel.

Per direction of the 100 x 200 grid, power 2.0 (min / max row length, directions over the cap):
  [250]  fov 119   57 /  66   316 over  64   one block        neighbours: fov 120 7.8 % over 64 (no cap), fov 116 none over
  [500]  fov  82   57 /  66   192 over  64   one block                    fov  83 11 % over 64,           fov  80 none over
  [500]  fov 120  120 / 131   308 over 128   two blocks                   fov 122 66 % over 128,          fov 117 none over
  [700]  fov 125  181 / 195   226 over 192   three blocks                 fov 126 24 % over 192,          fov 124 none over
  [1000] fov 103  182 / 195   382 over 192   three blocks                 fov 103.5 13 % over 192,        fov 102 none over
"""
import pytest

from tests import _cap_plans as cp


@pytest.mark.parametrize("plan", sorted(cp.CAPPED_PLANS), ids=lambda p: f"{p[0]}@{p[1]:g}")
def test_the_plan_caps_where_the_gpu_tests_expect(plan):
    want = cp.CAPPED_PLANS[plan]
    lengths = cp.row_lengths(*plan)
    cap, longer = cp.cap_rule(lengths)
    print(f"{plan}: rows {lengths.min()}..{lengths.max()}, cap {cap}, {longer} of {lengths.size} directions longer")
    assert cap == want
    # well inside the rule on both sides: the engine counts canonical rows, whose fractions differ slightly
    assert 64 <= longer <= lengths.size // 48
    assert lengths.min() > cap - cp.ROW_BLOCK and cap < lengths.max() <= cap + cp.ROW_BLOCK
    # the overflow tail of a row fits well inside its one side-table block
    assert lengths.max() - cap <= 8


@pytest.mark.parametrize("plan", sorted(cp.CAPPED_PLANS), ids=lambda p: f"{p[0]}@{p[1]:g}")
def test_the_neighbours_do_not(plan):
    """a slightly wider field of view has too many long rows to cap at that block count, a slightly narrower one none"""
    want = cp.CAPPED_PLANS[plan]
    wider, narrower = cp.NEIGHBOURS[plan]
    lw, ln = cp.row_lengths(*wider), cp.row_lengths(*narrower)
    cap_w, longer_w = cp.cap_rule(lw)
    print(f"{wider}: rows {lw.min()}..{lw.max()}, {(lw > want).sum()} over {want}, cap {cap_w}")
    assert (lw > want).sum() * 32 > 2 * lw.size, "clearly more than 1/32 of the rows"
    assert cap_w == want + cp.ROW_BLOCK and longer_w == 0, "whole rows of one more block: not capped"
    cap_n, longer_n = cp.cap_rule(ln)
    print(f"{narrower}: rows {ln.min()}..{ln.max()}, cap {cap_n}")
    assert ln.max() <= want and (cap_n, longer_n) == (want, 0), "every row fits: stride == cap, no side table"


def test_the_tile_field_of_the_compact_record_is_full():
    from oracle import vet_oracle as vo
    assert len(vo.fibonacci_lattice(1000)) == 1001 and (1000, 103.0) in cp.CAPPED_PLANS


def test_the_rule_on_made_up_rows():
    """cap_rule is ensure_wtab's loop: the first block count that at most 1/32 of the rows exceed decides"""
    import numpy as np
    base = np.full(3200, 60)
    assert cp.cap_rule(base) == (64, 0)                                  # stride 64: nothing to cap
    rows = base.copy(); rows[:100] = 66
    assert cp.cap_rule(rows) == (64, 100)
    rows[:101] = 66
    assert cp.cap_rule(rows) == (128, 0)                                 # 101 * 32 > 3200; 128 is the stride itself
    rows = base.copy(); rows[0] = 129
    assert cp.cap_rule(rows) == (192, 0)                                 # longest beyond cap + 64: whole rows
    rows = np.full(3200, 190); rows[:50] = 200; rows[50] = 128
    assert cp.cap_rule(rows) == (256, 0)                                 # a row that ends before the last block
    rows[50] = 129
    assert cp.cap_rule(rows) == (192, 50)
    assert cp.cap_rule(np.full(10, 300)) == (320, 0)                     # beyond three blocks
    rows = np.full(3200, 250); rows[:10] = 257
    assert cp.cap_rule(rows) == (320, 0)                                 # a cap of four blocks is not built
