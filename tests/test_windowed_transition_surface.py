"""Sliding-window (pooled) transition entropy, CPU side: the C-ABI surface, the row arithmetic over frame pairs, the analyzer's
argument handling, and the claim the GPU tests rest on — the numpy oracle's dict walk on a window's pooled (source, destination)
sequence reproduces golden G15, the REAL reference's compute_transition_entropy on the pooled dicts
(tools/gen_golden_windowed_transition.py), and the closed form the kernels evaluate equals the dict walk.  No GPU."""
import ctypes

import numpy as np
import pytest

from tests import _window_transition_oracle as wt
from tests._tol import W_RTOL

W, H = 100, 200
SYMBOLS = ("vet_transition_entropy_windowed", "vet_transition_entropy_windowed_ids", "vet_transition_entropy_windowed_host")


def test_library_exports_the_windowed_transition_entry_points():
    from viewport_entropy_toolkit import _native
    lib = ctypes.CDLL(str(_native.LIB_PATH))
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _native.SIGNATURES
    assert hasattr(_native.Plan, "transition_windowed")


def test_window_rows_arithmetic_for_pairs():
    from viewport_entropy_toolkit import _native
    rows = _native.load_library().vet_window_rows
    for T in (2, 3, 8, 60, 10000):
        P = T - 1
        for w in (1, 2, 20, P):
            if w > P:
                continue
            for s in (1, 7, w, w + 5):
                assert rows(P, w, s) == wt.n_rows(T, w, s) == len(range(0, P - w + 1, s))
    assert rows(59, 20, 1) == 40 and rows(59, 20, 7) == 6 and rows(59, 59, 7) == 1 and rows(9999, 20, 1) == 9980
    assert rows(0, 1, 1) < 0 and rows(59, 60, 1) < 0          # one frame has no pair; a window longer than the pairs


def test_analyzer_method_exists_and_validates_arguments():
    from viewport_entropy_toolkit import TransitionEntropyAnalyzer, ValidationError
    from viewport_entropy_toolkit.config import AnalyzerConfig
    mu = np.full((30, 4), 0.5)
    an = TransitionEntropyAnalyzer(AnalyzerConfig(tile_counts=[20]))
    with pytest.raises(ValidationError, match="No data available"):
        an.compute_windowed_entropy(5)
    an.load_arrays(np.arange(30) * 0.1, mu, mu)
    # 30 frames are 29 pairs: a window of 30 is too long
    for window, stride in ((0, 1), (-2, 1), (5, 0), (5, -1), (30, 1), (2.5, 1), (5, 1.5), (True, 1), ("5", 1)):
        with pytest.raises(ValueError):
            an.compute_windowed_entropy(window, stride)
    assert "frame pairs" in TransitionEntropyAnalyzer.compute_windowed_entropy.__doc__


# ------------------------------------------------------------------------------------------- golden G15
def _cases(g):
    return sorted({k.rsplit("__", 1)[0] for k in g.files if "__" in k})


def _parse(tag):
    parts = tag.split("_")
    return [int(x) for x in tag[2:].split("_w")[0].split("_")], int(parts[-2][1:]), int(parts[-1][1:])


def test_golden_holds_the_cases_the_feature_is_pinned_on(golden_dir):
    g = np.load(golden_dir / "g15_windowed_transition.npz")
    cases = _cases(g)
    assert cases == sorted(f"{tcs}_w{w}_s{s}" for tcs in ("tc50", "tc50_100_200") for w in (1, 2, 20) for s in (1, 7))
    assert g["mu"].shape == (60, 8) and 0 < np.isnan(g["mu"]).sum() < 60
    total = 0
    for c in cases:
        _, w, s = _parse(c)
        rows = g[f"{c}__rows"]
        total += len(rows)
        assert rows[0] == 0 and rows[-1] == wt.n_rows(60, w, s) - 1
        assert len(g[f"{c}__entropy"]) == len(rows) == len(g[f"{c}__samples"]) == len(g[f"{c}__srccount"])
    assert total >= 40


def test_oracle_dict_walk_reproduces_the_reference(golden_dir):
    """Entropy to the relative tolerance of tests/_tol.py (NaN = NaN); samples and lattice 0's source counts exact."""
    g = np.load(golden_dir / "g15_windowed_transition.npz")
    for tag in _cases(g):
        tcs, window, stride = _parse(tag)
        ent, samples, src = wt.literal(g["mu"], g["mv"], W, H, tcs, window, stride, rows=g[f"{tag}__rows"])
        np.testing.assert_allclose(ent, g[f"{tag}__entropy"], rtol=W_RTOL, atol=0, equal_nan=True, err_msg=tag)
        assert np.array_equal(samples, g[f"{tag}__samples"]), tag
        assert np.array_equal(src, g[f"{tag}__srccount"]), tag


def test_golden_window_of_one_pair_is_the_per_pair_oracle(golden_dir):
    from oracle import vet_oracle as vo
    g = np.load(golden_dir / "g15_windowed_transition.npz")
    for tcs, tag in (([50], "tc50_w1_s1"), ([50, 100, 200], "tc50_100_200_w1_s1")):
        ent, _ = vo.transition_series(g["mu"], g["mv"], W, H, tcs, closed_form=False)
        np.testing.assert_allclose(g[f"{tag}__entropy"], ent[g[f"{tag}__rows"]], rtol=W_RTOL, equal_nan=True)


def test_closed_form_equals_the_dict_walk_on_every_row():
    """The form the kernels evaluate against the literal walk, 1e-12, on every row (none left out) — with absent samples, a
    span of frames nobody is in (empty windows: NaN in both) and one-sample windows (the reference's 0 / 0)."""
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(7, 60, base_seed=41, p_absent=0.3)
    mu[20:27] = np.nan
    mv[20:27] = np.nan
    seen_empty = seen_one = False
    for tcs in ([20], [20, 50]):
        tiles = wt.tiles_of(mu, mv, W, H, tcs)
        for window, stride in ((1, 1), (2, 1), (5, 2), (20, 7), (59, 1)):
            a = wt.literal(mu, mv, W, H, tcs, window, stride, tiles=tiles)
            b = wt.fast(mu, mv, W, H, tcs, window, stride, tiles=tiles)
            assert len(a[0]) == wt.n_rows(60, window, stride)
            np.testing.assert_allclose(b[0], a[0], rtol=1e-12, atol=0, equal_nan=True)
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[2].sum(axis=1), a[1])
            assert np.array_equal(np.isnan(a[0][a[1] == 0]), np.ones((a[1] == 0).sum(), dtype=bool))
            seen_empty |= bool((a[1] == 0).any())
            seen_one |= bool((a[1] == 1).any()) and bool(np.isnan(a[0][a[1] == 1]).all())
    assert seen_empty and seen_one
