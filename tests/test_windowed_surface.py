"""Sliding-window (pooled) spatial entropy, CPU side: the C-ABI surface, the row arithmetic, the analyzers' argument handling,
and the claim the GPU tests rest on — "a window is one big frame" for the numpy oracle: oracle.vet_oracle.spatial_entropy_frame
on the window's concatenated directions reproduces golden G14, the REAL reference's compute_spatial_entropy on one dict that
holds every sample of the window (tools/gen_windowed_golden.py).  No GPU."""
import ctypes

import numpy as np
import pytest

from tests import _window_oracle as wo

W, H = 100, 200
SYMBOLS = ("vet_window_rows", "vet_spatial_entropy_windowed", "vet_spatial_entropy_windowed_ids",
           "vet_spatial_entropy_windowed_host")


def test_library_exports_the_windowed_entry_points():
    from viewport_entropy_toolkit import _native
    lib = ctypes.CDLL(str(_native.LIB_PATH))
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _native.SIGNATURES
    assert hasattr(_native.Plan, "spatial_windowed")


def test_window_rows_arithmetic():
    from viewport_entropy_toolkit import _native
    rows = _native.load_library().vet_window_rows
    for T in (1, 2, 7, 300, 30000):
        for w in (1, 2, 5, 20, T):
            if w > T:
                continue
            for s in (1, 3, 5, w, w + 5):
                assert rows(T, w, s) == (T - w) // s + 1 == len(range(0, T - w + 1, s))
    assert rows(300, 20, 1) == 281 and rows(300, 20, 20) == 15 and rows(300, 300, 7) == 1 and rows(30000, 20, 1) == 29981
    for bad in ((300, 0, 1), (300, -1, 1), (300, 20, 0), (300, 20, -3), (300, 301, 1), (0, 1, 1), (-5, 1, 1)):
        assert rows(*bad) < 0, bad


def test_analyzer_methods_exist_and_validate_arguments():
    from viewport_entropy_toolkit import NaiveSpatialEntropyAnalyzer, SpatialEntropyAnalyzer, ValidationError
    from viewport_entropy_toolkit.config import AnalyzerConfig, NaiveAnalyzerConfig
    mu = np.full((30, 4), 0.5)
    times = np.arange(30) * 0.1
    for an in (SpatialEntropyAnalyzer(AnalyzerConfig(tile_counts=[20])),
               NaiveSpatialEntropyAnalyzer(NaiveAnalyzerConfig(tile_height=10, tile_width=20))):
        with pytest.raises(ValidationError, match="No data available"):
            an.compute_windowed_entropy(5)
        an.load_arrays(times, mu, mu)
        for window, stride in ((0, 1), (-2, 1), (5, 0), (5, -1), (31, 1), (2.5, 1), (5, 1.5), (True, 1), ("5", 1)):
            with pytest.raises(ValueError):
                an.compute_windowed_entropy(window, stride)
        assert "rows of ``vectors_df``" in type(an).compute_windowed_entropy.__doc__


# ------------------------------------------------------------------------------------------- golden G14
def _cases(g):
    return sorted({k.rsplit("__", 1)[0] for k in g.files if "__" in k})


def _parse(tag):
    parts = tag.split("_")
    window, stride = int(parts[-2][1:]), int(parts[-1][1:])
    return parts[0], parts[1] == "w", window, stride


def test_golden_holds_the_cases_the_feature_is_pinned_on(golden_dir):
    g = np.load(golden_dir / "g14_windowed.npz")
    cases = _cases(g)
    for data in ("full", "absent"):
        for flag in "wu":
            for tcs in ("tc50", "tc50_100_200"):
                for w in (1, 5, 20):
                    for s in (1, 5):
                        assert f"{data}_{flag}_{tcs}_w{w}_s{s}" in cases
    assert any(c.startswith("naive_w_h10_w20") for c in cases) and any(c.startswith("naive_u_h10_w20") for c in cases)
    assert g["mu"].shape == (300, 8) and np.isnan(g["mu_absent"]).sum() == 80
    for c in cases:
        _, _, w, s = _parse(c)
        rows = g[f"{c}__rows"]
        assert rows[-1] == wo.n_rows(300, w, s) - 1 and len(g[f"{c}__entropy"]) == len(rows) == len(g[f"{c}__samples"])


def test_oracle_on_concatenated_directions_reproduces_the_reference(golden_dir):
    """rtol 1e-12, NaN = NaN, samples exact, lattice 0's dict (keys and values) on the three recorded rows."""
    g = np.load(golden_dir / "g14_windowed.npz")
    for tag in _cases(g):
        data, flag, window, stride = _parse(tag)
        rows = g[f"{tag}__rows"]
        if data == "naive":
            ent, samples = wo.naive(g["mu"], g["mv"], W, H, 10, 20, window, stride, use_weight_distribution=flag)
            np.testing.assert_allclose(ent[rows], g[f"{tag}__entropy"], rtol=1e-12, atol=0, equal_nan=True, err_msg=tag)
            assert np.array_equal(samples[rows], g[f"{tag}__samples"]), tag
            continue
        sfx = "" if data == "full" else "_absent"
        tcs = [int(x) for x in tag.split("_tc")[1].split("_w")[0].split("_")]
        ent, samples, weights = wo.literal(g["mu" + sfx], g["mv" + sfx], W, H, tcs, window, stride, rows=rows,
                                           use_weight_distribution=flag)
        np.testing.assert_allclose(ent, g[f"{tag}__entropy"], rtol=1e-12, atol=0, equal_nan=True, err_msg=tag)
        assert np.array_equal(samples, g[f"{tag}__samples"]), tag
        pick = np.searchsorted(rows, g[f"{tag}__weights_rows"])
        assert np.array_equal(wo.keys_of(weights[pick]), g[f"{tag}__keys"]), tag
        np.testing.assert_allclose(np.abs(weights[pick]), g[f"{tag}__weights"], rtol=1e-12, atol=0, err_msg=tag)


def test_golden_window_of_one_frame_is_the_per_frame_golden(golden_dir):
    """window = 1, stride = 1 is the per-frame series: G14's rows equal G4's (the same reference, the same inputs)."""
    g, g4 = np.load(golden_dir / "g14_windowed.npz"), np.load(golden_dir / "g4_spatial.npz")
    for tag14, tag4 in (("full_w_tc50_w1_s1", "w_tc50"), ("full_w_tc50_100_200_w1_s1", "w_tc50_100_200"), ("full_u_tc50_w1_s1", "u_tc50")):
        np.testing.assert_allclose(g[f"{tag14}__entropy"], g4[f"{tag4}__entropy"][g[f"{tag14}__rows"]], rtol=1e-13, equal_nan=True)


@pytest.mark.parametrize("flag", [True, False])
def test_fast_oracle_equals_the_literal_one(flag):
    """The series oracle of the GPU tests (per-frame sums, frames added in order) against the literal one."""
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(7, 60, base_seed=41, p_absent=0.2)
    mu[20:27] = np.nan
    mv[20:27] = np.nan
    for window, stride in ((1, 1), (5, 2), (20, 7), (60, 1)):
        a = wo.literal(mu, mv, W, H, [20, 50], window, stride, use_weight_distribution=flag)
        b = wo.fast(mu, mv, W, H, [20, 50], window, stride, use_weight_distribution=flag)
        np.testing.assert_allclose(b[0], a[0], rtol=1e-12, atol=0, equal_nan=True)
        assert np.array_equal(a[1], b[1]) and np.array_equal(wo.keys_of(a[2]), wo.keys_of(b[2]))
        np.testing.assert_allclose(b[2], a[2], rtol=1e-12, atol=0)
    assert np.isnan(wo.literal(mu, mv, W, H, [20], 5, 1)[0][21]) and wo.literal(mu, mv, W, H, [20], 5, 1)[1][21] == 0
