"""Window-to-window attention divergence (a lag band of Jensen-Shannon distances), CPU side: the C-ABI surface, the analyzers'
argument handling and result frame, and the claim the GPU tests rest on — the numpy oracles of tests/_window_divergence_oracle.py
reproduce golden G19, the REAL reference's compute_spatial_entropy / compute_naive_spatial_entropy on the dicts of row r, of row
r + l and of both (tools/gen_golden_window_divergence.py).  No GPU."""
import ctypes

import numpy as np
import pytest

from tests import _window_divergence_oracle as wdo
from tests import _window_oracle as wo

W, H = 100, 200
SYMBOLS = ("vet_window_divergence", "vet_window_divergence_ids", "vet_window_divergence_host",
           "vet_test_window_divergence_chunk_rows")
SHAPES = ((20, 20, 14), (20, 5, 8), (5, 1, 6), (1, 1, 3))          # (window, stride, max_lag)
CASES = ((True, [50]), (True, [50, 100, 200]), (False, [50]))
ATOL = 1e-12


@pytest.fixture(scope="module")
def g14(golden_dir):
    return np.load(golden_dir / "g14_windowed.npz")


@pytest.fixture(scope="module")
def g19(golden_dir):
    return np.load(golden_dir / "g19_window_divergence.npz")


def same(got, want, msg):
    err = float(np.nanmax(np.abs(got - want), initial=0.0))
    print(msg, "max abs err", err)
    assert np.array_equal(np.isnan(got), np.isnan(want)), msg
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL, equal_nan=True, err_msg=msg)


def tag_of(flag, tcs, w, s, L):
    return f"{'w' if flag else 'u'}_tc{'_'.join(map(str, tcs))}_w{w}_s{s}_l{L}"


def test_library_exports_the_window_divergence_entry_points():
    from viewport_entropy_toolkit import _native
    lib = ctypes.CDLL(str(_native.LIB_PATH))
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _native.SIGNATURES
    # vet_user_divergence's signatures with max_lag behind the stride
    for tail, at in (("", 7), ("_ids", 6), ("_host", 8)):
        res, args = _native.SIGNATURES["vet_user_divergence" + tail]
        assert _native.SIGNATURES["vet_window_divergence" + tail] == (res, args[:at] + [ctypes.c_int] + args[at:])
    for name in ("spatial_window_divergence", "spatial_window_divergence_device"):
        assert hasattr(_native.Plan, name)
    assert hasattr(_native.Engine, "test_window_divergence_chunk_rows")
    assert _native.load_library().vet_version() == 141


def test_header_and_ctypes_table_agree():
    import re
    from pathlib import Path
    from viewport_entropy_toolkit import _native
    text = re.sub(r"/\*.*?\*/", "", (Path(__file__).resolve().parent.parent / "include" / "vet.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(vet_[a-z0-9_]+)\s*\(", text))
    assert set(SYMBOLS) <= declared and declared == set(_native.SIGNATURES)
    for name in SYMBOLS:                # argument counts of the declarations
        args = re.search(rf"\b{name}\s*\(([^)]*)\)", text).group(1)
        assert len(args.split(",")) == len(_native.SIGNATURES[name][1]), name


# ------------------------------------------------------------------------------------------- golden G19
def test_golden_holds_the_cases_the_feature_is_pinned_on(g14, g19):
    mu = g14["mu_absent"]
    present = (~np.isnan(mu)).sum(axis=1)
    for w, s, L in SHAPES:
        R = wo.n_rows(300, w, s)
        tags = [tag_of(f, t, w, s, L) for f, t in CASES] + [f"naive_h10_w20_w{w}_s{s}_l{L}"]
        for tag in tags:
            rows = g19[f"{tag}__rows"]
            m, K = len(rows), 3 if "50_100_200" in tag else 1
            assert rows[0] == 0 and rows[-1] == R - 2 and (np.diff(rows) > 0).all(), tag
            if (w, s) == (20, 20):
                assert np.array_equal(rows, np.arange(R - 1)), tag                  # every pair
            else:
                assert set(range(0, R - 1, 7)) <= set(rows) and set(range(R - 2 - L, R - 1)) <= set(rows), tag
            D = g19[f"{tag}__divergence"]
            assert D.shape == (m, L) and g19[f"{tag}__samples"].shape == (m,), tag
            for name in ("bits", "total"):
                assert g19[f"{tag}__{name}"].shape == (m, K, L, 3), (tag, name)
            assert np.array_equal(g19[f"{tag}__samples"], [present[r * s:r * s + w].sum() for r in rows]), tag
            # NaN exactly where there is no partner row (this dataset has no empty window and no zero-valued key)
            lag = np.arange(1, L + 1)
            assert np.array_equal(np.isnan(D), rows[:, None] + lag[None, :] >= R), tag
            total = g19[f"{tag}__total"]
            with np.errstate(all="ignore"):
                bound = wdo.h2(total[..., 0] / (total[..., 0] + total[..., 1])).mean(axis=1)
            ok = ~np.isnan(D)
            assert (D[ok] >= -1e-12).all() and (D[ok] <= bound[ok] + 1e-12).all(), tag
            # the pooled dict holds both windows' mass
            np.testing.assert_allclose(total[..., 2][:, 0][ok], (total[..., 0] + total[..., 1])[:, 0][ok], rtol=1e-12)
        assert np.nanmax(g19[f"{tags[0]}__divergence"]) > 0.01                      # the attention does move


@pytest.mark.parametrize("w,s,L", SHAPES)
def test_literal_and_fast_oracles_reproduce_the_reference(g14, g19, w, s, L):
    """atol 1e-12 on D and on the three terms, NaN = NaN, samples exact, on every stored row."""
    mu, mv = g14["mu_absent"], g14["mv_absent"]
    for flag, tcs in CASES:
        tag = tag_of(flag, tcs, w, s, L)
        rows = g19[f"{tag}__rows"]
        div, samples, S, tot = wdo.fast(mu, mv, W, H, tcs, w, s, L, use_weight_distribution=flag, want_terms=True)
        same(div[rows], g19[f"{tag}__divergence"], tag + " fast")
        assert np.array_equal(samples[rows], g19[f"{tag}__samples"]), tag
        same(S[rows], g19[f"{tag}__bits"], tag + " fast S")
        np.testing.assert_allclose(tot[rows], g19[f"{tag}__total"], rtol=1e-12, atol=0, err_msg=tag)
        pick = np.arange(len(rows))
        div, samples, S, tot = wdo.literal(mu, mv, W, H, tcs, w, s, L, rows=rows, use_weight_distribution=flag, want_terms=True)
        same(div, g19[f"{tag}__divergence"][pick], tag + " literal")
        assert np.array_equal(samples, g19[f"{tag}__samples"][pick]), tag
        same(S, g19[f"{tag}__bits"][pick], tag + " literal S")
        np.testing.assert_allclose(tot, g19[f"{tag}__total"][pick], rtol=1e-12, atol=0, err_msg=tag)
    tag = f"naive_h10_w20_w{w}_s{s}_l{L}"
    div, samples, S, tot = wdo.naive(mu, mv, W, H, 10, 20, w, s, L, want_terms=True)
    rows = g19[f"{tag}__rows"]
    same(div[rows], g19[f"{tag}__divergence"], tag)
    assert np.array_equal(samples[rows], g19[f"{tag}__samples"]), tag
    same(S[rows], g19[f"{tag}__bits"], tag + " S")
    np.testing.assert_allclose(tot[rows], g19[f"{tag}__total"], rtol=1e-12, atol=0, err_msg=tag)


@pytest.mark.parametrize("flag", [True, False])
def test_fast_oracle_equals_the_literal_one(flag):
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(5, 60, base_seed=43, p_absent=0.2)
    mu[20:27] = np.nan                                                              # an all-absent stretch
    mv[20:27] = np.nan
    for window, stride, L in ((1, 7, 3), (5, 11, 2), (20, 7, 5), (5, 1, 4)):
        a = wdo.literal(mu, mv, W, H, [20, 50], window, stride, L, use_weight_distribution=flag)
        b = wdo.fast(mu, mv, W, H, [20, 50], window, stride, L, use_weight_distribution=flag)
        same(b[0], a[0], f"flag {flag} w{window} s{stride} l{L}")
        assert np.array_equal(a[1], b[1])
    d, n = wdo.literal(mu, mv, W, H, [20], 5, 1, 4, rows=[17, 21, 30])
    assert n.tolist()[1] == 0 and np.isnan(d[1]).all() and np.isnan(d[0, 3]) and not np.isnan(d[0, 0]) and not np.isnan(d[2]).any()


def test_oracle_on_cases_with_a_known_answer():
    """Disjoint supports: D = H2(mass split); equal histograms: 0; a key whose value is 0.0: NaN; no partner row: NaN."""
    h = np.array([[3.0, 1.0, 0, 0], [0, 0, 2.0, 2.0], [3.0, 1.0, 0, 0], [0.0, 1.0, 0, 0]])
    keys = h > 0
    keys[3, 0] = True                                                   # a key with the value 0.0
    D = wdo.band(h, keys, 3)
    assert D.shape == (4, 3)
    assert D[0, 0] == pytest.approx(1.0, abs=1e-15) and D[0, 1] == pytest.approx(0.0, abs=1e-15)
    assert np.isnan(D[0, 2]) and np.isnan(D[1, 1]) and np.isnan(D[2, 0])              # every pair with row 3
    assert np.isnan(D[3]).all() and np.isnan(D[2, 1:]).all() and np.isnan(D[1, 2])    # no partner row
    h[1] *= 3                                                           # masses 4 and 12
    assert wdo.band(h, keys, 1)[0, 0] == pytest.approx(float(wdo.h2(0.25)), abs=1e-15)
    from tests import _divergence_oracle as dvo                         # the band of from_hists
    full = dvo.from_hists(h, keys)
    for l in (1, 2):
        np.testing.assert_allclose(wdo.band(h, keys, 2)[:4 - l, l - 1], np.diagonal(full, l), rtol=0, atol=1e-15, equal_nan=True)


# ------------------------------------------------------------------------------------------- analyzers
def _analyzers():
    from viewport_entropy_toolkit import NaiveSpatialEntropyAnalyzer, SpatialEntropyAnalyzer
    from viewport_entropy_toolkit.config import AnalyzerConfig, NaiveAnalyzerConfig
    return (SpatialEntropyAnalyzer(AnalyzerConfig(tile_counts=[20])),
            NaiveSpatialEntropyAnalyzer(NaiveAnalyzerConfig(tile_height=10, tile_width=20)))


def test_analyzer_methods_exist_and_validate_arguments():
    from viewport_entropy_toolkit import ValidationError
    mu = np.full((30, 4), 0.5)
    times = np.arange(30) * 0.1
    for an in _analyzers():
        with pytest.raises(ValidationError, match="No data available"):
            an.compute_window_divergence(5)
        an.load_arrays(times, mu, mu)
        for window, stride in ((0, 1), (-2, 1), (5, 0), (5, -1), (31, 1), (2.5, 1), (5, 1.5), (True, 1), ("5", 1), (None, 1)):
            with pytest.raises(ValueError):
                an.compute_window_divergence(window, stride)
        # window 5, stride 5: 6 rows, so max_lag in 1..5; window 30: one row, no lag at all
        for window, stride, max_lag in ((5, 5, 0), (5, 5, 6), (5, 5, -1), (5, 5, 1.0), (5, 5, True), (5, 5, None), (30, 1, 1)):
            with pytest.raises(ValueError, match="max_lag"):
                an.compute_window_divergence(window, stride, max_lag)


def test_host_entry_refuses_bad_arguments_before_it_touches_a_device():
    """window 0, stride 0, window > T, max_lag 0 and missing pointers: VET_ERR_INVALID from the library itself (no plan is needed
    to be refused: the plan is checked first)."""
    from viewport_entropy_toolkit import _native
    lib = _native.load_library()
    out = np.zeros(64)
    mu = np.full((40, 2), 0.5)
    for window, stride, max_lag in ((0, 1, 1), (4, 0, 1), (41, 1, 1), (4, 4, 0), (4, 4, 10), (40, 1, 1)):
        rc = lib.vet_window_divergence_host(None, _native._ptr(mu), _native._ptr(mu), None, 2, 40, window, stride, max_lag,
                                            _native._ptr(out), None)
        assert rc == _native.VET_ERR_INVALID and lib.vet_last_error()
    assert lib.vet_test_window_divergence_chunk_rows(None, 1) == _native.VET_ERR_INVALID


def test_no_cpu_fallback_without_a_device():
    from viewport_entropy_toolkit import _native
    if _native.load_library().vet_device_count() > 0:
        pytest.skip("a GPU is visible; the refusal path is for GPU-less hosts")
    mu = np.full((30, 4), 0.5)
    for an in _analyzers():
        an.load_arrays(np.arange(30) * 0.1, mu, mu)
        with pytest.raises(_native.NativeUnavailable):
            an.compute_window_divergence(5, 5, 2)


class _FakePlan:
    """What Plan.spatial_window_divergence returns, without a device: divergence[r][l - 1] = 100 r + l."""

    def __init__(self):
        self.calls, self.last = [], None

    def spatial_window_divergence(self, mu=None, mv=None, ids=None, window=None, stride=1, max_lag=1, check=True):
        T, U = (mu if ids is None else ids).shape
        R = (T - window) // stride + 1
        self.calls.append((window, stride, max_lag))
        div = 100.0 * np.arange(R)[:, None] + np.arange(1, max_lag + 1)[None, :]
        div[np.arange(R)[:, None] + np.arange(1, max_lag + 1)[None, :] >= R] = np.nan
        samples = np.full(R, window * U, dtype=np.int32)
        div[1, :] = np.nan
        samples[1] = 0
        self.last = dict(divergence=div, samples=samples, code=0)
        return self.last


def test_result_frame_schema_views_and_lags():
    mu = np.full((30, 3), 0.5)
    times = np.arange(30) * 0.1
    for an in _analyzers():
        an.load_arrays(times, mu, mu)
        plan = _FakePlan()
        an._get_plan = lambda *a, plan=plan, **k: plan
        an._naive_plan = lambda plan=plan: plan
        cached = an._entropy_results
        df = an.compute_window_divergence(10, 7, 2)             # R = 3 rows: frames 0-9, 7-16, 14-23
        assert an._entropy_results is cached
        assert list(df.columns) == ["time", "time_end", "samples", "shift", "divergence"] and len(df) == 3
        assert df.attrs["lags"] == [1, 2] and df.attrs["lag_frames"] == [7, 14]
        assert np.array_equal(df["time"], times[[0, 7, 14]]) and np.array_equal(df["time_end"], times[[9, 16, 23]])
        assert plan.calls == [(10, 7, 2)]
        whole = plan.last["divergence"]
        assert df["shift"].dtype == np.float64 and np.array_equal(df["shift"], whole[:, 0], equal_nan=True)
        assert df["samples"].tolist() == [30, 0, 30]
        for r in range(3):
            cell = df["divergence"][r]
            assert cell.shape == (2,) and np.shares_memory(cell, whole) and cell.base is not None      # a view, no copy
            assert np.array_equal(cell, whole[r], equal_nan=True)
        assert np.isnan(df["divergence"][1]).all() and np.isnan(df["divergence"][2]).all()            # returned, not raised
        assert df["divergence"][0].tolist() == [1.0, 2.0]
        one = an.compute_window_divergence(10)                  # the defaults: stride 1, lag 1
        assert plan.calls[-1] == (10, 1, 1) and len(one) == 21 and one.attrs["lags"] == [1] and one.attrs["lag_frames"] == [1]


def test_out_of_range_samples_raise_validation_error():
    from viewport_entropy_toolkit import _native, ValidationError

    class _RangePlan:
        def spatial_window_divergence(self, **kw):
            raise _native.NativeError(_native.VET_ERR_RANGE, "Normalized coordinates must be between 0 and 1")

    mu = np.full((30, 3), 0.5)
    for an in _analyzers():
        an.load_arrays(np.arange(30) * 0.1, mu, mu)
        an._get_plan = lambda *a, **k: _RangePlan()
        an._naive_plan = lambda: _RangePlan()
        with pytest.raises(ValidationError, match="between 0 and 1"):
            an.compute_window_divergence(5)
