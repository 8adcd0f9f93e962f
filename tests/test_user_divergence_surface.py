"""Pairwise viewer divergence (a U x U Jensen-Shannon matrix per window), CPU side: the C-ABI surface, the analyzers' argument
handling and result frame, and the claim the GPU tests rest on — the numpy oracles of tests/_divergence_oracle.py reproduce
golden G18, the REAL reference's compute_spatial_entropy / compute_naive_spatial_entropy on the dicts of one viewer and of two
(tools/gen_golden_user_divergence.py).  No GPU."""
import ctypes

import numpy as np
import pytest

from tests import _divergence_oracle as do
from tests import _user_oracle as uo

W, H = 100, 200
SYMBOLS = ("vet_user_divergence", "vet_user_divergence_ids", "vet_user_divergence_host", "vet_test_divergence_chunk_rows")
SHAPES = ((300, 1), (20, 20), (20, 7), (1, 1))
ABSENT_USER = 3
ATOL = 1e-12


@pytest.fixture(scope="module")
def g16(golden_dir):
    return np.load(golden_dir / "g16_user_entropy.npz")


@pytest.fixture(scope="module")
def g18(golden_dir):
    return np.load(golden_dir / "g18_user_divergence.npz")


def same(got, want, msg):
    err = float(np.nanmax(np.abs(got - want), initial=0.0))
    print(msg, "max abs err", err)
    assert np.array_equal(np.isnan(got), np.isnan(want)), msg
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL, equal_nan=True, err_msg=msg)


def test_library_exports_the_divergence_entry_points():
    from viewport_entropy_toolkit import _native
    lib = ctypes.CDLL(str(_native.LIB_PATH))
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _native.SIGNATURES
    # vet_user_entropy's signatures without the d_weights / h_weights pointer
    for tail in ("", "_ids", "_host"):
        res, args = _native.SIGNATURES["vet_user_entropy" + tail]
        assert _native.SIGNATURES["vet_user_divergence" + tail] == (res, args[:-1])
    for name in ("spatial_user_divergence", "spatial_user_divergence_device"):
        assert hasattr(_native.Plan, name)
    assert hasattr(_native.Engine, "test_divergence_chunk_rows")
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


# ------------------------------------------------------------------------------------------- golden G18
def g18_tags(w, s):
    return (f"w_tc50_w{w}_s{s}", f"w_tc50_100_200_w{w}_s{s}", f"u_tc50_w{w}_s{s}", f"naive_h10_w20_w{w}_s{s}")


def test_golden_holds_the_cases_the_feature_is_pinned_on(g16, g18):
    for w, s in SHAPES:
        for tag in g18_tags(w, s):
            rows = g18[f"{tag}__rows"]
            m, K = len(rows), 3 if "50_100_200" in tag else 1
            assert 1 <= m <= 15 and rows[0] == 0 and rows[-1] == uo.n_rows(300, w, s) - 1, tag
            D = g18[f"{tag}__divergence"]
            assert D.shape == (m, 8, 8) and g18[f"{tag}__samples"].shape == (8, m), tag
            for name in ("entropy", "bits", "total"):
                assert g18[f"{tag}__{name}"].shape == (m, K, 8, 8), (tag, name)
            # the same samples as G16's rows of the same case
            pick = np.searchsorted(g16[f"{tag}__rows"], rows)
            assert np.array_equal(g16[f"{tag}__rows"][pick], rows)
            assert np.array_equal(g18[f"{tag}__samples"], g16[f"{tag}__samples"][:, pick]), tag
            # the reference's returned entropy of one viewer's dict is G16's (one lattice: G16 stores the mean)
            if K == 1:
                own = np.diagonal(g18[f"{tag}__entropy"][:, 0], axis1=1, axis2=2).T
                np.testing.assert_allclose(own, g16[f"{tag}__entropy"][:, pick], rtol=1e-12, atol=0, equal_nan=True, err_msg=tag)
            # the absent viewer: NaN rows and columns, no sample; everyone else has numbers, symmetric, +0.0 diagonal
            gone = (rows * s >= 100) & (rows * s + w <= 200)
            assert gone.any() == (w < 300)
            assert np.isnan(D[gone][:, ABSENT_USER, :]).all() and np.isnan(D[gone][:, :, ABSENT_USER]).all(), tag
            assert not g18[f"{tag}__samples"][ABSENT_USER][gone].any()
            present = g18[f"{tag}__samples"].T > 0                                     # [m][8]
            assert np.array_equal(np.isnan(D), ~(present[:, :, None] & present[:, None, :])), tag
            assert np.array_equal(D, D.transpose(0, 2, 1), equal_nan=True)
            diag = np.diagonal(D, axis1=1, axis2=2)
            assert not diag[present].any() and not np.signbit(diag[present]).any()
            total = g18[f"{tag}__total"]
            Wd = np.diagonal(total, axis1=2, axis2=3)                                  # [m][K][8]
            split = Wd[:, :, :, None] / (Wd[:, :, :, None] + Wd[:, :, None, :])
            with np.errstate(all="ignore"):
                bound = do.h2(split).mean(axis=1)
            ok = ~np.isnan(D)
            assert (D[ok] >= -1e-12).all() and (D[ok] <= bound[ok] + 1e-12).all(), tag
        if w == 20:
            assert np.nanmax(g18[f"w_tc50_w{w}_s{s}__divergence"]) > 0.1                # the viewers do differ


@pytest.mark.parametrize("w,s", SHAPES)
def test_literal_oracle_reproduces_the_reference(g16, g18, w, s):
    """atol 1e-12 on D and on the three terms, NaN = NaN, samples exact, on every stored row."""
    mu, mv = g16["mu"], g16["mv"]
    for flag, tcs in ((True, [50]), (True, [50, 100, 200]), (False, [50])):
        tag = f"{'w' if flag else 'u'}_tc{'_'.join(map(str, tcs))}_w{w}_s{s}"
        div, samples, S, tot = do.literal(mu, mv, W, H, tcs, w, s, rows=g18[f"{tag}__rows"], use_weight_distribution=flag,
                                          want_terms=True)
        same(div, g18[f"{tag}__divergence"], tag)
        assert np.array_equal(samples, g18[f"{tag}__samples"]), tag
        same(S, g18[f"{tag}__bits"], tag + " S")
        np.testing.assert_allclose(tot, np.nan_to_num(g18[f"{tag}__total"]), rtol=1e-12, atol=0, err_msg=tag)
    tag = f"naive_h10_w20_w{w}_s{s}"
    div, samples = do.naive(mu, mv, W, H, 10, 20, w, s)
    rows = g18[f"{tag}__rows"]
    same(div[rows], g18[f"{tag}__divergence"], tag)
    assert np.array_equal(samples[:, rows], g18[f"{tag}__samples"]), tag


@pytest.mark.parametrize("flag", [True, False])
def test_fast_oracle_equals_the_literal_one(flag):
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(5, 60, base_seed=43, p_absent=0.2)
    mu[20:27, 1] = np.nan
    mv[20:27, 1] = np.nan
    for window, stride in ((1, 7), (5, 11), (20, 7), (60, 1)):
        a = do.literal(mu, mv, W, H, [20, 50], window, stride, use_weight_distribution=flag)
        b = do.fast(mu, mv, W, H, [20, 50], window, stride, use_weight_distribution=flag)
        same(b[0], a[0], f"flag {flag} w{window} s{stride}")
        assert np.array_equal(a[1], b[1])
    d, n = do.literal(mu, mv, W, H, [20], 5, 1, rows=[21])
    assert n[1, 0] == 0 and np.isnan(d[0, 1]).all() and np.isnan(d[0, :, 1]).all() and not np.isnan(d[0, 0, 2])


def test_oracle_on_cases_with_a_known_answer():
    """Disjoint supports: D = H2(mass split); equal histograms: 0; a key whose value is 0.0: NaN."""
    h = np.array([[3.0, 1.0, 0, 0], [0, 0, 2.0, 2.0], [3.0, 1.0, 0, 0], [0.0, 1.0, 0, 0]])
    keys = h > 0
    keys[3, 0] = True                                                   # a key with the value 0.0
    D = do.from_hists(h, keys)
    assert D[0, 1] == pytest.approx(1.0, abs=1e-15) and D[0, 2] == pytest.approx(0.0, abs=1e-15) and D[0, 0] == 0.0
    assert np.isnan(D[3]).all() and np.isnan(D[:, 3]).all()
    h[1] *= 3                                                           # masses 4 and 12
    assert do.from_hists(h, keys)[0, 1] == pytest.approx(float(do.h2(0.25)), abs=1e-15)


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
            an.compute_user_divergence()
        an.load_arrays(times, mu, mu)
        for window, stride in ((0, 1), (-2, 1), (5, 0), (5, -1), (31, 1), (2.5, 1), (5, 1.5), (True, 1), ("5", 1), (None, 0)):
            with pytest.raises(ValueError):
                an.compute_user_divergence(window, stride)


def test_host_entry_refuses_bad_arguments_before_it_touches_a_device():
    """window 0, stride 0, window > T and missing pointers: VET_ERR_INVALID from the library itself (no plan is needed to be
    refused: the plan is checked first)."""
    from viewport_entropy_toolkit import _native
    lib = _native.load_library()
    out = np.zeros(16)
    mu = np.full((40, 2), 0.5)
    for window, stride in ((0, 1), (4, 0), (41, 1)):
        rc = lib.vet_user_divergence_host(None, _native._ptr(mu), _native._ptr(mu), None, 2, 40, window, stride,
                                          _native._ptr(out), None)
        assert rc == _native.VET_ERR_INVALID and lib.vet_last_error()
    assert lib.vet_test_divergence_chunk_rows(None, 1) == _native.VET_ERR_INVALID
    assert lib.vet_window_rows(40, 0, 1) < 0 and lib.vet_window_rows(40, 4, 0) < 0 and lib.vet_window_rows(40, 41, 1) < 0


class _FakePlan:
    """What Plan.spatial_user_divergence returns, without a device: divergence[r][u][v] = 100 r + |u - v|."""

    def __init__(self):
        self.calls, self.last = [], None

    def spatial_user_divergence(self, mu=None, mv=None, ids=None, window=None, stride=1, check=True):
        T, U = (mu if ids is None else ids).shape
        R = (T - window) // stride + 1
        self.calls.append((window, stride))
        u = np.arange(U)
        div = 100.0 * np.arange(R)[:, None, None] + np.abs(u[:, None] - u[None, :])[None]
        samples = np.full((U, R), window, dtype=np.int32)
        div[0, 1, :] = div[0, :, 1] = np.nan
        samples[1, 0] = 0
        self.last = dict(divergence=div, samples=samples, code=0)
        return self.last


def test_result_frame_schema_views_and_user_order():
    mu = np.full((30, 3), 0.5)
    times = np.arange(30) * 0.1
    names = ["carol", "alice", "bob"]
    for an in _analyzers():
        an.load_arrays(times, mu, mu, user_names=names)
        plan = _FakePlan()
        an._get_plan = lambda *a, plan=plan, **k: plan
        an._naive_plan = lambda plan=plan: plan
        cached = an._entropy_results
        df = an.compute_user_divergence(10, 7)                  # R = 3 rows: frames 0-9, 7-16, 14-23
        assert an._entropy_results is cached
        assert list(df.columns) == ["time", "time_end", "divergence", "samples"] and len(df) == 3
        assert df.attrs["users"] == names                                                       # matrix order = ingest order
        assert np.array_equal(df["time"], times[[0, 7, 14]]) and np.array_equal(df["time_end"], times[[9, 16, 23]])
        assert plan.calls == [(10, 7)]
        whole = plan.last["divergence"]
        for r in range(3):
            cell = df["divergence"][r]
            assert cell.shape == (3, 3) and np.shares_memory(cell, whole) and cell.base is not None      # a view, no copy
            assert np.array_equal(cell, whole[r], equal_nan=True)
            assert df["samples"][r].tolist() == plan.last["samples"][:, r].tolist()
        assert np.isnan(df["divergence"][0][1]).all() and df["samples"][0].tolist() == [10, 0, 10]  # the NaN viewer is returned
        one = an.compute_user_divergence()                      # window=None: the whole video, one row
        assert plan.calls[-1] == (30, 1) and len(one) == 1 and one["time"][0] == 0.0 and one["time_end"][0] == times[-1]


def test_out_of_range_samples_raise_validation_error():
    from viewport_entropy_toolkit import _native, ValidationError

    class _RangePlan:
        def spatial_user_divergence(self, **kw):
            raise _native.NativeError(_native.VET_ERR_RANGE, "Normalized coordinates must be between 0 and 1")

    mu = np.full((30, 3), 0.5)
    for an in _analyzers():
        an.load_arrays(np.arange(30) * 0.1, mu, mu)
        an._get_plan = lambda *a, **k: _RangePlan()
        an._naive_plan = lambda: _RangePlan()
        with pytest.raises(ValidationError, match="between 0 and 1"):
            an.compute_user_divergence(5)
