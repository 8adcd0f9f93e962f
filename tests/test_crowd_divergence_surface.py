"""Viewer-to-crowd divergence (each viewer's KL from the pooled crowd, per window), CPU side: the C-ABI surface, the analyzers'
argument handling and result frame, and the claim the GPU tests rest on — the numpy oracles of tests/_crowd_oracle.py reproduce
golden G20, the REAL reference's compute_spatial_entropy / compute_naive_spatial_entropy on the dicts of one viewer and of the
whole audience (tools/gen_golden_crowd_divergence.py).  No GPU."""
import ctypes

import numpy as np
import pytest

from tests import _crowd_oracle as co
from tests import _user_oracle as uo

W, H = 100, 200
SYMBOLS = ("vet_crowd_divergence", "vet_crowd_divergence_ids", "vet_crowd_divergence_host", "vet_test_crowd_divergence_chunk_rows")
SHAPES = ((300, 1), (20, 20), (20, 7), (1, 1))
ABSENT_USER = 3
ATOL = 1e-12


@pytest.fixture(scope="module")
def g16(golden_dir):
    return np.load(golden_dir / "g16_user_entropy.npz")


@pytest.fixture(scope="module")
def g20(golden_dir):
    return np.load(golden_dir / "g20_crowd_divergence.npz")


def same(got, want, msg):
    err = float(np.nanmax(np.abs(got - want), initial=0.0))
    print(msg, "max abs err", err)
    assert np.array_equal(np.isnan(got), np.isnan(want)), msg
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL, equal_nan=True, err_msg=msg)


def test_library_exports_the_crowd_entry_points():
    from viewport_entropy_toolkit import _native
    lib = ctypes.CDLL(str(_native.LIB_PATH))
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _native.SIGNATURES
    # vet_user_entropy's signatures: d_rows stands where d_weights does
    for tail in ("", "_ids", "_host"):
        assert _native.SIGNATURES["vet_crowd_divergence" + tail] == _native.SIGNATURES["vet_user_entropy" + tail]
    for name in ("spatial_crowd_divergence", "spatial_crowd_divergence_device"):
        assert hasattr(_native.Plan, name)
    assert hasattr(_native.Engine, "test_crowd_divergence_chunk_rows")
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


# ------------------------------------------------------------------------------------------- golden G20
def g20_tags(w, s):
    return (f"w_tc50_w{w}_s{s}", f"w_tc50_100_200_w{w}_s{s}", f"u_tc50_w{w}_s{s}", f"naive_h10_w20_w{w}_s{s}")


def test_golden_holds_the_cases_the_feature_is_pinned_on(g16, g20, golden_dir):
    assert (golden_dir / "g20_crowd_divergence.npz").stat().st_size <= (golden_dir / "g19_window_divergence.npz").stat().st_size
    for w, s in SHAPES:
        for tag in g20_tags(w, s):
            rows = g20[f"{tag}__rows"]
            m, K = len(rows), 3 if "50_100_200" in tag else 1
            assert 1 <= m <= 15 and rows[0] == 0 and rows[-1] == uo.n_rows(300, w, s) - 1, tag
            D, series, samples = g20[f"{tag}__divergence"], g20[f"{tag}__series"], g20[f"{tag}__samples"]
            assert D.shape == (8, m) and series.shape == (3, m) and samples.shape == (8, m), tag
            for name in ("own_bits", "own_total", "kl"):
                assert g20[f"{tag}__{name}"].shape == (m, K, 8), (tag, name)
            for name in ("pooled_bits", "pooled_total", "pooled_entropy"):
                assert g20[f"{tag}__{name}"].shape == (m, K), (tag, name)
            # the same samples as G16's rows of the same case; the viewers' own entropy is G16's (one lattice: G16 stores the mean)
            pick = np.searchsorted(g16[f"{tag}__rows"], rows)
            assert np.array_equal(g16[f"{tag}__rows"][pick], rows)
            assert np.array_equal(samples, g16[f"{tag}__samples"][:, pick]), tag
            # the absent viewer is NaN without a sample; everyone else has a number; the rows all have samples
            gone = (rows * s >= 100) & (rows * s + w <= 200)
            assert gone.any() == (w < 300)
            assert np.isnan(D[ABSENT_USER][gone]).all() and not samples[ABSENT_USER][gone].any()
            assert np.array_equal(np.isnan(D), samples == 0), tag
            assert not np.isnan(series).any(), tag
            # 0 <= D_k <= log2(W_r / W_u), and the identity pooled = within + between
            kl, Wu, Wr = g20[f"{tag}__kl"], g20[f"{tag}__own_total"], g20[f"{tag}__pooled_total"]
            ok = ~np.isnan(kl)
            with np.errstate(all="ignore"):
                bound = np.log2(Wr[:, :, None] / Wu)
            assert (kl[ok] >= -1e-12).all() and (kl[ok] <= bound[ok] + 1e-12).all(), tag
            np.testing.assert_allclose(np.nansum(Wu, axis=2), Wr, rtol=1e-12, err_msg=tag)
            np.testing.assert_allclose(series[0], series[1] + series[2], rtol=0, atol=1e-12, err_msg=tag)
            np.testing.assert_allclose(series[0], g20[f"{tag}__pooled_bits"].mean(axis=1), rtol=0, atol=1e-14, err_msg=tag)
            e = g20[f"{tag}__pooled_entropy"]
            assert np.isfinite(e).all() and (e >= 0).all() and (e <= 1 + 1e-12).all(), tag
            if w == 1 and tag.startswith(("u_", "naive")):             # one sample per viewer: no own entropy, all of it is between
                np.testing.assert_allclose(series[1], 0.0, rtol=0, atol=1e-12, err_msg=tag)
        if w == 20:
            assert np.nanmax(g20[f"w_tc50_w{w}_s{s}__series"][2]) > 0.1                 # the viewers do differ


@pytest.mark.parametrize("w,s", SHAPES)
def test_literal_oracle_reproduces_the_reference(g16, g20, w, s):
    """atol 1e-12 on D, the three row series and the per-lattice terms, NaN = NaN, samples exact, on every stored row."""
    mu, mv = g16["mu"], g16["mv"]
    for flag, tcs in ((True, [50]), (True, [50, 100, 200]), (False, [50])):
        tag = f"{'w' if flag else 'u'}_tc{'_'.join(map(str, tcs))}_w{w}_s{s}"
        div, series, samples, kl, own_tot, p_tot = co.literal(mu, mv, W, H, tcs, w, s, rows=g20[f"{tag}__rows"],
                                                             use_weight_distribution=flag, want_terms=True)
        same(div, g20[f"{tag}__divergence"], tag)
        same(series, g20[f"{tag}__series"], tag + " series")
        assert np.array_equal(samples, g20[f"{tag}__samples"]), tag
        same(kl, g20[f"{tag}__kl"], tag + " kl")
        np.testing.assert_allclose(own_tot, np.nan_to_num(g20[f"{tag}__own_total"]), rtol=1e-12, atol=0, err_msg=tag)
        np.testing.assert_allclose(p_tot, g20[f"{tag}__pooled_total"], rtol=1e-12, atol=0, err_msg=tag)
    tag = f"naive_h10_w20_w{w}_s{s}"
    div, series, samples = co.naive(mu, mv, W, H, 10, 20, w, s)
    rows = g20[f"{tag}__rows"]
    same(div[:, rows], g20[f"{tag}__divergence"], tag)
    same(series[:, rows], g20[f"{tag}__series"], tag + " series")
    assert np.array_equal(samples[:, rows], g20[f"{tag}__samples"]), tag


@pytest.mark.parametrize("flag", [True, False])
def test_fast_oracle_equals_the_literal_one(flag):
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(5, 60, base_seed=43, p_absent=0.2)
    mu[20:27, 1] = np.nan
    mv[20:27, 1] = np.nan
    mu[30:33], mv[30:33] = np.nan, np.nan                                # three frames without anybody
    for window, stride in ((1, 7), (5, 11), (20, 7), (60, 1), (2, 1)):
        a = co.literal(mu, mv, W, H, [20, 50], window, stride, use_weight_distribution=flag)
        b = co.fast(mu, mv, W, H, [20, 50], window, stride, use_weight_distribution=flag)
        same(b[0], a[0], f"flag {flag} w{window} s{stride}")
        same(b[1], a[1], f"flag {flag} w{window} s{stride} series")
        assert np.array_equal(a[2], b[2])
    d, sr, n = co.literal(mu, mv, W, H, [20], 5, 1, rows=[21])
    assert n[1, 0] == 0 and np.isnan(d[1, 0]) and not np.isnan(d[0, 0]) and not np.isnan(sr).any()
    d, sr, n = co.literal(mu, mv, W, H, [20], 2, 1, rows=[30, 31])
    assert n[:, 1].sum() == 0 and np.isnan(d[:, 1]).all() and np.isnan(sr[:, 1]).all()   # row 31: frames 31 and 32, nobody there


def test_oracle_on_cases_with_a_known_answer():
    """A lone viewer: D = log2(W / W_u); the crowd's own proportions: 0; a key whose value is 0.0: NaN for that viewer and for
    within / between, not for pooled or the others."""
    h = np.array([[3.0, 1.0, 0, 0], [0, 0, 2.0, 2.0], [0, 0, 4.0, 4.0]])
    keys = h > 0
    P = h.sum(axis=0)
    D, series, Wu, Wr = co.from_hists(h, keys, P, P > 0)
    assert Wr == 16.0 and Wu.tolist() == [4.0, 4.0, 8.0]
    assert D[0] == pytest.approx(2.0, abs=1e-15) and D[1] == pytest.approx(np.log2(16 / 12), abs=1e-15) and D[1] == D[2]
    assert series[0] == pytest.approx(series[1] + series[2], abs=1e-15)
    assert series[2] == pytest.approx(0.25 * 2.0 + 0.75 * np.log2(16 / 12), abs=1e-15)
    one = co.from_hists(h[:1], keys[:1], h[0], keys[0])
    assert one[0][0] == 0.0 and one[1][2] == 0.0 and one[1][0] == one[1][1]
    keys[1, 0] = True                                                   # viewer 1: a key with the value 0.0
    D, series, _, _ = co.from_hists(h, keys, P, P > 0)
    assert np.isnan(D[1]) and not np.isnan(D[[0, 2]]).any() and not np.isnan(series[0]) and np.isnan(series[1:]).all()
    D, series, _, _ = co.from_hists(np.zeros((2, 4)), np.zeros((2, 4), dtype=bool), np.zeros(4), np.zeros(4, dtype=bool))
    assert np.isnan(D).all() and np.isnan(series).all()


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
            an.compute_crowd_divergence()
        an.load_arrays(times, mu, mu)
        for window, stride in ((0, 1), (-2, 1), (5, 0), (5, -1), (31, 1), (2.5, 1), (5, 1.5), (True, 1), ("5", 1), (None, 0)):
            with pytest.raises(ValueError):
                an.compute_crowd_divergence(window, stride)


def test_host_entry_refuses_bad_arguments_before_it_touches_a_device():
    """window 0, stride 0, window > T: VET_ERR_INVALID from the library itself (no plan is needed to be refused: the plan is
    checked first)."""
    from viewport_entropy_toolkit import _native
    lib = _native.load_library()
    out = np.zeros(16)
    mu = np.full((40, 2), 0.5)
    for window, stride in ((0, 1), (4, 0), (41, 1)):
        rc = lib.vet_crowd_divergence_host(None, _native._ptr(mu), _native._ptr(mu), None, 2, 40, window, stride,
                                           _native._ptr(out), None, None)
        assert rc == _native.VET_ERR_INVALID and lib.vet_last_error()
    assert lib.vet_test_crowd_divergence_chunk_rows(None, 1) == _native.VET_ERR_INVALID


class _FakePlan:
    """What Plan.spatial_crowd_divergence returns, without a device: divergence[u][r] = 100 u + r."""

    def __init__(self):
        self.calls, self.last = [], None

    def spatial_crowd_divergence(self, mu=None, mv=None, ids=None, window=None, stride=1, check=True):
        T, U = (mu if ids is None else ids).shape
        R = (T - window) // stride + 1
        self.calls.append((window, stride))
        div = 100.0 * np.arange(U)[:, None] + np.arange(R)[None, :]
        samples = np.full((U, R), window, dtype=np.int32)
        div[1, 0] = np.nan
        samples[1, 0] = 0
        rows = np.stack([np.arange(R) + 0.5, np.arange(R) + 0.25, np.full(R, 0.25)])
        self.last = dict(divergence=div, rows=rows, samples=samples, code=0)
        return self.last


def test_result_frame_schema_and_user_order():
    mu = np.full((30, 3), 0.5)
    times = np.arange(30) * 0.1
    names = ["carol", "alice", "bob"]
    for an in _analyzers():
        an.load_arrays(times, mu, mu, user_names=names)
        plan = _FakePlan()
        an._get_plan = lambda *a, plan=plan, **k: plan
        an._naive_plan = lambda plan=plan: plan
        cached = an._entropy_results
        df = an.compute_crowd_divergence(10, 7)                 # R = 3 rows: frames 0-9, 7-16, 14-23
        assert an._entropy_results is cached
        assert list(df.columns) == ["user", "time", "time_end", "divergence", "samples"] and len(df) == 9
        assert df.attrs["users"] == names and df["user"].tolist() == [n for n in names for _ in range(3)]      # user-major
        assert np.array_equal(df["time"], np.tile(times[[0, 7, 14]], 3)) and np.array_equal(df["time_end"], np.tile(times[[9, 16, 23]], 3))
        assert plan.calls == [(10, 7)]
        assert np.array_equal(df["divergence"], plan.last["divergence"].reshape(-1), equal_nan=True)
        assert np.isnan(df["divergence"][3]) and df["samples"][3] == 0                                         # the NaN slot is returned
        rows = df.attrs["rows"]
        assert list(rows.columns) == ["time", "time_end", "samples", "pooled", "within", "between"] and len(rows) == 3
        assert np.array_equal(rows["time"], times[[0, 7, 14]]) and np.array_equal(rows["time_end"], times[[9, 16, 23]])
        assert rows["samples"].tolist() == [20, 30, 30]
        for i, name in enumerate(("pooled", "within", "between")):
            assert np.array_equal(rows[name], plan.last["rows"][i])
        one = an.compute_crowd_divergence()                     # window=None: the whole video, one row per user
        assert plan.calls[-1] == (30, 1) and len(one) == 3 and one["time"][0] == 0.0 and one["time_end"][0] == times[-1]
        assert len(one.attrs["rows"]) == 1


def test_out_of_range_samples_raise_validation_error():
    from viewport_entropy_toolkit import _native, ValidationError

    class _RangePlan:
        def spatial_crowd_divergence(self, **kw):
            raise _native.NativeError(_native.VET_ERR_RANGE, "Normalized coordinates must be between 0 and 1")

    mu = np.full((30, 3), 0.5)
    for an in _analyzers():
        an.load_arrays(np.arange(30) * 0.1, mu, mu)
        an._get_plan = lambda *a, **k: _RangePlan()
        an._naive_plan = lambda: _RangePlan()
        with pytest.raises(ValidationError, match="between 0 and 1"):
            an.compute_crowd_divergence(5)
