"""Attention coverage (top-k tile sets per window and the share of later windows they hold), CPU side: the C-ABI surface, the
analyzers' argument handling and result frame, and the claim the GPU tests rest on — the numpy oracles of
tests/_coverage_oracle.py reproduce golden G23, the definition applied in plain Python floats to the REAL reference's
compute_spatial_entropy / compute_naive_spatial_entropy histogram of every row (tools/gen_golden_coverage.py).  No GPU."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from tests import _coverage_oracle as co
from tests import _window_oracle as wo

W, H = 100, 200
SYMBOLS = ("vet_coverage", "vet_coverage_ids", "vet_coverage_host", "vet_test_coverage_chunk_rows")
SHAPES = ((20, 20, 14), (5, 1, 6), (1, 1, 3))                      # (window, stride, max_lag)
CASES = (("w_tc50", True, [50]), ("w_tc50_100_200", True, [50, 100, 200]), ("u_tc50", False, [50]))
FRACTIONS = (0.5, 0.8, 0.95, 1.0)
ATOL = 1e-12


@pytest.fixture(scope="module")
def g14(golden_dir):
    return np.load(golden_dir / "g14_windowed.npz")


@pytest.fixture(scope="module")
def g23(golden_dir):
    return np.load(golden_dir / "g23_coverage.npz")


def same(got, want, msg):
    print(msg, "max abs err", float(np.nanmax(np.abs(got - want), initial=0.0)))
    assert np.array_equal(np.isnan(got), np.isnan(want)), msg
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL, equal_nan=True, err_msg=msg)


def tags_of(w, s, L):
    return [f"{tag}_w{w}_s{s}_l{L}" for tag, _, _ in CASES] + [f"naive_h10_w20_w{w}_s{s}_l{L}"]


def test_library_exports_the_coverage_entry_points():
    from viewport_entropy_toolkit import _native
    lib = ctypes.CDLL(str(_native.LIB_PATH))
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _native.SIGNATURES
    # vet_window_divergence's signatures with (fractions, n_fractions, d_tiles) behind max_lag and d_order behind the primary output
    P, I = ctypes.c_void_p, ctypes.c_int
    for tail, at in (("", 8), ("_ids", 7), ("_host", 9)):
        res, args = _native.SIGNATURES["vet_window_divergence" + tail]
        assert _native.SIGNATURES["vet_coverage" + tail] == (res, args[:at] + [P, I, P] + args[at:at + 1] + [P] + args[at + 1:])
    for name in ("spatial_coverage", "spatial_coverage_device"):
        assert hasattr(_native.Plan, name)
    assert hasattr(_native.Engine, "test_coverage_chunk_rows")
    assert "spatial_coverage" in _native._ROW_CALLS
    assert _native.load_library().vet_version() == 141


def test_header_and_ctypes_table_agree():
    from viewport_entropy_toolkit import _native
    text = re.sub(r"/\*.*?\*/", "", (Path(__file__).resolve().parent.parent / "include" / "vet.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(vet_[a-z0-9_]+)\s*\(", text))
    assert set(SYMBOLS) <= declared and declared == set(_native.SIGNATURES)
    for name in SYMBOLS:                # argument counts of the declarations
        args = re.search(rf"\b{name}\s*\(([^)]*)\)", text).group(1)
        assert len(args.split(",")) == len(_native.SIGNATURES[name][1]), name
    assert "#define VET_VERSION 141" in (Path(__file__).resolve().parent.parent / "include" / "vet.h").read_text()


# ------------------------------------------------------------------------------------------- golden G23
def test_golden_holds_the_cases_the_feature_is_pinned_on(g14, g23):
    mu = g14["mu_absent"]
    present = (~np.isnan(mu)).sum(axis=1)
    assert np.array_equal(g23["fractions"], FRACTIONS)
    for w, s, L in SHAPES:
        R = wo.n_rows(300, w, s)
        for tag in tags_of(w, s, L):
            rows = g23[f"{tag}__rows"]
            m, n = len(rows), 361 if tag.startswith("naive") else 51
            assert rows[0] == 0 and rows[-1] == R - 1 and (np.diff(rows) > 0).all(), tag
            if (w, s) == (20, 20):
                assert np.array_equal(rows, np.arange(R)), tag
            else:
                assert set(range(0, R, 7)) <= set(rows) and set(range(R - 1 - L, R)) <= set(rows), tag
            assert g23[f"{tag}__weights"].shape == (m, n) and g23[f"{tag}__order"].shape == (m, n), tag
            assert g23[f"{tag}__tiles"].shape == (m, 4) and g23[f"{tag}__hit"].shape == (m, L + 1, 4), tag
            assert np.array_equal(g23[f"{tag}__samples"], [present[r * s:r * s + w].sum() for r in rows]), tag
            assert (g23[f"{tag}__weights"] >= 0).all() and (g23[f"{tag}__samples"] > 0).all(), tag      # no empty window here
        # only lattice 0 takes part
        a, b = tags_of(w, s, L)[:2]
        for name in ("weights", "tiles", "order", "hit"):
            assert g23[f"{a}__{name}"].tobytes() == g23[f"{b}__{name}"].tobytes(), name


def check_properties(tiles, order, hit, weights, fractions, rows, R, tag):
    """What holds for every coverage result: ``rows`` are the row numbers of the entries, R the rows of the call."""
    q = np.asarray(fractions)
    n = order.shape[1]
    L = hit.shape[1] - 1
    assert (np.diff(tiles, axis=1) >= 0).all(), tag                                     # non-decreasing in q
    assert (np.sort(order, axis=1) == np.arange(n)[None, :]).all(), tag                 # a permutation
    mass = weights.sum(axis=1) > 0
    assert ((tiles > 0) == mass[:, None]).all() and (tiles <= n).all(), tag
    gone = (np.asarray(rows)[:, None] + np.arange(L + 1)[None, :] >= R) | ~mass[:, None]
    nan = np.isnan(hit[..., 0])
    assert nan[gone].all() and np.array_equal(np.isnan(hit), np.repeat(nan[..., None], len(q), axis=2)), tag
    if len(rows) == R:                                                                  # every row is here: a lag may reach a massless row
        for l in range(L + 1):
            gone[:R - l, l] |= ~mass[l:]
        assert np.array_equal(nan, gone), tag
    assert (np.isnan(hit) | ((hit >= 0) & (hit <= 1 + 1e-12))).all(), tag
    assert (hit[mass, 0, :] >= q[None, :] - 1e-12).all(), tag                           # lag 0: the share asked for is reached
    if q[-1] == 1.0:
        assert np.array_equal(tiles[:, -1], (weights > 0).sum(axis=1)), tag             # every positive tile, no other
    for r in range(len(tiles)):                                                         # rank order: weight descending, index ascending
        w = weights[r][order[r]]
        assert (np.diff(w) <= 0).all() and (np.diff(order[r])[np.diff(w) == 0] > 0).all(), (tag, r)


def test_golden_properties(g23):
    for w, s, L in SHAPES:
        for tag in tags_of(w, s, L):
            rows = g23[f"{tag}__rows"]
            hit = g23[f"{tag}__hit"]
            check_properties(g23[f"{tag}__tiles"].astype(np.int64), g23[f"{tag}__order"].astype(np.int64), hit,
                             g23[f"{tag}__weights"], FRACTIONS, rows, wo.n_rows(300, w, s), tag)
            assert np.array_equal(np.isnan(hit[..., 0]), rows[:, None] + np.arange(L + 1)[None, :] >= wo.n_rows(300, w, s)), tag
    assert g23["w_tc50_w20_s20_l14__tiles"].max() > 10 and np.nanmin(g23["w_tc50_w20_s20_l14__hit"][:, 1:]) < 0.9   # attention moves


@pytest.mark.parametrize("w,s,L", SHAPES)
def test_literal_and_fast_oracles_reproduce_the_reference(g14, g23, w, s, L):
    """tiles and order exact, hit to atol 1e-12 with NaN in the same places, samples exact, on every stored row."""
    mu, mv = g14["mu_absent"], g14["mv_absent"]
    worst_gap, worst_margin = np.inf, np.inf
    for (tag, flag, tcs), full in zip(CASES, tags_of(w, s, L)):
        rows = g23[f"{full}__rows"]
        for name, fn in (("fast", co.fast), ("literal", co.literal)):
            got = fn(mu, mv, W, H, tcs, w, s, L, FRACTIONS, use_weight_distribution=flag)
            assert np.array_equal(got["tiles"][rows], g23[f"{full}__tiles"]), (full, name)
            assert np.array_equal(got["order"][rows], g23[f"{full}__order"]), (full, name)
            assert np.array_equal(got["samples"][rows], g23[f"{full}__samples"]), (full, name)
            same(got["hit"][rows], g23[f"{full}__hit"], f"{full} {name}")
            np.testing.assert_allclose(np.abs(got["weights"][rows]), g23[f"{full}__weights"], rtol=1e-12, atol=1e-300, err_msg=full)
        if flag:                                                    # the pinning condition: how far the entries are from moving
            pos = got["gap"][got["gap"] > 0]
            worst_gap = min(worst_gap, float(pos.min()))
            worst_margin = min(worst_margin, float(np.nanmin(got["margin"][:, :3])))
            assert (got["gap"][~np.isnan(got["gap"])] > 0).all(), full                  # no exact-zero gap in the weighted cases
    print(f"w{w} s{s}: smallest boundary gap {worst_gap:.3g} W, smallest threshold margin (q < 1) {worst_margin:.3g} W")
    assert worst_gap > 1e-13 and worst_margin > 1e-13
    full = tags_of(w, s, L)[-1]
    rows = g23[f"{full}__rows"]
    got = co.naive(mu, mv, W, H, 10, 20, w, s, L, FRACTIONS)
    assert np.array_equal(got["tiles"][rows], g23[f"{full}__tiles"]) and np.array_equal(got["order"][rows], g23[f"{full}__order"])
    assert np.array_equal(got["samples"][rows], g23[f"{full}__samples"]) and np.array_equal(got["weights"][rows], g23[f"{full}__weights"])
    same(got["hit"][rows], g23[f"{full}__hit"], full)


def test_oracle_properties_and_empty_rows():
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(5, 60, base_seed=43, p_absent=0.2)
    mu[20:27], mv[20:27] = np.nan, np.nan                            # an all-absent stretch
    for flag in (True, False):
        for window, stride, L in ((1, 7, 3), (5, 11, 2), (5, 1, 4)):
            a = co.literal(mu, mv, W, H, [20, 50], window, stride, L, FRACTIONS, use_weight_distribution=flag)
            b = co.fast(mu, mv, W, H, [20], window, stride, L, FRACTIONS, use_weight_distribution=flag)
            assert np.array_equal(a["samples"], b["samples"])
            R = len(a["samples"])
            for got in (a, b):
                check_properties(got["tiles"], got["order"], got["hit"], np.abs(got["weights"]), FRACTIONS, np.arange(R), R,
                                 f"flag {flag} w{window} s{stride}")
            if not flag:                                             # counts: exact in any order
                assert np.array_equal(a["tiles"], b["tiles"]) and np.array_equal(a["order"], b["order"])
                same(a["hit"], b["hit"], "literal against fast")
    got = co.fast(mu, mv, W, H, [20], 5, 1, 4, FRACTIONS)
    empty = got["samples"] == 0
    assert empty[20:23].all() and empty.sum() == 3
    assert (got["tiles"][empty] == 0).all() and np.isnan(got["hit"][empty]).all()
    assert np.isnan(got["hit"][19, 1:4]).all() and not np.isnan(got["hit"][19, 0]).any()     # lags that reach an empty row


def test_oracle_on_cases_with_a_known_answer():
    """Masses of 8 and binary fractions: every threshold is met exactly."""
    h = np.array([[4.0, 1.0, 2.0, 1.0, 0.0], [0.0, 0.0, 4.0, 4.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0], [2.0, 2.0, 2.0, 2.0, 0.0]])
    got = co.from_hists(h, (0.5, 0.75, 1.0), 2)
    assert got["order"].tolist() == [[0, 2, 1, 3, 4], [2, 3, 0, 1, 4], [0, 1, 2, 3, 4], [0, 1, 2, 3, 4]]   # ties by index
    assert got["tiles"].tolist() == [[1, 2, 4], [1, 2, 2], [0, 0, 0], [2, 3, 4]]
    assert got["hit"][0, 0].tolist() == [0.5, 0.75, 1.0]
    assert got["hit"][0, 1].tolist() == [0.0, 0.5, 1.0]            # tiles {0}, {0, 2}, {0, 2, 1, 3} on row 1
    assert np.isnan(got["hit"][0, 2]).all() and np.isnan(got["hit"][2]).all() and np.isnan(got["hit"][1, 1]).all()
    assert got["hit"][1, 2].tolist() == [0.25, 0.5, 0.5] and np.isnan(got["hit"][3, 1:]).all()
    assert got["gap"][0].tolist() == [0.25, 0.125, 0.125] and got["margin"][0].tolist() == [0.0, 0.0, 0.0]
    assert np.isnan(got["gap"][2]).all() and got["mass"].tolist() == [8.0, 8.0, 0.0, 8.0]


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
            an.compute_coverage(5)
        an.load_arrays(times, mu, mu)
        for window, stride in ((0, 1), (-2, 1), (5, 0), (5, -1), (31, 1), (2.5, 1), (5, 1.5), (True, 1), ("5", 1), (None, 1)):
            with pytest.raises(ValueError):
                an.compute_coverage(window, stride)
        for fractions in ((), (0.0, 0.5), (0.5, 1.5), (0.5, 0.5), (0.8, 0.5), (-0.1,), (float("nan"),), 0.5, "0.5", (True,),
                          ("0.5",), tuple(np.linspace(0.1, 0.9, 9)), None):
            with pytest.raises(ValueError, match="fraction"):
                an.compute_coverage(5, 5, fractions)
        # window 5, stride 5: 6 rows, so max_lag in 0..5; window 30: one row, lag 0 only
        for window, stride, max_lag in ((5, 5, 6), (5, 5, -1), (5, 5, 1.0), (5, 5, True), (5, 5, None), (30, 1, 1)):
            with pytest.raises(ValueError, match="max_lag"):
                an.compute_coverage(window, stride, (0.5,), max_lag)


def test_host_entry_refuses_bad_arguments_before_it_touches_a_device():
    """VET_ERR_INVALID from the library itself (no plan is needed to be refused: the plan is checked first)."""
    from viewport_entropy_toolkit import _native
    lib = _native.load_library()
    tiles, hit = np.zeros(64, np.int32), np.zeros(512)
    mu = np.full((40, 2), 0.5)
    f = np.array([0.5, 0.8])
    for window, stride, max_lag in ((0, 1, 0), (4, 0, 0), (41, 1, 0), (4, 4, -1), (4, 4, 10), (40, 1, 1)):
        rc = lib.vet_coverage_host(None, _native._ptr(mu), _native._ptr(mu), None, 2, 40, window, stride, max_lag, _native._ptr(f), 2,
                                   _native._ptr(tiles), _native._ptr(hit), None, None)
        assert rc == _native.VET_ERR_INVALID and lib.vet_last_error()
    assert lib.vet_test_coverage_chunk_rows(None, 1) == _native.VET_ERR_INVALID


def test_plan_wrapper_refuses_bad_fractions_without_a_device():
    from viewport_entropy_toolkit import _native
    for fractions in ((), (0.0,), (1.5,), (0.5, 0.5), (0.9, 0.8), tuple(np.linspace(0.1, 0.9, 9)), ((0.5,),), "ab"):
        with pytest.raises(ValueError, match="fraction"):
            _native.Plan._fraction_array(fractions)
    assert _native.Plan._fraction_array((0.5, 1.0)).tolist() == [0.5, 1.0]


def test_no_cpu_fallback_without_a_device():
    from viewport_entropy_toolkit import _native
    if _native.load_library().vet_device_count() > 0:
        pytest.skip("a GPU is visible; the refusal path is for GPU-less hosts")
    mu = np.full((30, 4), 0.5)
    for an in _analyzers():
        an.load_arrays(np.arange(30) * 0.1, mu, mu)
        with pytest.raises(_native.NativeUnavailable):
            an.compute_coverage(5, 5)


class _FakePlan:
    """What Plan.spatial_coverage returns, without a device: tiles[r][i] = r + i + 1, hit[r][l][i] = (100 r + 10 l + i) / 1000."""

    n_tiles = [40]

    def __init__(self):
        self.calls, self.last = [], None

    def spatial_coverage(self, mu=None, mv=None, ids=None, window=None, stride=1, max_lag=0, fractions=(0.5, 0.8, 0.95),
                         want_order=False, check=True):
        T, U = (mu if ids is None else ids).shape
        R, Q = (T - window) // stride + 1, len(fractions)
        self.calls.append((window, stride, max_lag, tuple(fractions), want_order))
        tiles = (np.arange(R)[:, None] + np.arange(Q)[None, :] + 1).astype(np.int32)
        hit = (100.0 * np.arange(R)[:, None, None] + 10.0 * np.arange(max_lag + 1)[None, :, None] + np.arange(Q)[None, None, :]) / 1000.0
        hit[np.arange(R)[:, None] + np.arange(max_lag + 1)[None, :] >= R] = np.nan
        samples = np.full(R, window * U, dtype=np.int32)
        tiles[1], hit[1], samples[1] = 0, np.nan, 0
        order = np.tile(np.arange(40, dtype=np.int32), (R, 1)) if want_order else None
        self.last = dict(tiles=tiles, hit=hit, order=order, samples=samples, code=0)
        return self.last


def test_result_frame_schema_views_and_attrs():
    mu = np.full((30, 3), 0.5)
    times = np.arange(30) * 0.1
    for an in _analyzers():
        an.load_arrays(times, mu, mu)
        plan = _FakePlan()
        an._get_plan = lambda *a, plan=plan, **k: plan
        an._naive_plan = lambda plan=plan: plan
        n = 40 if hasattr(an.config, "tile_height") else 21
        cached = an._entropy_results
        df = an.compute_coverage(10, 7, (0.5, 0.9), 2)              # R = 3 rows: frames 0-9, 7-16, 14-23
        assert an._entropy_results is cached
        assert list(df.columns) == ["time", "time_end", "samples", "tiles", "share", "covered", "forecast"] and len(df) == 3
        assert df.attrs == {"fractions": (0.5, 0.9), "lags": [1, 2], "lag_frames": [7, 14], "n_tiles": n}
        assert np.array_equal(df["time"], times[[0, 7, 14]]) and np.array_equal(df["time_end"], times[[9, 16, 23]])
        assert plan.calls == [(10, 7, 2, (0.5, 0.9), False)]
        tiles, hit = plan.last["tiles"], plan.last["hit"]
        assert df["samples"].tolist() == [30, 0, 30]
        for r in range(3):
            assert df["tiles"][r].shape == (2,) and np.shares_memory(df["tiles"][r], tiles) and np.array_equal(df["tiles"][r], tiles[r])
            assert np.array_equal(df["share"][r], tiles[r] / n)
            assert df["covered"][r].shape == (2,) and np.shares_memory(df["covered"][r], hit)       # views, no copies
            assert df["forecast"][r].shape == (2, 2) and np.shares_memory(df["forecast"][r], hit)
            assert np.array_equal(df["covered"][r], hit[r, 0], equal_nan=True)
            assert np.array_equal(df["forecast"][r], hit[r, 1:], equal_nan=True)
        assert df["tiles"][1].tolist() == [0, 0] and np.isnan(df["covered"][1]).all()              # returned, not raised
        assert np.isnan(df["forecast"][2]).all() and df["forecast"][0].tolist() == [[0.01, 0.011], [0.02, 0.021]]
        one = an.compute_coverage()                                 # the defaults: window 1, stride 1, lag 0, three fractions
        assert plan.calls[-1] == (1, 1, 0, (0.5, 0.8, 0.95), False) and len(one) == 30
        assert one.attrs["lags"] == [] and one.attrs["lag_frames"] == [] and one["forecast"][0].shape == (0, 3)
        kept = an.compute_coverage(10, 7, (1.0,), 0, keep_order=True)
        assert list(kept.columns)[-1] == "order" and plan.calls[-1][-1] is True
        assert kept["order"][2].shape == (40,) and np.shares_memory(kept["order"][2], plan.last["order"])


def test_out_of_range_samples_raise_validation_error():
    from viewport_entropy_toolkit import _native, ValidationError

    class _RangePlan:
        def spatial_coverage(self, **kw):
            raise _native.NativeError(_native.VET_ERR_RANGE, "Normalized coordinates must be between 0 and 1")

    mu = np.full((30, 3), 0.5)
    for an in _analyzers():
        an.load_arrays(np.arange(30) * 0.1, mu, mu)
        an._get_plan = lambda *a, **k: _RangePlan()
        an._naive_plan = lambda: _RangePlan()
        with pytest.raises(ValidationError, match="between 0 and 1"):
            an.compute_coverage(5)
