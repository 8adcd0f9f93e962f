"""Bootstrap confidence bands over viewers (include/vet.h: vet_bootstrap_entropy), CPU side: the C-ABI surface, the draw, the
analyzers' argument handling and result frame, and the claim the GPU tests rest on — the numpy oracles of tests/_bootstrap_oracle.py
reproduce golden G21, the REAL reference's compute_spatial_entropy / compute_naive_spatial_entropy on the dict of a resampled
audience (tools/gen_golden_bootstrap.py).  No GPU."""
import ctypes

import numpy as np
import pytest

from tests import _bootstrap_oracle as bo
from tests import _user_oracle as uo

W, H = 100, 200
SYMBOLS = ("vet_bootstrap_entropy", "vet_bootstrap_entropy_ids", "vet_bootstrap_entropy_host", "vet_bootstrap_counts_host",
           "vet_test_bootstrap_chunk_rows")
SHAPES = ((300, 1), (20, 20), (20, 7), (1, 1))
CASES = (("w", True, [50]), ("w", True, [50, 100, 200]), ("u", False, [50]))


@pytest.fixture(scope="module")
def g16(golden_dir):
    return np.load(golden_dir / "g16_user_entropy.npz")


@pytest.fixture(scope="module")
def g21(golden_dir):
    return np.load(golden_dir / "g21_bootstrap.npz")


def same(got, want, msg, rtol, atol=0.0):
    with np.errstate(all="ignore"):
        err = float(np.nanmax(np.abs(got - want) / np.maximum(np.abs(want), 1e-300), initial=0.0))
    print(msg, "max rel err", err)
    assert np.array_equal(np.isnan(got), np.isnan(want)), msg
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, equal_nan=True, err_msg=msg)


def test_library_exports_the_bootstrap_entry_points():
    from viewport_entropy_toolkit import _native
    lib = ctypes.CDLL(str(_native.LIB_PATH))
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _native.SIGNATURES
    # the row calls' arguments, then replicates, seed, confidence, then four outputs
    sig = _native.SIGNATURES
    assert sig["vet_bootstrap_entropy"][1][:7] == sig["vet_user_entropy"][1][:7]
    assert sig["vet_bootstrap_entropy"][1][7:10] == [ctypes.c_int, ctypes.c_uint64, ctypes.c_double]
    assert len(sig["vet_bootstrap_entropy"][1]) == len(sig["vet_bootstrap_entropy_ids"][1]) + 1 == 16
    assert len(sig["vet_bootstrap_entropy_host"][1]) == 15
    for name in ("spatial_bootstrap", "spatial_bootstrap_device", "bootstrap_counts"):
        assert hasattr(_native.Plan, name)
    assert hasattr(_native.Engine, "test_bootstrap_chunk_rows")
    assert "spatial_bootstrap" in _native._ROW_CALLS
    assert _native.load_library().vet_version() == 141


def test_header_declares_the_definition():
    import re
    from pathlib import Path
    from viewport_entropy_toolkit import _native
    raw = (Path(__file__).resolve().parent.parent / "include" / "vet.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in SYMBOLS:                # argument counts of the declarations
        args = re.search(rf"\b{name}\s*\(([^)]*)\)", text).group(1)
        assert len(args.split(",")) == len(_native.SIGNATURES[name][1]), name
    for words in ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "viewer = ((z >> 32) * U) >> 32",
                  "Replicate b does not depend on B", "PLAIN VALUES"):
        assert words in raw, words


# ------------------------------------------------------------------------------------------- the draw
def test_draw_properties():
    for U in (1, 3, 8, 130):
        c40, p40 = bo.draw(U, 40, 7)
        c5, p5 = bo.draw(U, 5, 7)
        assert c40.dtype == np.uint16 and c40.shape == (40, U)
        assert (c40.sum(axis=1) == U).all()                                  # every replicate draws U viewers
        assert np.array_equal(c40[:5], c5) and np.array_equal(p40[:5], p5)   # replicate b does not depend on B
        assert ((p40 >= 0) & (p40 < U)).all()
        for b in range(5):
            assert np.array_equal(np.bincount(p40[b], minlength=U), c40[b])
    assert not np.array_equal(bo.draw(130, 5, 7)[0], bo.draw(130, 5, 8)[0])
    # the first draws written out by hand in Python integers
    M = (1 << 64) - 1
    U, seed = 130, 7
    for i in (0, 1, 129, 130, 777):
        z = (seed + (i + 1) * 0x9E3779B97F4A7C15) & M
        z ^= z >> 30
        z = (z * 0xBF58476D1CE4E5B9) & M
        z ^= z >> 27
        z = (z * 0x94D049BB133111EB) & M
        z ^= z >> 31
        assert bo.draw(U, 6, seed)[1].reshape(-1)[i] == ((z >> 32) * U) >> 32


def test_draw_equals_the_goldens(g21):
    counts, picks = bo.draw(8, 12, int(g21["seed"]))
    assert np.array_equal(counts, g21["counts"]) and np.array_equal(picks, g21["picks"])
    assert g21["counts"].dtype == np.uint16 and g21["counts"].shape == (12, 8)
    assert len({tuple(c) for c in g21["counts"]}) > 6                        # the replicates differ


# ------------------------------------------------------------------------------------------- golden G21
def test_golden_holds_the_cases_the_feature_is_pinned_on(g16, g21, golden_dir):
    assert (golden_dir / "g21_bootstrap.npz").stat().st_size < 1 << 20
    for w, s in SHAPES:
        for tag in (f"w_tc50_w{w}_s{s}", f"w_tc50_100_200_w{w}_s{s}", f"u_tc50_w{w}_s{s}", f"naive_h10_w20_w{w}_s{s}"):
            rows = g21[f"{tag}__rows"]
            assert np.array_equal(rows, g16[f"{tag}__rows"]), tag             # G16's rows of the same case
            e, n = g21[f"{tag}__entropy"], g21[f"{tag}__samples"]
            assert e.shape == n.shape == (len(rows), 12), tag
            # NaN: nobody drawn has a sample — and, unweighted, the reference's 0 / 0 of a dict with ONE sample
            assert np.array_equal(np.isnan(e), n <= 1 if tag.startswith("u_") else n == 0), tag
            # the dict of replicate b is the drawn viewers' samples, a viewer drawn c times entered c times
            want = g21["counts"].astype(np.int64) @ g16[f"{tag}__samples"].astype(np.int64)          # [12][m]
            assert np.array_equal(n, want.T), tag
            ok = ~np.isnan(e)
            assert (e[ok] >= 0).all() and (e[ok] <= 1 + 1e-12).all(), tag
        assert f"w_tc50_w{w}_s{s}__weights" in g21.files and f"u_tc50_w{w}_s{s}__weights" in g21.files
    assert np.nanstd(g21["w_tc50_w20_s20__entropy"], axis=1).min() > 0        # resampling moves the value


@pytest.mark.parametrize("w,s", SHAPES)
def test_literal_oracle_reproduces_the_reference(g16, g21, w, s):
    """rtol 1e-9 on every replicate of every stored row, NaN = NaN; lattice 0's histograms likewise."""
    mu, mv = g16["mu"], g16["mv"]
    picks = g21["picks"]
    for flag_tag, flag, tcs in CASES:
        tag = f"{flag_tag}_tc{'_'.join(map(str, tcs))}_w{w}_s{s}"
        rep, weights = bo.literal(mu, mv, W, H, tcs, w, s, picks, rows=g21[f"{tag}__rows"], use_weight_distribution=flag)
        same(rep, g21[f"{tag}__entropy"], tag, rtol=1e-9)
        wtag = f"{flag_tag}_tc50_w{w}_s{s}"                                  # lattice 0 is stored once per flag
        same(weights, g21[f"{wtag}__weights"], tag + " weights", rtol=1e-9, atol=1e-15)
        assert np.array_equal(weights > 0, g21[f"{wtag}__keys"]), tag         # no zero-valued key in this dataset
    tag = f"naive_h10_w20_w{w}_s{s}"
    rep, _ = bo.literal(mu, mv, W, H, None, w, s, picks, rows=g21[f"{tag}__rows"], naive=(10, 20))
    same(rep, g21[f"{tag}__entropy"], tag, rtol=1e-9)


def _video():
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(5, 60, base_seed=43, p_absent=0.2)
    mu[20:27, 1] = np.nan
    mv[20:27, 1] = np.nan
    mu[30:33], mv[30:33] = np.nan, np.nan                                    # three frames without anybody
    return mu, mv


@pytest.mark.parametrize("flag", [True, False])
def test_fast_oracle_equals_the_literal_one(flag):
    mu, mv = _video()
    counts, picks = bo.draw(5, 9, 11)
    for window, stride in ((1, 7), (5, 11), (20, 7), (60, 1), (2, 1)):
        a, wa = bo.literal(mu, mv, W, H, [20, 50], window, stride, picks, use_weight_distribution=flag)
        b, wb, n = bo.fast(mu, mv, W, H, [20, 50], window, stride, counts, use_weight_distribution=flag)
        same(b, a, f"flag {flag} w{window} s{stride}", rtol=1e-12, atol=1e-12)
        same(wb, wa, f"flag {flag} w{window} s{stride} weights", rtol=1e-12, atol=1e-15)
        # NaN: nobody drawn has a sample — and, unweighted, the reference's 0 / 0 of a dict with ONE sample
        assert np.array_equal(np.isnan(b), n == 0 if flag else n <= 1)
    rep, _, n = bo.fast(mu, mv, W, H, [20], 2, 1, counts, use_weight_distribution=flag)
    assert np.isnan(rep[30:32]).all() and not n[30:32].any()                  # rows 30, 31: nobody there at all
    # a frame where only viewer 4 is there: the replicates that did not draw viewer 4 are NaN, the others are not
    mu[10, :4], mv[10, :4], mu[10, 4], mv[10, 4] = np.nan, np.nan, 0.5, 0.5
    rep, _, n = bo.fast(mu, mv, W, H, [20], 1, 1, counts, use_weight_distribution=True)
    assert np.array_equal(np.isnan(rep[10]), counts[:, 4] == 0) and 0 < (counts[:, 4] == 0).sum() < 9
    assert np.array_equal(n[10], counts[:, 4])


def test_fast_naive_oracle_equals_the_literal_one():
    mu, mv = _video()
    counts, picks = bo.draw(5, 9, 11)
    for window, stride in ((1, 7), (5, 11), (60, 1)):
        a, _ = bo.literal(mu, mv, W, H, None, window, stride, picks, naive=(10, 20))
        b, _, n = bo.fast(mu, mv, W, H, None, window, stride, counts, naive=(10, 20))
        same(b, a, f"naive w{window} s{stride}", rtol=1e-12, atol=1e-12)
        assert np.array_equal(np.isnan(b), n == 0)                            # weighted normaliser: log2(cells) whatever N


def test_vectorised_oracle_equals_the_fast_one():
    mu, mv = _video()
    counts, _ = bo.draw(5, 9, 11)
    for window in (1, 5, 60):
        for flag in (True, False):
            a, wa, na = bo.fast(mu, mv, W, H, [20, 50], window, 1, counts, use_weight_distribution=flag)
            b, wb, nb = bo.fast_rows(mu, mv, W, H, [20, 50], window, counts, use_weight_distribution=flag)
            same(b, a, f"rows flag {flag} w{window}", rtol=1e-12, atol=1e-12)
            same(wb, wa, f"rows flag {flag} w{window} weights", rtol=1e-12, atol=1e-15)
            assert np.array_equal(na, nb)
        a, _, na = bo.fast(mu, mv, W, H, None, window, 1, counts, naive=(10, 20))
        b, wb, nb = bo.fast_rows(mu, mv, W, H, None, window, counts, naive=(10, 20))
        same(b, a, f"rows naive w{window}", rtol=1e-12, atol=1e-12)
        assert np.array_equal(na, nb) and np.array_equal(wb.sum(axis=-1), nb) and wb.shape[-1] == 19 * 19


def test_one_viewer_is_the_per_user_row():
    """U = 1: every replicate draws the one viewer once; the value is the per-viewer entropy of the row."""
    mu, mv = _video()
    counts, picks = bo.draw(1, 4, 3)
    assert (counts == 1).all()
    rep, _, _ = bo.fast(mu[:, :1], mv[:, :1], W, H, [20, 50], 5, 3, counts)
    ent, _, _ = uo.fast(mu[:, :1], mv[:, :1], W, H, [20, 50], 5, 3)
    for b in range(4):
        same(rep[:, b], ent[0], f"replicate {b}", rtol=1e-12)


def test_summary_on_cases_with_a_known_answer():
    rep = np.array([[1.0, 2.0, 3.0, 4.0, np.nan], [np.nan] * 5, [0.5, np.nan, np.nan, np.nan, np.nan], [4.0, 1.0, 3.0, 2.0, 0.0]])
    out, valid = bo.summary(rep, 0.5)
    assert valid.tolist() == [4, 0, 1, 5]
    assert out[:, 0].tolist() == pytest.approx([2.5, np.sqrt(5.0 / 3.0), 1.75, 3.25], rel=1e-15)
    assert np.isnan(out[:, 1]).all()
    assert out[0, 2] == 0.5 and np.isnan(out[1, 2]) and out[2, 2] == out[3, 2] == 0.5      # m = 1: no sd, the value itself
    assert out[:, 3].tolist() == pytest.approx([2.0, np.sqrt(2.5), 1.0, 3.0], rel=1e-15)


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
            an.compute_entropy_bootstrap()
        an.load_arrays(times, mu, mu)
        for window, stride in ((0, 1), (-2, 1), (5, 0), (5, -1), (31, 1), (2.5, 1), (5, 1.5), (True, 1), ("5", 1), (None, 1)):
            with pytest.raises(ValueError):
                an.compute_entropy_bootstrap(window, stride)
        for kw in (dict(replicates=0), dict(replicates=4097), dict(replicates=2.5), dict(replicates=True), dict(confidence=0.0),
                   dict(confidence=1.0), dict(confidence=-0.1), dict(confidence="0.9"), dict(confidence=float("nan")),
                   dict(seed=-1), dict(seed=1 << 64), dict(seed=0.5)):
            with pytest.raises(ValueError):
                an.compute_entropy_bootstrap(5, 1, **kw)


def test_host_entries_refuse_bad_arguments_before_they_touch_a_device():
    """window 0, stride 0, window > T: VET_ERR_INVALID from the library itself (the plan is checked first)."""
    from viewport_entropy_toolkit import _native
    lib = _native.load_library()
    out = np.zeros(64)
    mu = np.full((40, 2), 0.5)
    for window, stride in ((0, 1), (4, 0), (41, 1)):
        rc = lib.vet_bootstrap_entropy_host(None, _native._ptr(mu), _native._ptr(mu), None, 2, 40, window, stride, 8, 0, 0.9,
                                            _native._ptr(out), None, None, None)
        assert rc == _native.VET_ERR_INVALID and lib.vet_last_error()
    assert lib.vet_bootstrap_counts_host(None, 2, 8, 0, _native._ptr(out)) == _native.VET_ERR_INVALID
    assert lib.vet_test_bootstrap_chunk_rows(None, 1) == _native.VET_ERR_INVALID
    for args in ((0, 0, 0.9), (4097, 0, 0.9), (8, -1, 0.9), (8, 1 << 64, 0.9), (8, 0, 0.0), (8, 0, 1.0)):
        with pytest.raises(ValueError):
            _native.Plan._bootstrap_scalars(*args)
    assert _native.Plan._bootstrap_scalars(np.int64(8), np.uint64(5), 0.9) == (8, 5, 0.9)


class _FakePlan:
    """What Plan.spatial_windowed and Plan.spatial_bootstrap return, without a device."""

    def __init__(self):
        self.calls, self.point, self.boot = [], None, None

    def spatial_windowed(self, mu=None, mv=None, ids=None, window=None, stride=1, want_weights=False, check=True):
        T, U = (mu if ids is None else ids).shape
        R = (T - window) // stride + 1
        self.calls.append(("windowed", window, stride, check))
        ent, samples = np.arange(R) / 10.0, np.full(R, window * U, dtype=np.int32)
        ent[1], samples[1] = np.nan, 0
        self.point = dict(entropy=ent, weights=None, samples=samples, code=-4)
        return self.point

    def spatial_bootstrap(self, mu=None, mv=None, ids=None, window=None, stride=1, replicates=200, seed=0, confidence=0.95,
                          want_replicates=False, want_weights=False, check=True):
        T, U = (mu if ids is None else ids).shape
        R = (T - window) // stride + 1
        self.calls.append(("bootstrap", window, stride, replicates, seed, confidence, want_replicates))
        rep = np.arange(R * replicates, dtype=np.float64).reshape(R, replicates)
        summary = np.stack([np.arange(R) + 0.1 * k for k in range(4)])
        self.boot = dict(summary=summary, replicates=rep if want_replicates else None, weights=None,
                         valid=np.full(R, replicates, dtype=np.int32), code=0)
        return self.boot


def test_result_frame_schema():
    mu = np.full((30, 3), 0.5)
    times = np.arange(30) * 0.1
    for an in _analyzers():
        an.load_arrays(times, mu, mu)
        plan = _FakePlan()
        an._get_plan = lambda *a, plan=plan, **k: plan
        an._naive_plan = lambda plan=plan: plan
        cached = an._entropy_results
        df = an.compute_entropy_bootstrap(10, 7, replicates=16, confidence=0.9, seed=5)        # R = 3 rows
        assert an._entropy_results is cached
        assert list(df.columns) == ["time", "time_end", "entropy", "samples", "mean", "sd", "lo", "hi", "valid"] and len(df) == 3
        assert df.attrs == dict(replicates=16, seed=5, confidence=0.9)
        assert plan.calls == [("windowed", 10, 7, False), ("bootstrap", 10, 7, 16, 5, 0.9, False)]
        assert np.array_equal(df["time"], times[[0, 7, 14]]) and np.array_equal(df["time_end"], times[[9, 16, 23]])
        assert np.array_equal(df["entropy"], plan.point["entropy"], equal_nan=True) and np.isnan(df["entropy"][1])
        assert np.array_equal(df["samples"], plan.point["samples"])            # the empty window is returned, not raised
        for i, name in enumerate(("mean", "sd", "lo", "hi")):
            assert np.array_equal(df[name], plan.boot["summary"][i])
        assert df["valid"].tolist() == [16, 16, 16]
        kept = an.compute_entropy_bootstrap(10, 7, replicates=16, keep_replicates=True)
        assert list(kept.columns)[-1] == "replicates" and kept.attrs["seed"] == 0 and kept.attrs["confidence"] == 0.95
        for r in range(3):
            assert np.shares_memory(kept["replicates"][r], plan.boot["replicates"]) and kept["replicates"][r].shape == (16,)
            assert np.array_equal(kept["replicates"][r], plan.boot["replicates"][r])
        one = an.compute_entropy_bootstrap(replicates=4)                      # the per-frame series
        assert plan.calls[-1][:4] == ("bootstrap", 1, 1, 4) and len(one) == 30


def test_out_of_range_samples_raise_validation_error():
    from viewport_entropy_toolkit import _native, ValidationError

    class _RangePlan(_FakePlan):
        def spatial_bootstrap(self, **kw):
            raise _native.NativeError(_native.VET_ERR_RANGE, "Normalized coordinates must be between 0 and 1")

    class _RangeCodePlan(_FakePlan):
        def spatial_windowed(self, **kw):
            return dict(super().spatial_windowed(**kw), code=_native.VET_ERR_RANGE)

    mu = np.full((30, 3), 0.5)
    for cls in (_RangePlan, _RangeCodePlan):
        for an in _analyzers():
            an.load_arrays(np.arange(30) * 0.1, mu, mu)
            an._get_plan = lambda *a, **k: cls()
            an._naive_plan = lambda: cls()
            with pytest.raises(ValidationError, match="between 0 and 1"):
                an.compute_entropy_bootstrap(5)
