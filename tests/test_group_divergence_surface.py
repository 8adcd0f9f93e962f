"""The two-audience permutation test (include/vet.h: vet_group_divergence), CPU side: the C-ABI surface, the draw, the analyzers'
argument handling and result frame, and the claim the GPU tests rest on — the numpy oracles of tests/_group_oracle.py reproduce
golden G22, the REAL reference's compute_spatial_entropy / compute_naive_spatial_entropy on the dicts of audience A, audience B and
both (tools/gen_golden_group_divergence.py).  Tolerance against the golden: tests/test_window_divergence_surface.py's, ATOL = 1e-12
absolute on D (a difference of entropies of a few bits).  No GPU."""
import ctypes

import numpy as np
import pytest

from tests import _group_oracle as go
from tests import _user_oracle as uo

W, H = 100, 200
ATOL = 1e-12
SYMBOLS = ("vet_group_divergence", "vet_group_divergence_ids", "vet_group_divergence_host", "vet_group_labels_host",
           "vet_test_group_chunk_rows")
SHAPES = ((300, 1), (20, 20), (20, 7), (1, 1))
CASES = (("w", True, [50]), ("w", True, [50, 100, 200]), ("u", False, [50]))
GROUPS = [0, 0, 0, 1, 1, 1, 1, -1]


@pytest.fixture(scope="module")
def g16(golden_dir):
    return np.load(golden_dir / "g16_user_entropy.npz")


@pytest.fixture(scope="module")
def g22(golden_dir):
    return np.load(golden_dir / "g22_group_divergence.npz")


def same(got, want, msg, atol=ATOL):
    print(msg, "max abs err", float(np.nanmax(np.abs(got - want), initial=0.0)))
    assert got.shape == want.shape, msg
    assert np.array_equal(np.isnan(got), np.isnan(want)), msg
    np.testing.assert_allclose(got, want, rtol=0, atol=atol, equal_nan=True, err_msg=msg)


def test_library_exports_the_group_entry_points():
    from viewport_entropy_toolkit import _native
    lib = ctypes.CDLL(str(_native.LIB_PATH))
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _native.SIGNATURES
    # the row calls' arguments, then groups, permutations, seed, confidence, then five outputs
    sig = _native.SIGNATURES
    assert sig["vet_group_divergence"][1][:7] == sig["vet_user_entropy"][1][:7]
    assert sig["vet_group_divergence"][1][7:11] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_double]
    assert len(sig["vet_group_divergence"][1]) == len(sig["vet_group_divergence_ids"][1]) + 1 == 18
    assert len(sig["vet_group_divergence_host"][1]) == 17 and len(sig["vet_group_labels_host"][1]) == 6
    for name in ("spatial_group_divergence", "spatial_group_divergence_device", "group_labels"):
        assert hasattr(_native.Plan, name)
    assert hasattr(_native.Engine, "test_group_chunk_rows")
    assert "spatial_group_divergence" in _native._ROW_CALLS
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
    for words in ("key = (z >> 16 << 16) | i", "Permutation b does not depend on P", "p_adjusted", "never computed as pooled - A",
                  "N <= 16384", "HOST memory"):
        assert words in re.sub(r"\s*\n \*\s*", " ", raw), words           # the comment's line breaks taken out


# ------------------------------------------------------------------------------------------- the draw
def test_draw_properties():
    rng = np.random.default_rng(3)
    for U in (2, 3, 8, 130):
        groups = rng.integers(-1, 2, U)
        groups[0], groups[1] = 0, 1
        l40, l5 = go.draw(groups, 40, 7), go.draw(groups, 5, 7)
        assert l40.dtype == np.uint8 and l40.shape == (41, U)
        assert np.array_equal(l40[0], np.where(groups >= 0, groups, 255))
        assert np.array_equal(l40[:6], l5)                                   # permutation b does not depend on P
        assert ((l40 == 0).sum(axis=1) == (groups == 0).sum()).all()         # every permutation keeps U_A and U_B
        assert ((l40 == 1).sum(axis=1) == (groups == 1).sum()).all()
        assert ((l40 == 255) == (groups < 0)[None, :]).all()                 # excluded viewers stay excluded
    assert not np.array_equal(go.draw(np.arange(130) % 2, 5, 7), go.draw(np.arange(130) % 2, 5, 8))
    assert len({tuple(r) for r in go.draw(np.arange(130) % 2, 40, 7)}) == 41
    # one permutation written out by hand in Python integers
    M = (1 << 64) - 1
    groups, seed = [1, -1, 0, 0, 1, 1, -1, 0, 1], 12345
    inc = [u for u, g in enumerate(groups) if g >= 0]
    N, UA = len(inc), 3
    for b in (0, 1, 5):
        keys = []
        for i in range(N):
            z = (seed + (b * N + i + 1) * 0x9E3779B97F4A7C15) & M
            z ^= z >> 30
            z = (z * 0xBF58476D1CE4E5B9) & M
            z ^= z >> 27
            z = (z * 0x94D049BB133111EB) & M
            z ^= z >> 31
            keys.append((z >> 16 << 16) | i)
        want = [255] * len(groups)
        for rank, k in enumerate(sorted(keys)):
            want[inc[k & 0xFFFF]] = 0 if rank < UA else 1
        assert go.draw(groups, 6, seed)[b + 1].tolist() == want


def test_draw_equals_the_goldens(g22):
    labels = go.draw(g22["groups"], 11, int(g22["seed"]))
    assert np.array_equal(labels, g22["labels"]) and g22["labels"].dtype == np.uint8 and g22["labels"].shape == (12, 8)
    assert g22["groups"].tolist() == GROUPS
    assert len({tuple(r) for r in g22["labels"]}) > 6                        # the labellings differ


# ------------------------------------------------------------------------------------------- golden G22
def test_golden_holds_the_cases_the_feature_is_pinned_on(g16, g22, golden_dir):
    assert (golden_dir / "g22_group_divergence.npz").stat().st_size < 1 << 20
    labels = g22["labels"]
    for w, s in SHAPES:
        for tag in (f"w_tc50_w{w}_s{s}", f"w_tc50_100_200_w{w}_s{s}", f"u_tc50_w{w}_s{s}", f"naive_h10_w20_w{w}_s{s}"):
            rows = g22[f"{tag}__rows"]
            assert np.array_equal(rows, g16[f"{tag}__rows"]), tag             # G16's rows of the same case
            D, n = g22[f"{tag}__divergence"], g22[f"{tag}__samples"]
            assert D.shape == (len(rows), 12) and n.shape == (len(rows), 12, 2), tag
            # NaN: an audience without a sample, nothing else in this dataset (S is taken before the normaliser: one unweighted
            # sample is S = 0, not the reference's 0 / 0)
            assert np.array_equal(np.isnan(D), (n == 0).any(axis=-1)), tag
            per_user = g16[f"{tag}__samples"].astype(np.int64)                # [8][m]
            for g in (0, 1):
                assert np.array_equal(n[..., g], ((labels == g).astype(np.int64) @ per_user).T), tag
            ok = ~np.isnan(D)
            assert (D[ok] >= -ATOL).all() and (D[ok] <= 1 + ATOL).all(), tag  # a Jensen-Shannon divergence of two parts, in bits
        assert f"w_tc50_w{w}_s{s}__weights" in g22.files and f"u_tc50_w{w}_s{s}__weights" in g22.files
    assert np.nanstd(g22["w_tc50_w20_s20__divergence"], axis=1).min() > 0     # relabelling moves the value


@pytest.mark.parametrize("w,s", SHAPES)
def test_literal_oracle_reproduces_the_reference(g16, g22, w, s):
    """atol 1e-12 on every labelling of every stored row, NaN = NaN, samples exact."""
    mu, mv = g16["mu"], g16["mv"]
    labels = g22["labels"]
    for flag_tag, flag, tcs in CASES:
        tag = f"{flag_tag}_tc{'_'.join(map(str, tcs))}_w{w}_s{s}"
        D, n = go.literal(mu, mv, W, H, tcs, w, s, labels, rows=g22[f"{tag}__rows"], use_weight_distribution=flag)
        same(D, g22[f"{tag}__divergence"], tag)
        assert np.array_equal(n, g22[f"{tag}__samples"]), tag
    tag = f"naive_h10_w20_w{w}_s{s}"
    D, n = go.naive(mu, mv, W, H, 10, 20, w, s, labels)
    rows = g22[f"{tag}__rows"]
    same(D[rows], g22[f"{tag}__divergence"], tag)
    assert np.array_equal(n[rows], g22[f"{tag}__samples"]), tag


def test_fast_oracle_reproduces_the_goldens_histograms(g16, g22):
    mu, mv = g16["mu"], g16["mv"]
    for flag_tag, flag in (("w", True), ("u", False)):
        tag = f"{flag_tag}_tc50_w20_s7"
        D, n, wts = go.fast(mu, mv, W, H, [50], 20, 7, g22["labels"], use_weight_distribution=flag, want_weights=True)
        rows = g22[f"{tag}__rows"]
        same(D[rows], g22[f"{tag}__divergence"], tag)
        np.testing.assert_allclose(wts[rows], g22[f"{tag}__weights"], rtol=1e-9, atol=1e-15, err_msg=tag)
        assert np.array_equal(wts[rows] > 0, g22[f"{tag}__keys"]), tag        # no zero-valued key in this dataset


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
    labels = go.draw([0, 1, 1, -1, 0], 9, 11)
    for window, stride in ((1, 7), (5, 11), (20, 7), (60, 1), (2, 1)):
        a, na = go.literal(mu, mv, W, H, [20, 50], window, stride, labels, use_weight_distribution=flag)
        b, nb = go.fast(mu, mv, W, H, [20, 50], window, stride, labels, use_weight_distribution=flag)
        same(b, a, f"flag {flag} w{window} s{stride}")
        assert np.array_equal(na, nb)
        assert np.array_equal(np.isnan(b), (nb == 0).any(axis=-1))
    D, n = go.fast(mu, mv, W, H, [20], 2, 1, labels, use_weight_distribution=flag)
    assert np.isnan(D[30:32]).all() and not n[30:32].any()                    # rows 30, 31: nobody there at all


def test_fast_naive_and_vectorised_oracles_agree():
    mu, mv = _video()
    labels = go.draw([0, 1, 1, -1, 0], 9, 11)
    for window in (1, 5, 60):
        for flag in (True, False):
            a, na, wa = go.fast(mu, mv, W, H, [20, 50], window, 1, labels, use_weight_distribution=flag, want_weights=True)
            b, nb, wb = go.fast_rows(mu, mv, W, H, [20, 50], window, labels, use_weight_distribution=flag)
            same(b, a, f"rows flag {flag} w{window}")
            assert np.array_equal(na, nb)
            np.testing.assert_allclose(wb, wa, rtol=1e-12, atol=1e-15)
        a, na, wa = go.naive(mu, mv, W, H, 10, 20, window, 1, labels, want_weights=True)
        b, nb, wb = go.fast_rows(mu, mv, W, H, None, window, labels, naive=(10, 20))
        same(b, a, f"rows naive w{window}")
        assert np.array_equal(na, nb) and np.array_equal(wa, wb) and wb.shape[-1] == 19 * 19
        assert np.array_equal(wb.sum(axis=-1), nb[:, 0])


def test_summary_on_cases_with_a_known_answer():
    observed = np.array([2.0, np.nan, 0.5, 5.0])
    null = np.array([[1.0, 2.0, 3.0, 4.0, np.nan], [1.0, 1.0, 1.0, 1.0, 1.0], [np.nan] * 5, [4.0, 1.0, 3.0, 2.0, 0.0]])
    out, valid = go.summary(observed, null, 0.5)
    assert valid.tolist() == [4, 5, 0, 5]
    assert np.array_equal(out[0], observed, equal_nan=True)
    assert out[1].tolist()[0] == 4 / 5 and np.isnan(out[1, 1]) and out[1, 2] == 1.0 and out[1, 3] == 1 / 6      # ties count
    # maxnull = [4, 2, 3, 4, 1], M = 5
    assert out[2, 0] == 5 / 6 and np.isnan(out[2, 1]) and out[2, 2] == 1.0 and out[2, 3] == 1 / 6
    assert out[3].tolist()[:2] == [2.5, 1.0] and np.isnan(out[3, 2]) and out[3, 3] == 2.0
    assert out[4].tolist()[:2] == [2.5, 1.0] and np.isnan(out[4, 2]) and out[4, 3] == 2.0
    assert (out[2][[0, 3]] >= out[1][[0, 3]]).all()


# ------------------------------------------------------------------------------------------- analyzers
def _analyzers():
    from viewport_entropy_toolkit import NaiveSpatialEntropyAnalyzer, SpatialEntropyAnalyzer
    from viewport_entropy_toolkit.config import AnalyzerConfig, NaiveAnalyzerConfig
    return (SpatialEntropyAnalyzer(AnalyzerConfig(tile_counts=[20])),
            NaiveSpatialEntropyAnalyzer(NaiveAnalyzerConfig(tile_height=10, tile_width=20)))


class _NoEngine:
    def __getattr__(self, name):
        raise AssertionError("the engine was touched")


def test_analyzer_methods_exist_and_validate_arguments():
    from viewport_entropy_toolkit import ValidationError
    mu = np.full((30, 4), 0.5)
    times = np.arange(30) * 0.1
    ok = ["a", "b", "a", None]
    for an in _analyzers():
        with pytest.raises(ValidationError, match="No data available"):
            an.compute_group_divergence(ok)
        an.load_arrays(times, mu, mu, ["u0", "u1", "u2", "u3"])
        an._get_plan = lambda *a, **k: _NoEngine()
        an._naive_plan = lambda: _NoEngine()
        for groups in (None, "abab", 5, ["a", "b", "a"], ["a", "a", "a", "a"], ["a", "b", "c", "a"], ["a", None, None, "a"],
                       [None] * 4, ["a", 1, "a", 1], {"u0": "a", "nobody": "b"}, {"u0": "a"}, {"u0": "a", "u1": "b", "u2": "c"}):
            with pytest.raises(ValueError):
                an.compute_group_divergence(groups)
        for window, stride in ((0, 1), (-2, 1), (5, 0), (5, -1), (31, 1), (2.5, 1), (5, 1.5), (True, 1), ("5", 1)):
            with pytest.raises(ValueError):
                an.compute_group_divergence(ok, window, stride)
        for kw in (dict(permutations=0), dict(permutations=4097), dict(permutations=2.5), dict(permutations=True),
                   dict(confidence=0.0), dict(confidence=1.0), dict(confidence="0.9"), dict(confidence=float("nan")),
                   dict(seed=-1), dict(seed=1 << 64), dict(seed=0.5)):
            with pytest.raises(ValueError):
                an.compute_group_divergence(ok, 5, 1, **kw)
        with pytest.raises(ValueError, match="permutations"):
            an.compute_group_divergence(ok, permutations=0)


def test_plan_argument_checks_raise_before_the_engine_is_touched():
    """window 0, stride 0, window > T: VET_ERR_INVALID from the library itself (the plan is checked first); the Python checks."""
    from viewport_entropy_toolkit import _native
    lib = _native.load_library()
    out = np.zeros(64)
    mu = np.full((40, 2), 0.5)
    g = np.array([0, 1], dtype=np.int8)
    for window, stride in ((0, 1), (4, 0), (41, 1)):
        rc = lib.vet_group_divergence_host(None, _native._ptr(mu), _native._ptr(mu), None, 2, 40, window, stride, _native._ptr(g), 8,
                                           0, 0.9, _native._ptr(out), None, None, None, None)
        assert rc == _native.VET_ERR_INVALID and lib.vet_last_error()
    assert lib.vet_group_labels_host(None, 2, _native._ptr(g), 8, 0, _native._ptr(out)) == _native.VET_ERR_INVALID
    assert lib.vet_test_group_chunk_rows(None, 1) == _native.VET_ERR_INVALID
    for args in ((0, 0, 0.9), (4097, 0, 0.9), (8, -1, 0.9), (8, 1 << 64, 0.9), (8, 0, 0.0), (8, 0, 1.0)):
        with pytest.raises(ValueError):
            _native.Plan._group_scalars(*args)
    assert _native.Plan._group_scalars(np.int64(8), np.uint64(5), 0.9) == (8, 5, 0.9)
    for groups, U in (([0, 0, 1], 4), ([0, 0, 0], 3), ([1, -1], 2), ([0, 2], 2), ([0, -2, 1], 3), ([0.0, 1.0], 2), ([[0, 1]], None),
                      ([], None), (None, None)):
        with pytest.raises(ValueError):
            _native.Plan._group_array(groups, U)
    got = _native.Plan._group_array([0, -1, 1], 3)
    assert got.dtype == np.int8 and got.tolist() == [0, -1, 1]
    plan = _native.Plan.__new__(_native.Plan)                                 # no engine behind it
    plan.lib = _NoEngine()
    plan.handle = None
    for kw in (dict(groups=[0, 0]), dict(groups=[0, 1, 1]), dict(groups=[0, 1], permutations=0), dict(groups=[0, 1], confidence=1.0),
               dict(groups=None)):
        with pytest.raises(ValueError):
            plan.spatial_group_divergence(mu=mu, mv=mu, window=5, **kw)
    with pytest.raises(ValueError):
        plan.group_labels([0, 0, 0], 4)


class _FakePlan:
    """What Plan.spatial_group_divergence returns, without a device."""

    def __init__(self):
        self.calls, self.res = [], None

    def spatial_group_divergence(self, mu=None, mv=None, ids=None, groups=None, window=None, stride=1, permutations=999, seed=0,
                                 confidence=0.95, want_null=False, want_weights=False, check=True):
        T, U = (mu if ids is None else ids).shape
        R = (T - window) // stride + 1
        self.calls.append((np.asarray(groups).tolist(), window, stride, permutations, seed, confidence, want_null, check))
        null = np.arange(R * permutations, dtype=np.float64).reshape(R, permutations)
        self.res = dict(summary=np.stack([np.arange(R) + 0.1 * k for k in range(5)]), null=null if want_null else None,
                        weights=None, samples=np.stack([np.full(R, 7, np.int32), np.full(R, 9, np.int32)]),
                        valid=np.full(R, permutations, dtype=np.int32), code=0)
        return self.res


def test_result_frame_schema():
    mu = np.full((30, 4), 0.5)
    times = np.arange(30) * 0.1
    names = ["ann", "bob", "cy", "dee"]
    for an in _analyzers():
        an.load_arrays(times, mu, mu, names)
        plan = _FakePlan()
        an._get_plan = lambda *a, plan=plan, **k: plan
        an._naive_plan = lambda plan=plan: plan
        cached = an._entropy_results
        df = an.compute_group_divergence(["hmd", "desktop", None, "hmd"], 10, 7, permutations=16, confidence=0.9, seed=5)
        assert an._entropy_results is cached
        assert list(df.columns) == ["time", "time_end", "samples_a", "samples_b", "divergence", "p_value", "p_adjusted",
                                    "null_mean", "null_crit", "valid"] and len(df) == 3
        assert df.attrs == dict(groups=("desktop", "hmd"), sizes=(1, 2), users=(["bob"], ["ann", "dee"]), permutations=16, seed=5,
                                confidence=0.9)
        assert plan.calls == [([1, 0, -1, 1], 10, 7, 16, 5, 0.9, False, False)]   # sorted: "desktop" is A
        assert np.array_equal(df["time"], times[[0, 7, 14]]) and np.array_equal(df["time_end"], times[[9, 16, 23]])
        for i, name in enumerate(("divergence", "p_value", "p_adjusted", "null_mean", "null_crit")):
            assert np.array_equal(df[name], plan.res["summary"][i])
        assert df["samples_a"].tolist() == [7] * 3 and df["samples_b"].tolist() == [9] * 3 and df["valid"].tolist() == [16] * 3
        kept = an.compute_group_divergence({"ann": 2, "cy": 1, "dee": float("nan")}, 10, 7, permutations=16, keep_null=True)
        assert plan.calls[-1][0] == [1, -1, 0, -1] and kept.attrs["groups"] == (1, 2) and kept.attrs["users"] == (["cy"], ["ann"])
        assert list(kept.columns)[-1] == "null" and kept.attrs["seed"] == 0 and kept.attrs["confidence"] == 0.95
        for r in range(3):
            assert np.shares_memory(kept["null"][r], plan.res["null"]) and kept["null"][r].shape == (16,)
        whole = an.compute_group_divergence([0, 1, 1, 0], permutations=4)       # window=None: the whole video, one row
        assert plan.calls[-1][1:4] == (30, 1, 4) and len(whole) == 1


def test_out_of_range_samples_raise_validation_error():
    from viewport_entropy_toolkit import _native, ValidationError

    class _RangePlan(_FakePlan):
        def spatial_group_divergence(self, **kw):
            raise _native.NativeError(_native.VET_ERR_RANGE, "Normalized coordinates must be between 0 and 1")

    class _RangeCodePlan(_FakePlan):
        def spatial_group_divergence(self, **kw):
            return dict(super().spatial_group_divergence(**kw), code=_native.VET_ERR_RANGE)

    mu = np.full((30, 3), 0.5)
    for cls in (_RangePlan, _RangeCodePlan):
        for an in _analyzers():
            an.load_arrays(np.arange(30) * 0.1, mu, mu)
            an._get_plan = lambda *a, **k: cls()
            an._naive_plan = lambda: cls()
            with pytest.raises(ValidationError, match="between 0 and 1"):
                an.compute_group_divergence([0, 1, 0], 5)
