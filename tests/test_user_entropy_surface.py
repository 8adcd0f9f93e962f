"""Per-viewer spatial entropy (each user's own tile histogram over time), CPU side: the C-ABI surface, the analyzers' argument
handling and result frame, and the claim the GPU tests rest on — the numpy oracle of tests/_user_oracle.py reproduces golden G16,
the REAL reference's compute_spatial_entropy / compute_naive_spatial_entropy on one dict that holds one user's samples of a run
of frames (tools/gen_golden_user_entropy.py).  No GPU."""
import ctypes

import numpy as np
import pytest

from tests import _user_oracle as uo
from tests._tol import w_atol

W, H = 100, 200
SYMBOLS = ("vet_user_entropy", "vet_user_entropy_ids", "vet_user_entropy_host")
SHAPES = ((300, 1), (20, 20), (20, 7), (1, 1))
ABSENT_USER = 3


@pytest.fixture(scope="module")
def g16(golden_dir):
    return np.load(golden_dir / "g16_user_entropy.npz")


def test_library_exports_the_per_user_entry_points():
    from viewport_entropy_toolkit import _native
    lib = ctypes.CDLL(str(_native.LIB_PATH))
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _native.SIGNATURES
    assert _native.SIGNATURES["vet_user_entropy"] == _native.SIGNATURES["vet_spatial_entropy_windowed"]
    assert _native.SIGNATURES["vet_user_entropy_ids"] == _native.SIGNATURES["vet_spatial_entropy_windowed_ids"]
    assert _native.SIGNATURES["vet_user_entropy_host"] == _native.SIGNATURES["vet_spatial_entropy_windowed_host"]
    assert hasattr(_native.Plan, "spatial_per_user") and hasattr(_native.Plan, "spatial_per_user_device")


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


# ------------------------------------------------------------------------------------------- golden G16
def test_golden_holds_the_cases_the_feature_is_pinned_on(g16):
    assert g16["mu"].shape == (300, 8)
    absent = np.isnan(g16["mu"])
    assert absent[100:200, ABSENT_USER].all() and not absent[0].any() and 0.05 < absent.mean() < 0.2
    for w, s in SHAPES:
        for tag in (f"w_tc50_w{w}_s{s}", f"w_tc50_100_200_w{w}_s{s}", f"u_tc50_w{w}_s{s}", f"naive_h10_w20_w{w}_s{s}"):
            rows = g16[f"{tag}__rows"]
            assert g16[f"{tag}__entropy"].shape == g16[f"{tag}__samples"].shape == (8, len(rows)), tag
            assert rows[-1] == uo.n_rows(300, w, s) - 1
            if not tag.startswith("naive"):
                assert g16[f"{tag}__weights"].shape == g16[f"{tag}__keys"].shape == (8, len(rows), 51), tag
            if (w, s) == (1, 1):
                assert 35 <= len(rows) <= 45
            # the absent user's rows: NaN, no sample
            gone = (rows * s >= 100) & (rows * s + w <= 200)
            assert gone.any() == (w < 300)
            assert np.isnan(g16[f"{tag}__entropy"][ABSENT_USER][gone]).all() and not g16[f"{tag}__samples"][ABSENT_USER][gone].any()


@pytest.mark.parametrize("w,s", SHAPES)
def test_literal_oracle_reproduces_the_reference(g16, w, s):
    """rtol 1e-12, NaN = NaN, samples exact, lattice 0's dict (keys and values) on every stored row."""
    mu, mv = g16["mu"], g16["mv"]
    for flag, tcs in ((True, [50]), (True, [50, 100, 200]), (False, [50])):
        tag = f"{'w' if flag else 'u'}_tc{'_'.join(map(str, tcs))}_w{w}_s{s}"
        ent, samples, weights = uo.literal(mu, mv, W, H, tcs, w, s, rows=g16[f"{tag}__rows"], use_weight_distribution=flag)
        np.testing.assert_allclose(ent, g16[f"{tag}__entropy"], rtol=1e-12, atol=0, equal_nan=True, err_msg=tag)
        assert np.array_equal(samples, g16[f"{tag}__samples"]), tag
        assert np.array_equal(uo.keys_of(weights), g16[f"{tag}__keys"]), tag
        np.testing.assert_allclose(np.abs(weights), g16[f"{tag}__weights"], rtol=1e-12, atol=0, err_msg=tag)
    tag = f"naive_h10_w20_w{w}_s{s}"
    ent, samples = uo.naive(mu, mv, W, H, 10, 20, w, s, use_weight_distribution=True)
    rows = g16[f"{tag}__rows"]
    np.testing.assert_allclose(ent[:, rows], g16[f"{tag}__entropy"], rtol=1e-12, atol=0, equal_nan=True, err_msg=tag)
    assert np.array_equal(samples[:, rows], g16[f"{tag}__samples"]), tag


@pytest.mark.parametrize("flag", [True, False])
def test_fast_oracle_equals_the_literal_one(flag):
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(5, 60, base_seed=43, p_absent=0.2)
    mu[20:27, 1] = np.nan
    mv[20:27, 1] = np.nan
    for window, stride in ((1, 1), (5, 2), (20, 7), (60, 1)):
        a = uo.literal(mu, mv, W, H, [20, 50], window, stride, use_weight_distribution=flag)
        b = uo.fast(mu, mv, W, H, [20, 50], window, stride, use_weight_distribution=flag)
        np.testing.assert_allclose(b[0], a[0], rtol=1e-12, atol=0, equal_nan=True)
        assert np.array_equal(a[1], b[1]) and np.array_equal(uo.keys_of(a[2]), uo.keys_of(b[2]))
        # the two forms take the sample x tile dot products in matrices of different shapes: a distance may differ by an ulp,
        # which a tile on the cone's rim turns into tests/_tol.py's absolute term per contributing sample
        np.testing.assert_allclose(b[2], a[2], rtol=1e-12, atol=w_atol(window))
    e, n, _ = uo.literal(mu, mv, W, H, [20], 5, 1)
    assert np.isnan(e[1, 21]) and n[1, 21] == 0 and n.shape == (5, 56)


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
            an.compute_user_entropy()
        an.load_arrays(times, mu, mu)
        for window, stride in ((0, 1), (-2, 1), (5, 0), (5, -1), (31, 1), (2.5, 1), (5, 1.5), (True, 1), ("5", 1), (None, 0)):
            with pytest.raises(ValueError):
                an.compute_user_entropy(window, stride)


class _FakePlan:
    """What Plan.spatial_per_user returns, without a device: entropy[u][r] = 100 u + r."""
    n0 = 21

    def __init__(self):
        self.calls = []

    def spatial_per_user(self, mu=None, mv=None, ids=None, window=None, stride=1, want_weights=False, check=True):
        T, U = (mu if ids is None else ids).shape
        R = (T - window) // stride + 1
        self.calls.append((window, stride, want_weights))
        ent = 100.0 * np.arange(U)[:, None] + np.arange(R)[None, :]
        ent[1, 0] = np.nan
        weights = np.zeros((U, R, self.n0))
        weights[..., 2] = ent
        weights[..., 5] = -0.0
        samples = np.full((U, R), window, dtype=np.int32)
        samples[1, 0] = 0
        return dict(entropy=ent, weights=weights if want_weights else None, samples=samples, code=0)


def test_result_frame_schema_and_row_order():
    mu = np.full((30, 3), 0.5)
    times = np.arange(30) * 0.1
    names = ["carol", "alice", "bob"]
    fib, nv = _analyzers()
    for an in (fib, nv):
        an.load_arrays(times, mu, mu, user_names=names)
        plan = _FakePlan()
        an._get_plan = lambda *a, plan=plan, **k: plan
        an._naive_plan = lambda plan=plan: plan
        cached = an._entropy_results
        df = an.compute_user_entropy(10, 7)                     # R = 3 rows per user: frames 0-9, 7-16, 14-23
        assert an._entropy_results is cached
        want = ["user", "time", "time_end", "entropy", "samples"] + (["tile_weights"] if an is fib else [])
        assert list(df.columns) == want and len(df) == 9
        assert list(df["user"]) == ["carol"] * 3 + ["alice"] * 3 + ["bob"] * 3                     # user-major, ingest order
        assert np.array_equal(df["time"], np.tile(times[[0, 7, 14]], 3)) and np.array_equal(df["time_end"], np.tile(times[[9, 16, 23]], 3))
        assert np.array_equal(df["entropy"].to_numpy(), [0, 1, 2, np.nan, 101, 102, 200, 201, 202], equal_nan=True)
        assert list(df["samples"]) == [10, 10, 10, 0, 10, 10, 10, 10, 10]                          # the NaN row is returned
        assert plan.calls == [(10, 7, an is fib)]
        if an is fib:
            tiles = an._fibonacci_vectors[20]
            cell = df["tile_weights"][7]
            assert set(cell) == {tiles[2], tiles[5]} and cell[tiles[2]] == 201.0 and cell[tiles[5]] == 0.0
        whole = an.compute_user_entropy()                       # window=None: the whole video, one row per user
        assert plan.calls[-1][:2] == (30, 1) and list(whole["user"]) == names
        assert np.array_equal(whole["time"], [0.0] * 3) and np.array_equal(whole["time_end"], [times[-1]] * 3)


def test_out_of_range_samples_raise_validation_error():
    from viewport_entropy_toolkit import _native, ValidationError

    class _RangePlan:
        def spatial_per_user(self, **kw):
            raise _native.NativeError(_native.VET_ERR_RANGE, "Normalized coordinates must be between 0 and 1")

    mu = np.full((30, 3), 0.5)
    for an in _analyzers():
        an.load_arrays(np.arange(30) * 0.1, mu, mu)
        an._get_plan = lambda *a, **k: _RangePlan()
        an._naive_plan = lambda: _RangePlan()
        with pytest.raises(ValidationError, match="between 0 and 1"):
            an.compute_user_entropy(5)
