"""Head-motion statistics (angular speed per window and per viewer), CPU side: the C-ABI surface, the argument handling of the
analyzers and of Plan, the row arithmetic, the DataFrame, and the claims the GPU tests rest on — the numpy oracle of
tests/_motion_oracle.py reproduces golden G25 (the REAL reference's ``vector_angle_distance`` on the reference's own Vectors,
tools/gen_golden_motion.py) wherever the two Vectors differ and is 0 where they coincide, and its angle function reproduces golden
G13's ``raw_dist``.  No GPU."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from tests import _motion_oracle as mo
from tests._tol import W_RTOL

W, H = 100, 200
T, U = 60, 8
SYMBOLS = ("vet_head_motion", "vet_head_motion_ids", "vet_head_motion_host", "vet_test_motion_lds_values")


@pytest.fixture(scope="module")
def g15(golden_dir):
    return np.load(golden_dir / "g15_windowed_transition.npz")


@pytest.fixture(scope="module")
def g25(golden_dir):
    return np.load(golden_dir / "g25_head_motion.npz")


def test_library_exports_the_head_motion_entry_points():
    from viewport_entropy_toolkit import _native
    lib = ctypes.CDLL(str(_native.LIB_PATH))
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _native.SIGNATURES
    # vet_transition_markov's leading arguments (samples, U, T, window, stride, lag), then per_user, (fractions, Q), (edges, B)
    i, p = ctypes.c_int, ctypes.c_void_p
    for tail, at in (("", 8), ("_ids", 7), ("_host", 9)):
        res, args = _native.SIGNATURES["vet_transition_markov" + tail]
        mine = _native.SIGNATURES["vet_head_motion" + tail]
        assert mine[0] == res and mine[1][:at] == args[:at], tail
        assert mine[1][at:at + 5] == [i, p, i, p, i], tail
        assert mine[1][at + 5:] == [p] * (5 if tail == "_host" else 7), tail     # five outputs (+ status, stream)
    assert _native.SIGNATURES["vet_test_motion_lds_values"] == _native.SIGNATURES["vet_test_markov_chunk_rows"]
    for name in ("head_motion", "head_motion_device"):
        assert hasattr(_native.Plan, name)
    assert hasattr(_native.Engine, "test_motion_lds_values")
    assert len(_native._ROW_CALLS) == 11 and "head_motion" not in _native._ROW_CALLS     # described in a table of its own
    for per_user, lead in ((False, ""), (True, "U")):
        stem, pairs, whole, empty_ok, outputs = _native._MOTION_CALLS[per_user]
        assert (stem, pairs, whole, empty_ok) == ("vet_head_motion", True, True, False)
        assert [(key, dims, optional) for key, dims, _, optional in outputs] == \
            [("stats", "4" + lead + "R", False), ("quantiles", lead + "RQ", True), ("hist", lead + "RH", True),
             ("still", lead + "R", False), ("samples", lead + "R", False)]
    assert _native.load_library().vet_version() == 141


def test_header_and_ctypes_table_agree():
    from viewport_entropy_toolkit import _native
    header = (Path(__file__).resolve().parent.parent / "include" / "vet.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(vet_[a-z0-9_]+)\s*\(", text))
    assert set(SYMBOLS) <= declared and declared == set(_native.SIGNATURES)
    for name in SYMBOLS:                # argument counts of the declarations
        args = re.search(rf"\b{name}\s*\(([^)]*)\)", text).group(1)
        assert len(args.split(",")) == len(_native.SIGNATURES[name][1]), name
    assert "#define VET_VERSION 141" in header
    # the definition is written out: what a reader needs to recompute a value
    for phrase in ("vet_head_motion", "+0.0 exactly", "ddof = 1", "blocks of 1024", "EXACT order statistics", "e_b <= a < e_(b+1)"):
        assert phrase in header, phrase


def test_window_rows_arithmetic_for_lagged_pairs():
    from viewport_entropy_toolkit import _native
    rows = _native.load_library().vet_window_rows
    for frames in (2, 40, 60, 130, 30000):
        for lag in (1, 3, frames - 1):
            P = frames - lag
            if P < 1:
                continue
            for w in (1, 2, 20, P):
                if w > P:
                    continue
                for s in (1, 7, w):
                    assert rows(P, w, s) == mo.n_rows(frames, w, s, lag) == len(range(0, P - w + 1, s))
    assert rows(1, 1, 1) == 1 and rows(57, 57, 7) == 1 and rows(57, 58, 1) < 0
    # the oracle's row shapes: pooled [R], per viewer [U][R]
    ang = np.zeros((57, 3))
    assert mo.rows(ang, 20, 7)["samples"].shape == (6,) and mo.rows(ang, 20, 7, per_user=True)["stats"].shape == (4, 3, 6)


@pytest.mark.parametrize("which", ["SpatialEntropyAnalyzer", "NaiveSpatialEntropyAnalyzer", "TransitionEntropyAnalyzer"])
def test_analyzers_validate_arguments_before_the_engine(which):
    """No GPU here: every refusal below comes before a plan is built.  All three analyzers have the call."""
    import viewport_entropy_toolkit as vet
    from viewport_entropy_toolkit import ValidationError
    from viewport_entropy_toolkit.config import AnalyzerConfig
    cls = getattr(vet, which, None)
    if cls is None:
        from viewport_entropy_toolkit import analyzers
        cls = getattr(analyzers, which)
    an = cls() if which.startswith("Naive") else cls(AnalyzerConfig(tile_counts=[20]))
    with pytest.raises(ValidationError, match="No data available"):
        an.compute_head_motion()
    mu = np.full((30, 4), 0.5)
    an.load_arrays(np.arange(30) * 0.1, mu, mu)

    def no_engine(*a, **k):
        raise AssertionError("the engine was touched before the arguments were checked")

    an._get_plan = no_engine
    an._grid_plan = no_engine
    big = [i / 10 for i in range(9)]
    for kw in (dict(window=0), dict(window=5, stride=0), dict(window=30), dict(window=28, lag=3), dict(window=2.5),
               dict(window=True), dict(window=5, stride=1.5), dict(lag=0), dict(lag=30), dict(lag=1.0), dict(lag="1"),
               dict(quantiles=(0.5, 0.5)), dict(quantiles=(0.9, 0.5)), dict(quantiles=(-0.1,)), dict(quantiles=(1.5,)),
               dict(quantiles=big), dict(quantiles="0.5"), dict(quantiles=(float("nan"),)), dict(bins_deg=(0.0,)),
               dict(bins_deg=(0.0, 1.0, 1.0)), dict(bins_deg=(2.0, 1.0)), dict(bins_deg=list(range(66))),
               dict(bins_deg=(0.0, float("inf")))):
        with pytest.raises(ValueError):
            an.compute_head_motion(**kw)
    doc = cls.compute_head_motion.__doc__
    assert "DEGREES" in doc and "pair_seconds" in doc and "per_user" in doc


def test_plan_wrapper_refuses_bad_arrays_before_the_library_is_called():
    from viewport_entropy_toolkit import _native
    check = _native.Plan._motion_arrays
    for q in ((0.5, 0.5), (0.9, 0.1), (-0.01,), (1.01,), [i / 10 for i in range(9)], ((0.5,),), ("a",)):
        with pytest.raises(ValueError, match="quantiles"):
            check(q, None)
    for e in ((0.0,), (0.0, 1.0, 1.0), (1.0, 0.5), np.arange(66.0), (0.0, np.nan), ((0.0, 1.0),)):
        with pytest.raises(ValueError, match="edges"):
            check((0.5,), e)
    f, e = check((0.0, 0.5, 1.0), np.linspace(0.0, np.pi, 65))
    assert f.dtype == np.float64 and f.tolist() == [0.0, 0.5, 1.0] and e.shape == (65,)
    assert check((), None) == (None, None) and check(None, None) == (None, None)
    for lag in (0, -1, 1.5, True, "1"):
        with pytest.raises(ValueError, match="lag"):
            _native.Plan._pair_lag(lag, 30)


# ------------------------------------------------------------------------------------------- golden G25, golden G13
def test_oracle_angles_reproduce_the_reference(g15, g25):
    """Where the two Vectors differ the oracle's angle is the reference's (1e-9 relative: the smallest is 0.0157 rad, where a few
    ulps of the dot are 1e-14 relative); where they coincide the oracle is +0.0 and the reference's own value is below 3e-8."""
    ids = mo.ids_of(g15["mu"], g15["mv"], W, H)
    table = mo.grid_table(W, H)
    assert sorted(g25.files) == ["angles_l1", "angles_l3", "same_l1", "same_l3"]
    for lag in (1, 3):
        want, same = g25[f"angles_l{lag}"], g25[f"same_l{lag}"]
        assert want.shape == same.shape == (T - lag, U) and same.dtype == bool
        got, got_same = mo.angles(table, ids, lag)
        assert np.array_equal(got_same, same) and np.array_equal(np.isnan(got), np.isnan(want))
        moved = ~same & ~np.isnan(want)
        assert moved.sum() > 300 and same.sum() > 10
        print("lag", lag, "max rel err", float(np.max(np.abs(got[moved] - want[moved]) / want[moved])))
        np.testing.assert_allclose(got[moved], want[moved], rtol=W_RTOL, atol=0)
        assert (got[same] == 0.0).all() and not np.signbit(got[same]).any()
        assert (want[same] < 3e-8).all() and (want[moved] > 1e-3).all()


def test_oracle_angle_function_reproduces_golden_g13(golden_dir):
    g = np.load(golden_dir / "g13_angular.npz")
    got = mo.raw_angles(g["raw_a"], g["raw_b"])
    np.testing.assert_allclose(got, g["raw_dist"], rtol=1e-14, atol=3e-8)        # the bound golden G13 is pinned with
    pair, _ = mo.vector_angles(g["raw_a"][:, None, :], g["raw_b"][None, :, :])
    differ = ~(g["raw_a"][:, None, :] == g["raw_b"][None, :, :]).all(axis=-1)
    np.testing.assert_allclose(pair[differ], g["raw_dist"][differ], rtol=1e-14, atol=3e-8)


def test_oracle_rows_on_known_values():
    ang = np.array([[0.0, 0.3], [0.1, np.nan], [0.0, 0.2], [np.nan, np.nan]])
    r = mo.rows(ang, 3, 1, fractions=(0.0, 0.5, 1.0), edges=(0.0, 0.1, 0.25))
    assert r["samples"].tolist() == [5, 3] and r["still"].tolist() == [2, 1]
    np.testing.assert_allclose(r["stats"][:, 0], [0.12, np.std([0, 0.3, 0.1, 0, 0.2], ddof=1), 0.3, 0.6])
    np.testing.assert_allclose(r["quantiles"][0], [0.0, 0.1, 0.3])
    assert r["hist"].tolist() == [[2, 2], [1, 2]]                  # half-open: 0.1 falls in the second bin, 0.3 in none
    one = mo.rows(ang, 1, 1, per_user=True, fractions=(0.5,))
    assert one["samples"].tolist() == [[1, 1, 1, 0], [1, 0, 1, 0]]
    assert np.isnan(one["stats"][1]).all()                         # N = 1: sd is NaN; N = 0: everything is
    assert np.isnan(one["stats"][0, 0, 3]) and one["stats"][0, 1, 0] == 0.3 and one["quantiles"][1, 2, 0] == 0.2


# ------------------------------------------------------------------------------------------- the DataFrame
def test_dataframe_assembles_from_a_canned_result():
    from viewport_entropy_toolkit.analyzers._base import _EntropyAnalyzerBase as Base
    times = np.arange(10) * 0.5
    rad = np.radians
    res = dict(stats=np.array([rad([1.0, np.nan]), rad([0.5, np.nan]), rad([3.0, np.nan]), rad([8.0, np.nan])]),
               quantiles=rad(np.array([[1.0, 2.5], [np.nan, np.nan]])), hist=np.array([[5, 3], [0, 0]], dtype=np.int32),
               still=np.array([2, 0], dtype=np.int32), samples=np.array([8, 0], dtype=np.int32), code=0)
    df = Base._motion_frame(times, ["a", "b"], 4, 3, 2, False, res, (0.5, 0.9), (0.0, 1.0, 5.0))
    assert list(df.columns) == ["time", "time_end", "samples", "still", "still_share", "mean", "sd", "max", "total", "quantiles",
                                "hist"]
    assert df["time"].tolist() == [1.0, 2.5] and df["time_end"].tolist() == [2.5, 4.0]      # the later frame of the pair
    np.testing.assert_allclose(df.loc[0, ["mean", "sd", "max", "total"]].astype(float), [1.0, 0.5, 3.0, 8.0])
    assert df["still_share"][0] == 0.25 and np.isnan(df["still_share"][1]) and np.isnan(df["mean"][1])
    np.testing.assert_allclose(df["quantiles"][0], [1.0, 2.5])
    assert df["hist"][0].tolist() == [5, 3] and np.shares_memory(df["hist"][0], res["hist"])
    assert df.attrs == dict(lag=2, lag_frames=2, quantiles=(0.5, 0.9), bins_deg=(0.0, 1.0, 5.0), users=["a", "b"], pair_seconds=1.0)
    # per viewer: user-major, `user` first; no histogram asked
    res_u = dict(stats=np.zeros((4, 2, 3)), quantiles=np.zeros((2, 3, 1)), hist=None, still=np.zeros((2, 3), np.int32),
                 samples=np.arange(6, dtype=np.int32).reshape(2, 3), code=0)
    du = Base._motion_frame(times, ["a", "b"], 2, 3, 1, True, res_u, (0.5,), None)
    assert list(du.columns)[0] == "user" and "hist" not in du.columns and len(du) == 6
    assert du["user"].tolist() == ["a"] * 3 + ["b"] * 3 and du["samples"].tolist() == list(range(6))
    assert du["time"].tolist() == [0.5, 2.0, 3.5] * 2 and du["time_end"].tolist() == [1.0, 2.5, 4.0] * 2
    assert du.attrs["bins_deg"] is None and du.attrs["pair_seconds"] == 0.5
