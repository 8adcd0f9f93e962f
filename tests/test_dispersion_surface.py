"""Audience dispersion (pairwise viewer angles per window and per viewer), CPU side: the C-ABI surface, the argument handling of the
analyzers and of Plan, the DataFrame, and the claims the GPU tests rest on — the numpy oracle of tests/_dispersion_oracle.py
reproduces golden G26 (the REAL reference's ``vector_angle_distance`` on the reference's own Vectors,
tools/gen_golden_dispersion.py) wherever the two Vectors differ and is 0 where they coincide, and its pooled and per-viewer
integers agree.  No GPU."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from tests import _dispersion_oracle as do
from tests._tol import W_RTOL

W, H = 100, 200
T, U = 60, 8
SYMBOLS = ("vet_dispersion", "vet_dispersion_ids", "vet_dispersion_host", "vet_test_dispersion_tile")


@pytest.fixture(scope="module")
def g15(golden_dir):
    return np.load(golden_dir / "g15_windowed_transition.npz")


@pytest.fixture(scope="module")
def g26(golden_dir):
    return np.load(golden_dir / "g26_dispersion.npz")


def test_library_exports_the_dispersion_entry_points():
    from viewport_entropy_toolkit import _native
    lib = ctypes.CDLL(str(_native.LIB_PATH))
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _native.SIGNATURES
    # the leading arguments of the other row calls (samples, U, T, window, stride), then per_user, (edges, B), the four outputs
    i, p = ctypes.c_int, ctypes.c_void_p
    for tail, at in (("", 7), ("_ids", 6), ("_host", 8)):
        res, args = _native.SIGNATURES["vet_head_motion" + tail]
        mine = _native.SIGNATURES["vet_dispersion" + tail]
        assert mine[0] == res and mine[1][:at] == args[:at], tail
        assert mine[1][at:at + 3] == [i, p, i], tail
        assert mine[1][at + 3:] == [p] * (4 if tail == "_host" else 6), tail     # four outputs (+ status, stream)
    assert _native.SIGNATURES["vet_test_dispersion_tile"] == _native.SIGNATURES["vet_test_motion_lds_values"]
    for name in ("dispersion", "dispersion_device"):
        assert hasattr(_native.Plan, name)
    assert hasattr(_native.Engine, "test_dispersion_tile")
    assert len(_native._ROW_CALLS) == 11 and "dispersion" not in _native._ROW_CALLS       # described in a table of its own
    assert sorted(_native._MOTION_CALLS) == [False, True]
    for per_user, lead in ((False, ""), (True, "U")):
        stem, pairs, whole, empty_ok, outputs = _native._DISPERSION_CALLS[per_user]
        assert (stem, pairs, whole, empty_ok) == ("vet_dispersion", False, True, False)
        assert [(key, dims, np.dtype(dt).name, optional) for key, dims, dt, optional in outputs] == \
            [("stats", "3" + lead + "R", "float64", False), ("centroid", lead + "R3", "float64", False),
             ("hist", lead + "RH", "int64", True), ("counts", "4" + lead + "R", "int64", False)]
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
    for phrase in ("vet_dispersion", "PAIR SAMPLE", "+0.0 exactly", "ASCENDING v", "blocks of 1024", "e_b <= a < e_(b+1)",
                   "nearest-neighbour", "ALL ORDERED PAIRS", "No FP atomics", "Not built"):
        assert phrase in header, phrase


def frame_of(res, times, names, window, stride, per_user, bins_deg=None):
    """an oracle result (radians, shaped as Plan.dispersion returns it) through the analyzers' DataFrame glue"""
    from viewport_entropy_toolkit.analyzers._base import _EntropyAnalyzerBase as Base
    return Base._dispersion_frame(times, names, window, stride, per_user, dict(res, code=0), bins_deg)


def test_oracle_row_shapes_match_the_binding_descriptors():
    """the oracle returns what Plan.dispersion allocates: the shapes and dtypes of _DISPERSION_CALLS"""
    from viewport_entropy_toolkit import _native
    rows = _native.load_library().vet_window_rows
    for frames in (1, 40, 60):
        for w in (1, 20, frames):
            if w > frames:
                continue
            for s in (1, 7):
                assert rows(frames, w, s) == do.n_rows(frames, w, s) == len(range(0, frames - w + 1, s))
    ids = np.zeros((57, 3), dtype=np.int32)
    table = do.grid_table(W, H)
    ang, _ = do.frame_angles(table, ids)
    r = do.rows(ang, ids, table, 20, 7, edges=(0.0, 1.0))
    assert r["stats"].shape == (3, 6) and r["centroid"].shape == (6, 3) and r["hist"].shape == (6, 1) and r["counts"].shape == (4, 6)
    ru = do.rows(ang, ids, table, 20, 7, per_user=True)
    assert ru["stats"].shape == (3, 3, 6) and ru["centroid"].shape == (3, 6, 3) and ru["hist"] is None and ru["counts"].shape == (4, 3, 6)
    dims = {"U": 3, "R": 6, "H": 1, "3": 3, "4": 4}
    for per_user, got in ((False, r), (True, ru)):
        for key, shape, dtype, optional in _native._DISPERSION_CALLS[per_user][4]:
            if got[key] is not None:
                assert got[key].shape == tuple(dims[d] for d in shape) and got[key].dtype == np.dtype(dtype), (per_user, key)
    # three viewers on one pixel: every pair is `same`
    assert (r["counts"][0] == 60).all() and (r["counts"][1] == 60).all() and (r["stats"] == 0.0).all() and (r["hist"] == 60).all()
    assert (r["counts"][2] == 60).all() and (r["counts"][3] == 60).all()


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
        an.compute_dispersion()
    mu = np.full((30, 4), 0.5)
    an.load_arrays(np.arange(30) * 0.1, mu, mu)

    def no_engine(*a, **k):
        raise AssertionError("the engine was touched before the arguments were checked")

    an._get_plan = no_engine
    an._grid_plan = no_engine
    for kw in (dict(window=0), dict(window=5, stride=0), dict(window=31), dict(window=2.5), dict(window=True),
               dict(window=5, stride=1.5), dict(window="5"), dict(bins_deg=(0.0,)), dict(bins_deg=(0.0, 1.0, 1.0)),
               dict(bins_deg=(2.0, 1.0)), dict(bins_deg=list(range(66))), dict(bins_deg=(0.0, float("inf"))), dict(bins_deg="0,1"),
               dict(per_user=True, bins_deg=(0.0, 1.0, 5.0))):
        with pytest.raises(ValueError):
            an.compute_dispersion(**kw)
    doc = cls.compute_dispersion.__doc__
    assert "DEGREES" in doc and "nearest" in doc and "per_user" in doc and "resultant" in doc


def test_plan_wrapper_refuses_bad_edges_before_the_library_is_called():
    from viewport_entropy_toolkit import _native
    check = _native.Plan._dispersion_edges
    for e in ((0.0,), (0.0, 1.0, 1.0), (1.0, 0.5), np.arange(66.0), (0.0, np.nan), ((0.0, 1.0),)):
        with pytest.raises(ValueError, match="edges"):
            check(e)
    with pytest.raises(ValueError, match="edges"):
        check((0.0, 1.0), per_user=True)
    e = check(np.linspace(0.0, np.pi, 65))
    assert e.dtype == np.float64 and e.shape == (65,) and check(None) is None and check(None, per_user=True) is None


# ------------------------------------------------------------------------------------------- golden G26
def test_oracle_angles_reproduce_the_reference(g15, g26):
    """Where the two Vectors differ the oracle's angle is the reference's (W_RTOL relative + 4e-16: the smallest is 0.0157 rad, where
    a few ulps of the dot are 1e-14 relative); where they coincide the oracle is +0.0 and the reference's own value is below 3e-8."""
    ids = do.ids_of(g15["mu"], g15["mv"], W, H)
    table = do.grid_table(W, H)
    assert sorted(g26.files) == ["angles", "same"]
    want, same = g26["angles"], g26["same"]
    assert want.shape == same.shape == (T, U, U) and same.dtype == bool
    got, got_same = do.frame_angles(table, ids)
    assert np.array_equal(got_same, same) and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.isnan(want), ~((ids >= 0)[:, :, None] & (ids >= 0)[:, None, :]) | np.eye(U, dtype=bool)[None])
    moved = ~same & ~np.isnan(want)
    assert moved.sum() > 3000 and same.sum() >= 8
    print("max rel err", float(np.max(np.abs(got[moved] - want[moved]) / want[moved])))
    np.testing.assert_allclose(got[moved], want[moved], rtol=W_RTOL, atol=4e-16)
    assert (got[same] == 0.0).all() and not np.signbit(got[same]).any()
    assert (want[same] < 3e-8).all() and (want[moved] > 1e-3).all()
    assert np.array_equal(got, np.swapaxes(got, 1, 2), equal_nan=True)              # a(u, v) = a(v, u)
    # the reference's angles as the analyzers present them: per viewer at window 1, `nearest` and `max` are the smallest and the
    # largest of the viewer's golden angles in the frame, in degrees
    per = do.rows(got, ids, table, 1, 1, per_user=True)
    df = frame_of(per, np.arange(T) * 0.1, [f"u{i}" for i in range(U)], 1, 1, True)
    ref = np.where(same, 0.0, want)
    has = ~np.isnan(ref).all(axis=-1)
    lo = np.degrees(np.nanmin(np.where(has[..., None], ref, 0.0), axis=-1))
    hi = np.degrees(np.nanmax(np.where(has[..., None], ref, 0.0), axis=-1))
    np.testing.assert_allclose(df["nearest"].to_numpy()[has.T.ravel()], lo.T[has.T], rtol=W_RTOL, atol=4e-16)
    np.testing.assert_allclose(df["max"].to_numpy()[has.T.ravel()], hi.T[has.T], rtol=W_RTOL, atol=4e-16)
    assert np.isnan(df["nearest"].to_numpy()[~has.T.ravel()]).all() and (df["samples"].to_numpy() == (~np.isnan(ref)).sum(axis=-1).T.ravel()).all()


def test_oracle_pooled_and_per_viewer_integers_agree(g15):
    ids = do.ids_of(g15["mu"], g15["mv"], W, H)
    table = do.grid_table(W, H)
    ang, _ = do.frame_angles(table, ids)
    for window, stride in ((1, 1), (20, 7), (None, 1)):
        pooled = do.rows(ang, ids, table, window, stride, edges=np.radians([0.0, 1.0, 30.0, 180.0]))
        per = do.rows(ang, ids, table, window, stride, per_user=True)
        assert np.array_equal(per["counts"][:2].sum(axis=1), 2 * pooled["counts"][:2])           # samples, same
        assert np.array_equal(per["counts"][2:].sum(axis=1), pooled["counts"][2:])               # slots, present
        assert np.array_equal(do.counts(ang, ids, window, stride), pooled["counts"])
        assert np.array_equal(do.counts(ang, ids, window, stride, per_user=True), per["counts"])
        assert (pooled["hist"].sum(axis=-1) <= pooled["counts"][0]).all() and (pooled["hist"][:, 0] >= pooled["counts"][1]).all()
        with np.errstate(invalid="ignore"):
            assert np.array_equal(np.fmax.reduce(per["stats"][1], axis=0), pooled["stats"][1], equal_nan=True)
        np.testing.assert_allclose(per["centroid"].sum(axis=0), pooled["centroid"], rtol=0, atol=1e-12)
        # the same through the analyzers' DataFrame: the columns a user sums
        w = T if window is None else window
        times, names = np.arange(T) * 0.1, [f"u{i}" for i in range(U)]
        df = frame_of(pooled, times, names, w, stride, False, (0.0, 1.0, 30.0, 180.0))
        du = frame_of(per, times, names, w, stride, True)
        for col in ("samples", "same"):
            assert np.array_equal(du.groupby("time", sort=True)[col].sum().to_numpy(), 2 * df[col].to_numpy()), col
        assert np.array_equal(du.groupby("time", sort=True)["present"].sum().to_numpy(), df["present"].to_numpy())
        assert np.array_equal(du.groupby("time", sort=True)["max"].max().to_numpy(), df["max"].to_numpy(), equal_nan=True)
        assert np.array_equal(np.stack(list(df["hist"])), pooled["hist"]) and (df["resultant"].dropna() <= 1.0).all()


def test_oracle_rows_on_known_values():
    """three viewers on the equator at longitudes 0, 90 and 180 degrees, a fourth absent; then only one viewer"""
    table = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])
    ids = np.array([[0, 1, 2, -1], [0, -1, -1, -1]], dtype=np.int32)
    ang, same = do.frame_angles(table, ids)
    r = do.rows(ang, ids, table, 1, 1, edges=(0.0, 2.0, 4.0))
    assert r["counts"].T.tolist() == [[3, 0, 3, 3], [0, 0, 0, 1]] and r["hist"].tolist() == [[2, 1], [0, 0]]
    np.testing.assert_allclose(r["stats"][:, 0], [(np.pi / 2 + np.pi / 2 + np.pi) / 3, np.pi, np.pi / 2])
    assert np.isnan(r["stats"][:, 1]).all() and r["centroid"].tolist() == [[0.0, 1.0, 0.0], [1.0, 0.0, 0.0]]
    u = do.rows(ang, ids, table, 2, 1, per_user=True)
    assert u["counts"][:, :, 0].T.tolist() == [[2, 0, 1, 2], [2, 0, 1, 1], [2, 0, 1, 1], [0, 0, 0, 0]]
    np.testing.assert_allclose(u["stats"][:, 0, 0], [0.75 * np.pi, np.pi, np.pi / 2])
    assert np.isnan(u["stats"][:, 3]).all() and (u["centroid"][3] == 0.0).all() and u["centroid"][0, 0].tolist() == [2.0, 0.0, 0.0]
    # the same rows as the analyzers present them: degrees, the resultant and the mean direction
    df = frame_of(r, np.array([0.0, 0.5]), list("abcd"), 1, 1, False, (0.0, np.degrees(2.0), np.degrees(4.0)))
    np.testing.assert_allclose(df.loc[0, ["mean", "max", "nearest"]].astype(float), [120.0, 180.0, 90.0])
    assert df["resultant"].tolist() == [1.0 / 3.0, 1.0] and df["center"][0].tolist() == [0.0, 1.0, 0.0]
    assert df["samples"].tolist() == [3, 0] and np.isnan(df["mean"][1]) and df["hist"][0].tolist() == [2, 1]
    du = frame_of(u, np.array([0.0, 0.5]), list("abcd"), 2, 1, True)
    assert du["user"].tolist() == list("abcd") and du["samples"].tolist() == [2, 2, 2, 0] and du["present"].tolist() == [2, 1, 1, 0]
    np.testing.assert_allclose(du["mean"][0], 135.0)
    assert du["resultant"][0] == 1.0 and np.isnan(du["resultant"][3]) and np.isnan(du["center"][3]).all()


# ------------------------------------------------------------------------------------------- the DataFrame
def test_dataframe_assembles_from_a_canned_result():
    from viewport_entropy_toolkit.analyzers._base import _EntropyAnalyzerBase as Base
    times = np.arange(10) * 0.5
    rad = np.radians
    res = dict(stats=np.array([rad([10.0, np.nan]), rad([30.0, np.nan]), rad([2.0, np.nan])]),
               centroid=np.array([[0.0, 3.0, 4.0], [0.0, 0.0, 0.0]]), hist=np.array([[5, 3], [0, 0]], dtype=np.int64),
               counts=np.array([[8, 0], [2, 0], [6, 0], [10, 0]], dtype=np.int64), code=0)
    df = Base._dispersion_frame(times, ["a", "b"], 4, 3, False, res, (0.0, 15.0, 180.0))
    assert list(df.columns) == ["time", "time_end", "samples", "same", "same_share", "mean", "max", "nearest", "present", "resultant",
                                "center", "hist"]
    assert df["time"].tolist() == [0.0, 1.5] and df["time_end"].tolist() == [1.5, 3.0]      # the first / last frame of the row
    np.testing.assert_allclose(df.loc[0, ["mean", "max", "nearest"]].astype(float), [10.0, 30.0, 2.0])
    assert df["same_share"][0] == 0.25 and np.isnan(df["same_share"][1]) and np.isnan(df["mean"][1])
    assert df["resultant"][0] == 0.5 and np.isnan(df["resultant"][1])
    np.testing.assert_allclose(df["center"][0], [0.0, 0.6, 0.8])
    assert np.isnan(df["center"][1]).all() and df["center"][0].shape == (3,)
    assert df["hist"][0].tolist() == [5, 3] and np.shares_memory(df["hist"][0], res["hist"])
    assert df.attrs == dict(bins_deg=(0.0, 15.0, 180.0), users=["a", "b"], window=4, stride=3)
    # per viewer: user-major, `user` first; no histogram
    res_u = dict(stats=np.zeros((3, 2, 3)), centroid=np.ones((2, 3, 3)), hist=None,
                 counts=np.arange(24, dtype=np.int64).reshape(4, 2, 3), code=0)
    du = Base._dispersion_frame(times, ["a", "b"], 2, 3, True, res_u, None)
    assert list(du.columns)[0] == "user" and "hist" not in du.columns and len(du) == 6
    assert du["user"].tolist() == ["a"] * 3 + ["b"] * 3 and du["samples"].tolist() == list(range(6))
    assert du["time"].tolist() == [0.0, 1.5, 3.0] * 2 and du["time_end"].tolist() == [0.5, 2.0, 3.5] * 2
    assert du.attrs["bins_deg"] is None and du["present"].tolist() == list(range(18, 24))
