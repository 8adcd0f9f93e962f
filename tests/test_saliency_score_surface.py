"""Saliency scoring (AUC, NSS, information gain, CC, SIM, JSD, KL of a predicted map against where the audience looked), CPU side:
the C-ABI surface, the argument handling of the analyzers and of Plan, the DataFrame, and the numpy oracle of
tests/_saliency_score_oracle.py checked against closed forms — a constant map, a half-sphere map, the two forms of the AUC against
each other, and the exact scaling of a map by a power of two.  No GPU."""
import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest

from tests import _saliency_oracle as so
from tests import _saliency_score_oracle as sco

W, H = 100, 200
SYMBOLS = ("vet_saliency_score", "vet_saliency_score_ids", "vet_saliency_score_host")
COLUMNS = ["time", "time_end", "samples", "distinct", "auc", "nss", "info_gain", "cc", "sim", "jsd", "kl", "mass", "mass_pred"]


@pytest.fixture(scope="module")
def table():
    return so.grid_table(W, H)


@pytest.fixture(scope="module")
def g15_ids(golden_dir):
    g = np.load(golden_dir / "g15_windowed_transition.npz")
    return so.ids_of(*so.off_centre(g["mu"], g["mv"]), W, H)


def test_library_exports_the_entry_points():
    from viewport_entropy_toolkit import _native
    lib = ctypes.CDLL(str(_native.LIB_PATH))
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _native.SIGNATURES
    # the leading arguments of the saliency call (samples, U, T, window, stride), then sigma, W, H, pred, n_pred, want_dist, the outputs
    i, p, d = ctypes.c_int, ctypes.c_void_p, ctypes.c_double
    for tail, at in (("", 7), ("_ids", 6), ("_host", 8)):
        res, args = _native.SIGNATURES["vet_saliency" + tail]
        mine = _native.SIGNATURES["vet_saliency_score" + tail]
        assert mine[0] == res and mine[1][:at] == args[:at], tail
        assert mine[1][at:at + 6] == [d, i, i, p, i, i], tail
        assert mine[1][at + 6:] == [p] * (3 if tail == "_host" else 5), tail     # map, stats, counts (+ status, stream)
    for name in ("saliency_score", "saliency_score_device"):
        assert hasattr(_native.Plan, name)
    stem, pairs, whole, empty_ok, outputs = _native._SALIENCY_SCORE_CALL
    assert (stem, pairs, whole, empty_ok) == ("vet_saliency_score", False, True, False)
    assert [(key, dims, np.dtype(dt).name, optional) for key, dims, dt, optional in outputs] == \
        [("map", "RYX", "float64", True), ("stats", "9R", "float64", False), ("counts", "2R", "int64", False)]
    assert _native.SALIENCY_SCORE_STATS == sco.STATS
    assert len(_native._ROW_CALLS) == 11                          # the other tables as they were
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
        flat = re.sub(r"\s+", " ", args)
        assert "double sigma_rad, int W, int H, const double *" in flat and "int n_pred, int want_dist, double *" in flat, name
    assert "#define VET_VERSION 141" in header
    # the definition is written out: what a reader needs to recompute a value
    for phrase in ("vet_saliency_score", "BILINEAR", "atan2(y, x)", "fx = (lon + pi) / (2 * pi) * W - 0.5", "wrap modulo W",
                   "top + ty * (bot - top)", "a + t * (b - a)", "mass_pred", "var_pred", "info_gain", "-inf", "L(v_i) + 0.5 * E(v_i)",
                   "acc = acc + a_y * (double)count", "Mann-Whitney", "STATED DEPARTURE", "kl_ab", "+inf", "n_pred = 1", "n_pred = R",
                   "PRECONDITION", "[9][R]", "[2][R]", "k_score_sort", "k_score_points", "k_score_rows", "No FP atomics",
                   "pred NULL", "n_pred other than 1 or R", "auc, nss, info_gain, cc, sim, jsd, kl, mass, mass_pred"):
        assert phrase in header, phrase


def good_map(h=18, w=36):
    return np.random.default_rng(0).uniform(0.5, 1.5, size=(h, w))


BAD_MAPS = [None, [[1.0, 2.0]], np.ones((18, 36), dtype=np.float32), np.ones((18, 36), dtype=np.int64), np.ones(36), np.ones((1, 2, 18, 36)),
            np.ones((5, 18, 36)), np.ones((27, 18, 36)), np.ones((18, 1)), np.ones((2049, 4)), np.ones((3, 4097))]


def poisoned(value):
    m = good_map()
    m[3, 4] = value
    return m


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
        an.compute_saliency_score(good_map())
    mu = np.full((80, 4), 0.5)
    an.load_arrays(np.arange(80) * 0.1, mu, mu)

    def no_engine(*a, **k):
        raise AssertionError("the engine was touched before the arguments were checked")

    an._get_plan = no_engine
    an._grid_plan = no_engine
    for kw in (dict(window=0), dict(window=5, stride=0), dict(window=81), dict(window=2.5), dict(window=True),
               dict(window=5, stride=1.5), dict(window="5"), dict(sigma_deg=0.0), dict(sigma_deg=-1.0), dict(sigma_deg=float("nan")),
               dict(sigma_deg=float("inf")), dict(sigma_deg=180.5), dict(sigma_deg="5")):
        with pytest.raises(ValueError):
            an.compute_saliency_score(good_map(), **kw)
    for bad in BAD_MAPS:                                           # window 5, stride 1: 76 rows — 5 and 27 maps are the wrong number
        with pytest.raises(ValueError):
            an.compute_saliency_score(bad, window=5)
    for value in (-1e-300, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="finite and non-negative"):
            an.compute_saliency_score(poisoned(value), window=5)
    with pytest.raises(ValueError, match="beyond 4 GiB"):
        an.compute_saliency_score(np.ones((2048, 4096)), window=1, keep_maps=True)       # 80 maps of 64 MiB
    with pytest.raises(AssertionError, match="engine was touched"):
        an.compute_saliency_score(good_map())
    with pytest.raises(AssertionError, match="engine was touched"):
        an.compute_saliency_score(np.ones((76, 18, 36)), window=5, sigma_deg=2.0, distribution=False)
    with pytest.raises(AssertionError, match="engine was touched"):
        an.compute_saliency_score(np.ones((2048, 4096)), window=None, keep_maps=True)    # one map: 64 MiB
    doc = cls.compute_saliency_score.__doc__
    for word in ("auc", "nss", "info_gain", "cc", "sim", "jsd", "kl", "mass_pred", "-inf", "+inf", "Mann-Whitney", "static", "distribution"):
        assert word in doc, word


def test_plan_wrapper_refuses_bad_arguments_before_the_library_is_called():
    from viewport_entropy_toolkit import _native

    class NoLibrary(_native.Plan):
        def __init__(self):
            pass

        def close(self):
            pass

        def _row_host(self, *a, **k):
            raise AssertionError("the library was called")

        def _row_device(self, *a, **k):
            raise AssertionError("the library was called")

    plan = NoLibrary()
    ids = np.zeros((30, 4), dtype=np.int32)
    for kw in (dict(sigma_deg=0.0), dict(sigma_deg=np.nan), dict(sigma_deg=181.0), dict(sigma_deg=True), dict(sigma_deg="5")):
        with pytest.raises(ValueError):
            plan.saliency_score(ids=ids, maps=good_map(), **kw)
        with pytest.raises(ValueError):
            plan.saliency_score_device(8, 8, 4, 30, 1, 1, 8, 1, 36, 18, kw["sigma_deg"], d_stats=8)
    for kw in (dict(width=1), dict(width=4097), dict(height=0), dict(height=2049)):
        with pytest.raises(ValueError):
            plan.saliency_score_device(8, 8, 4, 30, 1, 1, 8, 1, **dict(dict(width=36, height=18), **kw), d_stats=8)
    for bad in BAD_MAPS:
        with pytest.raises(ValueError):
            plan.saliency_score(ids=ids, maps=bad, window=5)
    for value in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite and non-negative"):
            plan.saliency_score(ids=ids, maps=poisoned(value), window=5)
        with pytest.raises(AssertionError, match="library was called"):             # check=False: the caller vouches for the map
            plan.saliency_score(ids=ids, maps=poisoned(value), window=5, check=False)
    with pytest.raises(AssertionError, match="library was called"):
        plan.saliency_score(ids=ids, maps=good_map())
    with pytest.raises(AssertionError, match="library was called"):
        plan.saliency_score(ids=ids, maps=np.ones((26, 18, 36)), window=5)
    # window and stride are refused by _row_host, as for every row call: from vet_window_rows, a host function without a device
    real = _native.Plan._row_host
    lib_only = NoLibrary()
    lib_only.lib = _native.load_library()
    lib_only.n_tiles = [1]
    pred = good_map()
    for kw in (dict(window=0), dict(window=31), dict(stride=0)):
        with pytest.raises(ValueError, match="window"):
            real(lib_only, _native._SALIENCY_SCORE_CALL, None, None, ids, kw.get("window", 1), kw.get("stride", 1), set(), True,
                 extra=(0.1, 36, 18, _native._ptr(pred), 1, 1), extra_dims={"Y": 18, "X": 36, "2": 2, "9": 9})
    assert "info_gain" in _native.Plan.saliency_score.__doc__


def test_dataframe_assembles_from_a_canned_result():
    from viewport_entropy_toolkit.analyzers._base import _EntropyAnalyzerBase as Base
    times = np.arange(10) * 0.5
    stats = np.arange(9 * 2, dtype=np.float64).reshape(9, 2)
    stats[:8, 1] = np.nan
    stats[2, 0], stats[6, 0] = -np.inf, np.inf
    counts = np.array([[7, 0], [5, 0]], dtype=np.int64)
    maps = np.arange(2 * 3 * 4, dtype=np.float64).reshape(2, 3, 4)
    df = Base._saliency_score_frame(times, ["a", "b", "c"], 4, 3, dict(stats=stats, counts=counts, map=maps, code=0), 5.0, 4, 3, True, True)
    assert list(df.columns) == COLUMNS + ["map"] and len(df) == 2
    assert df["time"].tolist() == [0.0, 1.5] and df["time_end"].tolist() == [1.5, 3.0]
    assert df["samples"].tolist() == [7, 0] and df["distinct"].tolist() == [5, 0]
    for k, name in enumerate(sco.STATS):
        assert df[name].to_numpy().tobytes() == stats[k].tobytes(), name
    assert df["info_gain"][0] == -np.inf and df["kl"][0] == np.inf and np.isnan(df["auc"][1]) and df["mass_pred"][1] == 17.0
    assert df["map"][1].shape == (3, 4) and np.shares_memory(df["map"][1], maps) and np.array_equal(df["map"][1], maps[1])
    assert df.attrs == dict(sigma_deg=5.0, kappa=1.0 / math.radians(5.0) ** 2, width=4, height=3, window=4, stride=3,
                            users=["a", "b", "c"], static=True, distribution=True)
    plain = Base._saliency_score_frame(times, ["a"], 4, 3, dict(stats=stats, counts=counts, map=None, code=0), 5.0, 4, 3, False, False)
    assert list(plain.columns) == COLUMNS and plain.attrs["static"] is False and plain.attrs["distribution"] is False


# ------------------------------------------------------------------------------------------- the oracle against the definition
def test_sample_returns_the_cell_value_at_cell_centres_and_wraps():
    """at a cell centre the interpolation weights are 0 up to the rounding of atan2 / acos: the cell's value to 1e-12 of the map's
    range; halfway across the antimeridian the mean of the first and the last column; beyond the outermost cell-centre latitudes
    the rows clamp"""
    mw, mh = 12, 6
    P = np.random.default_rng(1).uniform(1.0, 2.0, size=(mh, mw))
    centres, lon, lat = so.cell_centres(mw, mh)
    np.testing.assert_allclose(sco.sample(P, centres), P.reshape(-1), rtol=0, atol=1e-12)
    phi = np.radians(90.0 - lat[2])
    seam = np.array([[-math.sin(phi), 0.0, math.cos(phi)]])       # lon = 180: atan2(0, -x) = pi, halfway between columns 11 and 0
    np.testing.assert_allclose(sco.sample(P, seam), 0.5 * (P[2, 11] + P[2, 0]), rtol=1e-12)
    seam[0, 1] = -1e-300                                          # lon = -180: the other wrap
    np.testing.assert_allclose(sco.sample(P, seam), 0.5 * (P[2, 11] + P[2, 0]), rtol=1e-12)
    top = np.radians(3.0)                                         # 3 degrees from the pole: above the first cell-centre latitude (75)
    theta = np.radians(lon[4])
    north = np.array([[math.sin(top) * math.cos(theta), math.sin(top) * math.sin(theta), math.cos(top)]])
    np.testing.assert_allclose(sco.sample(P, north), P[0, 4], rtol=1e-12)
    np.testing.assert_allclose(sco.sample(P, north * [1, 1, -1]), P[5, 4], rtol=1e-12)
    # the pole: lon 0 by definition, halfway between columns 5 and 6 of the top row
    np.testing.assert_allclose(sco.sample(P, np.array([[0.0, 0.0, 1.0]])), 0.5 * (P[0, 5] + P[0, 6]), rtol=1e-15)
    flat = np.full((mh, mw), 0.7)
    rnd = so.unit_rows(np.random.default_rng(2).normal(size=(500, 3)))
    assert (sco.sample(flat, rnd) == 0.7).all()                   # four equal corners: exactly their value


@pytest.mark.parametrize("mw,mh", [(4, 2), (2, 1)])
def test_oracle_constant_map(table, g15_ids, mw, mh):
    """a constant map: nothing is below any sample's value and everything ties: u = 0.5 * sum a_p = 0.5, auc 0.5 to 1e-15.  On 4 x 2 and
    2 x 1 cells every a_p is 0.125 or 0.5 exactly, so mass_pred is the constant, var_pred is 0.0 and nss is 0 / 0 = NaN; info_gain is
    log2(1) = 0"""
    o = sco.Oracle(table, mw, mh)
    r = o.row(g15_ids[:10], np.full((mh, mw), 3.0), math.radians(5.0))
    assert abs(r["stats"][0] - 0.5) <= 1e-15 and np.isnan(r["stats"][1]) and r["stats"][2] == 0.0 and r["stats"][8] == 3.0
    assert np.isnan(r["stats"][3]) and np.isfinite(r["stats"][4:8]).all()         # cc is 0 / 0 as well; sim, jsd, kl against uniform
    assert r["gap"] == np.inf                                    # no unequal pair
    wide = sco.Oracle(table, 36, 18).row(g15_ids[:10], np.full((18, 36), 0.25), math.radians(5.0), distribution=False)
    assert abs(wide["stats"][0] - 0.5) <= 1e-15 and np.isnan(wide["stats"][3:8]).all()


def test_oracle_half_sphere_map(table):
    """1 on the northern cell rows, 0 on the southern (H even), every sample at least one cell row north of the border: mass_pred is
    0.5, every v is exactly 1 (four equal corners), L = the southern half = 0.5, E = the northern half = 0.5: auc 0.75, info_gain
    log2(1 / 0.5) = 1 bit, nss = (1 - 0.5) / sqrt(0.25) = 1"""
    mw, mh = 36, 18
    P = np.zeros((mh, mw))
    P[:mh // 2] = 1.0
    rng = np.random.default_rng(5)
    py = rng.integers(1, 80, size=(6, 5))                         # polar angle < 72 degrees: north of the centre of cell row 7
    px = rng.integers(0, W + 1, size=(6, 5))
    ids = (py * (W + 1) + px).astype(np.int32)
    ids[2, 3] = -1
    o = sco.Oracle(table, mw, mh)
    r = o.row(ids, P, math.radians(5.0), distribution=False)
    assert (r["v"] == 1.0).all()
    np.testing.assert_allclose(r["stats"][[0, 1, 2, 8]], [0.75, 1.0, 1.0, 0.5], rtol=0, atol=1e-14)
    assert r["counts"][0] == 29
    south = o.row(((200 - py) * (W + 1) + px).astype(np.int32), P, math.radians(5.0))      # mirrored: every sample on a zero
    assert np.isneginf(south["stats"][2]) and abs(south["stats"][0] - 0.25) <= 1e-14 and np.isposinf(south["stats"][6])


@pytest.mark.parametrize("mw,mh,sigma,window", [(36, 18, 5.0, 5), (37, 19, 2.0, 1), (18, 9, 10.0, 60), (50, 25, 5.0, 20)])
def test_the_two_auc_forms_agree_and_the_test_maps_meet_the_gap_condition(table, g15_ids, mw, mh, sigma, window):
    o = sco.Oracle(table, mw, mh)
    P = sco.density_map(o, g15_ids, math.radians(sigma), 7)
    assert (P > 0).all() and len(np.unique(P)) == P.size
    for r in range(0, 60 - window + 1, max(window, 7)):
        uniq, _ = np.unique(g15_ids[r:r + window][g15_ids[r:r + window] >= 0], return_counts=True)
        v = sco.sample(P, o.o.unit[uniq])
        a, b = sco.auc_ranks(v, P, o.a_y), sco.auc_ranks_brute(v, P, o.a_y)
        assert a.tobytes() == b.tobytes() and ((a > 0) & (a < 1)).all()
        assert sco.auc_gap(v, P) >= sco.GAP_MIN
    # the guard sees what it is for: a value a rounding away from a cell's value, and not a value equal to one
    assert sco.auc_gap(np.array([np.nextafter(P[1, 1], 2 * P[1, 1])]), P) < 1e-15 and sco.auc_gap(np.array([P[1, 1]]), P) >= sco.GAP_MIN
    tie = sco.auc_ranks(np.array([P[1, 1]]), P, o.a_y) - sco.auc_ranks(np.array([np.nextafter(P[1, 1], 0)]), P, o.a_y)
    np.testing.assert_allclose(tie, 0.5 * o.a_y[1], rtol=1e-9)    # a tie counts a half


def test_scaling_a_map_by_a_power_of_two_scales_mass_pred_alone(table, g15_ids):
    o = sco.Oracle(table, 36, 18)
    P = sco.density_map(o, g15_ids, math.radians(5.0), 3)
    P[4:7, 10:14] = 0.0                                           # a zero region too
    base = o.rows(g15_ids, P, 5, 5, math.radians(5.0))
    for k in (-20, 1, 20):
        got = o.rows(g15_ids, P * 2.0 ** k, 5, 5, math.radians(5.0))
        assert got["stats"][:8].tobytes() == base["stats"][:8].tobytes(), k
        assert got["stats"][8].tobytes() == (base["stats"][8] * 2.0 ** k).tobytes(), k
        assert got["counts"].tobytes() == base["counts"].tobytes()


def test_oracle_shapes_and_empty_rows(table, g15_ids):
    o = sco.Oracle(table, 18, 9)
    ids = np.array(g15_ids[:12])
    ids[4] = -1
    P = sco.density_map(o, g15_ids, math.radians(10.0), 1, n=12)
    r = o.rows(ids, P, 1, 1, math.radians(10.0))
    assert r["stats"].shape == (9, 12) and r["counts"].shape == (2, 12) and r["map"].shape == (12, 9, 18) and r["counts"].dtype == np.int64
    assert np.isnan(r["stats"][:8, 4]).all() and r["stats"][8, 4] > 0 and r["counts"][:, 4].tolist() == [0, 0]
    assert not np.isnan(np.delete(r["stats"], 4, axis=1)).any()
    # a walk's own density predicts it: far above chance on every metric
    assert (np.delete(r["stats"][0], 4) > 0.9).all() and (np.delete(r["stats"][1], 4) > 1.0).all() and (np.delete(r["stats"][2], 4) > 1.0).all()
    loc = o.rows(ids, P, 1, 1, math.radians(10.0), distribution=False)
    assert loc["map"] is None and loc["stats"][[0, 1, 2, 8]].tobytes() == r["stats"][[0, 1, 2, 8]].tobytes() and np.isnan(loc["stats"][3:8]).all()
