"""Viewer congruency (each viewer's leave-one-out saliency score per window), CPU side: the C-ABI surface, the argument handling of
the analyzers and of Plan, the DataFrame, and the numpy oracle of tests/_congruency_oracle.py checked against closed forms — two
single samples a known angle apart, everyone on one direction, a far pair at a narrow kernel, the overlap integral G against a
quadrature, and the split Q - 2 B_u + A_u the library walks against the direct double sum.  No GPU."""
import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest

from tests import _congruency_oracle as co
from tests import _saliency_oracle as so

W, H = 100, 200
SYMBOLS = ("vet_congruency", "vet_congruency_ids", "vet_congruency_host")
COLUMNS = ["user", "time", "time_end", "samples", "distinct", "others", "lift", "info_gain", "nss"]
ROW_COLUMNS = ["time", "time_end", "scored", "lift", "info_gain", "nss"]


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
    # the leading arguments of the saliency call (samples, U, T, window, stride), then sigma, want_nss, the three outputs
    i, p, d = ctypes.c_int, ctypes.c_void_p, ctypes.c_double
    for tail, at in (("", 7), ("_ids", 6), ("_host", 8)):
        res, args = _native.SIGNATURES["vet_saliency" + tail]
        mine = _native.SIGNATURES["vet_congruency" + tail]
        assert mine[0] == res and mine[1][:at] == args[:at], tail
        assert mine[1][at:at + 2] == [d, i], tail
        assert mine[1][at + 2:] == [p] * (3 if tail == "_host" else 5), tail     # three outputs (+ status, stream)
    for name in ("congruency", "congruency_device"):
        assert hasattr(_native.Plan, name)
    stem, pairs, whole, empty_ok, outputs = _native._CONGRUENCY_CALL
    assert (stem, pairs, whole, empty_ok) == ("vet_congruency", False, True, False)
    assert [(key, dims, np.dtype(dt).name, optional) for key, dims, dt, optional in outputs] == \
        [("stats", "3UR", "float64", False), ("counts", "3UR", "int64", False), ("rows", "4R", "float64", False)]
    assert _native.CONGRUENCY_STATS == co.STATS
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
        assert "double sigma_rad, int want_nss" in re.sub(r"\s+", " ", args), name
    assert "#define VET_VERSION 141" in header
    # the definition is written out: what a reader needs to recompute a value
    for phrase in ("vet_congruency", "w_j = m_j - a_j", "fma((double)w_j", "N' = N - n_u", "-expm1(-2 * x)", "x < 1e-4",
                   "Q_u = (Q - 2 * B_u) + A_u", "lift", "info_gain", "-inf", "NOT SCORED", "[3][n_users][R]", "[4][R]",
                   "k_congruency_points", "k_congruency_users", "k_congruency_rows", "No FP atomics", "n_users < 2"):
        assert phrase in header, phrase


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
        an.compute_congruency()
    mu = np.full((30, 4), 0.5)
    an.load_arrays(np.arange(30) * 0.1, mu, mu)

    def no_engine(*a, **k):
        raise AssertionError("the engine was touched before the arguments were checked")

    an._get_plan = no_engine
    an._grid_plan = no_engine
    for kw in (dict(window=0), dict(window=5, stride=0), dict(window=31), dict(window=2.5), dict(window=True),
               dict(window=5, stride=1.5), dict(window="5"), dict(sigma_deg=0.0), dict(sigma_deg=-1.0), dict(sigma_deg=float("nan")),
               dict(sigma_deg=float("inf")), dict(sigma_deg=180.5), dict(sigma_deg="5")):
        with pytest.raises(ValueError):
            an.compute_congruency(**kw)
    with pytest.raises(AssertionError, match="engine was touched"):
        an.compute_congruency()                                   # window=None: the whole video
    with pytest.raises(AssertionError, match="engine was touched"):
        an.compute_congruency(window=5, stride=5, sigma_deg=2.0, nss=False)
    an.load_arrays(np.arange(30) * 0.1, mu[:, :1], mu[:, :1])    # one viewer: nobody to be congruent with
    an._get_plan = no_engine
    an._grid_plan = no_engine
    with pytest.raises(ValueError, match="two viewers"):
        an.compute_congruency(window=5)
    doc = cls.compute_congruency.__doc__
    for word in ("lift", "info_gain", "nss", "others", "scored", "-inf", 'attrs["rows"]'):
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
    ids = np.zeros((10, 4), dtype=np.int32)
    for kw in (dict(sigma_deg=0.0), dict(sigma_deg=np.nan), dict(sigma_deg=181.0), dict(sigma_deg=True), dict(sigma_deg="5")):
        with pytest.raises(ValueError):
            plan.congruency(ids=ids, **kw)
        with pytest.raises(ValueError):
            plan.congruency_device(8, 8, 4, 10, 1, 1, kw["sigma_deg"], d_stats=8)
    with pytest.raises(AssertionError, match="library was called"):
        plan.congruency(ids=ids)
    # window and stride are refused by _row_host, as for every row call: from vet_window_rows, a host function without a device
    real = _native.Plan._row_host
    lib_only = NoLibrary()
    lib_only.lib = _native.load_library()
    lib_only.n_tiles = [1]
    for kw in (dict(window=0), dict(window=11), dict(stride=0)):
        with pytest.raises(ValueError, match="window"):
            real(lib_only, _native._CONGRUENCY_CALL, None, None, ids, kw.get("window", 1), kw.get("stride", 1), set(), True,
                 extra=(0.1, 1))
    assert "info_gain" in _native.Plan.congruency.__doc__


def test_dataframe_assembles_from_a_canned_result():
    from viewport_entropy_toolkit.analyzers._base import _EntropyAnalyzerBase as Base
    times = np.arange(10) * 0.5
    stats = np.arange(3 * 3 * 2, dtype=np.float64).reshape(3, 3, 2)
    stats[:, 2, 1] = np.nan
    stats[1, 0, 0] = -np.inf
    counts = np.arange(100, 118, dtype=np.int64).reshape(3, 3, 2)
    rows = np.array([[3.0, 2.0], [1.5, 2.5], [-np.inf, 0.25], [0.5, np.nan]])
    res = dict(stats=stats, counts=counts, rows=rows, code=0)
    df = Base._congruency_frame(times, ["a", "b", "c"], 4, 3, res, 5.0)
    assert list(df.columns) == COLUMNS and len(df) == 6
    assert df["user"].tolist() == ["a", "a", "b", "b", "c", "c"]                   # user-major
    assert df["time"].tolist() == [0.0, 1.5] * 3 and df["time_end"].tolist() == [1.5, 3.0] * 3
    assert df["samples"].tolist() == list(range(100, 106)) and df["distinct"].tolist() == list(range(106, 112))
    assert df["others"].tolist() == list(range(112, 118))
    for k, name in enumerate(co.STATS):
        assert df[name].to_numpy().tobytes() == stats[k].reshape(-1).tobytes(), name
    assert df["info_gain"][0] == -np.inf and np.isnan(df["nss"][5]) and np.isnan(df["lift"][5])
    per_row = df.attrs["rows"]
    assert list(per_row.columns) == ROW_COLUMNS
    assert per_row["time"].tolist() == [0.0, 1.5] and per_row["time_end"].tolist() == [1.5, 3.0]
    assert per_row["scored"].tolist() == [3, 2] and per_row["scored"].dtype == np.int64
    assert per_row["lift"].tolist() == [1.5, 2.5] and per_row["info_gain"][0] == -np.inf and np.isnan(per_row["nss"][1])
    rest = {k: v for k, v in df.attrs.items() if k != "rows"}
    assert rest == dict(users=["a", "b", "c"], sigma_deg=5.0, kappa=1.0 / math.radians(5.0) ** 2, window=4, stride=3)


# ------------------------------------------------------------------------------------------- the oracle against the definition
def vmf_c(kappa):
    return kappa / (2.0 * math.pi * (1.0 - math.exp(-2.0 * kappa)))


@pytest.mark.parametrize("sigma_deg,theta_deg", [(10.0, 15.0), (5.0, 3.0), (30.0, 120.0)])
def test_oracle_two_viewers_one_sample_each(sigma_deg, theta_deg):
    """Each viewer's others are the one sample of the other: lift = 4 pi C exp(kappa (cos theta - 1)), info_gain its log2, Q_u = G(1) —
    the overlap of a kernel with itself — and nss from them"""
    sigma, theta = math.radians(sigma_deg), math.radians(theta_deg)
    kappa = 1.0 / sigma ** 2
    table = np.array([[math.cos(0.3), math.sin(0.3), 0.0], [math.cos(0.3 + theta), math.sin(0.3 + theta), 0.0]])
    o = co.Oracle(table)
    r = o.row(np.array([[0, 1]]), sigma)
    C = vmf_c(kappa)
    lift = 4.0 * math.pi * C * math.exp(kappa * (math.cos(theta) - 1.0))
    np.testing.assert_allclose(r["stats"][0], lift, rtol=1e-12)
    np.testing.assert_allclose(r["stats"][1], math.log2(lift), rtol=1e-12, atol=1e-12)
    G1 = float(co.overlap(1.0, kappa))
    np.testing.assert_allclose(r["Q"], G1, rtol=1e-14)
    # G(1) in closed form: (2 pi / (2 kappa)) (1 - exp(-4 kappa)), the integral of exp(2 kappa (cos - 1))
    np.testing.assert_allclose(G1, math.pi / kappa * (1.0 - math.exp(-4.0 * kappa)), rtol=1e-14)
    mu = 1.0 / (4.0 * math.pi)
    nss = (lift * mu - mu) / math.sqrt(C * C * G1 * mu - mu * mu)
    np.testing.assert_allclose(r["stats"][2], nss, rtol=1e-11)
    assert r["counts"].tolist() == [[1, 1], [1, 1], [1, 1]] and r["row"][0] == 2.0
    np.testing.assert_allclose(r["row"][1:], [lift, math.log2(lift), nss], rtol=1e-11, atol=1e-12)


def test_oracle_everyone_on_one_direction(table):
    """Five viewers, three frames, one direction: the others' density at it is C whoever is left out: lift = 4 pi C"""
    sigma = math.radians(5.0)
    ids = np.full((3, 5), 77 * 101 + 31)
    ids[1, 2] = -1                                                # one viewer with a sample less
    r = co.Oracle(table).row(ids, sigma)
    C = vmf_c(1.0 / sigma ** 2)
    # the fused dot of a rounded unit vector with itself is 1 up to three roundings: exp(kappa * (c - 1)) is 1 up to 3 kappa 2**-53
    tol = 4.0 / sigma ** 2 * 2.0 ** -53
    np.testing.assert_allclose(r["stats"][0], 4.0 * math.pi * C, rtol=tol)
    np.testing.assert_allclose(r["stats"][1], math.log2(4.0 * math.pi * C), rtol=tol)
    assert r["counts"][0].tolist() == [3, 3, 2, 3, 3] and r["counts"][1].tolist() == [1] * 5 and r["counts"][2].tolist() == [11, 11, 12, 11, 11]
    assert (r["stats"][2] > 0).all() and np.ptp(r["stats"][2]) < 1e-12 * r["stats"][2][0]       # one density, whoever is left out
    assert r["row"][0] == 5.0


def test_oracle_far_pair_at_a_narrow_kernel():
    """sigma 1 degree, two viewers 90 degrees apart: exp(-kappa) = exp(-3283) is 0.0, so the other's density is 0.0 at the viewer's
    sample: lift 0.0, info_gain -inf, nss finite and negative (the density is below its sphere average)"""
    table = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    r = co.Oracle(table).row(np.array([[0, 1]]), math.radians(1.0))
    assert (r["stats"][0] == 0.0).all() and np.isneginf(r["stats"][1]).all()
    assert np.isfinite(r["stats"][2]).all() and (r["stats"][2] < 0).all()
    assert r["row"][1] == 0.0 and np.isneginf(r["row"][2]) and r["row"][3] < 0


def test_oracle_absent_and_lonely_viewers(table):
    ids = np.array([[5, -1, -1], [7, -1, -1]])                    # viewer 0 alone, the others absent
    r = co.Oracle(table).row(ids, math.radians(5.0))
    assert np.isnan(r["stats"]).all() and r["counts"].tolist() == [[2, 0, 0], [2, 0, 0], [0, 2, 2]]
    assert r["row"][0] == 0.0 and np.isnan(r["row"][1:]).all()


@pytest.mark.parametrize("sigma_deg", [5.0, 30.0])
def test_overlap_against_a_quadrature(sigma_deg):
    """G(cos theta) against the midpoint rule on a 2 880 x 1 440 lat/lon grid (cells of 0.125 degrees: within h^2 / (24 sigma^2),
    2.6e-5 at sigma 5 degrees, of a smooth integral; allowed 1e-4) for centres 0, 7, 40, 90, 170 and 180 degrees apart"""
    kappa = 1.0 / math.radians(sigma_deg) ** 2
    nlon, nlat = 2880, 1440
    lon = (np.arange(nlon) + 0.5) / nlon * 2.0 * np.pi
    pol = (np.arange(nlat) + 0.5) / nlat * np.pi
    area = (np.cos(np.pi * np.arange(nlat) / nlat) - np.cos(np.pi * (np.arange(nlat) + 1) / nlat)) * (2.0 * np.pi / nlon)
    x = np.sin(pol)[:, None] * np.cos(lon)[None, :]
    z = np.broadcast_to(np.cos(pol)[:, None], x.shape)
    k0 = np.exp(kappa * (x - 1.0))                                # a kernel centred on +x
    for theta_deg in (0.0, 7.0, 40.0, 90.0, 170.0, 180.0):
        t = math.radians(theta_deg)
        k1 = np.exp(kappa * (math.cos(t) * x + math.sin(t) * z - 1.0))             # a kernel theta away, in the x-z plane
        want = float(((k0 * k1).sum(axis=1) * area).sum())
        got = float(co.overlap(math.cos(t), kappa))
        assert abs(got - want) <= 1e-4 * want + 1e-300, (sigma_deg, theta_deg, got, want)


def test_overlap_small_branch_meets_the_main_branch():
    """at x = kappa * r = 1e-4 the series 4 pi exp(-2 kappa) (1 + x^2 / 6) and the main branch agree to the series' next term, x^4 / 120"""
    for kappa in (1.0 / math.radians(30.0) ** 2, 1.0 / math.radians(60.0) ** 2, 0.5):
        x = 1e-4
        r = x / kappa
        main = 2.0 * math.pi * math.exp(kappa * (r - 2.0)) * (-math.expm1(-2.0 * x)) / x
        small = 4.0 * math.pi * math.exp(-2.0 * kappa) * (1.0 + x * x / 6.0)
        assert abs(main - small) <= 4e-15 * small, (kappa, main, small)       # the roundings of kappa * (r - 2)
        c = r * r / 2.0 - 1.0                                     # the cosine with sqrt(2 + 2c) = r
        below, above = co.overlap(np.array([c * (1 + 1e-14), c * (1 - 1e-14)]), kappa)       # either side of the switch
        assert abs(below - above) <= 1e-12 * small


@pytest.mark.parametrize("sigma_deg", [1.0, 5.0, 60.0])
def test_split_quadratic_form_against_the_direct_sum(table, g15_ids, sigma_deg):
    """Q - 2 B_u + A_u, as the library takes it, against w . G . w on golden G15, rows of 20 frames: the split is of Q's size, so the
    subtraction costs a few ulp of Q — held to 1e-12 of Q_u here"""
    kappa = 1.0 / math.radians(sigma_deg) ** 2
    unit = so.unit_rows(table)
    for r in range(3):
        uniq, m, A = co.lists(g15_ids[20 * r:20 * r + 20], len(unit))
        c = so.cosines(unit[uniq], unit[uniq]) if len(uniq) ** 2 <= co.EXACT_PAIRS else unit[uniq] @ unit[uniq].T
        direct, split = co.split_forms(m, A, co.overlap(c, kappa))
        assert (direct > 0).all()
        np.testing.assert_allclose(split, direct, rtol=1e-12)


def test_oracle_shapes_and_window_one(table, g15_ids):
    o = co.Oracle(table)
    r = o.rows(g15_ids, 1, 1, math.radians(2.0))
    assert r["stats"].shape == (3, 8, 60) and r["counts"].shape == (3, 8, 60) and r["rows"].shape == (4, 60)
    assert r["counts"].dtype == np.int64
    absent = r["counts"][0] == 0
    assert absent.sum() == 16 and np.array_equal(np.isnan(r["stats"][0]), absent)          # the 16 absent samples of G15
    assert np.array_equal(r["rows"][0], (~absent).sum(axis=0).astype(np.float64))
    five = o.rows(g15_ids, 5, 5, math.radians(5.0))
    assert not np.isnan(five["stats"]).any() and (five["rows"][0] == 8.0).all()
    # viewers of one walk look where the others look: far above chance
    assert (five["rows"][1] > 1.0).all() and (five["rows"][3] > 0.0).all()
