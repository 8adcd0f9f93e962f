"""Saliency similarity (CC, SIM, JSD, KL and NSS between the saliency maps of two audiences), CPU side: the C-ABI surface, the
argument handling of the analyzers and of Plan, the DataFrame, and the numpy oracle of tests/_saliency_similarity_oracle.py checked
against what the definition implies — symmetry under exchanging the labels, identical audiences, the closed forms of two single
samples a known angle apart, a far pair at a narrow kernel.  No GPU."""
import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest

from tests import _saliency_oracle as so
from tests import _saliency_similarity_oracle as sso

W, H = 100, 200
SYMBOLS = ("vet_saliency_similarity", "vet_saliency_similarity_ids", "vet_saliency_similarity_host")
COLUMNS = ["time", "time_end", "samples_a", "samples_b", "distinct_a", "distinct_b", "cc", "sim", "jsd", "kl_ab", "kl_ba", "nss_ab",
           "nss_ba", "mass_a", "mass_b"]


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
    # the leading arguments of the saliency call (samples, U, T, window, stride), then groups, sigma, W, H, the three outputs
    i, p, d = ctypes.c_int, ctypes.c_void_p, ctypes.c_double
    for tail, at in (("", 7), ("_ids", 6), ("_host", 8)):
        res, args = _native.SIGNATURES["vet_saliency" + tail]
        mine = _native.SIGNATURES["vet_saliency_similarity" + tail]
        assert mine[0] == res and mine[1][:at] == args[:at], tail
        assert mine[1][at:at + 4] == [p, d, i, i], tail
        assert mine[1][at + 4:] == [p] * (3 if tail == "_host" else 5), tail     # three outputs (+ status, stream)
    for name in ("saliency_similarity", "saliency_similarity_device"):
        assert hasattr(_native.Plan, name)
    stem, pairs, whole, empty_ok, outputs = _native._SALIENCY_SIMILARITY_CALL
    assert (stem, pairs, whole, empty_ok) == ("vet_saliency_similarity", False, True, False)
    assert [(key, dims, np.dtype(dt).name, optional) for key, dims, dt, optional in outputs] == \
        [("maps", "2RYX", "float64", True), ("stats", "9R", "float64", False), ("counts", "4R", "int64", False)]
    assert _native.SALIENCY_SIMILARITY_STATS == sso.STATS
    assert len(_native._ROW_CALLS) == 11 and sorted(_native._SALIENCY_CALLS) == [False, True]        # the other tables as they were
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
        assert "const int8_t *groups" in args, name
    assert "#define VET_VERSION 141" in header
    # the definition is written out: what a reader needs to recompute a value
    for phrase in ("vet_saliency_similarity", "cov / sqrt(va*vb)", "fmin(qa, qb)", "qa*log2(qa/m)", "qa*log2(qa/qb)", "+inf",
                   "NSS BY POINT EVALUATION", "g_Y = C / (double)N_Y", "byte for byte", "[9][Rows]", "[4][Rows]", "[2][Rows][H][W]",
                   "k_saliency_mask", "k_saliency_points", "k_saliency_compare", "No FP atomics"):
        assert phrase in header, phrase
    switch = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int vet_test_saliency_tile", header, flags=re.S).group(1)
    assert "k_saliency_points" in switch and "k_saliency_map" in switch


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
        an.compute_saliency_similarity([0, 1])
    mu = np.full((30, 4), 0.5)
    an.load_arrays(np.arange(30) * 0.1, mu, mu)

    def no_engine(*a, **k):
        raise AssertionError("the engine was touched before the arguments were checked")

    an._get_plan = no_engine
    an._grid_plan = no_engine
    good = ["x", "x", "y", None]
    for groups in (None, "xxyy", 5, ["x", "x", "y"], ["x"] * 4, ["x", "y", "z", "x"], ["x", 1, "y", "x"], {"nobody": "x"},
                   [None, None, None, "x"]):
        with pytest.raises(ValueError):
            an.compute_saliency_similarity(groups)
    for kw in (dict(window=0), dict(window=5, stride=0), dict(window=31), dict(window=2.5), dict(window=True),
               dict(window=5, stride=1.5), dict(window="5"), dict(sigma_deg=0.0), dict(sigma_deg=-1.0), dict(sigma_deg=float("nan")),
               dict(sigma_deg=float("inf")), dict(sigma_deg=180.5), dict(sigma_deg="5"), dict(width=1), dict(width=4097),
               dict(width=36.0), dict(height=0), dict(height=2049), dict(height=True)):
        with pytest.raises(ValueError):
            an.compute_saliency_similarity(good, **kw)
    # the 4 GiB guard counts both maps: 30 rows x 2 maps of 4096 x 2048 are 3.75 GiB, of 4096 x 2048 at 40 rows it would be 5 GiB
    with pytest.raises(AssertionError, match="engine was touched"):
        an.compute_saliency_similarity(good, width=4096, height=2048, keep_maps=True)
    an.load_arrays(np.arange(40) * 0.1, np.full((40, 4), 0.5), np.full((40, 4), 0.5))
    an._get_plan = no_engine
    an._grid_plan = no_engine
    with pytest.raises(ValueError, match="4 GiB.*larger stride.*coarser map.*keep_maps=False"):
        an.compute_saliency_similarity(good, width=4096, height=2048, keep_maps=True)
    with pytest.raises(AssertionError, match="engine was touched"):           # without the maps the call goes on to the engine
        an.compute_saliency_similarity(good, width=4096, height=2048)
    with pytest.raises(AssertionError, match="engine was touched"):
        an.compute_saliency_similarity(good, window=None)
    doc = cls.compute_saliency_similarity.__doc__
    for word in ("groups", "cc", "sim", "jsd", "kl_ab", "nss_ab", "mass_a", "keep_maps", "+inf"):
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
    good = dict(ids=ids, groups=[0, 0, 1, -1])
    for kw in (dict(groups=None), dict(groups=[0, 1, 1]), dict(groups=[0, 0, 0, 0]), dict(groups=[1, 1, -1, 1]), dict(groups=[0, 1, 2, 0]),
               dict(groups=[0.0, 1.0, 0.0, 1.0]), dict(groups=[[0, 1, 0, 1]]), dict(sigma_deg=0.0), dict(sigma_deg=np.nan),
               dict(sigma_deg=181.0), dict(sigma_deg=True), dict(width=1), dict(width=4097), dict(width=2.0), dict(height=0),
               dict(height=2049)):
        with pytest.raises(ValueError):
            plan.saliency_similarity(**dict(good, **kw))
        with pytest.raises(ValueError):
            a = dict(dict(groups=[0, 0, 1, -1], sigma_deg=5.0, width=180, height=90), **kw)
            plan.saliency_similarity_device(8, 8, 4, 10, 1, 1, a["groups"], a["sigma_deg"], a["width"], a["height"], d_stats=8)
    with pytest.raises(AssertionError, match="library was called"):
        plan.saliency_similarity(**good)
    # window and stride are refused by _row_host, as for every row call: from vet_window_rows, a host function without a device
    real = _native.Plan._row_host
    lib_only = NoLibrary()
    lib_only.lib = _native.load_library()
    lib_only.n_tiles = [1]
    for kw in (dict(window=0), dict(window=11), dict(stride=0)):
        with pytest.raises(ValueError, match="window"):
            real(lib_only, _native._SALIENCY_SIMILARITY_CALL, None, None, ids, kw.get("window", 1), kw.get("stride", 1), set(), True,
                 extra=(None, 0.1, 36, 18), extra_dims={"Y": 18, "X": 36, "2": 2, "9": 9})
    assert "nss_ab" in _native.Plan.saliency_similarity.__doc__


def test_dataframe_assembles_from_a_canned_result():
    from viewport_entropy_toolkit.analyzers._base import _EntropyAnalyzerBase as Base
    times = np.arange(10) * 0.5
    maps = np.arange(2 * 2 * 3 * 4, dtype=np.float64).reshape(2, 2, 3, 4)
    stats = np.arange(18, dtype=np.float64).reshape(9, 2)
    stats[:7, 1] = np.nan
    stats[3, 0] = np.inf
    counts = np.array([[8, 0], [5, 4], [3, 0], [2, 1]], dtype=np.int64)
    code = np.array([1, 0, -1, 0], dtype=np.int8)
    res = dict(maps=maps, stats=stats, counts=counts, code=0)
    df = Base._saliency_similarity_frame(times, ["a", "b", "c", "d"], 4, 3, code, ("hmd", "screen"), res, 5.0, 4, 3)
    assert list(df.columns) == COLUMNS + ["map_a", "map_b"]
    assert df["time"].tolist() == [0.0, 1.5] and df["time_end"].tolist() == [1.5, 3.0]
    assert df["samples_a"].tolist() == [8, 0] and df["samples_b"].tolist() == [5, 4]
    assert df["distinct_a"].tolist() == [3, 0] and df["distinct_b"].tolist() == [2, 1]
    for k, name in enumerate(sso.STATS):
        assert df[name].to_numpy().tobytes() == stats[k].tobytes(), name
    assert df["kl_ab"][0] == np.inf and np.isnan(df["cc"][1]) and df["mass_b"][1] == 17.0
    for g, name in enumerate(("map_a", "map_b")):
        assert df[name][1].shape == (3, 4) and np.shares_memory(df[name][1], maps) and df[name][1][0, 0] == maps[g, 1, 0, 0]
    assert df.attrs == dict(groups=("hmd", "screen"), sizes=(2, 1), users=(["b", "d"], ["a"]), sigma_deg=5.0,
                            kappa=1.0 / math.radians(5.0) ** 2, width=4, height=3, window=4, stride=3)
    no_maps = Base._saliency_similarity_frame(times, ["a", "b", "c", "d"], 4, 3, code, ("hmd", "screen"), dict(res, maps=None), 5.0, 4, 3)
    assert list(no_maps.columns) == COLUMNS


# ------------------------------------------------------------------------------------------- the oracle against the definition
def test_oracle_swap_symmetry_and_shapes(table, g15_ids):
    code = np.array([0, 0, 0, 0, 1, 1, 1, 1])
    o = sso.Oracle(table, 18, 9)
    r = o.rows(g15_ids, code, 5, 5, math.radians(5.0))
    s = o.rows(g15_ids, 1 - code, 5, 5, math.radians(5.0))
    assert r["maps"].shape == (2, 12, 9, 18) and r["stats"].shape == (9, 12) and r["counts"].shape == (4, 12)
    assert r["counts"].dtype == np.int64 and np.array_equal(r["counts"][[1, 0, 3, 2]], s["counts"])
    assert r["maps"][::-1].tobytes() == s["maps"].tobytes()
    for k in (0, 1, 2):                                          # cc, sim, jsd: unchanged
        np.testing.assert_allclose(r["stats"][k], s["stats"][k], rtol=1e-13, atol=1e-15)
    for a, b in ((3, 4), (5, 6), (7, 8)):                        # kl, nss, mass: exchanged
        assert r["stats"][a].tobytes() == s["stats"][b].tobytes() and r["stats"][b].tobytes() == s["stats"][a].tobytes()
    ok = ~np.isnan(r["stats"][0])
    assert ok.sum() >= 10
    assert (r["stats"][0][ok] <= 1 + 1e-12).all() and (r["stats"][0][ok] >= -1 - 1e-12).all()
    assert (r["stats"][1][ok] >= 0).all() and (r["stats"][1][ok] <= 1 + 1e-12).all()
    assert (r["stats"][2][ok] >= -1e-12).all() and (r["stats"][2][ok] <= 1 + 1e-12).all()
    assert (r["stats"][3:5, ok] >= -1e-12).all()
    # the masked ids give the audience's own saliency row
    a = o.o.rows(sso.masked(g15_ids, code, 0), 5, 5, math.radians(5.0), 2)
    assert a["map"].tobytes() == r["maps"][0].tobytes() and a["stats"][0].tobytes() == r["stats"][7].tobytes()
    assert np.array_equal(a["counts"], r["counts"][[0, 2]])


def test_oracle_identical_and_empty_audiences(table, g15_ids):
    ids = np.concatenate([g15_ids[:20, :3], g15_ids[:20, :3]], axis=1)         # B a column copy of A
    ids[7] = -1                                                   # a frame with nobody
    ids[9, 3:] = -1                                               # a frame without B
    r = sso.Oracle(table, 18, 9).rows(ids, [0, 0, 0, 1, 1, 1], 1, 1, math.radians(5.0))
    same = np.ones(20, dtype=bool)
    same[[7, 9]] = False
    same &= r["counts"][0] > 0
    assert same.sum() >= 15
    assert (r["stats"][2][same] == 0.0).all() and (r["stats"][3][same] == 0.0).all() and (r["stats"][4][same] == 0.0).all()
    np.testing.assert_allclose(r["stats"][0][same], 1.0, rtol=0, atol=1e-13)
    np.testing.assert_allclose(r["stats"][1][same], 1.0, rtol=0, atol=1e-13)
    assert r["stats"][5][same].tobytes() == r["stats"][6][same].tobytes() and (r["stats"][5][same] > 0).all()
    assert np.isnan(r["stats"][:, 7]).all() and r["counts"][:, 7].tolist() == [0, 0, 0, 0]
    assert np.isnan(r["stats"][:7, 9]).all() and np.isnan(r["stats"][8, 9]) and r["stats"][7, 9] > 0 and r["counts"][1, 9] == 0


def hemisphere_share(kappa, theta, n=200001):
    """the share of a von Mises-Fisher density that lies beyond the plane bisecting its mean and a direction theta away: with z
    along the plane's normal, the azimuth integrates to 2 pi I0(kappa cos(theta/2) sqrt(1 - z^2)); the trapezoid rule over z"""
    s, c = math.sin(theta / 2.0), math.cos(theta / 2.0)
    z = np.linspace(-1.0, 0.0, n)
    f = np.exp(kappa * s * z - kappa) * np.i0(kappa * c * np.sqrt(1.0 - z * z))
    C = kappa / (2.0 * math.pi * (1.0 - math.exp(-2.0 * kappa)))
    h = z[1] - z[0]
    return C * 2.0 * math.pi * h * (f.sum() - 0.5 * (f[0] + f[-1]))


def test_oracle_two_samples_a_known_angle_apart():
    """Two single-sample audiences 15 degrees apart at sigma 10 degrees, on a 180 x 90 map.  Over the sphere the product of two von
    Mises-Fisher densities of one kappa integrates to (kappa / (4 pi sinh kappa))^2 * 4 pi sinh(k') / k', k' = 2 kappa cos(theta / 2),
    and the mean of each is 1 / (4 pi): cc = (I(theta) - 1 / (4 pi)) / (I(0) - 1 / (4 pi)); sim = twice the share of one density
    beyond the bisecting plane.  The midpoint rule on cells of 2 degrees is within h^2 / (24 sigma^2) = 1.7e-3 of a smooth integral;
    allowed: 5e-3."""
    sigma, theta = math.radians(10.0), math.radians(15.0)
    kappa = 1.0 / sigma ** 2
    table = np.array([[math.cos(0.3), math.sin(0.3), 0.0], [math.cos(0.3 + theta), math.sin(0.3 + theta), 0.0]])
    r = sso.Oracle(table, 180, 90).rows(np.array([[0, 1]]), [0, 1], 1, 1, sigma)
    overlap = lambda kp: (kappa / (4.0 * math.pi * math.sinh(kappa))) ** 2 * 4.0 * math.pi * math.sinh(kp) / kp     # noqa: E731
    mean = 1.0 / (4.0 * math.pi)
    cc = (overlap(2.0 * kappa * math.cos(theta / 2.0)) - mean) / (overlap(2.0 * kappa) - mean)
    sim = 2.0 * hemisphere_share(kappa, theta)
    print("cc", r["stats"][0, 0], cc, "sim", r["stats"][1, 0], sim)
    assert 0.3 < cc < 0.7 and 0.3 < sim < 0.6                    # a pair that overlaps in part
    assert abs(r["stats"][0, 0] - cc) < 5e-3 and abs(r["stats"][1, 0] - sim) < 5e-3
    np.testing.assert_allclose(4.0 * math.pi * r["stats"][7:, 0], 1.0, rtol=2e-3)
    # the density of B at A's one sample is C exp(kappa (cos theta - 1)): nss in closed form from the oracle's own mass and variance
    C = kappa / (2.0 * math.pi * (1.0 - math.exp(-2.0 * kappa)))
    var = overlap(2.0 * kappa) * mean - mean ** 2
    nss = (C * math.exp(kappa * (math.cos(theta) - 1.0)) - mean) / math.sqrt(var)
    np.testing.assert_allclose(r["stats"][5:7, 0], nss, rtol=5e-3)


def test_oracle_far_pair_at_a_narrow_kernel():
    """sigma 1 degree, the two samples 90 degrees apart: exp(-kappa) = exp(-3283) is 0.0, so each map is 0.0 where the other has its
    weight: kl = +inf, jsd = 1 bit, sim = 0, and the densities anti-correlate slightly"""
    table = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    r = sso.Oracle(table, 90, 45).rows(np.array([[0, 1]]), [0, 1], 1, 1, math.radians(1.0))
    cc, sim, jsd, kl_ab, kl_ba, nss_ab, nss_ba = r["stats"][:7, 0]
    assert kl_ab == np.inf and kl_ba == np.inf
    assert abs(jsd - 1.0) < 1e-12 and sim < 1e-12 and -0.01 < cc < 0.0
    assert nss_ab < 0 and nss_ba < 0                              # each looks where the other's density is below its average
