"""Saliency maps (the spherical kernel density of attention per window and per viewer), CPU side: the C-ABI surface, the argument
handling of the analyzers and of Plan, the DataFrame, the map's orientation — against ``pixel_to_spherical`` and against golden G27
(the REAL reference's ``Vector.from_spherical`` of the cell centres and its ``vector_angle_distance``, tools/gen_golden_saliency.py)
— and the claims the GPU tests rest on, recomputed here with the numpy oracle of tests/_saliency_oracle.py.  No GPU."""
import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest

from tests import _saliency_oracle as so

W, H = 100, 200
T, U = 60, 8
SYMBOLS = ("vet_saliency", "vet_saliency_ids", "vet_saliency_host", "vet_test_saliency_tile")
COLUMNS = ["time", "time_end", "samples", "distinct", "mass", "peak", "peak_lon", "peak_lat", "entropy", "area", "map"]
# the GPU tests' maps and settings (tests/test_saliency_gpu.py: SETTINGS): (map width, map height, sigma in degrees, window)
SETTINGS = [(36, 18, 5.0, 5), (36, 18, 2.0, 1), (18, 9, 10.0, 60), (37, 19, 1.0, 5)]


@pytest.fixture(scope="module")
def g15(golden_dir):
    return np.load(golden_dir / "g15_windowed_transition.npz")


@pytest.fixture(scope="module")
def g27(golden_dir):
    return np.load(golden_dir / "g27_saliency.npz")


@pytest.fixture(scope="module")
def table():
    return so.grid_table(W, H)


def test_library_exports_the_saliency_entry_points():
    from viewport_entropy_toolkit import _native
    lib = ctypes.CDLL(str(_native.LIB_PATH))
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _native.SIGNATURES
    # the leading arguments of the other row calls (samples, U, T, window, stride), then per_user, sigma, W, H, scale, the four outputs
    i, p, d = ctypes.c_int, ctypes.c_void_p, ctypes.c_double
    for tail, at in (("", 7), ("_ids", 6), ("_host", 8)):
        res, args = _native.SIGNATURES["vet_head_motion" + tail]
        mine = _native.SIGNATURES["vet_saliency" + tail]
        assert mine[0] == res and mine[1][:at] == args[:at], tail
        assert mine[1][at:at + 5] == [i, d, i, i, i], tail
        assert mine[1][at + 5:] == [p] * (4 if tail == "_host" else 6), tail     # four outputs (+ status, stream)
    assert _native.SIGNATURES["vet_test_saliency_tile"] == _native.SIGNATURES["vet_test_motion_lds_values"]
    for name in ("saliency", "saliency_device"):
        assert hasattr(_native.Plan, name)
    assert hasattr(_native.Engine, "test_saliency_tile")
    # described in a table of its own; the other tables are as they were
    assert len(_native._ROW_CALLS) == 11 and "saliency" not in _native._ROW_CALLS
    assert sorted(_native._MOTION_CALLS) == [False, True] and sorted(_native._DISPERSION_CALLS) == [False, True]
    assert sorted(_native._SALIENCY_CALLS) == [False, True]
    for per_user, lead in ((False, ""), (True, "U")):
        stem, pairs, whole, empty_ok, outputs = _native._SALIENCY_CALLS[per_user]
        assert (stem, pairs, whole, empty_ok) == ("vet_saliency", False, True, False)
        assert [(key, dims, np.dtype(dt).name, optional) for key, dims, dt, optional in outputs] == \
            [("map", lead + "RYX", "float64", True), ("stats", "4" + lead + "R", "float64", False),
             ("peak", lead + "R", "int32", False), ("counts", "2" + lead + "R", "int64", False)]
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
    for phrase in ("vet_saliency", "MAP GRID", "ASCENDING id", "exp(kappa * (c - 1))", "NO TRUNCATION", "blocks of 1024", "peak_index",
                   "exp2(entropy)", "kappa / (2 pi (1 - exp(-2 kappa)))", "No FP atomics", "VGPRs", "vet_test_saliency_tile"):
        assert phrase in header, phrase


def frame_of(res, times, names, window, stride, per_user, sigma_deg, mw, mh, normalize="density"):
    """an oracle result (shaped as Plan.saliency returns it) through the analyzers' DataFrame glue"""
    from viewport_entropy_toolkit.analyzers._base import _EntropyAnalyzerBase as Base
    return Base._saliency_frame(times, names, window, stride, per_user, dict(res, code=0), sigma_deg, mw, mh, normalize)


def test_oracle_row_shapes_match_the_binding_descriptors(table):
    """the oracle returns what Plan.saliency allocates: the shapes and dtypes of _SALIENCY_CALLS"""
    from viewport_entropy_toolkit import _native
    rows = _native.load_library().vet_window_rows
    for frames in (1, 40, 60):
        for w in (1, 20, frames):
            if w <= frames:
                for s in (1, 7):
                    assert rows(frames, w, s) == so.n_rows(frames, w, s) == len(range(0, frames - w + 1, s))
    ids = np.full((57, 3), 77 * (W + 1) + 31, dtype=np.int32)
    o = so.Oracle(table, 12, 6)
    r = o.rows(ids, 20, 7, math.radians(5.0), 2)
    ru = o.rows(ids, 20, 7, math.radians(5.0), 2, per_user=True)
    dims = {"U": 3, "R": 6, "Y": 6, "X": 12, "2": 2, "4": 4}
    for per_user, got in ((False, r), (True, ru)):
        for key, shape, dtype, optional in _native._SALIENCY_CALLS[per_user][4]:
            assert got[key].shape == tuple(dims[d] for d in shape) and got[key].dtype == np.dtype(dtype), (per_user, key)
    # three viewers on one pixel: one list entry of multiplicity 60 (20 per viewer); the scale divides it out
    assert (r["counts"][0] == 60).all() and (r["counts"][1] == 1).all() and (ru["counts"][0] == 20).all()
    np.testing.assert_allclose(r["map"], ru["map"][0], rtol=1e-15)
    np.testing.assert_allclose(r["stats"], ru["stats"][:, 0], rtol=1e-13, atol=1e-13)


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
        an.compute_saliency()
    mu = np.full((30, 4), 0.5)
    an.load_arrays(np.arange(30) * 0.1, mu, mu)

    def no_engine(*a, **k):
        raise AssertionError("the engine was touched before the arguments were checked")

    an._get_plan = no_engine
    an._grid_plan = no_engine
    for kw in (dict(window=0), dict(window=5, stride=0), dict(window=31), dict(window=2.5), dict(window=True),
               dict(window=5, stride=1.5), dict(window="5"), dict(sigma_deg=0.0), dict(sigma_deg=-1.0), dict(sigma_deg=float("nan")),
               dict(sigma_deg=float("inf")), dict(sigma_deg=180.5), dict(sigma_deg="5"), dict(width=1), dict(width=4097),
               dict(width=36.0), dict(height=0), dict(height=2049), dict(height=True), dict(normalize="max"), dict(normalize=2)):
        with pytest.raises(ValueError):
            an.compute_saliency(**kw)
    # the 4 GiB guard: 30 maps of 4096 x 2048 are 1.9 GiB, 30 x 4 per-viewer maps 7.5 GiB; raised before anything is staged
    with pytest.raises(ValueError, match="larger stride.*coarser map.*keep_maps=False"):
        an.compute_saliency(width=4096, height=2048, per_user=True)
    with pytest.raises(ValueError, match="4 GiB"):
        an.compute_saliency(width=4096, height=2048, window=1, stride=1, per_user=True, keep_maps=True)
    with pytest.raises(AssertionError, match="engine was touched"):           # within the guard: the call goes on to the engine
        an.compute_saliency(width=4096, height=2048)
    with pytest.raises(AssertionError, match="engine was touched"):
        an.compute_saliency(width=4096, height=2048, per_user=True, keep_maps=False)
    doc = cls.compute_saliency.__doc__
    assert "sigma_deg" in doc and "choice for head-direction data" in doc and "per_user" in doc and "area" in doc


def test_plan_wrapper_refuses_bad_arguments_before_the_library_is_called():
    from viewport_entropy_toolkit import _native
    check = _native.Plan._saliency_args
    for kw in (dict(sigma_deg=0.0), dict(sigma_deg=-3.0), dict(sigma_deg=np.nan), dict(sigma_deg=np.inf), dict(sigma_deg=181.0),
               dict(sigma_deg=True), dict(width=1), dict(width=4097), dict(width=2.0), dict(height=0), dict(height=2049),
               dict(scale="sum"), dict(scale=2), dict(scale=None)):
        a = dict(dict(sigma_deg=5.0, width=180, height=90, scale="density"), **kw)
        with pytest.raises(ValueError, match=next(iter(kw))):
            check(**a)
    assert check(5.0, 180, 90, "density") == (math.radians(5.0), 180, 90, 2)
    assert check(180.0, 2, 1, "none") == (math.pi, 2, 1, 0) and check(np.float32(1.0), np.int64(4096), 2048, "mean")[1:] == (4096, 2048, 1)
    assert "choice for head-direction data" in _native.Plan.saliency.__doc__


# ------------------------------------------------------------------------------------------- orientation
@pytest.mark.parametrize("mw,mh", [(36, 18), (37, 19), (90, 45)])
def test_single_sample_peaks_in_its_own_cell(table, mw, mh):
    """one sample at each of a dozen (mu, mv): the oracle's peak cell is the cell that contains the sample's pixel_to_spherical
    lon / lat — the map is neither flipped nor shifted"""
    o = so.Oracle(table, mw, mh)
    pts = [(0.031, 0.07), (0.26, 0.31), (0.52, 0.48), (0.74, 0.52), (0.97, 0.93), (0.13, 0.77), (0.88, 0.12), (0.49, 0.03),
           (0.51, 0.96), (0.333, 0.666), (0.62, 0.24), (0.05, 0.55)]
    for mu, mv in pts:
        ids = so.ids_of(np.array([[mu]]), np.array([[mv]]), W, H)
        px, py = int(mu * W), int(mv * H)
        lon, lat = px / W * 360.0 - 180.0, 90.0 - py / H * 180.0              # pixel_to_spherical
        col, row = int((lon + 180.0) / 360.0 * mw), int((90.0 - lat) / 180.0 * mh)
        if abs((lon + 180.0) / 360.0 * mw - round((lon + 180.0) / 360.0 * mw)) < 1e-9 or abs((90.0 - lat) / 180.0 * mh - round((90.0 - lat) / 180.0 * mh)) < 1e-9:
            continue                                             # on a cell border: two cells are equally near
        got = o.row(ids, math.radians(2.0), 2)
        assert got["samples"] == 1 and got["peak"] == row * mw + col, (mu, mv, got["peak"], row, col)
        assert o.lon[col] - 180.0 / mw <= lon <= o.lon[col] + 180.0 / mw and o.lat[row] - 90.0 / mh <= lat <= o.lat[row] + 90.0 / mh


def test_oracle_reproduces_the_reference(g27, golden_dir):
    """Golden G27: the oracle's unrounded cell directions are the reference's Vector.from_spherical up to its 6-decimal rounding, and
    the oracle's fused dot c of the reference's own Vectors is cos(vector_angle_distance) to 1e-9"""
    assert sorted(g27.files) == ["angles", "cells", "lonlat", "pix_id", "pixels"]
    assert g27["angles"].shape == (72, 40) and g27["cells"].shape == (72, 3) and g27["pixels"].shape == (40, 3)
    P, lon, lat = so.cell_centres(12, 6)
    assert np.array_equal(g27["lonlat"], np.stack([np.tile(lon, 6), np.repeat(lat, 12)], axis=1))
    assert np.abs(P - g27["cells"]).max() <= 5.0000001e-7 + 1e-6     # rounding to 6 decimals, then the oracle's normalisation
    assert np.abs(P - so.unit_rows(g27["cells"])).max() <= 2e-6
    grid = np.load(golden_dir / "g2_quantiser.npz")["vec_100x200"].reshape(-1, 3)
    assert np.array_equal(grid[g27["pix_id"]], g27["pixels"])
    c = so.cosines(so.unit_rows(g27["cells"]), so.unit_rows(g27["pixels"]))
    print("max |c - cos(angle)|", float(np.abs(c - np.cos(g27["angles"])).max()))
    np.testing.assert_allclose(c, np.cos(g27["angles"]), rtol=0, atol=1e-9)
    # and with the oracle's own, unrounded cell directions: the rounding of the reference's cell Vector is all that differs
    np.testing.assert_allclose(so.cosines(P, so.unit_rows(g27["pixels"])), np.cos(g27["angles"]), rtol=0, atol=3e-6)
    a = so.cell_area(12, 6)
    assert abs(12 * a.sum() - 1.0) < 1e-15 and (a > 0).all() and np.allclose(a, a[::-1], rtol=1e-12)


# ------------------------------------------------------------------------------------------- the claims the GPU tests rest on
@pytest.mark.parametrize("mw,mh,sigma,window", SETTINGS)
def test_cpu_claims_of_the_gpu_tests(g15, table, mw, mh, sigma, window):
    """On the GPU tests' inputs: the peak margin condition (at least 90 % of the rows with samples), and how far a sequential FP64
    sum and an extended-precision sum of the map, and the entropies computed from them, lie apart"""
    ids = so.ids_of(*so.off_centre(g15["mu"], g15["mv"]), W, H)
    o = so.Oracle(table, mw, mh)
    worst_sum = worst_ent = 0.0
    for per_user in (False, True):
        r = o.rows(ids, window, 5, math.radians(sigma), 2, per_user=per_user)
        ok = r["counts"][0] > 0
        margin = so.peak_margin(r["map"])
        share = float((margin[ok] > 1e-9).mean())
        print(f"{mw}x{mh} sigma={sigma} window={window} per_user={per_user}: margin condition on {share:.0%} of {int(ok.sum())} rows, "
              f"smallest margin {float(np.nanmin(margin[ok])):.3e}")
        assert share >= 0.9
        assert r["stats"][2][ok].max() <= 1e-12                   # <= 0: never flatter than uniform
        a = o.a_pix
        for M in r["map"].reshape(-1, mw * mh)[ok.reshape(-1)]:
            w = M * a
            seq = 0.0
            for v in w.tolist():
                seq += v
            ext = float(np.sum(w.astype(np.longdouble)))
            worst_sum = max(worst_sum, abs(seq - ext) / ext)

            def entropy(total):
                with np.errstate(divide="ignore", invalid="ignore"):
                    q = w / total
                    return -float(np.sum(np.where(w == 0, 0.0, q * np.log2(q / a))))
            worst_ent = max(worst_ent, abs(entropy(seq) - entropy(ext)))
    print("sequential against extended sum", worst_sum, "entropy", worst_ent)
    assert worst_sum <= 1e-13 and worst_ent <= 1e-12              # measured: 2.4e-15 and 6.3e-15; the GPU tests allow 1e-12 and 1e-10


def test_oracle_on_known_values():
    """two directions on the equator 90 degrees apart, one of them twice"""
    table = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 2.0]])
    o = so.Oracle(table, 8, 4)
    ids = np.array([[0, 1, 1, -1]])
    sigma = math.radians(20.0)
    r = o.rows(ids, 1, 1, sigma, 0)
    assert r["counts"].T.tolist() == [[3, 2]]
    kappa = 1.0 / sigma ** 2
    want = np.exp(kappa * (o.P @ table[0] - 1.0)) + 2.0 * np.exp(kappa * (o.P @ table[1] - 1.0))
    np.testing.assert_allclose(r["map"][0].reshape(-1), want, rtol=1e-12)
    d = o.rows(ids, 1, 1, sigma, 2)
    C = kappa / (2.0 * math.pi * (1.0 - math.exp(-2.0 * kappa)))
    assert d["map"].tobytes() == (r["map"] * (C / 3.0)).tobytes()
    # lon 90 (the +y direction) holds the double sample: columns 5 / 6 straddle lon 90 on an 8-column map, rows 1 / 2 the equator
    assert d["peak"][0] % 8 in (5, 6) and d["peak"][0] // 8 in (1, 2)
    assert -6.0 < d["stats"][2, 0] < 0.0 and d["stats"][3, 0] == 2.0 ** d["stats"][2, 0]
    e = o.rows(np.array([[-1, -1]]), 1, 1, sigma, 2)
    assert e["peak"].tolist() == [-1] and np.isnan(e["stats"]).all() and (e["map"] == 0.0).all() and e["counts"].T.tolist() == [[0, 0]]
    # the density integrates to 1 once the grid resolves sigma: mass is the mean over the sphere, the integral 4 pi times that
    fine = so.Oracle(table, 90, 45).rows(ids, 1, 1, sigma, 2)
    assert abs(4.0 * math.pi * fine["stats"][0, 0] - 1.0) < 1e-3
    # sigma = 180 degrees is nearly uniform: the effective area is nearly the sphere
    flat = so.Oracle(table, 36, 18).rows(ids, 1, 1, math.pi, 2)
    assert 0.9 < flat["stats"][3, 0] <= 1.0


# ------------------------------------------------------------------------------------------- the DataFrame
def test_dataframe_assembles_from_a_canned_result():
    times = np.arange(10) * 0.5
    maps = np.arange(2 * 3 * 4, dtype=np.float64).reshape(2, 3, 4)
    res = dict(map=maps, stats=np.array([[1.0, np.nan], [9.0, np.nan], [-2.0, np.nan], [0.25, np.nan]]),
               peak=np.array([6, -1], dtype=np.int32), counts=np.array([[8, 0], [5, 0]], dtype=np.int64))
    df = frame_of(res, times, ["a", "b"], 4, 3, False, 5.0, 4, 3)
    assert list(df.columns) == COLUMNS
    assert df["time"].tolist() == [0.0, 1.5] and df["time_end"].tolist() == [1.5, 3.0]      # the first / last frame of the row
    assert df["samples"].tolist() == [8, 0] and df["distinct"].tolist() == [5, 0]
    assert df["mass"][0] == 1.0 and df["peak"][0] == 9.0 and df["entropy"][0] == -2.0 and df["area"][0] == 0.25
    assert df["peak_lon"][0] == (2 + 0.5) / 4 * 360.0 - 180.0 and df["peak_lat"][0] == 90.0 - (1 + 0.5) / 3 * 180.0      # pixel 6 = (1, 2)
    assert np.isnan(df["peak_lon"][1]) and np.isnan(df["peak_lat"][1]) and np.isnan(df["mass"][1])
    assert df["map"][1].shape == (3, 4) and np.shares_memory(df["map"][1], maps) and df["map"][1][0, 0] == 12.0
    assert df.attrs == dict(sigma_deg=5.0, kappa=1.0 / math.radians(5.0) ** 2, width=4, height=3, normalize="density", window=4,
                            stride=3, users=["a", "b"])
    # per viewer: user-major, `user` first; without the maps
    res_u = dict(map=None, stats=np.zeros((4, 2, 3)), peak=np.arange(6, dtype=np.int32).reshape(2, 3),
                 counts=np.arange(12, dtype=np.int64).reshape(2, 2, 3))
    du = frame_of(res_u, times, ["a", "b"], 2, 3, True, 2.0, 4, 3, "mean")
    assert list(du.columns) == ["user"] + COLUMNS[:-1] and len(du) == 6
    assert du["user"].tolist() == ["a"] * 3 + ["b"] * 3 and du["samples"].tolist() == list(range(6))
    assert du["time"].tolist() == [0.0, 1.5, 3.0] * 2 and du["time_end"].tolist() == [0.5, 2.0, 3.5] * 2
    assert du.attrs["normalize"] == "mean" and du["distinct"].tolist() == list(range(6, 12))
