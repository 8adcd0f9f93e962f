"""GPU: the drop-in Python surface end to end (CSV directory -> run_analysis -> DataFrame / CSV /
png) and the operator-level functions, against the reference's golden vectors."""
import numpy as np
import pandas as pd
import pytest

import viewport_entropy_toolkit as vt
from viewport_entropy_toolkit.config import AnalyzerConfig, EntropyConfig
from viewport_entropy_toolkit.utilities import (calculate_tile_weights, compute_spatial_entropy,
                                                compute_transition_entropy, find_nearest_tile,
                                                generate_fibonacci_lattice)
from oracle import vet_oracle as vo
from tests._tol import W_RTOL, w_atol

pytestmark = pytest.mark.gpu
RTOL = 1e-8


def _write_config1(golden_dir, d, npz="g4_spatial.npz"):
    g = np.load(golden_dir / npz)
    d.mkdir()
    for u in range(len(g["mu_in"])):
        pd.DataFrame({"time": g["time_in"][u], "2dmu": g["mu_in"][u], "2dmv": g["mv_in"][u], "x": 1}).to_csv(
            d / f"user{u:03d}.csv", index=False)
    return g


@pytest.mark.parametrize("tag,tcs,ekw", [
    ("w_tc50", [50], {}),
    ("w_tc50_100_200", [50, 100, 200], {}),
    ("u_tc20_50", [20, 50], dict(use_weight_distribution=False)),
    ("w_tc50_fov90", [50], dict(fov_angle=90.0)),
])
def test_spatial_run_analysis(tmp_path, golden_dir, tag, tcs, ekw):
    g = _write_config1(golden_dir, tmp_path / "video")
    cfg = AnalyzerConfig(tile_counts=tcs, output_dir=tmp_path / "out", entropy_config=EntropyConfig(**ekw))
    an = vt.SpatialEntropyAnalyzer(cfg)
    an.run_analysis(tmp_path / "video", output_prefix="t")
    res = an._entropy_results
    assert list(res.columns) == ["time", "entropy", "tile_weights", "tile_assignments"]
    assert np.array_equal(res["time"], g[f"{tag}__time"])
    np.testing.assert_allclose(res["entropy"], g[f"{tag}__entropy"], rtol=RTOL)
    cols = [str(c) for c in g[f"{tag}__columns"]]
    tiles = an._fibonacci_vectors[tcs[0]]
    for i in (0, 150, 299):
        assert dict(res["tile_assignments"][i]) == {c: int(a) for c, a in zip(cols, g[f"{tag}__assign"][i])}
    for k, i in enumerate(g[f"{tag}__weights_frames"]):
        ref = {tiles[j]: w for j, w in enumerate(g[f"{tag}__weights"][k]) if w > 0}
        got = dict(res["tile_weights"][int(i)])
        assert set(got) == set(ref)          # exactly the reference's keys, whatever the formulation
        for key, w in ref.items():
            assert got[key] == pytest.approx(w, rel=W_RTOL, abs=w_atol(8, ekw.get("power_factor", 2.0)))     # no fixed-point term
    csvs = list((tmp_path / "out").glob("video_t_*.csv"))
    pngs = list((tmp_path / "out").glob("video_t_*_graph.png"))
    assert len(csvs) == 1 and len(pngs) == 1
    out = pd.read_csv(csvs[0])
    assert list(out.columns) == ["time", "entropy"] and len(out) == 300
    np.testing.assert_allclose(out["entropy"], g[f"{tag}__entropy"], rtol=RTOL)


@pytest.mark.parametrize("tag,tcs", [("tc200", [200]), ("tc20_50", [20, 50])])
def test_transition_analyzer(tmp_path, golden_dir, tag, tcs):
    g = _write_config1(golden_dir, tmp_path / "video", "g5_transition.npz")
    cfg = AnalyzerConfig(tile_counts=tcs, output_dir=tmp_path / "out")
    # (a) golden column order through the engine-native array ingest
    cols = [str(c) for c in g[f"{tag}__columns"]]
    order = [int(c[4:]) for c in cols]
    times, mu, mv = vo.format_trajectories([(g["time_in"][u], g["mu_in"][u], g["mv_in"][u]) for u in order])
    an = vt.TransitionEntropyAnalyzer(cfg)
    an.load_arrays(times, mu, mv, cols)
    res = an.compute_entropy()
    assert len(res) == 299 and np.array_equal(res["time"], g[f"{tag}__time"])
    np.testing.assert_allclose(res["entropy"], g[f"{tag}__entropy"], rtol=RTOL, equal_nan=True)
    tiles = an._fibonacci_vectors[tcs[0]]
    for i in (0, 100, 298):
        assert dict(res["tile_assignments"][i]) == {c: tuple(int(x) for x in p) for c, p in zip(cols, g[f"{tag}__pairs"][i])}
        assert dict(res["tile_weights"][i]) == {tiles[j]: int(n) for j, n in enumerate(g[f"{tag}__srccount"][i]) if n}
    # (b) from the CSV directory: column order is this box's glob order, so compare with the
    #     oracle run in that same order (the transition value depends on user order)
    an2 = vt.TransitionEntropyAnalyzer(cfg)
    an2.process_directory(tmp_path / "video")
    res2 = an2.compute_entropy()
    t2, mu2, mv2, names = an2._dense
    ent, _ = vo.transition_series(mu2, mv2, 100, 200, tcs)
    np.testing.assert_allclose(res2["entropy"], ent, rtol=RTOL, equal_nan=True)
    an2.create_visualization("tr")
    assert (tmp_path / "out" / "tr.csv").exists() and (tmp_path / "out" / "tr_graph.png").exists()


def test_hand_assigned_vector_frame(tmp_path, golden_dir):
    """A caller may replace ``_data_cache['vectors']`` with its own object frame (arbitrary
    Vectors): the analyzer must honour it (ids path)."""
    g = _write_config1(golden_dir, tmp_path / "video")
    cfg = AnalyzerConfig(tile_counts=[50], output_dir=tmp_path / "out")
    an = vt.SpatialEntropyAnalyzer(cfg)
    an.process_directory(tmp_path / "video")
    vec = an._data_cache["vectors"].iloc[:40].reset_index(drop=True)
    an._data_cache["vectors"] = vec
    res = an.compute_entropy()
    assert len(res) == 40
    names = [c for c in vec.columns if c != "time"]
    L = vo.fibonacci_lattice(50)
    for i in range(40):
        d = np.array([[vec[c][i].x, vec[c][i].y, vec[c][i].z] for c in names if vec[c][i] is not None])
        e, _, _ = vo.spatial_entropy_frame(d, L)
        assert res["entropy"][i] == pytest.approx(e, rel=RTOL)


def test_error_conventions(tmp_path, golden_dir):
    g = np.load(golden_dir / "g6_ingest.npz")
    d = tmp_path / "edge"
    d.mkdir()
    for c in ("ua", "ub", "uc"):
        a = g[f"in_{c}"]
        pd.DataFrame({"time": a[:, 0], "2dmu": a[:, 1], "2dmv": a[:, 2]}).to_csv(d / f"{c}.csv", index=False)
    cfg = AnalyzerConfig(tile_counts=[50], output_dir=tmp_path / "out")
    tr = vt.TransitionEntropyAnalyzer(cfg)
    tr.process_directory(d)
    with pytest.raises(ZeroDivisionError, match="^division by zero$"):      # reference: rows without a common user
        tr.compute_entropy()
    sp = vt.SpatialEntropyAnalyzer(cfg)
    sp.process_directory(d)
    assert len(sp.compute_entropy()) == len(g["w__time"])
    sp.load_arrays(np.arange(2) * 0.1, np.array([[0.5, np.nan], [np.nan, np.nan]]), np.full((2, 2), 0.5))
    with pytest.raises(vt.ValidationError):           # a frame without any user
        sp.compute_entropy()


def test_operator_level_functions(golden_dir):
    g = np.load(golden_dir / "g9_operator_edges.npz")
    L = generate_fibonacci_lattice(50)
    v, v2 = vt.Vector(*g["v"]), vt.Vector(*g["v2"])
    e, w, a = compute_spatial_entropy({"a": v}, L, EntropyConfig(use_weight_distribution=False))
    assert np.isnan(e) and np.isnan(g["single_unweighted"]) and a == {"a": find_nearest_tile(v, L)}
    e, w, a = compute_spatial_entropy({"a": v}, L, EntropyConfig())
    assert e == pytest.approx(float(g["single_weighted"]), rel=RTOL)
    e, w, a = compute_spatial_entropy({"a": v, "b": v2}, L, EntropyConfig(fov_angle=1.0))
    assert e == 0.0 and w == {} and [a["a"], a["b"]] == g["tiny_fov_assign"].tolist()
    e, _, _ = compute_spatial_entropy({"a": v, "b": v2}, generate_fibonacci_lattice(1), EntropyConfig())
    assert np.isnan(e)
    e, w, a = compute_transition_entropy({"a": v}, {"a": v2}, L, EntropyConfig(), 120)
    assert np.isnan(e) and a == {"a": (find_nearest_tile(v, L), find_nearest_tile(v2, L))}
    e, w, a = compute_transition_entropy({"a": v, "b": v2}, {"a": v2, "b": v}, L, EntropyConfig(), 120)
    assert e == pytest.approx(float(g["trans_two"]), rel=RTOL)
    assert sum(w.values()) == 2
    with pytest.raises(vt.ValidationError):
        compute_spatial_entropy({}, L, EntropyConfig())
    with pytest.raises(vt.ValidationError):
        compute_transition_entropy({}, {"a": v}, L, EntropyConfig(), 120)
    with pytest.raises(ZeroDivisionError):
        compute_transition_entropy({"a": v}, {"b": v}, L, EntropyConfig(), 120)


def test_calculate_tile_weights_rows(golden_dir):
    g = np.load(golden_dir / "g7_weight_rows.npz")
    grid = vo.direction_grid(100, 200)
    L = generate_fibonacci_lattice(500)
    for i in (0, 1, 5, 17):
        v = vt.Vector(*grid[g["py"][i], g["px"][i]])
        ref = g["tc500__rows"][i]
        got = calculate_tile_weights(v, L, EntropyConfig())
        assert find_nearest_tile(v, L) == int(g["tc500__nearest"][i])
        assert {L.index(t) for t in got} == set(np.nonzero(ref > 0)[0])
        for t, w in got.items():
            assert w == pytest.approx(ref[L.index(t)], rel=1e-9, abs=1e-15)
        keys = list(got)
        assert all(got[keys[k]] >= got[keys[k + 1]] for k in range(len(keys) - 1))   # ascending distance
    assert calculate_tile_weights(v, L, EntropyConfig(use_weight_distribution=False)) == \
        {L[find_nearest_tile(v, L)]: 1.0}


# ---------------------------------------------------------------- naive lat/lon analyzer (§8f rank 3)
@pytest.mark.parametrize("th,tw", [(10, 10), (30, 45), (20, 20), (90, 180)])
@pytest.mark.parametrize("flag", [True, False])
def test_naive_analyzer_vs_reference(tmp_path, golden_dir, th, tw, flag):
    from viewport_entropy_toolkit import NaiveSpatialEntropyAnalyzer
    from viewport_entropy_toolkit.config import NaiveAnalyzerConfig
    from viewport_entropy_toolkit.utilities import compute_naive_spatial_entropy, find_naive_tile_index
    g = _write_config1(golden_dir, tmp_path / "video", "g10_naive.npz")
    tag = f"h{th}_w{tw}_{'w' if flag else 'u'}"
    cfg = NaiveAnalyzerConfig(output_dir=tmp_path / "out", tile_height=th, tile_width=tw,
                              entropy_config=EntropyConfig(use_weight_distribution=flag))
    an = NaiveSpatialEntropyAnalyzer(cfg)
    an.run_analysis(tmp_path / "video", "n")
    res = an._entropy_results
    assert list(res.columns) == ["time", "entropy", "tile_weights", "tile_assignments"]
    assert np.array_equal(res["time"], g[f"{tag}__time"]) and all(w is None for w in res["tile_weights"])
    np.testing.assert_allclose(res["entropy"], g[f"{tag}__entropy"], rtol=1e-9)
    assert len(list((tmp_path / "out").glob("video_n_*.csv"))) == 1
    # operator level on the frames the fixture holds
    pts = an._data_cache["points"]
    cols = [str(c) for c in g[f"{tag}__columns"]]
    for fi in (0, 150, 299):
        row = pts.iloc[fi]
        pd_ = {c: row[c] for c in cols if row[c] is not None}
        e, w, a = compute_naive_spatial_entropy(pd_, th, tw, cfg.entropy_config)
        assert e == pytest.approx(float(g[f"{tag}__f{fi}_entropy"]), rel=1e-9)
        assert [a[c] for c in cols] == [str(x) for x in g[f"{tag}__f{fi}_assign"]]
        assert w == dict(zip([str(k) for k in g[f"{tag}__f{fi}_wkeys"]], g[f"{tag}__f{fi}_wvals"].tolist()))
        assert find_naive_tile_index(row[cols[0]], th, tw) == a[cols[0]]
    with pytest.raises(vt.ValidationError):
        compute_naive_spatial_entropy({"a": vt.RadialPoint(0.0, 0.0)}, 7, 10, cfg.entropy_config)
    with pytest.raises(vt.ValidationError):
        compute_naive_spatial_entropy({}, 10, 10, cfg.entropy_config)


def test_naive_config3_size_vs_oracle(tmp_path):
    """Large video through the naive analyzer's engine path (persistent LDS-LUT stream kernel)."""
    from viewport_entropy_toolkit import NaiveSpatialEntropyAnalyzer
    from viewport_entropy_toolkit.config import NaiveAnalyzerConfig
    rng = np.random.default_rng(3)
    U, T = 512, 2000
    mu = np.mod(0.5 + np.cumsum(rng.normal(0, 0.01, (T, U)), axis=0), 1.0)
    mv = np.clip(0.5 + np.cumsum(rng.normal(0, 0.005, (T, U)), axis=0), 0.0, 1.0)
    mu[rng.random((T, U)) < 0.05] = np.nan
    mu[:, 0] = 0.5
    for flag in (True, False):
        an = NaiveSpatialEntropyAnalyzer(NaiveAnalyzerConfig(output_dir=tmp_path, tile_height=10, tile_width=20,
                                                             entropy_config=EntropyConfig(use_weight_distribution=flag)))
        an.load_arrays(np.arange(T) * 0.1, mu, mv)
        ent = an.compute_entropy()["entropy"].to_numpy()
        ref, _, _ = vo.naive_series(mu, mv, 100, 200, 10, 20, flag)
        np.testing.assert_allclose(ent, ref, rtol=1e-9)


def test_analyze_directories_single_process(tmp_path, golden_dir):
    """The multi-GPU driver degenerates to a plain loop without a process group."""
    from viewport_entropy_toolkit import _dist
    g = _write_config1(golden_dir, tmp_path / "v0")
    _write_config1(golden_dir, tmp_path / "v1")
    cfg = AnalyzerConfig(tile_counts=[50], output_dir=tmp_path / "out")
    got = _dist.analyze_directories([tmp_path / "v0", tmp_path / "v1"], cfg)
    assert sorted(got) == [0, 1]
    for v in got.values():
        np.testing.assert_allclose(v, g["w_tc50__entropy"], rtol=RTOL)


def test_result_columns_are_fetched_from_the_device_on_access(tmp_path):
    """compute_entropy brings back the entropy series only; tile_weights / tile_assignments cells are built from
    device-resident rows when read, and equal the eager outputs of the engine (reference consumer:
    analyzers/spatial_entropy.py:152-163)."""
    from viewport_entropy_toolkit import AnalyzerConfig, SpatialEntropyAnalyzer, TransitionEntropyAnalyzer, _native, _synthetic
    from viewport_entropy_toolkit._results import FrameDictArray
    mu, mv = _synthetic.random_walk_video(40, 700, base_seed=31, p_absent=0.1)
    mu[:, 0] = np.where(np.isnan(mu[:, 0]), 0.5, mu[:, 0])
    mv[:, 0] = np.where(np.isnan(mv[:, 0]), 0.5, mv[:, 0])
    times = np.arange(700) * 0.1
    an = SpatialEntropyAnalyzer(AnalyzerConfig(tile_counts=[50, 100], output_dir=tmp_path))
    an.load_arrays(times, mu, mv)
    df = an.compute_entropy()
    assert isinstance(df["tile_weights"].array, FrameDictArray) and len(df) == 700
    eager = an._get_plan().spatial(mu=mu, mv=mv, want_assign=True, want_weights=True)
    assert np.array_equal(df["entropy"].to_numpy(), eager["entropy"])
    names = an._dense[3]
    tiles = an._fibonacci_vectors[50]
    for i in (0, 1, 255, 256, 257, 699, 300):
        assert dict(df["tile_assignments"][i]) == {names[u]: int(t) for u, t in enumerate(eager["assign"][i]) if t >= 0}
        assert dict(df.iloc[i]["tile_weights"]) == {tiles[t]: float(w) for t, w in enumerate(eager["weights"][i]) if w > 0}
    assert sum(len(r["tile_assignments"]) for _, r in df.iloc[500:520].iterrows()) == int((eager["assign"][500:520] >= 0).sum())
    # ... and they are the reference's values (entropy_utils.py:131-136, 190-192), not the table's fixed-point sums: the
    # plan ran the integer table for the entropy (28 000 samples, policy 0 -> sweep here; forced below), the weight rows
    # of a fetched block come from the weights-only pass of the precise sweep
    frames = [0, 255, 256, 699]
    _, _, wref = vo.spatial_series(mu[frames], mv[frames], 100, 200, [50, 100], want_weights=True)
    for k, i in enumerate(frames):
        got = dict(df["tile_weights"][i])
        assert set(got) == {tiles[t] for t in np.nonzero(wref[k] > 0)[0]}
        for t in np.nonzero(wref[k] > 0)[0]:
            assert got[tiles[t]] == pytest.approx(wref[k][t], rel=W_RTOL, abs=w_atol(40))
    plan = an._get_plan()
    plan.set_table_policy(1)
    df1 = an.compute_entropy()
    assert plan.last_formulation(0) == "table"
    for i in (0, 300, 699):
        assert dict(df1["tile_weights"][i]) == dict(df["tile_weights"][i])          # same values whatever the formulation
    plan.set_table_policy(0)
    tr = TransitionEntropyAnalyzer(AnalyzerConfig(tile_counts=[50], output_dir=tmp_path))
    tr.load_arrays(times, mu, mv)
    dt = tr.compute_entropy()
    eager = tr._get_plan().transition(mu=mu, mv=mv, want_pairs=True, want_srccount=True)
    assert np.array_equal(dt["entropy"].to_numpy(), eager["entropy"]) and len(dt) == 699
    for i in (0, 300, 698):
        assert dict(dt["tile_assignments"][i]) == {names[u]: (int(p), int(c)) for u, (p, c) in enumerate(eager["pairs"][i]) if p >= 0}
        assert dict(dt["tile_weights"][i]) == {tiles[t]: int(k) for t, k in enumerate(eager["srccount"][i]) if k}
    # the CSV the reference writes (time, entropy) needs no cell at all
    df[["time", "entropy"]].to_csv(tmp_path / "x.csv", index=False)
