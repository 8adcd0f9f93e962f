"""GPU: the `dtable` formulation (vet_plan_set_fp64, include/vet.h): weighted spatial entropy in FP64 from start to end —
the exact FP64 weight rows of every lattice gathered into FP64 histograms in the weights pass's order, the reference's
-sum q log2 q over the keys.  Against the golden vectors (G4, the NaN frames of G12), the oracle and `precise`; lattice 0's
sums are the weights pass's bits; deterministic; the default formulations are untouched."""
import numpy as np
import pandas as pd
import pytest
from hypothesis import HealthCheck, given, settings, strategies as st

from oracle import vet_oracle as vo
from tests._fp64 import fp64_form
from tests._tol import W_RTOL, w_atol

pytestmark = pytest.mark.gpu

RTOL = 1e-9
W, H = 100, 200
REFERENCE_TILE_COUNTS = [20, 50, 100, 250, 1000]


@pytest.fixture(scope="module")
def native():
    from viewport_entropy_toolkit import _native
    return _native


@pytest.fixture(scope="module")
def engine(native):
    return native.Engine.default()


def make_plan(native, engine, tcs, fov=120.0, power=2.0, policy=0, fp64=True, dir_table=None, grid=(W, H)):
    plan = native.Plan(engine, [vo.fibonacci_lattice(tc) for tc in tcs], fov, power, True, *grid, dir_table=dir_table)
    plan.set_table_policy(policy)
    if fp64:
        plan.set_fp64(True)
    return plan


def _g4_dense(g, tag):
    cols = [str(c) for c in g[f"{tag}__columns"]]
    order = [int(c[4:]) for c in cols]
    tracks = [(g["time_in"][u], g["mu_in"][u], g["mv_in"][u]) for u in order]
    return vo.format_trajectories(tracks)


def video(U, T, seed, p_absent=0.1):
    from viewport_entropy_toolkit import _synthetic
    return _synthetic.random_walk_video(U, T, base_seed=seed, p_absent=p_absent)


def grid_ids(mu, mv):
    present = ~(np.isnan(mu) | np.isnan(mv))
    px = vo.normalize_to_pixel(np.where(present, mu, 0.0), W)
    py = vo.normalize_to_pixel(np.where(present, mv, 0.0), H)
    return np.where(present, py * (W + 1) + px, -1).astype(np.int32)


def keys_of(weights):
    return (weights != 0) | np.signbit(weights)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# --------------------------------------------------------------------------- 1. goldens
@pytest.mark.parametrize("tag,tcs,kw", [
    ("w_tc50", [50], {}),
    ("w_tc50_100_200", [50, 100, 200], {}),
    ("w_tc50_p15", [50], dict(power=1.5)),
    ("w_tc50_fov90", [50], dict(fov=90.0)),
    ("w_tc100_fov200_p05", [100], dict(fov=200.0, power=0.5)),
])
def test_dtable_vs_reference_goldens(native, engine, golden_dir, tag, tcs, kw):
    g = np.load(golden_dir / "g4_spatial.npz")
    _, mu, mv = _g4_dense(g, tag)
    plan = make_plan(native, engine, tcs, policy=1, **kw)
    res = plan.spatial(mu=mu, mv=mv, want_assign=True, want_weights=True)
    assert [plan.last_formulation(k) for k in range(len(tcs))] == ["dtable"] * len(tcs)
    assert np.array_equal(res["assign"], g[f"{tag}__assign"])
    np.testing.assert_allclose(res["entropy"], g[f"{tag}__entropy"], rtol=RTOL, equal_nan=True)
    fr = g[f"{tag}__weights_frames"]
    np.testing.assert_allclose(res["weights"][fr], g[f"{tag}__weights"], rtol=W_RTOL, atol=w_atol(mu.shape[1], kw.get("power", 2.0)))
    assert np.array_equal(res["present"], np.full(len(mu), mu.shape[1]))
    plan.close()


# --------------------------------------------------------------------------- 2. the reference's NaN frames
G12_CONFIGS = [(tc, fov, power) for tc in (50, 500) for fov in (120, 60) for power in (50, 80, 100, 150, 200)]


def g12_samples(px, py):
    present = px >= 0
    mu = np.where(present, np.where(px == W, 1.0, (px + 0.5) / W), np.nan)
    mv = np.where(present, np.where(py == H, 1.0, (py + 0.5) / H), np.nan)
    return mu, mv


@pytest.mark.parametrize("tc,fov,power", G12_CONFIGS)
def test_dtable_nan_frames_g12(native, engine, golden_dir, tc, fov, power):
    g = np.load(golden_dir / "g12_underflow.npz")
    tag = f"tc{tc}_fov{fov}_p{power}"
    mu, mv = g12_samples(g["px"], g["py"])
    plan = make_plan(native, engine, [tc], float(fov), float(power), policy=1)
    res = plan.spatial(mu=mu, mv=mv, want_weights=True)
    assert plan.last_formulation(0) == "dtable"              # no hand-over to `precise`
    ref = g[f"{tag}__entropy"]
    assert np.array_equal(np.isnan(res["entropy"]), np.isnan(ref)), np.flatnonzero(np.isnan(res["entropy"]) != np.isnan(ref))
    ok = ~np.isnan(ref)
    np.testing.assert_allclose(res["entropy"][ok], ref[ok], rtol=RTOL, atol=1e-15)
    assert np.array_equal(keys_of(res["weights"]), g[f"{tag}__keys"])
    np.testing.assert_allclose(np.abs(res["weights"]), g[f"{tag}__hist"], rtol=1e-9, atol=0)
    plan.close()


# --------------------------------------------------------------------------- 3. lattice 0 = the weights pass, bit for bit
def test_weights_bit_identical_to_the_weights_pass_and_one_pass(native, engine):
    mu, mv = video(64, 3000, 21)
    tcs = [50, 100, 200]
    default = make_plan(native, engine, tcs, fp64=False)
    ref = default.spatial(mu=mu, mv=mv, want_weights=True)
    plan = make_plan(native, engine, tcs)
    engine.profile_enable(True)
    try:
        engine.profile_reset()
        res = plan.spatial(mu=mu, mv=mv, want_weights=True)
        _, n_weights = engine.profile_get("k_weights")
        _, n_spatial = engine.profile_get("k_spatial")
    finally:
        engine.profile_enable(False)
    assert [plan.last_formulation(k) for k in range(3)] == ["dtable"] * 3
    assert n_weights == 0 and n_spatial >= 1, (n_weights, n_spatial)
    assert np.array_equal(bits(res["weights"]), bits(ref["weights"]))
    assert np.array_equal(res["assign"], ref["assign"]) and np.array_equal(res["present"], ref["present"])
    np.testing.assert_allclose(res["entropy"], ref["entropy"], rtol=1e-6)        # the default path's contract
    # the resident result fetches its weight rows through the weights pass: the same bits again
    r = plan.spatial_resident(mu=mu, mv=mv)
    assert np.array_equal(bits(r["entropy"]), bits(res["entropy"]))
    assert np.array_equal(bits(r["result"].rows(1, 0, 3000)), bits(res["weights"]))
    r["result"].close()
    default.close()
    plan.close()


# --------------------------------------------------------------------------- 4. entropy = the call's own weights
def test_entropy_is_the_entropy_of_its_own_weights(native, engine):
    from viewport_entropy_toolkit import _quantiser
    mu, mv = video(1024, 256, 5, p_absent=0.05)
    plan = make_plan(native, engine, [500])
    res = plan.spatial(mu=mu, mv=mv, want_weights=True)
    assert plan.last_formulation(0) == "dtable"
    w = res["weights"]
    keys = w.view(np.uint64) != 0                          # +0.0 = no key; -0.0 = a key whose value is 0.0
    v = np.where(keys, np.abs(w), 0.0)
    tot = v.sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = v / tot
        h = -np.where(keys, q * np.log2(q), 0.0).sum(axis=1)
    np.testing.assert_allclose(res["entropy"], h / _quantiser.max_entropy(501), rtol=1e-12, equal_nan=True)
    plan.close()


# --------------------------------------------------------------------------- 5. against the oracle and `precise`
@pytest.mark.parametrize("tcs,U,T", [([50, 100, 200], 64, 3000), (REFERENCE_TILE_COUNTS, 256, 240)])
def test_dtable_vs_oracle_and_precise(native, engine, tcs, U, T):
    mu, mv = video(U, T, 77)
    plan = make_plan(native, engine, tcs, policy=1)
    res = plan.spatial(mu=mu, mv=mv, want_weights=True)
    assert [plan.last_formulation(k) for k in range(len(tcs))] == ["dtable"] * len(tcs)
    fr = np.unique(np.linspace(0, T - 1, 24).astype(int))
    ent, assign, weights = vo.spatial_series(mu[fr], mv[fr], W, H, tcs, want_weights=True)
    np.testing.assert_allclose(res["entropy"][fr], ent, rtol=RTOL)
    assert np.array_equal(res["assign"][fr], assign)
    np.testing.assert_allclose(res["weights"][fr], weights, rtol=W_RTOL, atol=w_atol(U))
    plan.set_table_policy(-1)                              # sweep-like under fp64: `precise`
    pre = plan.spatial(mu=mu, mv=mv, want_weights=True)
    assert [plan.last_formulation(k) for k in range(len(tcs))] == ["precise"] * len(tcs)
    rel = np.max(np.abs(res["entropy"] - pre["entropy"]) / np.abs(pre["entropy"]))
    print(f"dtable vs precise, {tcs} {U}x{T}: max relative difference {rel:.3e}")
    np.testing.assert_allclose(res["entropy"], pre["entropy"], rtol=RTOL)
    assert np.array_equal(bits(res["weights"]), bits(pre["weights"]))     # one weights producer for both
    plan.close()


def test_reference_default_tile_counts_one_launch(native, engine):
    """Sum n = 1425 tiles at 4 waves: one launch for all five lattices, no k_finalize."""
    mu, mv = video(256, 64, 8)
    plan = make_plan(native, engine, REFERENCE_TILE_COUNTS, policy=1)
    plan.spatial(mu=mu, mv=mv)                             # builds the rows
    engine.profile_enable(True)
    try:
        engine.profile_reset()
        plan.spatial(mu=mu, mv=mv)
        _, n_spatial = engine.profile_get("k_spatial")
        _, n_final = engine.profile_get("k_finalize")
    finally:
        engine.profile_enable(False)
    assert (n_spatial, n_final) == (1, 0)
    plan.close()


def test_split_launches_when_the_lattices_do_not_fit_one(native, engine):
    """2001 + 1501 tiles at lattice 0's 4 waves need 112 KB of LDS (> 80 KiB): lattice 0 runs alone at its weights-pass NW,
    lattice 1 in a launch of its own into the workspace, k_finalize forms the mean.  Against the oracle and `precise`, and
    lattice 0's sums are still the weights pass's bits."""
    tcs = [2000, 1500]
    mu, mv = video(64, 200, 91)
    plan = make_plan(native, engine, tcs, policy=1)
    plan.spatial(mu=mu, mv=mv)                             # builds the rows
    engine.profile_enable(True)
    try:
        engine.profile_reset()
        res = plan.spatial(mu=mu, mv=mv, want_weights=True)
        _, n_spatial = engine.profile_get("k_spatial")
        _, n_final = engine.profile_get("k_finalize")
        _, n_weights = engine.profile_get("k_weights")
    finally:
        engine.profile_enable(False)
    assert [plan.last_formulation(k) for k in range(2)] == ["dtable"] * 2
    assert (n_spatial, n_final, n_weights) == (2, 1, 0)
    fr = np.unique(np.linspace(0, len(mu) - 1, 12).astype(int))
    ent, assign, weights = vo.spatial_series(mu[fr], mv[fr], W, H, tcs, want_weights=True)
    np.testing.assert_allclose(res["entropy"][fr], ent, rtol=RTOL)
    assert np.array_equal(res["assign"][fr], assign)
    np.testing.assert_allclose(res["weights"][fr], weights, rtol=W_RTOL, atol=w_atol(64))
    plan.set_table_policy(-1)
    pre = plan.spatial(mu=mu, mv=mv, want_weights=True)
    assert [plan.last_formulation(k) for k in range(2)] == ["precise"] * 2
    np.testing.assert_allclose(res["entropy"], pre["entropy"], rtol=RTOL)
    assert np.array_equal(bits(res["weights"]), bits(pre["weights"]))
    # the mean over the split launches = the mean of single-lattice dtable plans, in k_finalize's order
    singles = []
    for tc in tcs:
        one = make_plan(native, engine, [tc], policy=1)
        singles.append(one.spatial(mu=mu, mv=mv)["entropy"])
        assert one.last_formulation(0) == "dtable"
        one.close()
    assert np.array_equal(bits(res["entropy"]), bits((0.0 + singles[0] + singles[1]) / 2.0))
    plan.close()


# --------------------------------------------------------------------------- 6. determinism
def test_dtable_deterministic(native, engine):
    tcs = [50, 100, 200]
    mu, mv = video(96, 400, 13)
    plan = make_plan(native, engine, tcs, policy=1)
    a = plan.spatial(mu=mu, mv=mv, want_weights=True)
    b = plan.spatial(mu=mu, mv=mv, want_weights=True)
    assert np.array_equal(bits(a["entropy"]), bits(b["entropy"])) and np.array_equal(bits(a["weights"]), bits(b["weights"]))
    h = len(mu) // 2
    lo = plan.spatial(mu=mu[:h], mv=mv[:h], want_weights=True)
    hi = plan.spatial(mu=mu[h:], mv=mv[h:], want_weights=True)
    assert plan.last_formulation(0) == "dtable"
    assert np.array_equal(bits(np.concatenate([lo["entropy"], hi["entropy"]])), bits(a["entropy"]))
    assert np.array_equal(bits(np.concatenate([lo["weights"], hi["weights"]])), bits(a["weights"]))
    c = plan.spatial(ids=grid_ids(mu, mv), want_weights=True)
    assert plan.last_formulation(0) == "dtable"
    assert np.array_equal(bits(c["entropy"]), bits(a["entropy"])) and np.array_equal(bits(c["weights"]), bits(a["weights"]))
    assert np.array_equal(c["assign"], a["assign"])
    plan.close()


@pytest.mark.parametrize("policy", [1, 0])
def test_batch_equals_single_video_calls(native, engine, policy):
    tcs = [50, 100, 200]
    vids = [video(64, 300, 40), video(48, 200, 41), video(64, 500, 42)]
    plan = make_plan(native, engine, tcs, policy=policy)
    batch = plan.spatial_batch(vids, want_assign=True)
    for (mu, mv), got in zip(vids, batch):
        one = plan.spatial(mu=mu, mv=mv)
        assert np.array_equal(bits(got["entropy"]), bits(one["entropy"]))
        assert np.array_equal(got["assign"], one["assign"]) and np.array_equal(got["present"], one["present"])
    plan.close()


# --------------------------------------------------------------------------- 7. default mode unchanged
@pytest.mark.parametrize("policy", [1, 0, -1])
def test_toggling_fp64_off_restores_the_default(native, engine, policy):
    tcs = [50, 100, 200]
    mu, mv = video(64, 600, 3)
    fresh = make_plan(native, engine, tcs, policy=policy, fp64=False)
    ref = fresh.spatial(mu=mu, mv=mv, want_weights=True)
    forms = [fresh.last_formulation(k) for k in range(3)]
    toggled = make_plan(native, engine, tcs, policy=policy)
    on = toggled.spatial(mu=mu, mv=mv, want_weights=True)
    if policy > 0:
        assert toggled.last_formulation(0) == "dtable"
    toggled.set_fp64(False)
    off = toggled.spatial(mu=mu, mv=mv, want_weights=True)
    assert [toggled.last_formulation(k) for k in range(3)] == forms
    assert "dtable" not in forms
    assert np.array_equal(bits(off["entropy"]), bits(ref["entropy"]))
    assert np.array_equal(bits(off["weights"]), bits(ref["weights"]))
    assert np.array_equal(bits(on["weights"]), bits(ref["weights"]))
    fresh.close()
    toggled.close()


# --------------------------------------------------------------------------- 8. the analyzer
def _write_csvs(golden_dir, d):
    g = np.load(golden_dir / "g4_spatial.npz")
    d.mkdir()
    for u in range(len(g["mu_in"])):
        pd.DataFrame({"time": g["time_in"][u], "2dmu": g["mu_in"][u], "2dmv": g["mv_in"][u], "x": 1}).to_csv(
            d / f"user{u:03d}.csv", index=False)
    return g


@pytest.mark.parametrize("tag,tcs", [("w_tc50", [50]), ("w_tc50_100_200", [50, 100, 200])])
def test_analyzer_fp64(tmp_path, golden_dir, tag, tcs):
    import viewport_entropy_toolkit as vt
    from viewport_entropy_toolkit.config import AnalyzerConfig
    g = _write_csvs(golden_dir, tmp_path / "video")
    an = vt.SpatialEntropyAnalyzer(AnalyzerConfig(tile_counts=tcs, output_dir=tmp_path / "out64"), fp64=True)
    an.run_analysis(tmp_path / "video", output_prefix="t")
    assert an._plan is not None and an._plan_key[-1] is True
    res = an._entropy_results
    np.testing.assert_allclose(res["entropy"], g[f"{tag}__entropy"], rtol=RTOL)
    base = vt.SpatialEntropyAnalyzer(AnalyzerConfig(tile_counts=tcs, output_dir=tmp_path / "out"))
    base.run_analysis(tmp_path / "video", output_prefix="t")
    ref = base._entropy_results
    assert len(res) == len(ref)
    for i in range(len(res)):
        assert dict(res["tile_weights"][i]) == dict(ref["tile_weights"][i]), i


# --------------------------------------------------------------------------- 9. the edge matrix under fp64
def fp64_oracle(mu, mv, tcs, fov=120.0, power=2.0, grid=(W, H)):
    """The oracle frame by frame (vo.spatial_entropy_frame: the reference's sums in user order, no table over the whole
    pixel grid); a frame without a user: entropy NaN, assign -1, no keys."""
    px, py, present, dirs_grid = vo.sample_directions(mu, mv, *grid)
    flat = dirs_grid.reshape(-1, 3)
    lattices = [vo.fibonacci_lattice(tc) for tc in tcs]
    T = len(mu)
    ent = np.full(T, np.nan)
    assign = np.full(mu.shape, -1, dtype=np.int32)
    weights = np.zeros((T, len(lattices[0])))
    for t in range(T):
        if not present[t].any():
            continue
        dirs = flat[(py[t] * (grid[0] + 1) + px[t])[present[t]]]
        s = 0.0
        for k, L in enumerate(lattices):
            e, hist, near = vo.spatial_entropy_frame(dirs, L, fov, power)
            s += e
            if k == 0:
                weights[t], assign[t][present[t]] = hist, near
        ent[t] = s / len(lattices)
    return ent, assign, weights


def max_rel(got, ref):
    ok = ~np.isnan(ref) & (ref != 0)
    return float(np.max(np.abs(got[ok] - ref[ok]) / np.abs(ref[ok]))) if ok.any() else 0.0


def profiled(engine, fn):
    engine.profile_enable(True)
    try:
        engine.profile_reset()
        out = fn()
        counts = tuple(engine.profile_get(k)[1] for k in ("k_spatial", "k_finalize", "k_weights"))
    finally:
        engine.profile_enable(False)
    return out, counts


# Fibonacci lattices have an odd number of tiles, at most 6783 (the plan's LDS tile cache: 24 bytes a tile), so every one fits
# `dtable` at the weights pass's NW.  What leaves a lattice to `precise` under a table request is the plan-wide cap on the exact
# rows (8 GB): at 640 x 480 pixels and fov 360, 6001 tiles need about 9 GB of rows, 51 tiles 0.1 GB.
BIG = dict(grid=(640, 480), fov=360.0)
MIXED_PLANS = [
    # tcs, plan keywords, per-lattice formulation, (k_spatial, k_finalize, k_weights) launches
    ([5000], {}, ["dtable"], (1, 0, 0)),                       # 5001 tiles: NW = 2
    ([6000], {}, ["dtable"], (1, 0, 0)),                       # 6001 tiles: NW = 1
    ([50, 5000], {}, ["dtable", "dtable"], (2, 1, 0)),         # 4 waves x 5052 tiles do not fit: a launch per lattice
    ([50, 6000], BIG, ["dtable", "precise"], (2, 1, 0)),       # lattice 1 without exact rows: `precise`
    ([6000, 50], BIG, ["precise", "dtable"], (2, 1, 1)),       # lattice 0 `precise`: the weights pass writes the weights
]


@pytest.mark.parametrize("tcs,kw,forms,launches", MIXED_PLANS)
def test_weights_pass_wave_counts_and_mixed_plans(native, engine, tcs, kw, forms, launches):
    """Lattices at the weights pass's 2 and 1 waves, and plans that mix `dtable` with `precise` (the per-lattice launches,
    then k_finalize): against the oracle on sampled frames; the weights are the fp64-off plan's weights-pass bits; the mean
    is k_finalize's (0.0 + e0 + e1) / 2 of single-lattice plans, bit for bit."""
    from viewport_entropy_toolkit import _quantiser
    U, T = 300, 16                                             # not a multiple of 64 * NW
    mu, mv = video(U, T, 31)
    plan = make_plan(native, engine, tcs, policy=1, **kw)
    plan.spatial(mu=mu, mv=mv)                                 # builds the rows
    res, counts = profiled(engine, lambda: plan.spatial(mu=mu, mv=mv, want_weights=True))
    assert [plan.last_formulation(k) for k in range(len(tcs))] == forms
    assert counts == launches, counts
    fr = np.array([0, 3, 7, 11, T - 1])
    ent, assign, weights = fp64_oracle(mu[fr], mv[fr], tcs, kw.get("fov", 120.0), grid=kw.get("grid", (W, H)))
    assert np.array_equal(res["assign"][fr], assign)
    print(f"fp64 {tcs} {kw} {U}x{T} vs oracle: max relative difference {max_rel(res['entropy'][fr], ent):.3e}")
    np.testing.assert_allclose(res["entropy"][fr], ent, rtol=RTOL)
    np.testing.assert_allclose(res["weights"][fr], weights, rtol=W_RTOL, atol=w_atol(U))
    off = make_plan(native, engine, tcs, policy=-1, fp64=False, **kw)
    ref = off.spatial(mu=mu, mv=mv, want_weights=True)
    off.close()
    assert np.array_equal(bits(res["weights"]), bits(ref["weights"]))
    singles = []
    for tc, form in zip(tcs, forms):
        one = make_plan(native, engine, [tc], policy=1, **kw)
        r = one.spatial(mu=mu, mv=mv, want_weights=True)
        assert one.last_formulation(0) == form
        singles.append(r["entropy"])
        if form == "dtable":                                   # entropy = the entropy of the call's own weights
            w = r["weights"]
            keys = w.view(np.uint64) != 0
            v = np.where(keys, np.abs(w), 0.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                q = v / v.sum(axis=1, keepdims=True)
                h = -np.where(keys, q * np.log2(q), 0.0).sum(axis=1)
            np.testing.assert_allclose(r["entropy"], h / _quantiser.max_entropy(tc + 1), rtol=1e-12, equal_nan=True)
        one.close()
    if len(tcs) == 1:
        assert np.array_equal(bits(res["entropy"]), bits(singles[0]))
    else:
        assert np.array_equal(bits(res["entropy"]), bits((0.0 + singles[0] + singles[1]) / 2.0))
    plan.close()


U_BOUNDARIES = [63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513]
fp64_problem = st.fixed_dictionaries(dict(
    U=st.one_of(st.integers(1, 300), st.sampled_from(U_BOUNDARIES)), T=st.integers(1, 12), seed=st.integers(0, 2 ** 31 - 1),
    p_absent=st.sampled_from([0.0, 0.1, 0.5]), empty_frame=st.booleans(),
    tcs=st.lists(st.sampled_from([1, 2, 3, 20, 50, 64, 65, 100, 129, 250, 500, 1000]), min_size=1, max_size=3),
    fov=st.sampled_from([0.5, 30.0, 90.0, 120.0, 150.0, 360.0]), power=st.sampled_from([0.01, 0.5, 1.0, 2.0, 3.0, 100.0]),
    policy=st.sampled_from([1, 0, -1]), ids=st.booleans(), edge=st.booleans()))


@settings(max_examples=80, deadline=None, derandomize=True, suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(fp64_problem)
def test_fp64_matches_oracle(native, engine, pr):
    """fp64 plans on small random problems: user counts around the 64-user steps of every wave count, 1-12 frames, the
    property test's lattices, empty cones (fov 0.5), an underflowing power (100: the reference's NaN frames), exact pixel
    corners, absent users and frames without a user, grid samples or direction ids, every table policy."""
    rng = np.random.default_rng(pr["seed"])
    U, T, tcs = pr["U"], pr["T"], pr["tcs"]
    if pr["edge"]:
        mu = rng.integers(0, W + 1, (T, U)) / W
        mv = rng.integers(0, H + 1, (T, U)) / H
    else:
        mu, mv = rng.random((T, U)), rng.random((T, U))
    gone = rng.random((T, U)) < pr["p_absent"]
    gone[:, 0] = False
    if pr["empty_frame"]:
        gone[rng.integers(0, T)] = True
    mu[gone] = np.nan
    mv[gone] = np.nan
    plan = make_plan(native, engine, tcs, pr["fov"], pr["power"], policy=pr["policy"])
    try:
        call = (lambda a, b: plan.spatial(ids=grid_ids(a, b), want_weights=True, check=False)) if pr["ids"] else \
               (lambda a, b: plan.spatial(mu=a, mv=b, want_weights=True, check=False))
        res = call(mu, mv)
        table_asked = pr["policy"] > 0       # policy 0: fewer samples than VET_TABLE_SAMPLES_PER_DIRECTION per direction
        assert [plan.last_formulation(k) for k in range(len(tcs))] == [fp64_form(tc + 1, table_asked) for tc in tcs]
        empty = gone.all(axis=1)
        assert res["code"] == (native.VET_ERR_EMPTY if empty.any() else native.VET_OK)
        assert np.array_equal(res["present"], (~gone).sum(axis=1))
        ent, assign, weights = fp64_oracle(mu, mv, tcs, pr["fov"], pr["power"])
        assert np.array_equal(res["assign"], assign)
        assert np.array_equal(np.isnan(res["entropy"]), np.isnan(ent))
        ok = ~np.isnan(ent)
        np.testing.assert_allclose(res["entropy"][ok], ent[ok], rtol=RTOL, atol=1e-15)
        np.testing.assert_allclose(res["weights"], weights, rtol=W_RTOL, atol=w_atol(U, pr["power"]))
        assert np.array_equal(bits(res["weights"][empty]), bits(np.zeros_like(weights[empty])))   # no keys
        if T >= 2:                                             # bit-identical under a split of the frame axis
            h = T // 2
            lo, hi = call(mu[:h], mv[:h]), call(mu[h:], mv[h:])
            assert np.array_equal(bits(np.concatenate([lo["entropy"], hi["entropy"]])), bits(res["entropy"]))
            assert np.array_equal(bits(np.concatenate([lo["weights"], hi["weights"]])), bits(res["weights"]))
    finally:
        plan.close()


@pytest.mark.parametrize("policy", [1, -1])
def test_explicit_direction_table_ids(native, engine, policy):
    """The *_ids entry points of an fp64 plan over arbitrary Vectors (no mirror sharing in the alias table), frame by frame
    against the oracle."""
    rng = np.random.default_rng(9)
    table = vo.vector_from_spherical(np.round(rng.uniform(-180, 180, 300), 1), np.round(rng.uniform(-90, 90, 300), 1))
    ids = rng.integers(0, 300, (50, 24)).astype(np.int32)
    ids[rng.random(ids.shape) < 0.1] = -1
    ids[:, 0] = np.abs(ids[:, 0])
    L = vo.fibonacci_lattice(100)
    plan = make_plan(native, engine, [100], policy=policy, dir_table=table)
    res = plan.spatial(ids=ids, want_weights=True)
    assert plan.last_formulation(0) == ("dtable" if policy > 0 else "precise")
    for t in range(len(ids)):
        e, hist, near = vo.spatial_entropy_frame(table[ids[t][ids[t] >= 0]], L)
        np.testing.assert_allclose(res["entropy"][t], e, rtol=RTOL)
        np.testing.assert_allclose(res["weights"][t], hist, rtol=W_RTOL, atol=w_atol(ids.shape[1]))
        assert np.array_equal(res["assign"][t][ids[t] >= 0], near)
    assert np.array_equal(res["present"], (ids >= 0).sum(1))
    plan.close()


@pytest.mark.parametrize("policy", [1, -1])
def test_ids_with_several_lattices(native, engine, policy):
    rng = np.random.default_rng(12)
    table = vo.vector_from_spherical(np.round(rng.uniform(-180, 180, 500), 1), np.round(rng.uniform(-90, 90, 500), 1))
    ids = rng.integers(0, 500, (30, 70)).astype(np.int32)
    ids[rng.random(ids.shape) < 0.2] = -1
    ids[:, 3] = 7
    tcs = [100, 20, 250]
    plan = make_plan(native, engine, tcs, policy=policy, dir_table=table)
    res = plan.spatial(ids=ids, want_weights=True)
    assert [plan.last_formulation(k) for k in range(3)] == ["dtable" if policy > 0 else "precise"] * 3
    ref = np.zeros(len(ids))
    for k, tc in enumerate(tcs):
        L = vo.fibonacci_lattice(tc)
        for t, r in enumerate(ids):
            e, hist, _ = vo.spatial_entropy_frame(table[r[r >= 0]], L)
            ref[t] += e
            if k == 0:
                np.testing.assert_allclose(res["weights"][t], hist, rtol=W_RTOL, atol=w_atol(ids.shape[1]))
    np.testing.assert_allclose(res["entropy"], ref / len(tcs), rtol=RTOL)
    assert np.array_equal(res["present"], (ids >= 0).sum(1))
    plan.close()


USER_SHARE_U = [1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 2049, 4097]


@pytest.mark.parametrize("tc,nw", [(500, 4), (4000, 2), (6000, 1)])
def test_user_share_edges(native, engine, tc, nw):
    """Users cut into NW contiguous shares: fewer users than waves (empty shares), partial 64-user steps, thousands of
    users (many steps per wave).  dtable's weights are the weights pass's bits, against the oracle; a frame without a
    user is NaN with no keys (VET_ERR_EMPTY); out-of-range samples and ids are VET_ERR_RANGE and count as absent."""
    from tests._fp64 import weights_nw
    assert weights_nw(tc + 1) == nw
    plan = make_plan(native, engine, [tc], policy=1)
    off = make_plan(native, engine, [tc], policy=-1, fp64=False)
    worst = 0.0
    for U in USER_SHARE_U:
        mu, mv = video(U, 3, 1000 + U)
        mu, mv = np.concatenate([mu, np.full((1, U), np.nan)]), np.concatenate([mv, np.full((1, U), np.nan)])
        res = plan.spatial(mu=mu, mv=mv, want_weights=True, check=False)
        assert plan.last_formulation(0) == "dtable"
        assert res["code"] == native.VET_ERR_EMPTY
        present = ~np.isnan(mu)
        assert np.array_equal(res["present"], present.sum(1))
        ref = off.spatial(mu=mu, mv=mv, want_weights=True, check=False)
        assert np.array_equal(bits(res["weights"]), bits(ref["weights"])), U
        ent, assign, weights = fp64_oracle(mu, mv, [tc])
        assert np.array_equal(res["assign"], assign)
        assert np.isnan(res["entropy"][3]) and np.array_equal(np.isnan(res["entropy"]), np.isnan(ent))
        worst = max(worst, max_rel(res["entropy"], ent))
        ok = ~np.isnan(ent)
        np.testing.assert_allclose(res["entropy"][ok], ent[ok], rtol=RTOL, err_msg=str(U))
        np.testing.assert_allclose(res["weights"], weights, rtol=W_RTOL, atol=w_atol(U), err_msg=str(U))
        assert np.array_equal(bits(res["weights"][3]), bits(np.zeros(tc + 1)))
        # out of range: flagged, treated as absent
        bad_mu, bad_mv = mu[:1].copy(), mv[:1].copy()
        bad_mu[0, U // 2], bad_mv[0, U // 2] = 1.5, 0.5
        r = plan.spatial(mu=bad_mu, mv=bad_mv, check=False)
        assert r["code"] == native.VET_ERR_RANGE
        assert r["present"][0] == present[0].sum() - (1 if present[0, U // 2] else 0)
        ids = grid_ids(mu[:1], mv[:1])
        ids[0, U - 1] = (W + 1) * (H + 1)
        r = plan.spatial(ids=ids, want_weights=True, check=False)
        assert r["code"] == native.VET_ERR_RANGE
        assert r["present"][0] == present[0].sum() - (1 if present[0, U - 1] else 0)
    print(f"dtable at NW = {nw}, U = {USER_SHARE_U}: max relative difference to the oracle {worst:.3e}")
    off.close()
    plan.close()


@pytest.mark.parametrize("policy", [1, 0])
def test_batch_shapes_equal_single_calls_and_the_oracle(native, engine, policy):
    shapes = [(1, 5), (33, 7), (3000, 4), (64, 100)]
    vids = [video(u, t, 50 + i) for i, (u, t) in enumerate(shapes)]
    tcs = [50, 100]
    plan = make_plan(native, engine, tcs, policy=policy)
    batch = plan.spatial_batch(vids, want_assign=True)
    for (mu, mv), got in zip(vids, batch):
        one = plan.spatial(mu=mu, mv=mv)
        assert np.array_equal(bits(got["entropy"]), bits(one["entropy"]))
        assert np.array_equal(got["assign"], one["assign"]) and np.array_equal(got["present"], one["present"])
        ent, assign, _ = vo.spatial_series(mu, mv, W, H, tcs)
        assert np.array_equal(got["assign"], assign)
        np.testing.assert_allclose(got["entropy"], ent, rtol=RTOL)
    plan.close()


NO_ROWS_CASES = (("k2", [100, 20], 70, 40), ("k1", [500], 130, 12))


def _no_exact_rows_worker(q, env):
    """Child process: fp64 plans with / without the exact weight rows (the knob is read at engine creation)."""
    import os
    os.environ.update(env)
    from viewport_entropy_toolkit import _native
    eng = _native.Engine(0)
    out = {}
    for name, tcs, U, T in NO_ROWS_CASES:
        mu, mv = video(U, T, U + T)
        plan = _native.Plan(eng, [vo.fibonacci_lattice(tc) for tc in tcs], 120.0, 2.0, True, W, H)
        plan.set_table_policy(1)
        plan.set_fp64(True)
        eager = plan.spatial(mu=mu, mv=mv, want_weights=True)
        forms = [plan.last_formulation(k) for k in range(len(tcs))]
        lazy = plan.spatial_resident(mu=mu, mv=mv)
        out[name] = (eager["entropy"], eager["assign"], eager["weights"], lazy["result"].rows(1, 3, T - 5), forms)
        lazy["result"].close()
        plan.close()
    q.put(out)


def test_fp64_plans_without_the_exact_rows():
    """VET_NO_EXACT_ROWS=1 (as if the rows did not fit the device): every lattice of an fp64 plan runs `precise`, the
    weights come from the precise sweep; oracle parity, eager weights == fetched weights."""
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_no_exact_rows_worker, args=(q, {"VET_NO_EXACT_ROWS": "1"}))
    p.start()
    out = q.get(timeout=600)
    p.join(60)
    assert p.exitcode == 0
    for name, tcs, U, T in NO_ROWS_CASES:
        e, a, w, fetched, forms = out[name]
        assert forms == ["precise"] * len(tcs)
        mu, mv = video(U, T, U + T)
        ent, assign, weights = vo.spatial_series(mu, mv, W, H, tcs, want_weights=True)
        assert np.array_equal(a, assign)
        np.testing.assert_allclose(e, ent, rtol=RTOL)
        np.testing.assert_allclose(w, weights, rtol=W_RTOL, atol=w_atol(U))
        assert np.array_equal(bits(fetched), bits(w[3:T - 2]))
