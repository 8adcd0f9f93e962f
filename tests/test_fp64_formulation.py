"""GPU: the `dtable` formulation (vet_plan_set_fp64, include/vet.h): weighted spatial entropy in FP64 from start to end —
the exact FP64 weight rows of every lattice gathered into FP64 histograms in the weights pass's order, the reference's
-sum q log2 q over the keys.  Against the golden vectors (G4, the NaN frames of G12), the oracle and `precise`; lattice 0's
sums are the weights pass's bits; deterministic; the default formulations are untouched."""
import numpy as np
import pandas as pd
import pytest

from oracle import vet_oracle as vo
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


def make_plan(native, engine, tcs, fov=120.0, power=2.0, policy=0, fp64=True, dir_table=None):
    plan = native.Plan(engine, [vo.fibonacci_lattice(tc) for tc in tcs], fov, power, True, W, H, dir_table=dir_table)
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
