"""GPU: sliding-window (pooled) transition entropy through the C-ABI (Plan.transition_windowed ->
vet_transition_entropy_windowed_host).  Row r pools the transitions of frame pairs [r * stride, r * stride + window); the
references are golden G15 (the real reference on the pooled dicts, tools/gen_golden_windowed_transition.py) and the numpy oracles
of tests/_window_transition_oracle.py (pinned against G15 in tests/test_windowed_transition_surface.py).  Entropy: the
project's contract, 1e-6 relative, NaN = NaN; samples and source counts exact."""
import numpy as np
import pytest

from oracle import vet_oracle as vo
from tests import _window_transition_oracle as wt

pytestmark = pytest.mark.gpu

W, H = 100, 200
RTOL = 1e-6
# k_window_transition's single-pass bucket bound in its 1024-thread shape: 0.6 * 8192 slots - n (vet_transition.hpp)
HASH_SLOTS = 8192


@pytest.fixture(scope="module")
def native():
    from viewport_entropy_toolkit import _native
    return _native


@pytest.fixture(scope="module")
def engine(native):
    return native.Engine.default()


def fib_plan(native, engine, tcs):
    return native.Plan(engine, [vo.fibonacci_lattice(t) for t in tcs], 120.0, 2.0, True, W, H)


def close(got, want, msg="", rtol=RTOL):
    print(msg, "max rel err", float(np.nanmax(np.abs(got - want) / np.maximum(np.abs(want), 1e-300), initial=0.0)))
    assert np.array_equal(np.isnan(got), np.isnan(want)), (msg, np.flatnonzero(np.isnan(got) != np.isnan(want))[:10])
    np.testing.assert_allclose(got, want, rtol=rtol, atol=0, equal_nan=True, err_msg=msg)


def ids_of(mu, mv):
    px, py, present, _ = vo.sample_directions(mu, mv, W, H)
    return np.where(present, py * (W + 1) + px, -1).astype(np.int32)


def pooled_counts(mu, mv, window, stride):
    """samples[R] of every row from the presence pattern alone"""
    present = ~(np.isnan(mu) | np.isnan(mv))
    per_pair = (present[:-1] & present[1:]).sum(axis=1)
    R = wt.n_rows(len(mu), window, stride)
    return np.array([per_pair[r * stride:r * stride + window].sum() for r in range(R)], dtype=np.int32)


def check_rows(res, mu, mv, tcs, tiles, window, stride, msg):
    """samples of EVERY row from the presence pattern; entropy and source counts against the closed-form oracle on the first,
    middle and last row and on the first empty and the first one-sample row"""
    samples = pooled_counts(mu, mv, window, stride)
    assert np.array_equal(res["samples"], samples), msg
    assert np.array_equal(res["srccount"].sum(axis=1), samples), msg
    assert np.array_equal(np.isnan(res["entropy"][samples <= 1]), np.ones((samples <= 1).sum(), dtype=bool)), msg
    R = len(samples)
    rows = {0, R // 2, R - 1}
    for special in (0, 1):
        if (samples == special).any():
            rows.add(int(np.argmax(samples == special)))
    rows = np.array(sorted(rows))
    ent, n, src = wt.fast(mu, mv, W, H, tcs, window, stride, rows=rows, tiles=tiles)
    close(res["entropy"][rows], ent, msg)
    assert np.array_equal(res["srccount"][rows], src) and np.array_equal(n, samples[rows]), msg
    return samples


# ------------------------------------------------------------------------------------------- the reference (golden G15)
def test_vs_reference_golden_grid_and_ids(native, engine, golden_dir):
    g = np.load(golden_dir / "g15_windowed_transition.npz")
    cases = sorted({k.rsplit("__", 1)[0] for k in g.files if "__" in k})
    assert len(cases) == 12
    mu, mv = g["mu"], g["mv"]
    ids = ids_of(mu, mv)
    plans = {}
    for tag in cases:
        tcs = tuple(int(x) for x in tag[2:].split("_w")[0].split("_"))
        window, stride = int(tag.split("_")[-2][1:]), int(tag.split("_")[-1][1:])
        plan = plans.get(tcs) or plans.setdefault(tcs, fib_plan(native, engine, tcs))
        rows = g[f"{tag}__rows"]
        for kw in (dict(mu=mu, mv=mv), dict(ids=ids)):
            res = plan.transition_windowed(window=window, stride=stride, want_srccount=True, **kw)
            assert len(res["entropy"]) == wt.n_rows(60, window, stride)
            close(res["entropy"][rows], g[f"{tag}__entropy"], tag)
            assert np.array_equal(res["samples"][rows], g[f"{tag}__samples"]), tag
            assert np.array_equal(res["srccount"][rows], g[f"{tag}__srccount"]), tag
    for p in plans.values():
        p.close()


# ------------------------------------------------------------------------------------------- the numpy oracle, seeded walks
def walk(U, T, p_absent, seed):
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(U, T, base_seed=seed, p_absent=p_absent)
    if p_absent:
        mu[8:31] = np.nan          # 23 frames without anybody: windows of up to 20 pairs fall inside (no common sample)
        mv[8:31] = np.nan
    return mu, mv


@pytest.mark.parametrize("p_absent", [0.0, 0.3], ids=["full", "absent"])
@pytest.mark.parametrize("tcs", [[50], [50, 100, 200]], ids=["tc50", "tc50_100_200"])
@pytest.mark.parametrize("U,T", [(1, 40), (7, 60), (64, 60), (512, 45)])
def test_vs_oracle(native, engine, U, T, tcs, p_absent):
    mu, mv = walk(U, T, p_absent, 500 + U)
    plan = fib_plan(native, engine, tcs)
    tiles = wt.tiles_of(mu, mv, W, H, tcs)
    seen = set()
    for window in (1, 2, 20, T - 1):
        for stride in sorted({1, 7, window}):
            msg = f"U{U} T{T} w{window} s{stride}"
            res = plan.transition_windowed(mu=mu, mv=mv, window=window, stride=stride, want_srccount=True, check=False)
            samples = check_rows(res, mu, mv, tcs, tiles, window, stride, msg)
            empty = bool((samples == 0).any())
            assert res["code"] == (native.VET_ERR_EMPTY if empty else native.VET_OK), msg
            if empty and stride == 1 and window == 20:
                with pytest.raises(native.NativeError) as e:
                    plan.transition_windowed(mu=mu, mv=mv, window=window, stride=stride)
                assert e.value.code == native.VET_ERR_EMPTY
            seen |= {"empty"} if empty else set()
            seen |= {"one"} if (samples == 1).any() else set()
            seen |= {"N<=n"} if ((samples > 1) & (samples <= tcs[0])).any() else set()
            seen |= {"N>n"} if (samples > max(tcs) + 1).any() else set()
    plan.close()
    # what this shape is in the matrix for
    if p_absent:
        assert "empty" in seen
    if U == 1:
        assert "one" in seen and "N<=n" in seen
    if U >= 64:
        assert "N>n" in seen


def test_uniform_on_sphere_takes_several_hash_passes(native, engine):
    from viewport_entropy_toolkit import _synthetic
    U, T, window, tc = 512, 45, 20, 200
    n = len(vo.fibonacci_lattice(tc))
    mu, mv = _synthetic.uniform_sphere_video(U, T, base_seed=77)
    tiles = wt.tiles_of(mu, mv, W, H, [tc])
    bound = min(wt.bucket_bound(tiles[0], f0, window, n) for f0 in range(T - window))
    assert bound > HASH_SLOTS * 6 // 10 - n, bound          # every row is cut into more than one range of source tiles
    plan = fib_plan(native, engine, [tc])
    for stride in (1, 7):
        res = plan.transition_windowed(mu=mu, mv=mv, window=window, stride=stride, want_srccount=True)
        check_rows(res, mu, mv, [tc], tiles, window, stride, f"uniform s{stride}")
    plan.close()


# ------------------------------------------------------------------------------------------- identities with the per-pair call
@pytest.mark.parametrize("U", [7, 512])
def test_window_of_one_pair_equals_the_per_pair_call(native, engine, U):
    mu, mv = walk(U, 45, 0.3, 900 + U)
    plan = fib_plan(native, engine, [50, 100, 200])
    a = plan.transition_windowed(mu=mu, mv=mv, window=1, stride=1, want_srccount=True, check=False)
    b = plan.transition(mu=mu, mv=mv, want_pairs=False, want_srccount=True, check=False)
    close(a["entropy"], b["entropy"], "window 1", rtol=1e-12)
    assert np.array_equal(a["samples"], b["common"]) and np.array_equal(a["srccount"], b["srccount"])
    assert a["code"] == b["code"] == native.VET_ERR_EMPTY
    plan.close()


@pytest.mark.parametrize("U,window", [(7, 20), (64, 4), (64, 20), (512, 20)])
def test_disjoint_windows_equal_the_materialised_per_pair_call(native, engine, U, window):
    """The parent commit's capability as an independent check: a [2R][window * U] input whose row 2r holds frames
    f0 .. f0 + w - 1 side by side and row 2r + 1 frames f0 + 1 .. f0 + w; the even output rows."""
    T = 3 * window + 1
    mu, mv = walk(U, T, 0.0, 55 + U)
    rng = np.random.default_rng(U)
    gone = rng.random(mu.shape) < 0.1
    mu[gone] = np.nan
    mv[gone] = np.nan
    plan = fib_plan(native, engine, [50, 100, 200])
    a = plan.transition_windowed(mu=mu, mv=mv, window=window, stride=window, want_srccount=True)
    R = len(a["entropy"])
    assert R == 3

    def materialise(x):
        return np.stack([x[r * window + o:r * window + o + window].reshape(-1) for r in range(R) for o in (0, 1)])
    b = plan.transition(mu=materialise(mu), mv=materialise(mv), want_pairs=False, want_srccount=True)
    close(a["entropy"], b["entropy"][::2], "materialised", rtol=1e-12)
    assert np.array_equal(a["samples"], b["common"][::2]) and np.array_equal(a["srccount"], b["srccount"][::2])
    plan.close()


# ------------------------------------------------------------------------------------------- purity
@pytest.mark.parametrize("U", [7, 64, 512])
def test_rows_are_pure_functions_of_their_frames(native, engine, U):
    mu, mv = walk(U, 60, 0.3, 7)
    ids = ids_of(mu, mv)
    plan = fib_plan(native, engine, [50, 100, 200])
    for window in (1, 2, 20):
        a = plan.transition_windowed(mu=mu, mv=mv, window=window, stride=1, want_srccount=True, check=False)
        b = plan.transition_windowed(mu=mu, mv=mv, window=window, stride=1, want_srccount=True, check=False)
        assert a["entropy"].tobytes() == b["entropy"].tobytes() and np.array_equal(a["srccount"], b["srccount"])   # run to run
        c = plan.transition_windowed(mu=mu, mv=mv, window=window, stride=7, want_srccount=True, check=False)
        assert c["entropy"].tobytes() == a["entropy"][::7].tobytes(), window          # whatever stride selected the row
        assert np.array_equal(c["samples"], a["samples"][::7]) and np.array_equal(c["srccount"], a["srccount"][::7])
        d = plan.transition_windowed(mu=mu[13:], mv=mv[13:], window=window, stride=1, check=False)    # a frame-shifted slice
        assert d["entropy"].tobytes() == a["entropy"][13:].tobytes(), window
        e = plan.transition_windowed(ids=ids, window=window, stride=1, want_srccount=True, check=False)   # grid and ids entries
        assert e["entropy"].tobytes() == a["entropy"].tobytes() and np.array_equal(e["srccount"], a["srccount"])
        assert e["code"] == a["code"]
    plan.close()


# ------------------------------------------------------------------------------------------- errors and limits
def test_errors_and_limits(native, engine):
    mu, mv = walk(16, 30, 0.0, 9)
    plan = fib_plan(native, engine, [50])
    bad_mu = mu.copy()
    bad_mu[5, 3] = 1.5
    r = plan.transition_windowed(mu=bad_mu, mv=mv, window=4, check=False)
    assert r["code"] == native.VET_ERR_RANGE
    covers = np.zeros(len(r["samples"]), dtype=np.int32)
    covers[1:6] = 1                                     # pairs 4 and 5 hold frame 5: rows 1..5 lose one sample each ...
    covers[2:5] = 2                                     # ... rows 2..4 hold both pairs
    assert np.array_equal(r["samples"], plan.transition_windowed(mu=mu, mv=mv, window=4)["samples"] - covers)
    for window, stride in ((0, 1), (4, 0), (30, 1), (-1, 1)):
        with pytest.raises(ValueError):
            plan.transition_windowed(mu=mu, mv=mv, window=window, stride=stride)
        ent = np.zeros(64)
        rc = plan.lib.vet_transition_entropy_windowed_host(plan.handle, native._ptr(mu), native._ptr(mv), None, 16, 30, window,
                                                           stride, native._ptr(ent), None, None)
        assert rc == native.VET_ERR_INVALID and plan.lib.vet_last_error()
    one = np.full((1, 16), 0.5)
    ent = np.zeros(4)
    assert plan.lib.vet_transition_entropy_windowed_host(plan.handle, native._ptr(one), native._ptr(one), None, 16, 1, 1, 1,
                                                         native._ptr(ent), None, None) == native.VET_ERR_INVALID
    # window * n_users = 2^19: refused before anything is staged or launched
    U, window = 1 << 15, 16
    big = np.full((window + 1, U), 0.5)
    with pytest.raises(native.NativeError) as e:
        plan.transition_windowed(mu=big, mv=big, window=window)
    assert e.value.code == native.VET_ERR_UNSUPPORTED
    ok = plan.transition_windowed(mu=big[:16], mv=big[:16], window=window - 1)       # just below the limit runs
    assert ok["samples"][0] == (window - 1) * U and np.isfinite(ok["entropy"][0])
    plan.close()


# ------------------------------------------------------------------------------------------- the analyzer
def test_analyzer_returns_the_windowed_frame(native, tmp_path):
    import pandas as pd
    from viewport_entropy_toolkit import TransitionEntropyAnalyzer, ValidationError
    from viewport_entropy_toolkit.config import AnalyzerConfig
    from viewport_entropy_toolkit import _synthetic
    U, T = 8, 60
    mu, mv = _synthetic.random_walk_video(U, T, base_seed=77)
    times = np.arange(T) * 0.1
    d = tmp_path / "video"
    d.mkdir()
    for u in range(U):
        pd.DataFrame({"time": times, "2dmu": mu[:, u], "2dmv": mv[:, u]}).to_csv(d / f"user{u:03d}.csv", index=False)
    an = TransitionEntropyAnalyzer(AnalyzerConfig(tile_counts=[50, 100], output_dir=tmp_path / "out"))
    an.process_directory(d)
    per_pair = an.compute_entropy()
    kept = per_pair["entropy"].to_numpy().copy()
    df = an.compute_windowed_entropy(20, 5)
    # the pooled order is pair-major, then the analyzer's user order: the directory order of the CSV files, as in the reference
    order = [int(name[4:]) for name in an._samples()[4]]
    assert sorted(order) == list(range(U))
    mu, mv = mu[:, order], mv[:, order]
    ent, samples, src = wt.fast(mu, mv, W, H, [50, 100], 20, 5)
    assert list(df.columns) == ["time", "time_end", "entropy", "samples", "tile_weights"] and len(df) == 8
    pair_time = per_pair["time"].to_numpy()
    assert np.array_equal(df["time"], pair_time[::5][:8]) and np.array_equal(df["time_end"], pair_time[19::5][:8])
    close(df["entropy"].to_numpy(), ent, "analyzer")
    assert np.array_equal(df["samples"], samples)
    tiles = an._fibonacci_vectors[50]
    cell = df["tile_weights"][3]
    assert {k: int(v) for k, v in dict(cell).items()} == {tiles[i]: int(src[3][i]) for i in np.flatnonzero(src[3])}
    assert type(cell) is type(per_pair["tile_weights"][3])
    assert an._entropy_results is per_pair and np.array_equal(per_pair["entropy"].to_numpy(), kept)      # left alone
    with pytest.raises(ValueError):
        an.compute_windowed_entropy(60)
    # empty windows: what the reference raises on the pooled dicts
    a2 = TransitionEntropyAnalyzer(AnalyzerConfig(tile_counts=[50]))
    m2, v2 = mu.copy(), mv.copy()
    m2[10:40] = np.nan
    v2[10:40] = np.nan
    a2.load_arrays(times, m2, v2)
    with pytest.raises(ValidationError, match="Empty vector dictionary"):
        a2.compute_windowed_entropy(20)
    m3, v3 = mu.copy(), mv.copy()
    m3[10:40:2, :4] = np.nan                            # users 0-3 only in odd frames, users 4-7 only in even ones:
    v3[10:40:2, :4] = np.nan                            # every frame has samples, no pair has a common user
    m3[11:40:2, 4:] = np.nan
    v3[11:40:2, 4:] = np.nan
    a3 = TransitionEntropyAnalyzer(AnalyzerConfig(tile_counts=[50]))
    a3.load_arrays(times, m3, v3)
    with pytest.raises(ZeroDivisionError):
        a3.compute_windowed_entropy(20)
