"""GPU: sliding-window (pooled) spatial entropy through the C-ABI (Plan.spatial_windowed -> vet_spatial_entropy_windowed_host).
Row r pools every present sample of frames [r * stride, r * stride + window) into one histogram per lattice; the references are
golden G14 (the real reference on the pooled dict, tools/gen_windowed_golden.py) and the numpy oracles of tests/_window_oracle.py
(pinned against G14 in tests/test_windowed_surface.py).  Entropy: the project's contract, 1e-6 relative, NaN = NaN; samples
exact; weights within tests/_tol.py."""
import numpy as np
import pytest

from oracle import vet_oracle as vo
from tests import _window_oracle as wo
from tests._tol import W_RTOL, w_atol

pytestmark = pytest.mark.gpu

W, H = 100, 200
WINDOWS = (1, 2, 20, 64, "T")
RTOL = 1e-6


@pytest.fixture(scope="module")
def native():
    from viewport_entropy_toolkit import _native
    return _native


@pytest.fixture(scope="module")
def engine(native):
    return native.Engine.default()


def fib_plan(native, engine, tcs, weighted=True, fov=120.0, power=2.0):
    return native.Plan(engine, [vo.fibonacci_lattice(t) for t in tcs], fov, power, weighted, W, H)


def naive_plan(weighted, th=10, tw=20):
    from viewport_entropy_toolkit import NaiveSpatialEntropyAnalyzer
    from viewport_entropy_toolkit.config import EntropyConfig, NaiveAnalyzerConfig
    an = NaiveSpatialEntropyAnalyzer(NaiveAnalyzerConfig(tile_height=th, tile_width=tw, video_width=W, video_height=H,
                                                         entropy_config=EntropyConfig(use_weight_distribution=weighted)))
    return an._naive_plan()


def strides(window):
    return sorted({1, 3, window, window + 5})


def close(got, want, msg=""):
    print(msg, "max rel err", float(np.nanmax(np.abs(got - want) / np.maximum(np.abs(want), 1e-300), initial=0.0)))
    assert np.array_equal(np.isnan(got), np.isnan(want)), (msg, np.flatnonzero(np.isnan(got) != np.isnan(want))[:10])
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0, equal_nan=True, err_msg=msg)


def check_weights(got, want, samples, power, msg=""):
    assert np.array_equal(wo.keys_of(got), wo.keys_of(want)), msg
    for g, w, n in zip(got, want, samples):
        np.testing.assert_allclose(np.abs(g), np.abs(w), rtol=W_RTOL, atol=w_atol(int(n), power), err_msg=msg)


# ------------------------------------------------------------------------------------------- the reference (golden G14)
def test_vs_reference_golden(native, engine, golden_dir):
    g = np.load(golden_dir / "g14_windowed.npz")
    cases = sorted({k.rsplit("__", 1)[0] for k in g.files if "__" in k})
    assert len(cases) == 60
    plans = {}
    for tag in cases:
        parts = tag.split("_")
        window, stride, flag = int(parts[-2][1:]), int(parts[-1][1:]), parts[1] == "w"
        rows = g[f"{tag}__rows"]
        if parts[0] == "naive":
            key, mu, mv = ("naive", flag), g["mu"], g["mv"]
            plan = plans.get(key) or plans.setdefault(key, naive_plan(flag))
        else:
            sfx = "" if parts[0] == "full" else "_absent"
            tcs = tuple(int(x) for x in tag.split("_tc")[1].split("_w")[0].split("_"))
            key, mu, mv = (tcs, flag), g["mu" + sfx], g["mv" + sfx]
            plan = plans.get(key) or plans.setdefault(key, fib_plan(native, engine, tcs, flag))
        res = plan.spatial_windowed(mu=mu, mv=mv, window=window, stride=stride, want_weights=parts[0] != "naive", check=False)
        assert res["code"] == native.VET_OK, tag
        assert len(res["entropy"]) == wo.n_rows(300, window, stride)
        close(res["entropy"][rows], g[f"{tag}__entropy"], tag)
        assert np.array_equal(res["samples"][rows], g[f"{tag}__samples"]), tag
        if parts[0] != "naive":
            wr = g[f"{tag}__weights_rows"]
            want = np.where(g[f"{tag}__keys"] & (g[f"{tag}__weights"] == 0), -0.0, g[f"{tag}__weights"])
            check_weights(res["weights"][wr], want, res["samples"][wr], 2.0, tag)
    for p in plans.values():
        p.close()


# ------------------------------------------------------------------------------------------- the numpy oracle, seeded walks
def walk(U, T, seed):
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(U, T, base_seed=seed, p_absent=0.1 if U > 1 else 0.0)
    mu[100:171] = np.nan           # 71 frames without any user: windows of up to 64 frames fall inside, longer ones straddle
    mv[100:171] = np.nan
    return mu, mv


@pytest.mark.parametrize("tcs", [[50], [50, 100, 200]], ids=["tc50", "tc50_100_200"])
@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "unweighted"])
@pytest.mark.parametrize("U,T", [(1, 600), (7, 600), (64, 600), (1024, 240)])
def test_fibonacci_vs_oracle(native, engine, U, T, weighted, tcs):
    mu, mv = walk(U, T, 100 + U)
    plan = fib_plan(native, engine, tcs, weighted)
    frames = wo.frame_sums(mu, mv, W, H, tcs, use_weight_distribution=weighted)
    for window in WINDOWS:
        window = T if window == "T" else window
        for stride in strides(window):
            msg = f"U{U} T{T} w{window} s{stride}"
            res = plan.spatial_windowed(mu=mu, mv=mv, window=window, stride=stride, want_weights=True, check=False)
            ent, samples, weights = wo.fast(mu, mv, W, H, tcs, window, stride, use_weight_distribution=weighted, frames=frames)
            empty = int((samples == 0).sum())
            assert res["code"] == (native.VET_ERR_EMPTY if empty else native.VET_OK), msg
            assert np.array_equal(res["samples"], samples), msg
            close(res["entropy"], ent, msg)
            check_weights(res["weights"], weights, samples, 2.0, msg)
            if empty and stride == 1:
                with pytest.raises(native.NativeError) as e:
                    plan.spatial_windowed(mu=mu, mv=mv, window=window, stride=stride)
                assert e.value.code == native.VET_ERR_EMPTY
    plan.close()


@pytest.mark.parametrize("weighted", [True, False], ids=["log2n", "log2samples"])
@pytest.mark.parametrize("U,T", [(1, 600), (7, 600), (64, 600), (1024, 240)])
def test_naive_vs_oracle(native, U, T, weighted):
    mu, mv = walk(U, T, 200 + U)
    plan = naive_plan(weighted)
    for window in WINDOWS:
        window = T if window == "T" else window
        for stride in strides(window):
            msg = f"naive U{U} T{T} w{window} s{stride}"
            res = plan.spatial_windowed(mu=mu, mv=mv, window=window, stride=stride, check=False)
            ent, samples = wo.naive(mu, mv, W, H, 10, 20, window, stride, use_weight_distribution=weighted)
            assert np.array_equal(res["samples"], samples), msg
            close(res["entropy"], ent, msg)


def test_underflow_configuration(native, engine, golden_dir):
    """Golden G12's plan (500 tiles, power factor 150: in-FoV weights underflow to 0.0 and stay keys): NaN rows are NaN."""
    g = np.load(golden_dir / "g12_underflow.npz")
    px, py = g["px"], g["py"]
    present = px >= 0
    mu = np.where(present, np.where(px == W, 1.0, (px + 0.5) / W), np.nan)
    mv = np.where(present, np.where(py == H, 1.0, (py + 0.5) / H), np.nan)
    for tc, fov, power in ((500, 120.0, 150.0), (50, 60.0, 200.0), (500, 120.0, 80.0)):
        plan = fib_plan(native, engine, [tc], True, fov, power)
        one = plan.spatial_windowed(mu=mu, mv=mv, window=1, want_weights=True)
        ref = g[f"tc{tc}_fov{int(fov)}_p{int(power)}__entropy"]
        close(one["entropy"], ref, "G12 per frame")
        assert np.array_equal(wo.keys_of(one["weights"]), g[f"tc{tc}_fov{int(fov)}_p{int(power)}__keys"])
        seen_nan = False
        for window in (2, 5, 20, 40):
            for stride in strides(window):
                res = plan.spatial_windowed(mu=mu, mv=mv, window=window, stride=stride, want_weights=True)
                ent, samples, weights = wo.fast(mu, mv, W, H, [tc], window, stride, fov_angle=fov, power_factor=power)
                close(res["entropy"], ent, f"G12 tc{tc} p{power} w{window} s{stride}")
                check_weights(res["weights"], weights, samples, power)
                seen_nan = seen_nan or bool(np.isnan(ent).any())
        assert seen_nan or not np.isnan(ref).any()
        plan.close()


# ------------------------------------------------------------------------------------------- purity
@pytest.mark.parametrize("kind", ["weighted", "weighted3", "unweighted", "naive"])
def test_rows_are_pure_functions_of_their_frames(native, engine, kind):
    mu, mv = walk(64, 400, 7)
    plan = (naive_plan(False) if kind == "naive" else
            fib_plan(native, engine, [50, 100, 200] if kind == "weighted3" else [50], kind != "unweighted"))
    ww = kind != "naive"
    for window in (1, 2, 20, 64):
        a = plan.spatial_windowed(mu=mu, mv=mv, window=window, stride=1, want_weights=ww, check=False)
        b = plan.spatial_windowed(mu=mu, mv=mv, window=window, stride=1, want_weights=ww, check=False)
        assert a["entropy"].tobytes() == b["entropy"].tobytes()                       # run to run
        if ww:
            assert a["weights"].tobytes() == b["weights"].tobytes()
        for s in (3, window, window + 5):
            c = plan.spatial_windowed(mu=mu, mv=mv, window=window, stride=s, want_weights=ww, check=False)
            assert c["entropy"].tobytes() == a["entropy"][::s].tobytes(), (window, s)  # whatever stride selected the row
            assert np.array_equal(c["samples"], a["samples"][::s])
            if ww:
                assert c["weights"].tobytes() == a["weights"][::s].tobytes(), (window, s)
        # the video cut into two calls that overlap by window - 1 frames
        cut = 217
        lo = plan.spatial_windowed(mu=mu[:cut + window - 1], mv=mv[:cut + window - 1], window=window, want_weights=ww, check=False)
        hi = plan.spatial_windowed(mu=mu[cut:], mv=mv[cut:], window=window, want_weights=ww, check=False)
        assert (lo["entropy"].tobytes() + hi["entropy"].tobytes()) == a["entropy"].tobytes(), window
        if ww:
            assert (lo["weights"].tobytes() + hi["weights"].tobytes()) == a["weights"].tobytes(), window


# ------------------------------------------------------------------------------------------- window = 1 is the per-frame series
@pytest.mark.parametrize("U", [7, 64, 1024])
def test_window_of_one_frame_equals_the_per_frame_call(native, engine, U):
    mu, mv = walk(U, 300, 300 + U)
    for kind in ("unweighted", "unweighted3", "naive_u", "naive_w"):
        plan = (naive_plan(kind == "naive_w") if kind.startswith("naive") else
                fib_plan(native, engine, [50, 100, 200] if kind.endswith("3") else [50], False))
        ww = not kind.startswith("naive")
        a = plan.spatial_windowed(mu=mu, mv=mv, window=1, want_weights=ww, check=False)
        b = plan.spatial(mu=mu, mv=mv, want_assign=False, want_weights=ww, check=False)
        assert a["entropy"].tobytes() == b["entropy"].tobytes(), kind                 # bit for bit
        assert np.array_equal(a["samples"], b["present"]) and a["code"] == b["code"] == native.VET_ERR_EMPTY
        if ww:
            assert a["weights"].tobytes() == b["weights"].tobytes(), kind
    for tcs in ([50], [50, 100, 200]):
        plan = fib_plan(native, engine, tcs, True)
        a = plan.spatial_windowed(mu=mu, mv=mv, window=1, want_weights=True, check=False)
        d = plan.spatial(mu=mu, mv=mv, want_assign=False, want_weights=True, check=False)
        close(a["entropy"], d["entropy"], "default formulation")                      # within the contract of the default one
        assert a["weights"].tobytes() == d["weights"].tobytes()                       # tile_weights: one producer, same bits
        fp = fib_plan(native, engine, tcs, True)
        fp.set_fp64(True)
        fp.set_table_policy(1)
        e = fp.spatial(mu=mu, mv=mv, want_assign=False, want_weights=True, check=False)
        assert all(fp.last_formulation(k) == "dtable" for k in range(len(tcs)))
        assert a["entropy"].tobytes() == e["entropy"].tobytes(), tcs                  # bit for bit against `dtable`
        assert a["weights"].tobytes() == e["weights"].tobytes()
        assert np.array_equal(a["samples"], e["present"])
        plan.close()
        fp.close()


# ------------------------------------------------------------------------------------------- stride = window: the reshaped per-frame call
@pytest.mark.parametrize("kind", ["weighted", "weighted3", "unweighted", "naive"])
@pytest.mark.parametrize("U,window", [(7, 20), (64, 4), (64, 20), (256, 4)])
def test_disjoint_windows_equal_the_reshaped_per_frame_call(native, engine, kind, U, window):
    """The parent commit's capability as a second, independent check: [T][U] viewed as [T / w][w * U]."""
    from viewport_entropy_toolkit import _synthetic
    T = 240
    mu, mv = _synthetic.random_walk_video(U, T, base_seed=55 + U, p_absent=0.1)
    plan = (naive_plan(False) if kind == "naive" else
            fib_plan(native, engine, [50, 100, 200] if kind == "weighted3" else [50], kind != "unweighted"))
    ww = kind != "naive"
    a = plan.spatial_windowed(mu=mu, mv=mv, window=window, stride=window, want_weights=ww)
    b = plan.spatial(mu=mu.reshape(T // window, window * U), mv=mv.reshape(T // window, window * U), want_assign=False,
                     want_weights=ww)
    close(a["entropy"], b["entropy"], f"{kind} reshape")
    assert np.array_equal(a["samples"], b["present"])
    if ww:
        check_weights(a["weights"], b["weights"], a["samples"], 2.0)


# ------------------------------------------------------------------------------------------- ids entry, errors, status words
def test_ids_entry_and_errors(native, engine):
    mu, mv = walk(16, 200, 9)
    mu[5, 3], mv[5, 3] = 0.3, 0.4
    px, py, present, _ = vo.sample_directions(mu, mv, W, H)
    ids = np.where(present, py * (W + 1) + px, -1).astype(np.int32)
    for weighted in (True, False):
        plan = fib_plan(native, engine, [50, 100], weighted)
        for window, stride in ((1, 1), (20, 3), (64, 64)):
            a = plan.spatial_windowed(mu=mu, mv=mv, window=window, stride=stride, want_weights=True, check=False)
            b = plan.spatial_windowed(ids=ids, window=window, stride=stride, want_weights=True, check=False)
            assert a["entropy"].tobytes() == b["entropy"].tobytes() and a["weights"].tobytes() == b["weights"].tobytes()
            assert np.array_equal(a["samples"], b["samples"]) and a["code"] == b["code"]
        # range errors as vet_spatial_entropy: VET_ERR_RANGE, the sample counts as absent
        bad_mu = mu.copy()
        bad_mu[5, 3] = 1.5
        clean = plan.spatial_windowed(mu=mu, mv=mv, window=4, check=False)
        r = plan.spatial_windowed(mu=bad_mu, mv=mv, window=4, check=False)
        covers = np.zeros(len(r["samples"]), dtype=np.int32)
        covers[2:6] = 1                                                             # rows 2..5 hold frame 5
        assert r["code"] == native.VET_ERR_RANGE and np.array_equal(r["samples"], clean["samples"] - covers)
        with pytest.raises(native.NativeError) as e:
            plan.spatial_windowed(mu=bad_mu, mv=mv, window=4)
        assert e.value.code == native.VET_ERR_RANGE
        bad_ids = ids.copy()
        bad_ids[0, 0] = plan.n_dirs
        assert plan.spatial_windowed(ids=bad_ids, window=4, check=False)["code"] == native.VET_ERR_RANGE
        for window, stride in ((0, 1), (4, 0), (201, 1), (-1, 1)):
            with pytest.raises(ValueError):
                plan.spatial_windowed(mu=mu, mv=mv, window=window, stride=stride)
            ent = np.zeros(8)
            rc = plan.lib.vet_spatial_entropy_windowed_host(plan.handle, native._ptr(mu), native._ptr(mv), None, 16, 200, window,
                                                            stride, native._ptr(ent), None, None)
            assert rc == native.VET_ERR_INVALID and plan.lib.vet_last_error()
        plan.close()


def test_analyzers_return_the_windowed_frame(native):
    from viewport_entropy_toolkit import NaiveSpatialEntropyAnalyzer, SpatialEntropyAnalyzer
    from viewport_entropy_toolkit.config import AnalyzerConfig, NaiveAnalyzerConfig
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(8, 120, base_seed=77, p_absent=0.1)
    times = np.arange(120) * 0.1
    an = SpatialEntropyAnalyzer(AnalyzerConfig(tile_counts=[50, 100]))
    an.load_arrays(times, mu, mv)
    df = an.compute_windowed_entropy(20, 5)
    ent, samples, weights = wo.fast(mu, mv, W, H, [50, 100], 20, 5)
    assert list(df.columns) == ["time", "time_end", "entropy", "samples", "tile_weights"] and len(df) == 21
    assert np.array_equal(df["time"], times[::5][:21]) and np.array_equal(df["time_end"], times[19::5][:21])
    close(df["entropy"].to_numpy(), ent, "analyzer")
    assert np.array_equal(df["samples"], samples)
    tiles = an._fibonacci_vectors[50]
    cell = df["tile_weights"][3]
    assert set(cell) == {tiles[i] for i in np.flatnonzero(wo.keys_of(weights[3]))}
    assert all(abs(cell[tiles[i]] - weights[3][i]) <= W_RTOL * weights[3][i] + w_atol(int(samples[3])) for i in np.flatnonzero(weights[3] > 0))
    nv = NaiveSpatialEntropyAnalyzer(NaiveAnalyzerConfig(tile_height=10, tile_width=20))
    nv.load_arrays(times, mu, mv)
    dn = nv.compute_windowed_entropy(20)
    e2, s2 = wo.naive(mu, mv, W, H, 10, 20, 20, 1)
    assert list(dn.columns) == ["time", "time_end", "entropy", "samples"]
    close(dn["entropy"].to_numpy(), e2, "naive analyzer")
    assert np.array_equal(dn["samples"], s2)


# ------------------------------------------------------------------------------------------- full size
def test_config3_shape_full_size(native, engine):
    """BASELINE config 3's shape (1024 users x 30 000 frames, 501 tiles, weighted), a 2-second window every frame."""
    U, T, window = 1024, 30000, 20
    rng = np.random.default_rng(2)
    mu = np.mod(0.5 + np.cumsum(rng.normal(0, 0.01, (T, U)), axis=0), 1.0)
    mv = np.clip(0.5 + np.cumsum(rng.normal(0, 0.005, (T, U)), axis=0), 0.0, 1.0)
    plan = fib_plan(native, engine, [500], True)
    a = plan.spatial_windowed(mu=mu, mv=mv, window=window, stride=1)
    assert len(a["entropy"]) == T - window + 1 and np.all(a["samples"] == window * U)
    assert np.all(np.isfinite(a["entropy"])) and a["entropy"].min() >= 0.0 and a["entropy"].max() <= 1.0
    rows = np.sort(rng.integers(0, T - window + 1, 32))
    for r in rows:
        ent, samples, _ = wo.literal(mu[r:r + window], mv[r:r + window], W, H, [500], window, 1)
        assert samples[0] == a["samples"][r]
        close(a["entropy"][r:r + 1], ent, f"row {r}")
    plan.close()
