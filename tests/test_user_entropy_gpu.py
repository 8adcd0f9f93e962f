"""GPU: per-viewer spatial entropy through the C-ABI (Plan.spatial_per_user -> vet_user_entropy_host, the device entry, both
analyzers).  Row (u, r) pools user u's present samples of frames [r * stride, r * stride + window) into one histogram per lattice;
the references are golden G16 (the real reference on that dict, tools/gen_golden_user_entropy.py) and the numpy oracles of
tests/_user_oracle.py (pinned against G16 in tests/test_user_entropy_surface.py).  Tolerances are those of
tests/test_windowed_gpu.py: entropy 1e-6 relative with NaN = NaN, samples and key sets exact, weights within tests/_tol.py."""
import ctypes

import numpy as np
import pytest

from oracle import vet_oracle as vo
from tests import _user_oracle as uo
from tests._tol import W_RTOL, w_atol

pytestmark = pytest.mark.gpu

W, H = 100, 200
RTOL = 1e-6
SHAPES = ((300, 1), (20, 20), (20, 7), (1, 1))
ABSENT_USER = 3


@pytest.fixture(scope="module")
def native():
    from viewport_entropy_toolkit import _native
    return _native


@pytest.fixture(scope="module")
def engine(native):
    return native.Engine.default()


@pytest.fixture(scope="module")
def g16(golden_dir):
    return np.load(golden_dir / "g16_user_entropy.npz")


def fib_plan(native, engine, tcs, weighted=True, fov=120.0, power=2.0):
    return native.Plan(engine, [vo.fibonacci_lattice(t) for t in tcs], fov, power, weighted, W, H)


def naive_analyzer(weighted=True):
    from viewport_entropy_toolkit import NaiveSpatialEntropyAnalyzer
    from viewport_entropy_toolkit.config import EntropyConfig, NaiveAnalyzerConfig
    return NaiveSpatialEntropyAnalyzer(NaiveAnalyzerConfig(tile_height=10, tile_width=20, video_width=W, video_height=H,
                                                           entropy_config=EntropyConfig(use_weight_distribution=weighted)))


def close(got, want, msg=""):
    print(msg, "max rel err", float(np.nanmax(np.abs(got - want) / np.maximum(np.abs(want), 1e-300), initial=0.0)))
    assert np.array_equal(np.isnan(got), np.isnan(want)), (msg, np.argwhere(np.isnan(got) != np.isnan(want))[:10])
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0, equal_nan=True, err_msg=msg)


def check_weights(got, want, samples, power=2.0, msg=""):
    got, want, samples = got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1]), np.asarray(samples).reshape(-1)
    assert np.array_equal(uo.keys_of(got), uo.keys_of(want)), msg
    for n in np.unique(samples):
        sel = samples == n
        np.testing.assert_allclose(np.abs(got[sel]), np.abs(want[sel]), rtol=W_RTOL, atol=w_atol(int(n), power), err_msg=msg)


def ids_of(mu, mv):
    return uo.direction_ids(mu, mv, W, H)[0].astype(np.int32)


def g16_cases(g16):
    for w, s in SHAPES:
        for flag, tcs in ((True, (50,)), (True, (50, 100, 200)), (False, (50,))):
            yield f"{'w' if flag else 'u'}_tc{'_'.join(map(str, tcs))}_w{w}_s{s}", flag, tcs, w, s
        yield f"naive_h10_w20_w{w}_s{s}", True, None, w, s


def check_g16(g16, tag, res, msg):
    rows = g16[f"{tag}__rows"]
    close(res["entropy"][:, rows], g16[f"{tag}__entropy"], msg)
    assert np.array_equal(res["samples"][:, rows], g16[f"{tag}__samples"]), msg
    if res.get("weights") is not None:
        want = np.where(g16[f"{tag}__keys"] & (g16[f"{tag}__weights"] == 0), -0.0, g16[f"{tag}__weights"])
        check_weights(res["weights"][:, rows], want, g16[f"{tag}__samples"], 2.0, msg)
    empty = res["samples"] == 0
    assert np.isnan(res["entropy"][empty]).all()
    w, s = int(tag.split("_")[-2][1:]), int(tag.split("_")[-1][1:])
    r = np.arange(res["samples"].shape[1])
    gone = (r * s >= 100) & (r * s + w <= 200)
    assert empty[ABSENT_USER][gone].all()                          # the absent user's rows: NaN with samples 0


# ------------------------------------------------------------------------------------------- the reference (golden G16)
def test_host_entry_vs_reference_golden(native, engine, g16):
    """Plan.spatial_per_user (vet_user_entropy_host), the grid and the ids entry points, every stored case."""
    mu, mv = g16["mu"], g16["mv"]
    ids = ids_of(mu, mv)
    plans = {}
    for tag, flag, tcs, w, s in g16_cases(g16):
        key = (tcs, flag)
        if key not in plans:
            plans[key] = naive_analyzer(flag)._naive_plan() if tcs is None else fib_plan(native, engine, tcs, flag)
        plan = plans[key]
        res = plan.spatial_per_user(mu=mu, mv=mv, window=None if w == 300 else w, stride=s, want_weights=tcs is not None)
        assert res["code"] == native.VET_OK and res["entropy"].shape == (8, uo.n_rows(300, w, s)), tag   # empty rows: no error
        check_g16(g16, tag, res, tag + " grid")
        if tcs is not None:                 # a naive plan has no ids entry of its own table
            res = plan.spatial_per_user(ids=ids, window=w, stride=s, want_weights=True)
            check_g16(g16, tag, res, tag + " ids")
    for key, p in plans.items():
        if key[0] is not None:
            p.close()


def test_device_entry_vs_reference_golden(native, engine, g16):
    """vet_user_entropy / vet_user_entropy_ids on device buffers; d_status = {0, rows without a sample}, added to."""
    lib = engine.lib
    mu, mv = np.ascontiguousarray(g16["mu"]), np.ascontiguousarray(g16["mv"])
    ids = ids_of(mu, mv)
    T, U = mu.shape
    bufs = []

    def dev(nbytes, src=None):
        p = ctypes.c_void_p()
        assert lib.vet_malloc(engine.handle, nbytes, ctypes.byref(p)) == 0
        bufs.append(p)
        if src is not None:
            assert lib.vet_memcpy_h2d(engine.handle, p, native._ptr(src), nbytes) == 0
        return p

    d_mu, d_mv, d_ids = dev(mu.nbytes, mu), dev(mv.nbytes, mv), dev(ids.nbytes, ids)
    plans = {}
    try:
        for tag, flag, tcs, w, s in g16_cases(g16):
            if tcs is None:
                continue
            plan = plans.get((tcs, flag)) or plans.setdefault((tcs, flag), fib_plan(native, engine, tcs, flag))
            R = uo.n_rows(T, w, s)
            n0 = plan.n_tiles[0]
            for entry in ("grid", "ids"):
                ent, wts, smp = np.empty((U, R)), np.empty((U, R, n0)), np.empty((U, R), np.int32)
                st = np.array([0, 1000], np.int32)
                d_ent, d_w, d_s, d_st = dev(ent.nbytes), dev(wts.nbytes), dev(smp.nbytes), dev(8, st)
                if entry == "grid":
                    plan.spatial_per_user_device(d_mu.value, d_mv.value, U, T, w, s, d_ent.value, d_w.value, d_s.value, d_st.value)
                else:
                    native._check(lib, lib.vet_user_entropy_ids(plan.handle, d_ids, U, T, w, s, d_ent, d_w, d_s, d_st, None))
                for h, d in ((ent, d_ent), (wts, d_w), (smp, d_s), (st, d_st)):
                    assert lib.vet_memcpy_d2h(engine.handle, native._ptr(h), d, h.nbytes) == 0
                check_g16(g16, tag, dict(entropy=ent, weights=wts, samples=smp), f"{tag} device {entry}")
                assert st.tolist() == [0, 1000 + int((smp == 0).sum())], tag
    finally:
        engine.synchronize()
        for p in bufs:
            lib.vet_free(engine.handle, p)
        for p in plans.values():
            p.close()


def test_analyzers_vs_reference_golden(native, g16):
    from viewport_entropy_toolkit import SpatialEntropyAnalyzer
    from viewport_entropy_toolkit.config import AnalyzerConfig, EntropyConfig
    mu, mv = g16["mu"], g16["mv"]
    times = np.arange(300) * 0.1
    names = [f"viewer{u}" for u in range(8)]
    ans = {}
    for tag, flag, tcs, w, s in g16_cases(g16):
        if (tcs, flag) not in ans:
            an = (naive_analyzer(flag) if tcs is None else
                  SpatialEntropyAnalyzer(AnalyzerConfig(tile_counts=list(tcs), entropy_config=EntropyConfig(use_weight_distribution=flag))))
            an.load_arrays(times, mu, mv, user_names=names)
            ans[(tcs, flag)] = an
        df = ans[(tcs, flag)].compute_user_entropy(None if w == 300 else w, s)
        R = uo.n_rows(300, w, s)
        assert list(df.columns) == ["user", "time", "time_end", "entropy", "samples"] + ([] if tcs is None else ["tile_weights"])
        assert len(df) == 8 * R and list(df["user"]) == [n for n in names for _ in range(R)]
        assert np.array_equal(df["time"], np.tile(times[np.arange(R) * s], 8))
        assert np.array_equal(df["time_end"], np.tile(times[np.arange(R) * s + w - 1], 8))
        res = dict(entropy=df["entropy"].to_numpy().reshape(8, R), samples=df["samples"].to_numpy().reshape(8, R))
        check_g16(g16, tag, res, tag + " analyzer")
        if tcs is not None:
            tiles = ans[(tcs, flag)]._fibonacci_vectors[tcs[0]]
            rows = g16[f"{tag}__rows"]
            u, i = 5, len(rows) // 2
            cell = df["tile_weights"][u * R + int(rows[i])]
            assert set(cell) == {tiles[t] for t in np.flatnonzero(g16[f"{tag}__keys"][u, i])}, tag


# ------------------------------------------------------------------------------------------- the transpose's edge tiles
@pytest.mark.parametrize("U,T", [(1, 1), (1, 65), (63, 64), (64, 63), (65, 129), (130, 67)])
def test_transpose_edges(native, engine, U, T):
    """window = 1 reads the transposed ids back sample by sample: the one-sample entropy of a weighted plan, and on an unweighted
    plan exactly one 1.0 at the sample's nearest tile (nothing for an absent sample)."""
    rng = np.random.default_rng(1000 * U + T)
    mu, mv = rng.random((T, U)), rng.random((T, U))
    absent = rng.random((T, U)) < 0.15
    mu[absent] = np.nan
    mv[absent] = np.nan
    ids, flat = uo.direction_ids(mu, mv, W, H)
    ids = ids.astype(np.int32)
    tiles = vo.fibonacci_lattice(50)
    near = np.where(ids >= 0, vo.nearest_tile(flat[np.maximum(ids, 0).reshape(-1)], tiles).reshape(T, U), -1)
    onehot = (near.T[:, :, None] == np.arange(len(tiles))[None, None, :]).astype(np.float64)       # [U][T][n]
    pw, pu = fib_plan(native, engine, [50], True), fib_plan(native, engine, [50], False)
    ent, samples, weights = uo.fast(mu, mv, W, H, [50], 1, 1)
    for kw in (dict(mu=mu, mv=mv), dict(ids=ids)):
        a = pw.spatial_per_user(window=1, want_weights=True, **kw)
        assert a["entropy"].shape == (U, T) and np.array_equal(a["samples"], (~absent).T.astype(np.int32))
        close(a["entropy"], ent, f"U{U} T{T} weighted")
        check_weights(a["weights"], weights, samples)
        b = pu.spatial_per_user(window=1, want_weights=True, **kw)
        assert np.array_equal(b["weights"], onehot), (U, T)
        assert np.array_equal(b["samples"], (~absent).T.astype(np.int32)) and np.isnan(b["entropy"]).all()   # one sample: 0 / 0
    pw.close()
    pu.close()


# ------------------------------------------------------------------------------------------- trusted device code
def test_whole_video_rows_equal_the_per_frame_call_on_transposed_ids(native, engine):
    """Frames as "users": Plan.spatial(ids=ids.T) under set_fp64 is the same statistic by independent device code."""
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(37, 500, base_seed=12, p_absent=0.1)
    mu[:, 4], mv[:, 4] = np.nan, np.nan                            # a viewer who never shows up
    ids = ids_of(mu, mv)
    for tcs in ([50], [50, 100, 200]):
        plan, fp = fib_plan(native, engine, tcs, True), fib_plan(native, engine, tcs, True)
        fp.set_fp64(True)
        fp.set_table_policy(1)
        a = plan.spatial_per_user(ids=ids, want_weights=True)
        b = fp.spatial(ids=ids.T, want_assign=False, want_weights=True, check=False)
        assert a["entropy"].shape == (37, 1) and np.isnan(a["entropy"][4, 0]) and a["samples"][4, 0] == 0
        np.testing.assert_allclose(a["entropy"][:, 0], b["entropy"], rtol=1e-12, atol=0, equal_nan=True)
        assert np.array_equal(a["samples"][:, 0], b["present"])
        assert np.array_equal(uo.keys_of(a["weights"][:, 0]), uo.keys_of(b["weights"]))
        np.testing.assert_allclose(a["weights"][:, 0], b["weights"], rtol=1e-12, atol=0)
        plan.close()
        fp.close()


# ------------------------------------------------------------------------------------------- purity
@pytest.mark.parametrize("kind", ["weighted", "weighted3", "unweighted", "naive"])
def test_rows_are_pure_functions_of_their_own_samples(native, engine, kind):
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(9, 150, base_seed=7, p_absent=0.1)
    mu[40:75, 2], mv[40:75, 2] = np.nan, np.nan
    ids = ids_of(mu, mv)
    plan = (naive_analyzer(False)._naive_plan() if kind == "naive" else
            fib_plan(native, engine, [50, 100, 200] if kind == "weighted3" else [50], kind != "unweighted"))
    ww = kind != "naive"

    def same(x, y, msg):
        assert x["entropy"].tobytes() == y["entropy"].tobytes(), msg
        assert np.array_equal(x["samples"], y["samples"]), msg
        if ww:
            assert x["weights"].tobytes() == y["weights"].tobytes(), msg

    a = plan.spatial_per_user(mu=mu, mv=mv, window=20, stride=7, want_weights=ww)
    same(a, plan.spatial_per_user(mu=mu, mv=mv, window=20, stride=7, want_weights=ww), "run to run")
    one = plan.spatial_per_user(mu=mu, mv=mv, window=20, stride=1, want_weights=ww)
    pick = {k: (v[:, ::7] if v is not None and k != "code" else v) for k, v in one.items()}
    same(a, pick, "the rows of the same frames at stride 1")
    if kind != "naive":
        same(a, plan.spatial_per_user(ids=ids, window=20, stride=7, want_weights=ww), "ids entry")
    for r in (0, 5, 7, a["entropy"].shape[1] - 1):                 # a call that holds only the row's 20 frames
        cut = plan.spatial_per_user(mu=mu[7 * r:7 * r + 20], mv=mv[7 * r:7 * r + 20], window=20, want_weights=ww)
        same({k: (v[:, r:r + 1] if v is not None and k != "code" else v) for k, v in a.items()}, cut, f"row {r} alone")
    solo = plan.spatial_per_user(mu=mu[:, 3:4], mv=mv[:, 3:4], window=20, stride=7, want_weights=ww)    # whichever other users
    same({k: (v[3:4] if v is not None and k != "code" else v) for k, v in a.items()}, solo, "user 3 alone")
    if kind != "naive":
        plan.close()


# ------------------------------------------------------------------------------------------- wave split of the weighted kernel
def test_wave_split_windows(native, engine):
    """Windows of 63, 64, 65, 257 and 1000 frames: 1, 1, 2, 4 and 4 waves per row, ragged last chunks."""
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(3, 1000, base_seed=31, p_absent=0.1)
    plan, plan2 = fib_plan(native, engine, [50], True), fib_plan(native, engine, [100, 200], True)
    for window in (63, 64, 65, 257, 1000):
        a = plan.spatial_per_user(mu=mu, mv=mv, window=window, stride=1, want_weights=True)
        ent, samples, weights = uo.fast(mu, mv, W, H, [50], window, 1)
        assert np.array_equal(a["samples"], samples)
        close(a["entropy"], ent, f"w{window}")
        check_weights(a["weights"], weights, samples, 2.0, f"w{window}")
        b = plan2.spatial_per_user(mu=mu, mv=mv, window=window, stride=53, want_weights=True)
        ent, samples, weights = uo.fast(mu, mv, W, H, [100, 200], window, 53)
        close(b["entropy"], ent, f"two lattices w{window}")
        check_weights(b["weights"], weights, samples, 2.0, f"two lattices w{window}")
    plan.close()
    plan2.close()


# ------------------------------------------------------------------------------------------- the counting kernel's slide
@pytest.mark.parametrize("kind", ["unweighted", "naive_u", "naive_w"])
def test_counting_kernel_slide(native, engine, kind):
    """T = 200, window 20: stride 1 and 7 (add and subtract; stride 1 gives a wave a run of several rows), stride = window and
    stride > window (every row counted afresh).  20 samples <= n: use_weight_distribution=False normalises by log2(samples)."""
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(64, 200, base_seed=77, p_absent=0.1)
    mu[30:90, 10], mv[30:90, 10] = np.nan, np.nan
    plan = fib_plan(native, engine, [50], False) if kind == "unweighted" else naive_analyzer(kind == "naive_w")._naive_plan()
    for stride in (1, 7, 20, 27):
        a = plan.spatial_per_user(mu=mu, mv=mv, window=20, stride=stride, want_weights=kind == "unweighted")
        if kind == "unweighted":
            ent, samples, weights = uo.fast(mu, mv, W, H, [50], 20, stride, use_weight_distribution=False)
            assert np.array_equal(a["weights"], weights), stride            # integer counts: exact
        else:
            ent, samples = uo.naive(mu, mv, W, H, 10, 20, 20, stride, use_weight_distribution=kind == "naive_w")
        assert np.array_equal(a["samples"], samples), stride
        close(a["entropy"], ent, f"{kind} s{stride}")
        assert (samples == 0).any()
    if kind == "unweighted":
        plan.close()


# ------------------------------------------------------------------------------------------- quirks
def test_quirks(native, engine, golden_dir):
    mu = np.full((40, 2), np.nan)
    mv = np.full((40, 2), np.nan)
    mu[7, 0], mv[7, 0] = 0.3, 0.4                                   # one sample in the whole video
    mu[:, 1], mv[:, 1] = np.linspace(0.1, 0.9, 40), 0.5
    pu = fib_plan(native, engine, [50], False)
    a = pu.spatial_per_user(mu=mu, mv=mv)
    assert a["samples"][:, 0].tolist() == [1, 40] and np.isnan(a["entropy"][0, 0])       # 0 / 0, as the reference
    ent, _, _ = uo.fast(mu, mv, W, H, [50], 40, 1, use_weight_distribution=False)
    close(a["entropy"], ent, "log2(samples) normaliser")                                # 40 samples <= 51 tiles
    bad = mu.copy()
    bad[3, 1] = 1.5
    r = pu.spatial_per_user(mu=bad, mv=mv, check=False)
    assert r["code"] == native.VET_ERR_RANGE and r["samples"][:, 0].tolist() == [1, 39]  # outputs still written
    with pytest.raises(native.NativeError):
        pu.spatial_per_user(mu=bad, mv=mv)
    for window, stride in ((0, 1), (4, 0), (41, 1), (-1, 1)):
        with pytest.raises(ValueError):
            pu.spatial_per_user(mu=mu, mv=mv, window=window, stride=stride)
        e = np.zeros(8)
        rc = pu.lib.vet_user_entropy_host(pu.handle, native._ptr(mu), native._ptr(mv), None, 2, 40, window, stride, native._ptr(e), None, None)
        assert rc == native.VET_ERR_INVALID and pu.lib.vet_last_error()
    pu.close()
    # golden G12's configuration (power factor 150: in-FoV weights underflow to 0.0 and stay keys): its NaN on a pooled row
    g = np.load(golden_dir / "g12_underflow.npz")
    px, py = g["px"], g["py"]
    present = px >= 0
    gm = np.where(present, np.where(px == W, 1.0, (px + 0.5) / W), np.nan)
    gv = np.where(present, np.where(py == H, 1.0, (py + 0.5) / H), np.nan)
    T = len(gm)
    window = min(T, 5)
    plan = fib_plan(native, engine, [500], True, 120.0, 150.0)
    res = plan.spatial_per_user(mu=gm, mv=gv, window=window, stride=window, want_weights=True)
    ent, samples, weights = uo.fast(gm, gv, W, H, [500], window, window, fov_angle=120.0, power_factor=150.0)
    assert np.isnan(ent[samples > 0]).any(), "the configuration no longer produces the reference's NaN on a pooled row"
    close(res["entropy"], ent, "G12 pooled")
    check_weights(res["weights"], weights, samples, 150.0)
    plan.close()
