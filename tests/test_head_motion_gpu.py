"""GPU: head-motion statistics through the C-ABI (Plan.head_motion -> vet_head_motion_host, the device entries through
Plan.head_motion_device, the analyzers' compute_head_motion).  Pair f is (frame f, frame f + lag); a (pair, viewer) present in both
frames is a sample, its angle the reference's vector_angle_distance, +0.0 where the two Vectors are the same.  The references are
golden G25 (the real reference's angles, tools/gen_golden_motion.py) and the numpy oracle of tests/_motion_oracle.py (pinned against
G25 and G13 in tests/test_head_motion_surface.py) — never the code under test.

``samples``, ``still`` and ``hist`` are compared for equality; for ``hist`` the test asserts on the ORACLE's angles that none lies
within 1e-9 relative of an edge, so a last-bit difference of an angle cannot move a count.

Tolerance of ``stats`` and ``quantiles``, derived, not measured: tests/_tol.py's W_RTOL = 1e-9 relative plus 4e-16 absolute (the ulp
of arccos), NaN equal to NaN.  At the 100 x 200 grid the smallest non-zero angle is about 1e-3 rad (two pixels next to the pole row).
The oracle evaluates the definition's fused dot with one rounding per fma (exact integer arithmetic), so the angles differ by the
two arccos implementations only: an ulp or two of the angle, 4e-16 relative.  (A dot that is off by one rounding of 1.1e-16 would
move an angle of 1e-3 rad by 1.1e-16 / sin(1e-3) = 1.1e-13 rad, 1.1e-10 relative — and the sd of a row whose two angles differ by
2e-7 rad by 8e-9 relative, beyond the bound: the sd of nearly equal angles is as ill-conditioned as their difference.)  The
sums add non-negative terms with at most W / 256 + 16 sequential roundings, 2e-13 relative at W = 66 000.  Order statistics and the
maximum are 1-Lipschitz in the values, so the same bound holds for them.  The test prints the largest error it saw."""
import numpy as np
import pytest

from tests import _motion_oracle as mo
from tests._tol import W_RTOL

pytestmark = pytest.mark.gpu

W, H = 100, 200
ATOL = 4e-16
FRACTIONS = (0.0, 0.25, 0.5, 0.9, 0.99, 1.0)
EDGES = np.array([0.0, 5e-4, 0.01, 0.03, 0.07, 0.15, 0.4, 1.0, 2.5])       # radians; edge 0 = 0.0 takes the still samples
KEYS = ("stats", "quantiles", "hist", "still", "samples")


@pytest.fixture(scope="module")
def native():
    from viewport_entropy_toolkit import _native
    return _native


@pytest.fixture(scope="module")
def engine(native):
    return native.Engine.default()


@pytest.fixture(scope="module")
def plan(native, engine):
    from oracle import vet_oracle as vo
    p = native.Plan(engine, [vo.fibonacci_lattice(50)], 120.0, 2.0, True, W, H)
    yield p
    p.close()


@pytest.fixture(scope="module")
def table(plan):
    """the plan's own direction table: the Vectors the oracle works on"""
    t = plan.read_dirs()
    assert np.array_equal(t, mo.grid_table(W, H))
    return t


def walk(U, T, p_absent, seed):
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(U, T, base_seed=seed, p_absent=p_absent)
    if p_absent:
        mu[8:31] = np.nan              # frames 8-30 without anybody: windows of up to 20 pairs fall inside
        mv[8:31] = np.nan
    return mu, mv


def clear_of_edges(ang, edges=EDGES):
    """the CPU-checked condition on the inputs: no oracle angle within 1e-9 relative of an edge"""
    v = ang[~np.isnan(ang)]
    if ((v > 0) & (v < 1e-12)).any():                            # edge 0 = 0.0: a value is exactly 0 or far from it
        return False
    return all((np.abs(v - e) > 1e-9 * e).all() for e in edges if e > 0)


def close(got, want, msg):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (msg, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), msg
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - want) / np.where(want == 0, 1.0, np.abs(want))
    print(msg, "max rel err", float(np.nanmax(err, initial=0.0)))
    np.testing.assert_allclose(got, want, rtol=W_RTOL, atol=ATOL, equal_nan=True, err_msg=msg)


def kept(R):
    return np.unique([0, R // 2, max(R - 2, 0), R - 1])


def check(res, ang, window, stride, per_user, msg, fractions=FRACTIONS, edges=EDGES):
    """a result dict against the oracle: the integers of every row, the FP outputs of the kept rows (and viewers)"""
    P, U = ang.shape
    w = P if window is None else window
    R = (P - w) // stride + 1
    lead = (U, R) if per_user else (R,)
    assert res["code"] == 0 and res["stats"].shape == (4,) + lead and res["samples"].shape == lead, msg
    samples, still = mo.counts(ang, w, stride, per_user)
    assert np.array_equal(res["samples"], samples) and np.array_equal(res["still"], still), msg
    assert res["samples"].dtype == res["still"].dtype == np.int32
    empty = samples == 0
    assert np.isnan(res["stats"][:, empty]).all() and not np.isnan(res["stats"][[0, 2, 3]][:, ~empty]).any(), msg
    assert np.array_equal(np.isnan(res["stats"][1]), samples <= 1), msg            # sd: NaN for N <= 1 only
    rows, users = kept(R), (np.unique([0, 1, U // 2, U - 2, U - 1]) if U > 8 else np.arange(U))
    want = mo.rows(ang, w, stride, per_user, fractions, edges, only=rows, users=users)
    close(res["stats"][:, users][:, :, rows] if per_user else res["stats"][:, rows], want["stats"], msg + " stats")
    if res["quantiles"] is not None:
        q = res["quantiles"][users][:, rows] if per_user else res["quantiles"][rows]
        close(q, want["quantiles"], msg + " quantiles")
        if 1.0 in fractions:                                     # q = 1 is the maximum, bit for bit, on every row
            assert res["quantiles"][..., list(fractions).index(1.0)].tobytes() == res["stats"][2].tobytes(), msg
        if 0.0 in fractions:
            assert (res["quantiles"][..., list(fractions).index(0.0)][still > 0] == 0.0).all(), msg
    if res["hist"] is not None:
        h = res["hist"][users][:, rows] if per_user else res["hist"][rows]
        assert res["hist"].dtype == np.int32 and np.array_equal(h, want["hist"]), msg
        assert (res["hist"].sum(axis=-1) <= samples).all() and np.array_equal(res["hist"][..., 0] >= still, np.ones(lead, bool)), msg
    return samples, still


def same_bytes(a, b, msg, keys=KEYS):
    for key in keys:
        if a[key] is None or b[key] is None:
            continue
        assert a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), (msg, key)


# ------------------------------------------------------------------------------------------- the reference's angles (golden G25)
def test_vs_golden_angles(plan, golden_dir):
    """window = 1 per viewer: row (u, f) holds one sample, whose ``total`` is the angle itself."""
    g = np.load(golden_dir / "g25_head_motion.npz")
    g15 = np.load(golden_dir / "g15_windowed_transition.npz")
    mu, mv = g15["mu"], g15["mv"]
    ids = mo.ids_of(mu, mv, W, H)
    for lag in (1, 3):
        want, same = g[f"angles_l{lag}"].T, g[f"same_l{lag}"].T
        for kw in (dict(mu=mu, mv=mv), dict(ids=ids)):
            res = plan.head_motion(window=1, lag=lag, per_user=True, quantiles=(0.5,), **kw)
            got = res["stats"][3]
            assert got.shape == want.shape == (8, 60 - lag)
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(res["samples"], ~np.isnan(want))
            moved = ~same & ~np.isnan(want)
            close(got[moved], want[moved], f"G25 lag {lag}")
            assert (got[same] == 0.0).all() and not np.signbit(got[same]).any()         # the stated departure: still is +0.0
            assert np.array_equal(res["still"], same.astype(np.int32))
            for k in (0, 2):                                     # one sample: mean = max = total = the quantile
                assert res["stats"][k].tobytes() == got.tobytes() and res["quantiles"][..., 0].tobytes() == got.tobytes()


# ------------------------------------------------------------------------------------------- the numpy oracle, seeded walks
@pytest.mark.parametrize("p_absent", [0.0, 0.3], ids=["full", "absent"])
@pytest.mark.parametrize("U,T", [(1, 40), (7, 60), (64, 60), (65, 130), (512, 40)])
def test_vs_oracle(plan, table, U, T, p_absent):
    mu, mv = walk(U, T, p_absent, 900 + U)
    ids = mo.ids_of(mu, mv, W, H)
    kinds = set()
    for lag in (1, 3, T - 1):
        ang, _ = mo.angles(table, ids, lag)
        assert clear_of_edges(ang)
        P = T - lag
        for window in (1, 2, 20, None):
            w = P if window is None else window
            if w > P:
                continue
            for stride in sorted({1, 7, w}):
                for per_user in (False, True):
                    msg = f"U={U} T={T} absent={p_absent} window={window} stride={stride} lag={lag} per_user={per_user}"
                    kw = dict(ids=ids) if (stride == 7) else dict(mu=mu, mv=mv)       # both entries
                    res = plan.head_motion(window=window, stride=stride, lag=lag, per_user=per_user, quantiles=FRACTIONS,
                                           edges=EDGES, **kw)
                    N, still = check(res, ang, window, stride, per_user, msg)
                    kinds |= {"empty"} if (N == 0).any() else set()
                    kinds |= {"one"} if (N == 1).any() else set()
                    kinds |= {"still"} if ((N > 1) & (still == N)).any() else set()
                    kinds |= {"many"} if (N > 1024).any() else set()
    assert "one" in kinds
    if p_absent:
        assert "empty" in kinds
    if U >= 64 and not p_absent:
        assert "many" in kinds


# ------------------------------------------------------------------------------------------- edge rows
def edge_video(T=200):
    """ids [T][8]: 0 parked on one pixel; 1 parked on the pole row, wandering along it (ids differ, one Vector); 2 still but for a
    few moves; 3 absent but for two frames a lag apart (N = 1 rows); 4 never there; 5-7 a walk"""
    rng = np.random.default_rng(5)
    ids = np.full((T, 8), -1, dtype=np.int32)
    ids[:, 0] = 77 * (W + 1) + 31
    ids[:, 1] = rng.integers(0, W + 1, T)                          # py = 0: every pixel of the row is the pole
    ids[:, 2] = 120 * (W + 1) + 50
    ids[[40, 41, 90, 150], 2] += [1, 2, W + 1, 3]
    ids[[60, 61], 3] = [100 * (W + 1) + 10, 100 * (W + 1) + 12]
    mu, mv = walk(3, T, 0.0, 77)
    ids[:, 5:] = mo.ids_of(mu, mv, W, H)
    return ids


@pytest.mark.parametrize("lds_values", [0, 1024], ids=["default", "chunked"])
def test_edge_rows(engine, plan, table, lds_values):
    ids = edge_video()
    ang, same = mo.angles(table, ids, 1)
    assert same[:, 1].all() and (ids[1:, 1] != ids[:-1, 1]).any() and (ang[:, 1] == 0).all()     # the pole row: still
    assert clear_of_edges(ang)
    engine.test_motion_lds_values(lds_values)
    try:
        for window, stride in ((None, 1), (20, 7), (1, 1)):
            res = plan.head_motion(ids=ids, window=window, stride=stride, per_user=True, quantiles=FRACTIONS, edges=EDGES)
            N, still = check(res, ang, window, stride, True, f"edge rows per viewer window={window}")
            for u in (0, 1):                                     # all-still rows: +0.0 exactly
                assert (still[u] == N[u]).all() and (N[u] > 0).all()
                block = np.concatenate([res["stats"][:, u].ravel(), res["quantiles"][u].ravel()]) if window != 1 else \
                    np.concatenate([res["stats"][[0, 2, 3], u].ravel(), res["quantiles"][u].ravel()])
                assert (block == 0.0).all() and not np.signbit(block).any()
                assert (res["hist"][u, :, 0] == N[u]).all() and (res["hist"][u, :, 1:] == 0).all()
            assert (N[4] == 0).all() and np.isnan(res["stats"][:, 4]).all() and np.isnan(res["quantiles"][4]).all()
            assert (res["hist"][4] == 0).all() and (still[4] == 0).all()
            if window is None:                                   # mostly zeros with a few moves: quantiles inside the run of ties
                assert N[2, 0] == 199 and still[2, 0] == 192             # seven pairs touch a moved frame
                assert (res["quantiles"][2, 0, :4] == 0.0).all() and res["quantiles"][2, 0, 5] > 0
                assert N[3, 0] == 1 and np.isnan(res["stats"][1, 3, 0]) and res["stats"][0, 3, 0] == res["stats"][2, 3, 0] > 0
        # pooled over the eight viewers: W = 199 * 8 = 1592 values, beyond 1024
        res = plan.head_motion(ids=ids, window=None, quantiles=FRACTIONS, edges=EDGES)
        check(res, ang, None, 1, False, "edge rows pooled")
        status = plan.head_motion(ids=ids[:, 4:5], window=10, stride=10)
        assert (status["samples"] == 0).all() and status["code"] == 0                  # rows without a sample are data
    finally:
        engine.test_motion_lds_values(0)


# ------------------------------------------------------------------------------------------- bit invariance
def test_bits_do_not_depend_on_stride_length_or_outputs(engine, plan):
    mu_long, mv_long = walk(65, 130, 0.3, 31)
    mu, mv = mu_long[:60], mv_long[:60]
    for per_user in (False, True):
        for lag in (1, 3):
            kw = dict(window=20, lag=lag, per_user=per_user, quantiles=FRACTIONS, edges=EDGES)
            s1 = plan.head_motion(mu=mu, mv=mv, stride=1, **kw)
            s7 = plan.head_motion(mu=mu, mv=mv, stride=7, **kw)
            R7 = s7["samples"].shape[-1]
            for key in KEYS:                                     # stride 1 against stride 7 on the shared rows
                a = s1[key][..., ::7, :][..., :R7, :] if key in ("quantiles", "hist") else s1[key][..., ::7][..., :R7]
                assert np.ascontiguousarray(a).tobytes() == s7[key].tobytes(), (per_user, lag, key)
            long = plan.head_motion(mu=mu_long, mv=mv_long, stride=1, **kw)     # a short video against the prefix of a long one
            R1 = s1["samples"].shape[-1]
            for key in KEYS:
                a = long[key][..., :R1, :] if key in ("quantiles", "hist") else long[key][..., :R1]
                assert np.ascontiguousarray(a).tobytes() == s1[key].tobytes(), (per_user, lag, key)
            whole = plan.head_motion(mu=mu, mv=mv, window=None, lag=lag, per_user=per_user, quantiles=FRACTIONS, edges=EDGES)
            same_bytes(whole, plan.head_motion(mu=mu, mv=mv, window=60 - lag, lag=lag, per_user=per_user, quantiles=FRACTIONS,
                                               edges=EDGES), "window=None is window = P")
            # with and without the optional outputs; one fraction against eight
            bare = plan.head_motion(mu=mu, mv=mv, window=20, stride=7, lag=lag, per_user=per_user, quantiles=None)
            assert bare["quantiles"] is None and bare["hist"] is None
            same_bytes(bare, s7, "optional outputs")
            eight = plan.head_motion(mu=mu, mv=mv, window=20, stride=7, lag=lag, per_user=per_user,
                                     quantiles=(0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 1.0))
            one = plan.head_motion(mu=mu, mv=mv, window=20, stride=7, lag=lag, per_user=per_user, quantiles=(0.9,))
            assert eight["quantiles"][..., 5].tobytes() == np.ascontiguousarray(one["quantiles"][..., 0]).tobytes()
            assert s7["quantiles"][..., 3].tobytes() == np.ascontiguousarray(one["quantiles"][..., 0]).tobytes()
            same_bytes(one, s7, "one fraction", keys=("stats", "still", "samples"))


@pytest.mark.parametrize("U,T", [(512, 40), (65, 60)])
def test_lds_bound_does_not_change_a_bit(engine, plan, table, U, T):
    """vet_test_motion_lds_values(1024): 512 x 20 = 10240 and 65 x 20 = 1300 values per row take the chunked shape (the radix
    selection), the whole video too; the default runs them in one workgroup (the LDS sort)."""
    mu, mv = walk(U, T, 0.3, 50 + U)
    ids = mo.ids_of(mu, mv, W, H)
    ang, _ = mo.angles(table, ids, 1)
    assert clear_of_edges(ang)
    shapes = ((20, 7, False), (20, 1, False), (None, 1, False), (None, 1, True))
    default = [plan.head_motion(mu=mu, mv=mv, window=w, stride=s, per_user=pu, quantiles=FRACTIONS, edges=EDGES) for w, s, pu in shapes]
    engine.test_motion_lds_values(1024)
    try:
        for (w, s, pu), ref in zip(shapes, default):
            res = plan.head_motion(mu=mu, mv=mv, window=w, stride=s, per_user=pu, quantiles=FRACTIONS, edges=EDGES)
            same_bytes(res, ref, f"lds bound 1024: window={w} stride={s} per_user={pu}")
            if not pu:
                check(res, ang, w, s, pu, f"chunked U={U} window={w} stride={s}")
            bare = plan.head_motion(ids=ids, window=w, stride=s, per_user=pu, quantiles=(0.9,))
            same_bytes(bare, ref, "chunked, ids, one fraction", keys=("stats", "still", "samples"))
            assert bare["quantiles"][..., 0].tobytes() == np.ascontiguousarray(ref["quantiles"][..., 3]).tobytes()
    finally:
        engine.test_motion_lds_values(0)


def test_device_entries_give_the_host_bytes(engine, plan):
    import torch
    mu, mv = walk(64, 60, 0.3, 23)
    ids = mo.ids_of(mu, mv, W, H)
    U, T, window, stride, lag = 64, 60, 20, 3, 3
    dev = torch.device("cuda", 0)
    d_mu, d_mv, d_ids = (torch.from_numpy(a).to(dev) for a in (mu, mv, ids))
    for per_user in (False, True):
        host = plan.head_motion(mu=mu, mv=mv, window=window, stride=stride, lag=lag, per_user=per_user, quantiles=FRACTIONS,
                                edges=EDGES)
        rows = host["samples"].size
        for src in ("mu_mv", "ids"):
            stats = torch.full((4, rows), -7.0, dtype=torch.float64, device=dev)
            quant = torch.full((rows, len(FRACTIONS)), -7.0, dtype=torch.float64, device=dev)
            hist = torch.full((rows, len(EDGES) - 1), -7, dtype=torch.int32, device=dev)
            still = torch.full((rows,), -7, dtype=torch.int32, device=dev)
            samples = torch.full((rows,), -7, dtype=torch.int32, device=dev)
            status = torch.zeros(2, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            plan.head_motion_device(d_mu.data_ptr(), d_mv.data_ptr(), U, T, window, stride, lag, per_user, FRACTIONS, EDGES,
                                    stats.data_ptr(), quant.data_ptr(), hist.data_ptr(), still.data_ptr(), samples.data_ptr(),
                                    status.data_ptr(), **(dict(d_ids=d_ids.data_ptr()) if src == "ids" else {}))
            engine.synchronize()
            got = dict(stats=stats, quantiles=quant, hist=hist, still=still, samples=samples)
            for key in KEYS:
                assert got[key].cpu().numpy().tobytes() == host[key].tobytes(), (per_user, src, key)
            assert status.cpu().numpy().tolist() == [0, int((host["samples"] == 0).sum())]


def test_per_viewer_rows_against_the_pooled_call_on_one_viewer(plan):
    mu, mv = walk(7, 60, 0.3, 61)
    for window, stride, lag in ((20, 7, 1), (None, 1, 3), (2, 1, 1)):
        per = plan.head_motion(mu=mu, mv=mv, window=window, stride=stride, lag=lag, per_user=True, quantiles=FRACTIONS, edges=EDGES)
        for u in range(7):
            alone = plan.head_motion(mu=mu[:, u:u + 1], mv=mv[:, u:u + 1], window=window, stride=stride, lag=lag,
                                     quantiles=FRACTIONS, edges=EDGES)
            assert np.array_equal(alone["samples"], per["samples"][u]) and np.array_equal(alone["still"], per["still"][u])
            assert np.array_equal(alone["hist"], per["hist"][u])
            close(per["stats"][:, u], alone["stats"], f"viewer {u} stats")
            close(per["quantiles"][u], alone["quantiles"], f"viewer {u} quantiles")


# ------------------------------------------------------------------------------------------- refusals, range, the analyzers
def test_illegal_arguments_are_refused_before_anything_runs(native, plan):
    mu, mv = walk(4, 30, 0.0, 33)
    lib = native.load_library()
    stats = np.empty((4, 64))
    f, e = np.array([0.5, 0.9]), np.array([0.0, 0.1, 0.2])
    good = dict(window=5, stride=1, lag=1, Q=2, B=2, f=f, e=e)
    bad = [dict(lag=0), dict(lag=30), dict(window=0), dict(window=30), dict(window=28, lag=3), dict(stride=0), dict(Q=9),
           dict(f=np.array([0.9, 0.5])), dict(f=np.array([0.5, 1.5])), dict(f=np.array([0.5, 0.5])), dict(B=65),
           dict(e=np.array([0.0, 0.2, 0.1])), dict(e=np.array([0.0, 0.1, 0.1]))]
    for change in bad:
        a = dict(good, **change)
        rc = lib.vet_head_motion_host(plan.handle, native._ptr(mu), native._ptr(mv), None, 4, 30, a["window"], a["stride"], a["lag"], 0,
                                      native._ptr(a["f"]), a["Q"], native._ptr(a["e"]), a["B"], native._ptr(stats), None, None, None,
                                      None)
        assert rc == native.VET_ERR_INVALID, change
    with pytest.raises(native.NativeError) as err:                # the device entry refuses before it looks at a pointer
        plan.head_motion_device(8, 8, 4, 30, 5, 1, 30, False, None, None, 8)
    assert err.value.code == native.VET_ERR_INVALID
    with pytest.raises(native.NativeError) as err:                # window * n_users above 2^31 - 1
        plan.head_motion_device(8, 8, 1 << 20, 4097, 4096, 1, 1, False, None, None, 8)
    assert err.value.code == native.VET_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        plan.head_motion(mu=mu, mv=mv, window=30)
    assert plan.head_motion(mu=mu, mv=mv, window=1, lag=29)["stats"].shape == (4, 1)


def test_sample_out_of_range(native, plan):
    mu, mv = walk(7, 40, 0.0, 41)
    bad_mu, gone_mu, gone_mv = mu.copy(), mu.copy(), mv.copy()
    bad_mu[39, 3] = 1.5                                           # the last frame: the later frame of a pair only
    gone_mu[39, 3] = gone_mv[39, 3] = np.nan
    with pytest.raises(native.NativeError) as e:
        plan.head_motion(mu=bad_mu, mv=mv, window=5)
    assert e.value.code == native.VET_ERR_RANGE
    for per_user in (False, True):
        res = plan.head_motion(mu=bad_mu, mv=mv, window=5, per_user=per_user, check=False)
        assert res["code"] == native.VET_ERR_RANGE                # the outputs are still written: the sample counts as absent
        same_bytes(res, plan.head_motion(mu=gone_mu, mv=gone_mv, window=5, per_user=per_user), "range")


def test_analyzers_return_degrees(plan, table):
    from viewport_entropy_toolkit import SpatialEntropyAnalyzer, TransitionEntropyAnalyzer
    from viewport_entropy_toolkit.config import AnalyzerConfig
    mu, mv = walk(7, 60, 0.3, 71)
    times = np.arange(60) / 30.0
    ang, _ = mo.angles(table, mo.ids_of(mu, mv, W, H), 3)
    bins = (0.0, 0.5, 2.0, 10.0, 180.0)
    frames = []
    for cls in (SpatialEntropyAnalyzer, TransitionEntropyAnalyzer):
        an = cls(AnalyzerConfig(tile_counts=[20], video_width=W, video_height=H))
        an.load_arrays(times, mu, mv)
        frames.append(an.compute_head_motion(window=20, stride=7, lag=3, quantiles=(0.5, 0.9), bins_deg=bins))
        per = an.compute_head_motion(window=20, stride=7, lag=3, per_user=True, quantiles=(0.5,))
        assert list(per.columns)[0] == "user" and len(per) == 7 * len(frames[-1]) and "hist" not in per.columns
    df = frames[0]
    for c in df.columns:                                         # the call is lattice-independent: both analyzers, the same values
        a, b = (np.stack(list(f[c])) if c in ("quantiles", "hist") else f[c].to_numpy() for f in frames)
        assert a.tobytes() == b.tobytes(), c
    want = mo.rows(ang, 20, 7, False, (0.5, 0.9), np.radians(bins))
    close(np.array([df["mean"], df["sd"], df["max"], df["total"]]), np.degrees(want["stats"]), "analyzer stats in degrees")
    close(np.stack(list(df["quantiles"])), np.degrees(want["quantiles"]), "analyzer quantiles in degrees")
    assert np.array_equal(df["samples"], want["samples"]) and np.array_equal(df["still"], want["still"])
    assert df.attrs["lag"] == 3 and df.attrs["bins_deg"] == bins and abs(df.attrs["pair_seconds"] - 0.1) < 1e-12
    assert df["time"].tolist() == times[3::7][:len(df)].tolist()
