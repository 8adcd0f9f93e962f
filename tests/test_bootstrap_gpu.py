"""GPU: bootstrap confidence bands over viewers through the C-ABI (Plan.spatial_bootstrap -> vet_bootstrap_entropy_host, the device
entries, Plan.bootstrap_counts, both analyzers).  Replicate b resamples the viewers with replacement; rep[r][b] is the reference's
entropy of the resampled audience's samples of frames [r * stride, r * stride + window).  The references are golden G21 (the real
reference's dicts, tools/gen_golden_bootstrap.py) and the numpy oracles of tests/_bootstrap_oracle.py (pinned against G21 in
tests/test_bootstrap_surface.py).

Tolerances:
  integer plans (unweighted, naive)   the replicate histograms are sums of small integers, exact in FP64 in any order: ``weights``
                                      array_equal; replicates rtol 1e-9 (the entropy loop's own summation order and log2);
  weighted plans                      replicates at the project's 1e-6 relative contract; ``weights`` within tests/_tol.py (W_RTOL
                                      relative, w_atol per contributing sample: the replicate's sample count);
  summary                             rtol 1e-12 against numpy on the device's own replicates.  sd also gets an absolute floor of
                                      m * 2^-52 * max|x|: the mean of m values carries a relative rounding error of up to
                                      m * 2^-52 under any summation order, every deviation x - mean inherits it absolutely, so
                                      the sd of m EQUAL replicates (a row in which the drawn viewers always reduce to the same
                                      one) is 0 in exact arithmetic and up to that floor in either implementation — a relative
                                      bound alone cannot hold at 0.
Where NaN sits must match exactly.  One oracle per (plan, U, window) — every row at stride 1, 40 replicates — serves every stride
and every B: rows at stride s are the rows r * s of stride 1, and replicate b does not depend on B."""
import ctypes

import numpy as np
import pytest

from oracle import vet_oracle as vo
from tests import _bootstrap_oracle as bo
from tests import _user_oracle as uo
from tests._tol import W_RTOL, w_atol

pytestmark = pytest.mark.gpu

W, H = 100, 200
T = 240
SEED = 2024
B_MAX = 40
WINDOWS = (1, 2, 20, 64, T)
EMPTY = (100, 104)                                      # frames without any viewer


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


@pytest.fixture(scope="module")
def g21(golden_dir):
    return np.load(golden_dir / "g21_bootstrap.npz")


def fib_plan(native, engine, tcs, weighted=True, fov=120.0, power=2.0):
    return native.Plan(engine, [vo.fibonacci_lattice(t) for t in tcs], fov, power, weighted, W, H)


def naive_analyzer(weighted=True):
    from viewport_entropy_toolkit import NaiveSpatialEntropyAnalyzer
    from viewport_entropy_toolkit.config import EntropyConfig, NaiveAnalyzerConfig
    return NaiveSpatialEntropyAnalyzer(NaiveAnalyzerConfig(tile_height=10, tile_width=20, video_width=W, video_height=H,
                                                           entropy_config=EntropyConfig(use_weight_distribution=weighted)))


def strides(window):
    return sorted({1, 3, window, window + 5})


def video(U, seed=0):
    """Random walks, 10 % absences, frames EMPTY without anybody: asymmetric in every direction the lane map could be wrong in."""
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(U, T, base_seed=300 + U + seed, p_absent=0.1)
    mu[EMPTY[0]:EMPTY[1]], mv[EMPTY[0]:EMPTY[1]] = np.nan, np.nan
    return mu, mv


def ids_of(mu, mv):
    return uo.direction_ids(mu, mv, W, H)[0].astype(np.int32)


def close(got, want, rtol, msg):
    with np.errstate(all="ignore"):
        print(msg, "max rel err", float(np.nanmax(np.abs(got - want) / np.maximum(np.abs(want), 1e-300), initial=0.0)))
    assert got.shape == want.shape, msg
    assert np.array_equal(np.isnan(got), np.isnan(want)), (msg, np.argwhere(np.isnan(got) != np.isnan(want))[:10])
    np.testing.assert_allclose(got, want, rtol=rtol, atol=0, equal_nan=True, err_msg=msg)


def check_weights(got, want, samples, power, msg):
    """Plain values: +0.0 = no weight; tolerance per replicate from its sample count."""
    assert got.shape == want.shape, msg
    atol = np.vectorize(lambda n: w_atol(int(n), power))(samples)[..., None]
    err = np.abs(got - want)
    print(msg, "weights max abs err", float(err.max(initial=0.0)))
    bad = err > W_RTOL * np.abs(want) + atol
    assert not bad.any(), (msg, np.argwhere(bad)[:10])
    assert not np.signbit(got).any(), msg


def check_summary(res, confidence, msg):
    """mean, lo, hi at rtol 1e-12; sd at rtol 1e-12 plus the floor of the module docstring."""
    want, valid = bo.summary(res["replicates"], confidence)
    assert np.array_equal(res["valid"], valid), msg
    close(res["summary"][[0, 2, 3]], want[[0, 2, 3]], 1e-12, msg + " summary")
    got_sd, want_sd = res["summary"][1], want[1]
    assert np.array_equal(np.isnan(got_sd), np.isnan(want_sd)), msg
    biggest = np.abs(np.where(np.isfinite(res["replicates"]), res["replicates"], 0.0)).max(axis=1)
    floor = valid * 2.0 ** -52 * biggest
    ok = ~np.isnan(want_sd)
    err = np.abs(np.where(ok, got_sd - want_sd, 0.0))
    print(msg, "sd max abs err", float(err.max(initial=0.0)))
    assert (err <= 1e-12 * np.where(ok, want_sd, 0.0) + floor).all(), (msg, np.flatnonzero(err > 1e-12 * np.where(ok, want_sd, 0.0) + floor)[:10])


# ------------------------------------------------------------------------------------------- the draw
@pytest.mark.parametrize("U", [1, 3, 130, 1024])
def test_counts_equal_the_numpy_draw(native, engine, U):
    plan = fib_plan(native, engine, [20])
    for seed in (0, 0xDEADBEEFCAFEF00D):
        for B in (1, 17, 40):
            got = plan.bootstrap_counts(U, B, seed)
            want, _ = bo.draw(U, B, seed)
            assert got.dtype == np.uint16 and np.array_equal(got, want), (U, B, seed)
    with pytest.raises(native.NativeError):
        plan.bootstrap_counts(65536, 2, 0)
    plan.close()


# ------------------------------------------------------------------------------------------- the shape matrix
def run_matrix(native, plan, U, kind, oracle, exact):
    """Every window; per window every stride at B = 40 and every B at stride 3, weights and summary included.
    ``oracle(mu, mv, window, counts)`` -> (rep[R1][40], weights[R1][40][n0], samples[R1][40]) for the rows of stride 1."""
    mu, mv = video(U)
    counts, _ = bo.draw(U, B_MAX, SEED)
    for window in WINDOWS:
        rep1, w1, n1 = oracle(mu, mv, window, counts)
        if window <= EMPTY[1] - EMPTY[0]:
            assert np.isnan(rep1[EMPTY[0]:EMPTY[1] - window + 1]).all() and not n1[EMPTY[0]:EMPTY[1] - window + 1].any()
        combos = [(s, B_MAX) for s in strides(window)] + [(3, B) for B in (1, 16, 17)]
        for stride, B in combos:
            msg = f"{kind} U{U} w{window} s{stride} B{B}"
            res = plan.spatial_bootstrap(mu=mu, mv=mv, window=window, stride=stride, replicates=B, seed=SEED, confidence=0.9,
                                         want_replicates=True, want_weights=True)
            R = uo.n_rows(T, window, stride)
            pick = np.arange(R) * stride
            assert res["code"] == native.VET_OK and res["replicates"].shape == (R, B) and res["summary"].shape == (4, R), msg
            close(res["replicates"], rep1[pick][:, :B], 1e-9 if exact else 1e-6, msg)
            if exact:
                assert np.array_equal(res["weights"], w1[pick][:, :B]), msg
                assert not np.signbit(res["weights"]).any(), msg
            else:
                check_weights(res["weights"], w1[pick][:, :B], n1[pick][:, :B], 2.0, msg)
            check_summary(res, 0.9, msg)
            if window <= 2 and stride == 1:                          # the empty stretch: rows without a finite replicate (m = 0)
                gone = slice(EMPTY[0], EMPTY[1] - window + 1)
                assert (res["valid"][gone] == 0).all() and np.isnan(res["summary"][:, gone]).all(), msg
            if B == 1:                                               # m = 1: the value itself, no sd
                one = res["valid"] == 1
                # (one unweighted sample is the reference's 0 / 0: with U = 1 and window 1 no replicate is finite)
                assert (one.any() or (kind == "unweighted" and U * window == 1)) and np.isnan(res["summary"][1][one]).all(), msg
                for k in (0, 2, 3):
                    assert np.array_equal(res["summary"][k][one], res["replicates"][one, 0]), msg


@pytest.mark.parametrize("U", [1, 3, 7, 66, 130])
def test_integer_plans_unweighted(native, engine, U):
    """The MFMA lane map on exact data: lattice 0's replicate histograms are the oracle's integers, bit for bit."""
    plan = fib_plan(native, engine, [50], weighted=False)

    def oracle(mu, mv, window, counts):
        return bo.fast_rows(mu, mv, W, H, [50], window, counts, use_weight_distribution=False)

    run_matrix(native, plan, U, "unweighted", oracle, exact=True)
    plan.close()


@pytest.mark.parametrize("U", [1, 3, 7, 66, 130])
def test_integer_plans_naive(native, engine, U):
    """Lat/lon cells (10 x 20 degrees: 361 bins, 23 column blocks, the last one ragged)."""
    an = naive_analyzer(True)
    plan = an._naive_plan()

    def oracle(mu, mv, window, counts):
        return bo.fast_rows(mu, mv, W, H, None, window, counts, naive=(10, 20))

    run_matrix(native, plan, U, "naive", oracle, exact=True)


@pytest.mark.parametrize("tcs", [(50,), (50, 100, 200)])
@pytest.mark.parametrize("U", [1, 3, 7, 66, 130])
def test_weighted_plans(native, engine, U, tcs):
    plan = fib_plan(native, engine, list(tcs))

    def oracle(mu, mv, window, counts):
        return bo.fast_rows(mu, mv, W, H, list(tcs), window, counts)

    run_matrix(native, plan, U, "weighted" + str(len(tcs)), oracle, exact=False)
    plan.close()


def test_lds_limit_and_the_plan_beyond_it(native, engine):
    """1001 tiles: the 16 x n block takes 128 128 bytes of the 160 KB; 1301 tiles do not fit: VET_ERR_UNSUPPORTED, nothing runs."""
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(5, 40, base_seed=77, p_absent=0.1)
    counts, _ = bo.draw(5, 17, SEED)
    plan = fib_plan(native, engine, [1000])
    for window, stride in ((40, 1), (7, 11)):
        res = plan.spatial_bootstrap(mu=mu, mv=mv, window=window, stride=stride, replicates=17, seed=SEED, want_replicates=True,
                                     want_weights=True)
        rep, w, n = bo.fast(mu, mv, W, H, [1000], window, stride, counts)
        close(res["replicates"], rep, 1e-6, f"tc1000 w{window}")
        check_weights(res["weights"], w, n, 2.0, f"tc1000 w{window}")
        check_summary(res, 0.95, f"tc1000 w{window}")
    plan.close()
    big = fib_plan(native, engine, [1300])
    with pytest.raises(native.NativeError) as e:
        big.spatial_bootstrap(mu=mu, mv=mv, window=5, replicates=4)
    assert e.value.code == native.VET_ERR_UNSUPPORTED and "LDS" in str(e.value)
    big.close()


# ------------------------------------------------------------------------------------------- the reference (golden G21)
def g21_cases():
    for w, s in ((300, 1), (20, 20), (20, 7), (1, 1)):
        for flag, tcs in ((True, (50,)), (True, (50, 100, 200)), (False, (50,))):
            yield f"{'w' if flag else 'u'}_tc{'_'.join(map(str, tcs))}_w{w}_s{s}", flag, tcs, w, s
        yield f"naive_h10_w20_w{w}_s{s}", True, None, w, s


def test_vs_reference_golden(native, engine, g16, g21):
    """Every stored case, the grid and the ids entry; G21's draw is the device's."""
    mu, mv = g16["mu"], g16["mv"]
    ids = ids_of(mu, mv)
    seed = int(g21["seed"])
    plans = {}
    for tag, flag, tcs, w, s in g21_cases():
        key = (tcs, flag)
        if key not in plans:
            plans[key] = naive_analyzer(flag)._naive_plan() if tcs is None else fib_plan(native, engine, tcs, flag)
        plan = plans[key]
        rows = g21[f"{tag}__rows"]
        entries = [dict(mu=mu, mv=mv)] + ([dict(ids=ids)] if tcs is not None else [])
        for kw in entries:
            res = plan.spatial_bootstrap(window=None if w == 300 else w, stride=s, replicates=12, seed=seed, want_replicates=True,
                                         want_weights=True, **kw)
            msg = f"{tag} {'ids' if 'ids' in kw else 'grid'}"
            close(res["replicates"][rows], g21[f"{tag}__entropy"], 1e-6, msg)
            if tcs is not None:
                wtag = f"{'w' if flag else 'u'}_tc50_w{w}_s{s}"
                want = g21[f"{wtag}__weights"]
                if flag:
                    check_weights(res["weights"][rows], want, g21[f"{tag}__samples"], 2.0, msg)
                else:
                    assert np.array_equal(res["weights"][rows], want), msg
            check_summary(res, 0.95, msg)
    assert np.array_equal(plans[((50,), True)].bootstrap_counts(8, 12, seed), g21["counts"])
    for key, p in plans.items():
        if key[0] is not None:
            p.close()


# ------------------------------------------------------------------------------------------- zero-valued keys (G12's plan)
def test_zero_valued_keys_follow_the_reference(native, engine):
    """power_factor 150 on 501 tiles: the direction of pixel (21, 61) has exactly one key whose weight underflows to 0.0 (tile
    146).  Viewer 0 looks there throughout.  Viewer 1 looks at pixel (23, 128), which gives tile 146 a weight, in frames 0-9 (row
    0: the zero tile is covered where viewer 1 is drawn) and elsewhere in frames 10-19 (row 1: it is not).  Viewers 2 and 3 look
    elsewhere.  The replicates' NaN pattern is the literal oracle's."""
    U, Tn, power = 4, 20, 150.0
    L = vo.fibonacci_lattice(500)
    grid = vo.direction_grid(W, H).reshape(-1, 3)
    pix = {"zero": (21, 61), "cover": (23, 128), "far_a": (35, 52), "far_b": (94, 122)}
    with np.errstate(all="ignore"):
        w, keys = vo.tile_weight_rows(grid[[py * (W + 1) + px for px, py in pix.values()]], L, 120.0, power, True, return_keys=True)
    zero = keys & (w == 0)
    assert zero[0].sum() == 1 and zero[0, 146] and not zero[1:].any() and w[1, 146] > 0 and not keys[2:, 146].any()
    px = np.zeros((Tn, U), dtype=np.int64)
    py = np.zeros((Tn, U), dtype=np.int64)
    for u, name in enumerate(("zero", "cover", "far_a", "far_b")):
        px[:, u], py[:, u] = pix[name]
    px[10:, 1], py[10:, 1] = pix["far_b"]
    mu, mv = (px + 0.5) / W, (py + 0.5) / H
    mu[3:6, 3], mv[3:6, 3] = np.nan, np.nan
    assert np.array_equal(vo.normalize_to_pixel(mu, W)[~np.isnan(mu)], px[~np.isnan(mu)])
    B = 40
    counts, picks = bo.draw(U, B, SEED)
    lit, _ = bo.literal(mu, mv, W, H, [500], 10, 10, picks, power_factor=power)
    fast, _, _ = bo.fast(mu, mv, W, H, [500], 10, 10, counts, power_factor=power)
    assert np.array_equal(np.isnan(lit), np.isnan(fast))
    has0, has1 = counts[:, 0] > 0, counts[:, 1] > 0
    assert np.array_equal(np.isnan(lit[0]), has0 & ~has1) and np.array_equal(np.isnan(lit[1]), has0)
    assert (has0 & has1).any() and (has0 & ~has1).any() and (~has0).any()
    plan = fib_plan(native, engine, [500], True, 120.0, power)
    res = plan.spatial_bootstrap(mu=mu, mv=mv, window=10, stride=10, replicates=B, seed=SEED, want_replicates=True)
    close(res["replicates"], lit, 1e-6, "zero-valued keys")
    check_summary(res, 0.95, "zero-valued keys")
    one = plan.spatial_bootstrap(mu=mu, mv=mv, window=1, stride=1, replicates=B, seed=SEED, want_replicates=True)
    lit1, _ = bo.literal(mu, mv, W, H, [500], 1, 1, picks, rows=[0, 4, 12], power_factor=power)
    close(one["replicates"][[0, 4, 12]], lit1, 1e-6, "zero-valued keys, per frame")
    plan.close()


# ------------------------------------------------------------------------------------------- invariance, bit for bit
@pytest.mark.parametrize("kind", ["weighted3", "unweighted", "naive"])
def test_replicates_are_pure_functions(native, engine, kind):
    U = 66
    mu, mv = video(U, seed=5)
    ids = ids_of(mu, mv)
    plan = (naive_analyzer(True)._naive_plan() if kind == "naive" else
            fib_plan(native, engine, [50, 100, 200] if kind == "weighted3" else [50], kind != "unweighted"))

    def run(B=40, stride=3, seed=SEED, window=20, **kw):
        kw = kw or dict(mu=mu, mv=mv)
        return plan.spatial_bootstrap(window=window, stride=stride, replicates=B, seed=seed, want_replicates=True,
                                      want_weights=True, **kw)

    def same(x, y, msg, keys=("summary", "replicates", "weights", "valid")):
        for k in keys:
            assert np.ascontiguousarray(x[k]).tobytes() == np.ascontiguousarray(y[k]).tobytes(), (msg, k)

    a = run()
    try:
        same(a, run(), "run to run")
        b5 = run(B=5)
        assert b5["replicates"].tobytes() == np.ascontiguousarray(a["replicates"][:, :5]).tobytes()      # b does not depend on B
        assert b5["weights"].tobytes() == np.ascontiguousarray(a["weights"][:, :5]).tobytes()
        one = run(stride=1)
        assert np.ascontiguousarray(one["replicates"][::3]).tobytes() == a["replicates"].tobytes()      # nor on the stride
        assert np.ascontiguousarray(one["summary"][:, ::3]).tobytes() == a["summary"].tobytes()
        for rows in (1, 7):
            engine.test_bootstrap_chunk_rows(rows)
            same(a, run(), f"{rows} rows per chunk")
        engine.test_bootstrap_chunk_rows(0)
        if kind != "naive":
            same(a, run(ids=ids), "ids entry")
        other = run(seed=SEED + 1)
        assert other["replicates"].tobytes() != a["replicates"].tobytes()
        assert not np.isnan(a["replicates"]).all() and np.nanstd(a["replicates"], axis=1).max() > 0
    finally:
        engine.test_bootstrap_chunk_rows(0)
        if kind != "naive":
            plan.close()


def test_device_entries_equal_the_host_entry(native, engine):
    """vet_bootstrap_entropy / _ids on device buffers: the _host entry's bits; d_status[0] is added to, d_status[1] left alone;
    the nullable outputs may be NULL."""
    lib = engine.lib
    U = 7
    mu, mv = video(U, seed=9)
    mu, mv = np.ascontiguousarray(mu), np.ascontiguousarray(mv)
    ids = ids_of(mu, mv)
    bufs = []

    def dev(nbytes, src=None):
        p = ctypes.c_void_p()
        assert lib.vet_malloc(engine.handle, nbytes, ctypes.byref(p)) == 0
        bufs.append(p)
        if src is not None:
            assert lib.vet_memcpy_h2d(engine.handle, p, native._ptr(src), nbytes) == 0
        return p

    plan = fib_plan(native, engine, [50, 100])
    try:
        d_mu, d_mv, d_ids = dev(mu.nbytes, mu), dev(mv.nbytes, mv), dev(ids.nbytes, ids)
        window, stride, B = 20, 7, 17
        host = plan.spatial_bootstrap(mu=mu, mv=mv, window=window, stride=stride, replicates=B, seed=SEED, confidence=0.8,
                                      want_replicates=True, want_weights=True)
        R = uo.n_rows(T, window, stride)
        for entry in ("grid", "ids"):
            summ, rep, wts, val = np.empty((4, R)), np.empty((R, B)), np.empty((R, B, 51)), np.empty(R, np.int32)
            st = np.array([5, 1000], np.int32)
            d = [dev(x.nbytes) for x in (summ, rep, wts, val)] + [dev(8, st)]
            plan.spatial_bootstrap_device(d_mu.value, d_mv.value, U, T, window, stride, B, SEED, 0.8, d[0].value, d[1].value,
                                          d[2].value, d[3].value, d[4].value, d_ids=d_ids.value if entry == "ids" else 0)
            for h, p in zip((summ, rep, wts, val, st), d):
                assert lib.vet_memcpy_d2h(engine.handle, native._ptr(h), p, h.nbytes) == 0
            for k, x in (("summary", summ), ("replicates", rep), ("weights", wts), ("valid", val)):
                assert host[k].tobytes() == x.tobytes(), (entry, k)
            assert st.tolist() == [5, 1000], entry
            summ2 = np.empty((4, R))
            d2 = dev(summ2.nbytes)
            plan.spatial_bootstrap_device(d_mu.value, d_mv.value, U, T, window, stride, B, SEED, 0.8, d2.value,
                                          d_ids=d_ids.value if entry == "ids" else 0)
            assert lib.vet_memcpy_d2h(engine.handle, native._ptr(summ2), d2, summ2.nbytes) == 0
            assert summ2.tobytes() == summ.tobytes(), entry
        lean = plan.spatial_bootstrap(mu=mu, mv=mv, window=window, stride=stride, replicates=B, seed=SEED, confidence=0.8)
        assert lean["replicates"] is None and lean["weights"] is None
        assert lean["summary"].tobytes() == host["summary"].tobytes() and np.array_equal(lean["valid"], host["valid"])
    finally:
        engine.synchronize()
        for p in bufs:
            lib.vet_free(engine.handle, p)
        plan.close()


def test_one_viewer_is_the_per_user_row(native, engine):
    """U = 1: every replicate draws the one viewer once: spatial_per_user's value of the row."""
    mu, mv = video(1)
    for tcs, weighted in (([50, 100], True), ([50], False)):
        plan = fib_plan(native, engine, tcs, weighted)
        for window, stride in ((1, 1), (20, 7), (T, 1)):
            res = plan.spatial_bootstrap(mu=mu, mv=mv, window=window, stride=stride, replicates=5, seed=3, want_replicates=True)
            own = plan.spatial_per_user(mu=mu, mv=mv, window=window, stride=stride)["entropy"][0]
            for b in range(5):
                close(res["replicates"][:, b], own, 1e-12, f"U1 {tcs} w{window} b{b}")
            finite = ~np.isnan(own)
            assert np.array_equal(res["valid"], np.where(finite, 5, 0))
            close(res["summary"][0], own, 1e-12, "U1 mean")
            assert (res["summary"][1][finite] <= 1e-12).all()
        plan.close()


# ------------------------------------------------------------------------------------------- arguments
def test_arguments(native, engine):
    mu, mv = video(3)
    plan = fib_plan(native, engine, [50])
    for kw in (dict(replicates=0), dict(replicates=4097), dict(confidence=0.0), dict(confidence=1.0), dict(window=0),
               dict(window=T + 1), dict(stride=0)):
        with pytest.raises(ValueError):
            plan.spatial_bootstrap(mu=mu, mv=mv, **dict(dict(window=5), **kw))
    out = np.zeros(4 * T)
    for B, conf in ((0, 0.9), (4097, 0.9), (8, 0.0), (8, 1.0), (8, float("nan"))):
        rc = plan.lib.vet_bootstrap_entropy_host(plan.handle, native._ptr(mu), native._ptr(mv), None, 3, T, 5, 1, B, 0, conf,
                                                 native._ptr(out), None, None, None)
        assert rc == native.VET_ERR_INVALID and plan.lib.vet_last_error()
    bad = mu.copy()
    bad[3, 1] = 1.5
    r = plan.spatial_bootstrap(mu=bad, mv=mv, window=5, replicates=4096, want_replicates=True, check=False)
    assert r["code"] == native.VET_ERR_RANGE and r["replicates"].shape == (T - 4, 4096)       # outputs still written
    check_summary(r, 0.95, "4096 replicates")
    assert (r["valid"][:90] == 4096).all()
    with pytest.raises(native.NativeError):
        plan.spatial_bootstrap(mu=bad, mv=mv, window=5, replicates=4)
    plan.close()


# ------------------------------------------------------------------------------------------- analyzers
def test_analyzers(native):
    from viewport_entropy_toolkit import SpatialEntropyAnalyzer
    from viewport_entropy_toolkit.config import AnalyzerConfig
    mu, mv = video(7)
    times = np.arange(T) * 0.1
    for an in (SpatialEntropyAnalyzer(AnalyzerConfig(tile_counts=[50, 100])), naive_analyzer(True)):
        an.load_arrays(times, mu, mv)
        df = an.compute_entropy_bootstrap(20, 20, replicates=32, confidence=0.9, seed=11, keep_replicates=True)
        assert list(df.columns) == ["time", "time_end", "entropy", "samples", "mean", "sd", "lo", "hi", "valid", "replicates"]
        assert df.attrs == dict(replicates=32, seed=11, confidence=0.9) and len(df) == 12
        point = an.compute_windowed_entropy(20, 20)
        assert df["entropy"].to_numpy().tobytes() == point["entropy"].to_numpy().tobytes()
        assert np.array_equal(df["samples"], point["samples"])
        assert np.array_equal(df["time"], point["time"]) and np.array_equal(df["time_end"], point["time_end"])
        rep = np.stack(list(df["replicates"]))
        want, valid = bo.summary(rep, 0.9)
        assert np.array_equal(df["valid"], valid) and (valid == 32).all()
        close(np.stack([df[k] for k in ("mean", "sd", "lo", "hi")]), want, 1e-12, "analyzer summary")
        assert (df["lo"] <= df["mean"]).all() and (df["mean"] <= df["hi"]).all() and (df["sd"] > 0).all()
        # the point estimate lies in the neighbourhood of its own band
        assert (np.abs(df["entropy"] - df["mean"]) <= 6 * df["sd"]).all()
        frames = an.compute_entropy_bootstrap(replicates=8)            # the per-frame series; the empty frames are returned
        assert len(frames) == T and "replicates" not in frames.columns
        assert (frames["valid"][EMPTY[0]:EMPTY[1]] == 0).all() and np.isnan(frames["entropy"][EMPTY[0]:EMPTY[1]]).all()
        assert (frames["samples"][EMPTY[0]:EMPTY[1]] == 0).all()
