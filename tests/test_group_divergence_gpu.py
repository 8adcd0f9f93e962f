"""GPU: the two-audience permutation test through the C-ABI (Plan.spatial_group_divergence -> vet_group_divergence_host, the device
entries, Plan.group_labels, both analyzers).  Labelling 0 is the observed grouping, labelling b + 1 permutation b; D[r][l] is the
mass-weighted Jensen-Shannon divergence, in bits, between the two audiences' pooled histograms of frames
[r * stride, r * stride + window).  The references are golden G22 (the real reference's dicts,
tools/gen_golden_group_divergence.py) and the numpy oracles of tests/_group_oracle.py (pinned against G22 in
tests/test_group_divergence_surface.py).

Tolerances:
  observed, null     ABSOLUTE, atol = 2 * log2(n_max) * W_RTOL (tests/test_window_divergence_gpu.py's rule: a histogram entry may
                     differ from the oracle's by tests/_tol.py's W_RTOL relative, and D is a difference of entropies of at most
                     log2(n) bits each); no relative term.  Where NaN sits must match exactly.
  integer plans      (unweighted, naive) the group histograms are sums of small integers, exact in FP64 in any order: ``weights``
                     array_equal, ``samples`` exact;
  weighted plans     ``weights`` within tests/_tol.py (W_RTOL relative, w_atol per contributing sample);
  summary            p_value, p_adjusted and valid EQUAL to numpy on the device's own observed and null (counts of comparisons
                     of stored doubles, one division); null_mean and null_crit rtol 1e-12.
One oracle per (plan, U, window) — every row at stride 1, 40 permutations of each grouping — serves every stride and every P: rows
at stride s are the rows r * s of stride 1, and permutation b does not depend on P."""
import ctypes

import numpy as np
import pytest

from oracle import vet_oracle as vo
from tests import _group_oracle as go
from tests import _user_oracle as uo
from tests._tol import W_RTOL, w_atol

pytestmark = pytest.mark.gpu

W, H = 100, 200
T = 240
SEED = 2025
P_MAX = 40
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
def g22(golden_dir):
    return np.load(golden_dir / "g22_group_divergence.npz")


def fib_plan(native, engine, tcs, weighted=True, fov=120.0, power=2.0):
    return native.Plan(engine, [vo.fibonacci_lattice(t) for t in tcs], fov, power, weighted, W, H)


def naive_analyzer(weighted=True):
    from viewport_entropy_toolkit import NaiveSpatialEntropyAnalyzer
    from viewport_entropy_toolkit.config import EntropyConfig, NaiveAnalyzerConfig
    return NaiveSpatialEntropyAnalyzer(NaiveAnalyzerConfig(tile_height=10, tile_width=20, video_width=W, video_height=H,
                                                           entropy_config=EntropyConfig(use_weight_distribution=weighted)))


def atol_of(plan):
    return 2.0 * np.log2(max(plan.n_tiles)) * W_RTOL


def strides(window):
    return sorted({1, 3, window, window + 5})


def video(U, seed=0):
    """Random walks, 10 % absences, frames EMPTY without anybody: asymmetric in every direction the lane map could be wrong in."""
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(U, T, base_seed=300 + U + seed, p_absent=0.1)
    mu[EMPTY[0]:EMPTY[1]], mv[EMPTY[0]:EMPTY[1]] = np.nan, np.nan
    return mu, mv


def groupings(U):
    """Balanced, one against the rest, and with excluded viewers (where U leaves room for them)."""
    out = {"balanced": np.arange(U) % 2, "one": np.r_[0, np.ones(U - 1, dtype=np.int64)]}
    if U >= 3:
        g = np.array([(0, 1, -1)[u % 3] for u in range(U)])
        g[-1] = 1 if U > 3 else g[-1]
        out["excluded"] = g
    return {k: v.astype(np.int8) for k, v in out.items()}


def ids_of(mu, mv):
    return uo.direction_ids(mu, mv, W, H)[0].astype(np.int32)


def close(got, want, atol, msg):
    print(msg, "max abs err", float(np.nanmax(np.abs(got - want), initial=0.0)), "atol", atol)
    assert got.shape == want.shape, msg
    assert np.array_equal(np.isnan(got), np.isnan(want)), (msg, np.argwhere(np.isnan(got) != np.isnan(want))[:10])
    np.testing.assert_allclose(got, want, rtol=0, atol=atol, equal_nan=True, err_msg=msg)


def check_weights(got, want, samples, power, msg):
    """Plain values: +0.0 = no weight; tolerance per group from its sample count.  got / want [R][2][n], samples [2][R]."""
    assert got.shape == want.shape, msg
    atol = np.vectorize(lambda n: w_atol(int(n), power))(samples.T)[..., None]
    err = np.abs(got - want)
    print(msg, "weights max abs err", float(err.max(initial=0.0)))
    bad = err > W_RTOL * np.abs(want) + atol
    assert not bad.any(), (msg, np.argwhere(bad)[:10])
    assert not np.signbit(got).any(), msg


def check_summary(res, confidence, msg):
    """p_value, p_adjusted, valid equal; null_mean, null_crit at rtol 1e-12 — against numpy on the device's own values."""
    want, valid = go.summary(res["summary"][0], res["null"], confidence)
    assert np.array_equal(res["valid"], valid), msg
    for k, name in ((1, "p_value"), (2, "p_adjusted")):
        assert np.array_equal(res["summary"][k], want[k], equal_nan=True), (msg, name, np.flatnonzero(res["summary"][k] != want[k])[:10])
    for k, name in ((3, "null_mean"), (4, "null_crit")):
        assert np.array_equal(np.isnan(res["summary"][k]), np.isnan(want[k])), (msg, name)
        np.testing.assert_allclose(res["summary"][k], want[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=f"{msg} {name}")


# ------------------------------------------------------------------------------------------- the draw
@pytest.mark.parametrize("U", [2, 3, 130, 1024])
def test_labels_equal_the_numpy_draw(native, engine, U):
    plan = fib_plan(native, engine, [20])
    rng = np.random.default_rng(U)
    cases = list(groupings(U).values()) + [np.r_[1, np.zeros(U - 1, dtype=np.int64)].astype(np.int8)]
    if U > 3:
        g = rng.integers(-1, 2, U).astype(np.int8)
        g[:2] = 0, 1
        cases.append(g)
    for groups in cases:
        for seed in (0, 0xDEADBEEFCAFEF00D):
            got = {P: plan.group_labels(groups, P, seed) for P in (1, 7, 40)}
            for P, lab in got.items():
                assert lab.dtype == np.uint8 and np.array_equal(lab, go.draw(groups, P, seed)), (U, P, seed)
                assert ((lab == 0).sum(axis=1) == (groups == 0).sum()).all() and ((lab == 1).sum(axis=1) == (groups == 1).sum()).all()
                assert ((lab == 255) == (groups < 0)[None, :]).all()
            assert np.array_equal(got[40][:8], got[7])                       # permutation b does not depend on P
    plan.close()


def test_more_than_16384_included_viewers_are_unsupported(native, engine):
    plan = fib_plan(native, engine, [20])
    groups = (np.arange(16386) % 2).astype(np.int8)
    groups[-1] = -1
    with pytest.raises(native.NativeError) as e:
        plan.group_labels(groups, 2, 0)                                      # N = 16385
    assert e.value.code == native.VET_ERR_UNSUPPORTED
    groups[-2] = -1
    lab = plan.group_labels(groups, 2, 5)                                    # N = 16384: the whole LDS sort
    assert np.array_equal(lab, go.draw(groups, 2, 5))
    plan.close()


# ------------------------------------------------------------------------------------------- the shape matrix
def run_matrix(native, plan, U, kind, oracle, exact):
    """Every window and grouping; per window every stride at P = 40 and every P at stride 3, weights, samples and summary
    included.  ``oracle(mu, mv, window, labels, observed)`` -> (D[R1][L], samples[R1][L][2], weights[R1][len(observed)][2][n0])
    for the rows of stride 1, the labellings of all groupings side by side."""
    mu, mv = video(U)
    groups = groupings(U)
    labels = np.concatenate([go.draw(g, P_MAX, SEED) for g in groups.values()])
    Lg = P_MAX + 1
    atol = atol_of(plan)
    for window in WINDOWS:
        D1, n1, w1 = oracle(mu, mv, window, labels, [v * Lg for v in range(len(groups))])
        if window <= EMPTY[1] - EMPTY[0]:
            assert np.isnan(D1[EMPTY[0]:EMPTY[1] - window + 1]).all() and not n1[EMPTY[0]:EMPTY[1] - window + 1].any()
        for v, (gname, g) in enumerate(groups.items()):
            combos = [(s, P_MAX) for s in strides(window)] + [(3, P) for P in (1, 6, 7, 8)]
            for stride, P in combos:
                msg = f"{kind} U{U} {gname} w{window} s{stride} P{P}"
                res = plan.spatial_group_divergence(mu=mu, mv=mv, groups=g, window=window, stride=stride, permutations=P, seed=SEED,
                                                    confidence=0.9, want_null=True, want_weights=True)
                R = uo.n_rows(T, window, stride)
                pick = np.arange(R) * stride
                assert res["code"] == native.VET_OK and res["null"].shape == (R, P) and res["summary"].shape == (5, R), msg
                want = D1[pick][:, v * Lg:v * Lg + P + 1]
                close(res["summary"][0], want[:, 0], atol, msg + " observed")
                close(res["null"], want[:, 1:], atol, msg + " null")
                assert np.array_equal(res["samples"], n1[pick][:, v * Lg].T), msg
                if exact:
                    assert np.array_equal(res["weights"], w1[pick][:, v]), msg
                    assert not np.signbit(res["weights"]).any(), msg
                else:
                    check_weights(res["weights"], w1[pick][:, v], res["samples"], 2.0, msg)
                check_summary(res, 0.9, msg)
                if window <= 2 and stride == 1:                          # the empty stretch: nothing finite
                    gone = slice(EMPTY[0], EMPTY[1] - window + 1)
                    assert (res["valid"][gone] == 0).all() and np.isnan(res["summary"][:, gone]).all(), msg


@pytest.mark.parametrize("U", [2, 3, 7, 66, 130])
def test_integer_plans_unweighted(native, engine, U):
    """The MFMA lane map and the 8 + 8 row split on exact data: the observed histograms are the oracle's integers, bit for bit."""
    plan = fib_plan(native, engine, [50], weighted=False)

    def oracle(mu, mv, window, labels, observed):
        return go.fast_rows(mu, mv, W, H, [50], window, labels, use_weight_distribution=False, observed=observed)

    run_matrix(native, plan, U, "unweighted", oracle, exact=True)
    plan.close()


@pytest.mark.parametrize("U", [2, 3, 7, 66, 130])
def test_integer_plans_naive(native, engine, U):
    """Lat/lon cells (10 x 20 degrees: 361 bins, 23 column blocks, the last one ragged)."""
    plan = naive_analyzer(True)._naive_plan()

    def oracle(mu, mv, window, labels, observed):
        return go.fast_rows(mu, mv, W, H, None, window, labels, naive=(10, 20), observed=observed)

    run_matrix(native, plan, U, "naive", oracle, exact=True)


@pytest.mark.parametrize("tcs", [(50,), (50, 100, 200)])
@pytest.mark.parametrize("U", [2, 3, 7, 66, 130])
def test_weighted_plans(native, engine, U, tcs):
    plan = fib_plan(native, engine, list(tcs))

    def oracle(mu, mv, window, labels, observed):
        return go.fast_rows(mu, mv, W, H, list(tcs), window, labels, observed=observed)

    run_matrix(native, plan, U, "weighted" + str(len(tcs)), oracle, exact=False)
    plan.close()


def test_lds_limit_and_the_plan_beyond_it(native, engine):
    """1001 tiles: the 16 x n block takes 128 128 bytes of the 160 KB; 1301 tiles do not fit: VET_ERR_UNSUPPORTED, nothing runs."""
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(5, 40, base_seed=77, p_absent=0.1)
    groups = np.array([0, 1, 1, 0, 1], dtype=np.int8)
    labels = go.draw(groups, 17, SEED)
    plan = fib_plan(native, engine, [1000])
    for window, stride in ((40, 1), (7, 11)):
        res = plan.spatial_group_divergence(mu=mu, mv=mv, groups=groups, window=window, stride=stride, permutations=17, seed=SEED,
                                            want_null=True, want_weights=True)
        D, n, w = go.fast(mu, mv, W, H, [1000], window, stride, labels, want_weights=True)
        close(np.c_[res["summary"][0], res["null"]], D, atol_of(plan), f"tc1000 w{window}")
        assert np.array_equal(res["samples"], n[:, 0].T)
        check_weights(res["weights"], w, res["samples"], 2.0, f"tc1000 w{window}")
        check_summary(res, 0.95, f"tc1000 w{window}")
    plan.close()
    big = fib_plan(native, engine, [1300])
    with pytest.raises(native.NativeError) as e:
        big.spatial_group_divergence(mu=mu, mv=mv, groups=groups, window=5, permutations=4)
    assert e.value.code == native.VET_ERR_UNSUPPORTED and "LDS" in str(e.value)
    big.close()


# ------------------------------------------------------------------------------------------- the reference (golden G22)
def g22_cases():
    for w, s in ((300, 1), (20, 20), (20, 7), (1, 1)):
        for flag, tcs in ((True, (50,)), (True, (50, 100, 200)), (False, (50,))):
            yield f"{'w' if flag else 'u'}_tc{'_'.join(map(str, tcs))}_w{w}_s{s}", flag, tcs, w, s
        yield f"naive_h10_w20_w{w}_s{s}", True, None, w, s


def device_run(native, engine, plan, bufs, mu, mv, ids, groups, window, stride, P, seed, confidence, entry, lean=False):
    """One call of vet_group_divergence / _ids on device buffers; returns the result dict and the status words."""
    lib = engine.lib
    Tn, U = mu.shape

    def dev(nbytes, src=None):
        p = ctypes.c_void_p()
        assert lib.vet_malloc(engine.handle, nbytes, ctypes.byref(p)) == 0
        bufs.append(p)
        if src is not None:
            assert lib.vet_memcpy_h2d(engine.handle, p, native._ptr(src), nbytes) == 0
        return p

    R, n0 = uo.n_rows(Tn, window, stride), plan.n_tiles[0]
    d_mu, d_mv, d_ids = (dev(mu.nbytes, mu), dev(mv.nbytes, mv), None) if entry == "grid" else (None, None, dev(ids.nbytes, ids))
    out = dict(summary=np.empty((5, R)), null=np.empty((R, P)), weights=np.empty((R, 2, n0)), samples=np.empty((2, R), np.int32),
               valid=np.empty(R, np.int32))
    st = np.array([5, 1000], np.int32)
    d = {k: dev(x.nbytes) for k, x in out.items()}
    d_st = dev(8, st)
    opt = {} if lean else dict(d_null=d["null"].value, d_weights=d["weights"].value, d_samples=d["samples"].value,
                               d_valid=d["valid"].value, d_status=d_st.value)
    plan.spatial_group_divergence_device(d_mu.value if d_mu else 0, d_mv.value if d_mv else 0, U, Tn, window, stride, groups, P, seed,
                                         confidence, d["summary"].value, d_ids=d_ids.value if d_ids else 0, **opt)
    engine.synchronize()
    for k in (("summary",) if lean else out):
        assert lib.vet_memcpy_d2h(engine.handle, native._ptr(out[k]), d[k], out[k].nbytes) == 0
    assert lib.vet_memcpy_d2h(engine.handle, native._ptr(st), d_st, 8) == 0
    return out, st


def test_vs_reference_golden(native, engine, g16, g22):
    """Every stored case through the grid, ids and device entries; G22's draw is the device's."""
    mu, mv = np.ascontiguousarray(g16["mu"]), np.ascontiguousarray(g16["mv"])
    ids = ids_of(mu, mv)
    seed, groups = int(g22["seed"]), g22["groups"]
    plans, bufs = {}, []
    try:
        for tag, flag, tcs, w, s in g22_cases():
            key = (tcs, flag)
            if key not in plans:
                plans[key] = naive_analyzer(flag)._naive_plan() if tcs is None else fib_plan(native, engine, tcs, flag)
            plan = plans[key]
            rows = g22[f"{tag}__rows"]
            runs = [("host grid", plan.spatial_group_divergence(mu=mu, mv=mv, groups=groups, window=None if w == 300 else w, stride=s,
                                                                 permutations=11, seed=seed, want_null=True, want_weights=True))]
            if tcs is not None:
                runs.append(("host ids", plan.spatial_group_divergence(ids=ids, groups=groups, window=w, stride=s, permutations=11,
                                                                       seed=seed, want_null=True, want_weights=True)))
                if s != 1 or w == 300:
                    runs.append(("device ids", device_run(native, engine, plan, bufs, mu, mv, ids, groups, w, s, 11, seed, 0.95, "ids")[0]))
            if s != 1 or w == 300:
                runs.append(("device grid", device_run(native, engine, plan, bufs, mu, mv, ids, groups, w, s, 11, seed, 0.95, "grid")[0]))
            for name, res in runs:
                msg = f"{tag} {name}"
                close(np.c_[res["summary"][0], res["null"]][rows], g22[f"{tag}__divergence"], atol_of(plan), msg)
                assert np.array_equal(res["samples"][:, rows], g22[f"{tag}__samples"][:, 0].T), msg
                if tcs is not None:
                    want = g22[f"{'w' if flag else 'u'}_tc50_w{w}_s{s}__weights"]
                    if flag:
                        check_weights(res["weights"][rows], want, res["samples"][:, rows], 2.0, msg)
                    else:
                        assert np.array_equal(res["weights"][rows], want), msg
                check_summary(res, 0.95, msg)
        assert np.array_equal(plans[((50,), True)].group_labels(groups, 11, seed), g22["labels"])
    finally:
        engine.synchronize()
        for p in bufs:
            engine.lib.vet_free(engine.handle, p)
        for key, p in plans.items():
            if key[0] is not None:
                p.close()


# ------------------------------------------------------------------------------------------- zero-valued keys (G12's plan)
def test_zero_valued_keys_follow_the_reference(native, engine):
    """power_factor 150 on 501 tiles: the direction of pixel (21, 61) has exactly one key whose weight underflows to 0.0 (tile
    146).  Viewer 0 looks there throughout.  Viewer 1 looks at pixel (23, 128), which gives tile 146 a weight, in frames 0-9 (row
    0) and elsewhere in frames 10-19 (row 1).  Viewers 2 and 3 look elsewhere.  A labelling is NaN in row 0 iff viewers 0 and 1
    are in different audiences (the zero tile is covered in one group and not in the other: S of viewer 0's group is NaN), and in
    row 1 always (the pooled dict has the zero key too).  The NaN pattern is the literal oracle's."""
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
    P = 40
    plan = fib_plan(native, engine, [500], True, 120.0, power)
    for groups in (np.array([0, 1, 0, 1], dtype=np.int8), np.array([0, 0, 1, 1], dtype=np.int8)):
        labels = go.draw(groups, P, SEED)
        lit, _ = go.literal(mu, mv, W, H, [500], 10, 10, labels, power_factor=power)
        fast, _ = go.fast(mu, mv, W, H, [500], 10, 10, labels, power_factor=power)
        assert np.array_equal(np.isnan(lit), np.isnan(fast))
        apart = labels[:, 0] != labels[:, 1]
        assert np.array_equal(np.isnan(lit[0]), apart) and np.isnan(lit[1]).all() and apart.any() and (~apart).any()
        res = plan.spatial_group_divergence(mu=mu, mv=mv, groups=groups, window=10, stride=10, permutations=P, seed=SEED,
                                            want_null=True)
        close(np.c_[res["summary"][0], res["null"]], lit, atol_of(plan), "zero-valued keys")
        check_summary(res, 0.95, "zero-valued keys")
        one = plan.spatial_group_divergence(mu=mu, mv=mv, groups=groups, window=1, stride=1, permutations=P, seed=SEED, want_null=True)
        lit1, _ = go.literal(mu, mv, W, H, [500], 1, 1, labels, rows=[0, 4, 12], power_factor=power)
        close(np.c_[one["summary"][0], one["null"]][[0, 4, 12]], lit1, atol_of(plan), "zero-valued keys, per frame")
    plan.close()


# ------------------------------------------------------------------------------------------- ties and purity, bit for bit
@pytest.mark.parametrize("U", [2, 3])
def test_ties_are_exact(native, engine, U):
    """Few viewers: most permutations reproduce the observed partition (or, U = 2, its complement: the statistic is symmetric, and
    so is every operation that forms it); each of those has the observed BITS, and p_value counts it."""
    mu, mv = video(U, seed=3)
    groups = np.r_[0, np.ones(U - 1, dtype=np.int64)].astype(np.int8)
    P = 40
    labels = go.draw(groups, P, SEED)
    same = (labels[1:] == labels[0]).all(axis=1)
    if U == 2:
        same |= (labels[1:] == 1 - labels[0]).all(axis=1)
        assert same.all()
    assert same.any() and (U == 2 or (~same).any())
    for plan in (fib_plan(native, engine, [50, 100]), fib_plan(native, engine, [50], False)):
        for window, stride in ((20, 7), (T, 1)):
            res = plan.spatial_group_divergence(mu=mu, mv=mv, groups=groups, window=window, stride=stride, permutations=P, seed=SEED,
                                                want_null=True)
            obs, null = res["summary"][0], res["null"]
            ok = ~np.isnan(obs)
            assert ok.any()
            assert (null[:, same].view(np.uint64) == obs.view(np.uint64)[:, None]).all()
            assert (res["summary"][1][ok] >= (1 + same.sum()) / (1 + P)).all()
            if U == 2:
                assert (res["summary"][1][ok] == 1.0).all() and (res["summary"][2][ok] == 1.0).all()
        plan.close()


@pytest.mark.parametrize("kind", ["weighted3", "unweighted", "naive"])
def test_labellings_are_pure_functions(native, engine, kind):
    U = 66
    mu, mv = video(U, seed=5)
    ids = ids_of(mu, mv)
    groups = groupings(U)["excluded"]
    plan = (naive_analyzer(True)._naive_plan() if kind == "naive" else
            fib_plan(native, engine, [50, 100, 200] if kind == "weighted3" else [50], kind != "unweighted"))
    KEYS = ("summary", "null", "weights", "samples", "valid")

    def run(P=40, stride=3, seed=SEED, window=20, **kw):
        kw = kw or dict(mu=mu, mv=mv)
        return plan.spatial_group_divergence(groups=groups, window=window, stride=stride, permutations=P, seed=seed, want_null=True,
                                             want_weights=True, **kw)

    def same(x, y, msg, keys=KEYS):
        for k in keys:
            assert np.ascontiguousarray(x[k]).tobytes() == np.ascontiguousarray(y[k]).tobytes(), (msg, k)

    a = run()
    try:
        same(a, run(), "run to run")
        p5 = run(P=5)
        assert p5["null"].tobytes() == np.ascontiguousarray(a["null"][:, :5]).tobytes()          # b does not depend on P
        assert p5["summary"][0].tobytes() == a["summary"][0].tobytes() and p5["weights"].tobytes() == a["weights"].tobytes()
        one = run(stride=1)
        for k in ("null", "weights", "valid"):                                                   # nor on the stride
            assert np.ascontiguousarray(one[k][::3]).tobytes() == a[k].tobytes(), k
        assert np.ascontiguousarray(one["samples"][:, ::3]).tobytes() == a["samples"].tobytes()
        assert np.ascontiguousarray(one["summary"][[0, 1, 3, 4]][:, ::3]).tobytes() == a["summary"][[0, 1, 3, 4]].tobytes()
        for rows in (1, 7):
            engine.test_group_chunk_rows(rows)
            same(a, run(), f"{rows} rows per chunk")
        engine.test_group_chunk_rows(0)
        if kind != "naive":
            same(a, run(ids=ids), "ids entry")
        other = run(seed=SEED + 1)
        assert other["null"].tobytes() != a["null"].tobytes() and other["summary"][0].tobytes() == a["summary"][0].tobytes()
        assert not np.isnan(a["null"]).all() and np.nanstd(a["null"], axis=1).max() > 0
    finally:
        engine.test_group_chunk_rows(0)
        if kind != "naive":
            plan.close()


def test_device_entries_equal_the_host_entry(native, engine):
    """vet_group_divergence / _ids on device buffers: the _host entry's bits; d_status[0] is added to, d_status[1] left alone;
    the nullable outputs may be NULL."""
    U = 7
    mu, mv = video(U, seed=9)
    mu, mv = np.ascontiguousarray(mu), np.ascontiguousarray(mv)
    ids = ids_of(mu, mv)
    groups = groupings(U)["excluded"]
    bufs = []
    plan = fib_plan(native, engine, [50, 100])
    try:
        window, stride, P = 20, 7, 17
        host = plan.spatial_group_divergence(mu=mu, mv=mv, groups=groups, window=window, stride=stride, permutations=P, seed=SEED,
                                             confidence=0.8, want_null=True, want_weights=True)
        for entry in ("grid", "ids"):
            out, st = device_run(native, engine, plan, bufs, mu, mv, ids, groups, window, stride, P, SEED, 0.8, entry)
            for k, x in out.items():
                assert host[k].tobytes() == x.tobytes(), (entry, k)
            assert st.tolist() == [5, 1000], entry
            lean, _ = device_run(native, engine, plan, bufs, mu, mv, ids, groups, window, stride, P, SEED, 0.8, entry, lean=True)
            assert lean["summary"].tobytes() == out["summary"].tobytes(), entry
        lean = plan.spatial_group_divergence(mu=mu, mv=mv, groups=groups, window=window, stride=stride, permutations=P, seed=SEED,
                                             confidence=0.8)
        assert lean["null"] is None and lean["weights"] is None
        assert lean["summary"].tobytes() == host["summary"].tobytes() and np.array_equal(lean["valid"], host["valid"])
    finally:
        engine.synchronize()
        for p in bufs:
            engine.lib.vet_free(engine.handle, p)
        plan.close()


# ------------------------------------------------------------------------------------------- meaning
@pytest.mark.parametrize("sizes", [(3, 3), (2, 5)])
def test_two_audiences_at_two_far_pixels(native, engine, sizes):
    """A always at one pixel, B always at a far one: the histograms do not overlap, D is the binary entropy of the mass split,
    and a relabelling is as divergent iff it reproduces the partition (or, for equal sizes, its complement)."""
    ua, ub = sizes
    U, Tn, P = ua + ub, 30, 60
    groups = np.r_[np.zeros(ua, dtype=np.int8), np.ones(ub, dtype=np.int8)]
    px = np.where(groups == 0, 35, 94)
    py = np.where(groups == 0, 52, 122)
    mu, mv = np.tile((px + 0.5) / W, (Tn, 1)), np.tile((py + 0.5) / H, (Tn, 1))
    labels = go.draw(groups, P, SEED)
    same = (labels[1:] == labels[0]).all(axis=1)
    if ua == ub:
        same |= (labels[1:] == 1 - labels[0]).all(axis=1)
    for plan, masses in ((fib_plan(native, engine, [50], False), None), (fib_plan(native, engine, [50]), "weights")):
        res = plan.spatial_group_divergence(mu=mu, mv=mv, groups=groups, window=10, stride=10, permutations=P, seed=SEED,
                                            want_null=True, want_weights=True)
        wa, wb = res["weights"][:, 0].sum(axis=1), res["weights"][:, 1].sum(axis=1)
        assert not ((res["weights"][:, 0] > 0) & (res["weights"][:, 1] > 0)).any()               # disjoint supports
        from tests._divergence_oracle import h2
        np.testing.assert_allclose(res["summary"][0], h2(wa / (wa + wb)), rtol=0, atol=atol_of(plan))
        assert (res["summary"][1] == (1 + same.sum()) / (1 + P)).all()
        assert (res["valid"] == P).all()
        plan.close()


def test_adjusted_p_is_not_below_the_raw_one(native, engine):
    """Two audiences drawn from the same random walks, no NaN rows: the max-statistic correction only raises p."""
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(12, 120, base_seed=900, p_absent=0.0)
    groups = (np.arange(12) % 2).astype(np.int8)
    plan = fib_plan(native, engine, [50, 100])
    res = plan.spatial_group_divergence(mu=mu, mv=mv, groups=groups, window=20, stride=10, permutations=40, seed=SEED, want_null=True)
    assert not np.isnan(res["summary"]).any() and (res["valid"] == 40).all()
    assert (res["summary"][2] >= res["summary"][1]).all() and (res["summary"][1] > 0).all() and (res["summary"][2] <= 1).all()
    check_summary(res, 0.95, "same walks")
    plan.close()


# ------------------------------------------------------------------------------------------- arguments
def test_arguments(native, engine):
    mu, mv = video(3)
    g = np.array([0, 1, 1], dtype=np.int8)
    plan = fib_plan(native, engine, [50])
    for kw in (dict(permutations=0), dict(permutations=4097), dict(confidence=0.0), dict(confidence=1.0), dict(window=0),
               dict(window=T + 1), dict(stride=0), dict(groups=[0, 0, 0]), dict(groups=[0, 1]), dict(groups=[0, 1, 2])):
        with pytest.raises(ValueError):
            plan.spatial_group_divergence(mu=mu, mv=mv, **dict(dict(window=5, groups=g), **kw))
    out = np.zeros(5 * T)
    for groups, P, conf in ((g, 0, 0.9), (g, 4097, 0.9), (g, 8, 0.0), (g, 8, 1.0), (g, 8, float("nan")),
                            (np.array([0, 0, 0], np.int8), 8, 0.9), (np.array([1, -1, 1], np.int8), 8, 0.9),
                            (np.array([0, 1, 2], np.int8), 8, 0.9), (np.array([0, 1, -2], np.int8), 8, 0.9), (None, 8, 0.9)):
        rc = plan.lib.vet_group_divergence_host(plan.handle, native._ptr(mu), native._ptr(mv), None, 3, T, 5, 1, native._ptr(groups),
                                                P, 0, conf, native._ptr(out), None, None, None, None)
        assert rc == native.VET_ERR_INVALID and plan.lib.vet_last_error()
    bad = mu.copy()
    bad[3, 1] = 1.5
    r = plan.spatial_group_divergence(mu=bad, mv=mv, groups=g, window=5, permutations=4096, want_null=True, check=False)
    assert r["code"] == native.VET_ERR_RANGE and r["null"].shape == (T - 4, 4096)             # outputs still written
    check_summary(r, 0.95, "4096 permutations")
    assert (r["valid"][:90] == 4096).all()
    with pytest.raises(native.NativeError):
        plan.spatial_group_divergence(mu=bad, mv=mv, groups=g, window=5, permutations=4)
    plan.close()


# ------------------------------------------------------------------------------------------- analyzers
def test_analyzers(native, engine):
    from viewport_entropy_toolkit import SpatialEntropyAnalyzer
    from viewport_entropy_toolkit.config import AnalyzerConfig
    mu, mv = video(7)
    times = np.arange(T) * 0.1
    names = [f"v{u}" for u in range(7)]
    by_name = {"v0": "hmd", "v1": "desktop", "v2": "hmd", "v3": None, "v4": "desktop", "v5": "hmd", "v6": "desktop"}
    code = np.array([1, 0, 1, -1, 0, 1, 0], dtype=np.int8)                    # sorted: "desktop" is A
    for an in (SpatialEntropyAnalyzer(AnalyzerConfig(tile_counts=[50, 100])), naive_analyzer(True)):
        an.load_arrays(times, mu, mv, names)
        df = an.compute_group_divergence(by_name, 20, 20, permutations=32, confidence=0.9, seed=11, keep_null=True)
        assert list(df.columns) == ["time", "time_end", "samples_a", "samples_b", "divergence", "p_value", "p_adjusted", "null_mean",
                                    "null_crit", "valid", "null"]
        assert df.attrs == dict(groups=("desktop", "hmd"), sizes=(3, 3), users=(["v1", "v4", "v6"], ["v0", "v2", "v5"]),
                                permutations=32, seed=11, confidence=0.9) and len(df) == 12
        plan = an._grid_plan()
        res = plan.spatial_group_divergence(mu=mu, mv=mv, groups=code, window=20, stride=20, permutations=32, seed=11, confidence=0.9,
                                            want_null=True)
        for k, name in enumerate(("divergence", "p_value", "p_adjusted", "null_mean", "null_crit")):
            assert df[name].to_numpy().tobytes() == res["summary"][k].tobytes(), name
        assert np.array_equal(df["samples_a"], res["samples"][0]) and np.array_equal(df["samples_b"], res["samples"][1])
        assert np.array_equal(np.stack(list(df["null"])), res["null"], equal_nan=True) and np.array_equal(df["valid"], res["valid"])
        aligned = an.compute_group_divergence([by_name[n] for n in names], 20, 20, permutations=32, confidence=0.9, seed=11)
        assert aligned["divergence"].to_numpy().tobytes() == df["divergence"].to_numpy().tobytes() and "null" not in aligned.columns
        whole = an.compute_group_divergence(by_name, permutations=8)           # the whole video: one row
        one = plan.spatial_group_divergence(mu=mu, mv=mv, groups=code, permutations=8)
        assert len(whole) == 1 and whole["divergence"].to_numpy().tobytes() == one["summary"][0].tobytes()
        assert whole["time"][0] == times[0] and whole["time_end"][0] == times[-1]
        for bad in (["a"] * 7, ["a", "b", "c", "a", "b", "c", "a"], ["a", "b"], {"nobody": "a", "v0": "b"}, None):
            with pytest.raises(ValueError):
                an.compute_group_divergence(bad)
