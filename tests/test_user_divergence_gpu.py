"""GPU: the pairwise viewer divergence through the C-ABI (Plan.spatial_user_divergence -> vet_user_divergence_host, the device
entry, both analyzers).  D(u, v) of row r is the mass-weighted Jensen-Shannon divergence, in bits, of the two viewers' tile
histograms of frames [r * stride, r * stride + window); the references are golden G18 (the real reference's dicts,
tools/gen_golden_user_divergence.py) and the numpy oracles of tests/_divergence_oracle.py (pinned against G18 in
tests/test_user_divergence_surface.py).

Tolerance: ABSOLUTE, atol = 2 * log2(n_max) * W_RTOL (1.1e-8 bits at 51 tiles): a histogram entry may differ from the oracle's by
tests/_tol.py's W_RTOL relative, and D is a difference of entropies of at most log2(n) bits each.  No relative tolerance: D goes
to 0 for similar viewers.  Where NaN sits and the integer samples must match exactly.  Every comparison prints its largest
absolute error."""
import ctypes

import numpy as np
import pytest

from oracle import vet_oracle as vo
from tests import _divergence_oracle as do
from tests import _user_oracle as uo
from tests._tol import W_RTOL

pytestmark = pytest.mark.gpu

W, H = 100, 200
B = 32                                                   # k_user_divergence's pair block (DIV_B)
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


@pytest.fixture(scope="module")
def g18(golden_dir):
    return np.load(golden_dir / "g18_user_divergence.npz")


def fib_plan(native, engine, tcs, weighted=True, fov=120.0, power=2.0):
    return native.Plan(engine, [vo.fibonacci_lattice(t) for t in tcs], fov, power, weighted, W, H)


def naive_analyzer(weighted=True):
    from viewport_entropy_toolkit import NaiveSpatialEntropyAnalyzer
    from viewport_entropy_toolkit.config import EntropyConfig, NaiveAnalyzerConfig
    return NaiveSpatialEntropyAnalyzer(NaiveAnalyzerConfig(tile_height=10, tile_width=20, video_width=W, video_height=H,
                                                           entropy_config=EntropyConfig(use_weight_distribution=weighted)))


def atol_of(plan):
    return 2.0 * np.log2(max(plan.n_tiles)) * W_RTOL


def close(got, want, atol, msg=""):
    print(msg, "max abs err", float(np.nanmax(np.abs(got - want), initial=0.0)), "atol", atol)
    assert got.shape == want.shape, msg
    assert np.array_equal(np.isnan(got), np.isnan(want)), (msg, np.argwhere(np.isnan(got) != np.isnan(want))[:10])
    np.testing.assert_allclose(got, want, rtol=0, atol=atol, equal_nan=True, err_msg=msg)


def ids_of(mu, mv):
    return uo.direction_ids(mu, mv, W, H)[0].astype(np.int32)


def g18_cases():
    for w, s in SHAPES:
        for flag, tcs in ((True, (50,)), (True, (50, 100, 200)), (False, (50,))):
            yield f"{'w' if flag else 'u'}_tc{'_'.join(map(str, tcs))}_w{w}_s{s}", flag, tcs, w, s
        yield f"naive_h10_w20_w{w}_s{s}", True, None, w, s


def check_structure(div, samples):
    """What every result must have, whatever the reference: bitwise symmetry, a +0.0 / NaN diagonal, NaN exactly for viewers
    without a sample unless a histogram makes the reference's NaN."""
    assert div.tobytes() == np.ascontiguousarray(div.transpose(0, 2, 1)).tobytes(), "the matrix is not bitwise symmetric"
    diag = np.diagonal(div, axis1=1, axis2=2)                                          # [R][U]
    assert (np.isnan(diag) | ((diag == 0) & ~np.signbit(diag))).all(), "diagonal is neither +0.0 nor NaN"
    absent = samples.T == 0
    assert np.isnan(div[absent]).all() and np.isnan(div.transpose(0, 2, 1)[absent]).all()


def check_g18(g18, tag, div, samples, atol, msg):
    rows = g18[f"{tag}__rows"]
    close(div[rows], g18[f"{tag}__divergence"], atol, msg)
    assert np.array_equal(samples[:, rows], g18[f"{tag}__samples"]), msg
    check_structure(div, samples)
    w, s = int(tag.split("_")[-2][1:]), int(tag.split("_")[-1][1:])
    r = np.arange(samples.shape[1])
    gone = (r * s >= 100) & (r * s + w <= 200)
    assert not samples[ABSENT_USER][gone].any()                    # the absent viewer: samples 0, NaN row and column
    assert np.isnan(div[gone][:, ABSENT_USER]).all() and np.isnan(div[gone][:, :, ABSENT_USER]).all()


# ------------------------------------------------------------------------------------------- the reference (golden G18)
def test_host_entry_vs_reference_golden(native, engine, g16, g18):
    """Plan.spatial_user_divergence (vet_user_divergence_host), the grid and the ids entry points, every stored case."""
    mu, mv = g16["mu"], g16["mv"]
    ids = ids_of(mu, mv)
    plans = {}
    for tag, flag, tcs, w, s in g18_cases():
        key = (tcs, flag)
        if key not in plans:
            plans[key] = naive_analyzer(flag)._naive_plan() if tcs is None else fib_plan(native, engine, tcs, flag)
        plan = plans[key]
        res = plan.spatial_user_divergence(mu=mu, mv=mv, window=None if w == 300 else w, stride=s)
        R = uo.n_rows(300, w, s)
        assert res["code"] == native.VET_OK and res["divergence"].shape == (R, 8, 8) and res["samples"].shape == (8, R), tag
        check_g18(g18, tag, res["divergence"], res["samples"], atol_of(plan), tag + " grid")
        if tcs is not None:                 # a naive plan has no ids entry of its own table
            res = plan.spatial_user_divergence(ids=ids, window=w, stride=s)
            check_g18(g18, tag, res["divergence"], res["samples"], atol_of(plan), tag + " ids")
    for key, p in plans.items():
        if key[0] is not None:
            p.close()


def test_device_entry_vs_reference_golden(native, engine, g16, g18):
    """vet_user_divergence / vet_user_divergence_ids on device buffers; d_status = {0, (row, viewer) slots without a sample},
    added to."""
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
        for tag, flag, tcs, w, s in g18_cases():
            if tcs is None:
                continue
            plan = plans.get((tcs, flag)) or plans.setdefault((tcs, flag), fib_plan(native, engine, tcs, flag))
            R = uo.n_rows(T, w, s)
            for entry in ("grid", "ids"):
                div, smp = np.empty((R, U, U)), np.empty((U, R), np.int32)
                st = np.array([0, 1000], np.int32)
                d_div, d_s, d_st = dev(div.nbytes), dev(smp.nbytes), dev(8, st)
                if entry == "grid":
                    plan.spatial_user_divergence_device(d_mu.value, d_mv.value, U, T, w, s, d_div.value, d_s.value, d_st.value)
                else:
                    native._check(lib, lib.vet_user_divergence_ids(plan.handle, d_ids, U, T, w, s, d_div, d_s, d_st, None))
                for h, d in ((div, d_div), (smp, d_s), (st, d_st)):
                    assert lib.vet_memcpy_d2h(engine.handle, native._ptr(h), d, h.nbytes) == 0
                check_g18(g18, tag, div, smp, atol_of(plan), f"{tag} device {entry}")
                assert st.tolist() == [0, 1000 + int((smp == 0).sum())], tag
    finally:
        engine.synchronize()
        for p in bufs:
            lib.vet_free(engine.handle, p)
        for p in plans.values():
            p.close()


def test_analyzers_vs_reference_golden(native, g16, g18):
    from viewport_entropy_toolkit import SpatialEntropyAnalyzer
    from viewport_entropy_toolkit.config import AnalyzerConfig, EntropyConfig
    mu, mv = g16["mu"], g16["mv"]
    times = np.arange(300) * 0.1
    names = [f"viewer{u}" for u in range(8)]
    ans = {}
    for tag, flag, tcs, w, s in g18_cases():
        if (tcs, flag) not in ans:
            an = (naive_analyzer(flag) if tcs is None else
                  SpatialEntropyAnalyzer(AnalyzerConfig(tile_counts=list(tcs), entropy_config=EntropyConfig(use_weight_distribution=flag))))
            an.load_arrays(times, mu, mv, user_names=names)
            ans[(tcs, flag)] = an
        an = ans[(tcs, flag)]
        df = an.compute_user_divergence(None if w == 300 else w, s)
        R = uo.n_rows(300, w, s)
        assert list(df.columns) == ["time", "time_end", "divergence", "samples"] and len(df) == R and df.attrs["users"] == names
        assert np.array_equal(df["time"], times[np.arange(R) * s]) and np.array_equal(df["time_end"], times[np.arange(R) * s + w - 1])
        whole = df["divergence"][0].base
        assert whole is not None and whole.shape == (R, 8, 8) and all(df["divergence"][r].base is whole for r in range(R))   # views into ONE array
        div = np.stack(list(df["divergence"]))
        samples = np.stack(list(df["samples"]), axis=1)
        n_max = max(an._naive_plan().n_tiles) if tcs is None else max(tcs) + 1
        check_g18(g18, tag, div, samples, 2.0 * np.log2(n_max) * W_RTOL, tag + " analyzer")


# ------------------------------------------------------------------------------------------- pair-block edges
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("U", [1, 2, B - 1, B, B + 1, 2 * B + 1])
def test_pair_block_edges(native, engine, U, weighted):
    """One, two, a ragged, a full, a full plus one and three blocks of viewers (six pair blocks, three on the diagonal); T = 40,
    the whole video."""
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(U, 40, base_seed=500 + U, p_absent=0.1)
    if U > 2:
        mu[:, 2], mv[:, 2] = np.nan, np.nan                         # a viewer who never shows up
    plan = fib_plan(native, engine, [50], weighted)
    res = plan.spatial_user_divergence(mu=mu, mv=mv)
    div, samples = do.fast(mu, mv, W, H, [50], 40, 1, use_weight_distribution=weighted)
    assert res["divergence"].shape == (1, U, U) and np.array_equal(res["samples"], samples)
    close(res["divergence"], div, atol_of(plan), f"U{U} weighted {weighted}")
    check_structure(res["divergence"], res["samples"])
    plan.close()


# ------------------------------------------------------------------------------------------- tile-chunk edges, several lattices
@pytest.mark.parametrize("tcs", [(200,), (1000,), (50, 100, 200)])
def test_tile_chunk_edges_and_several_lattices(native, engine, tcs):
    """201 and 1001 tiles (7 and 32 LDS stages of 32 tiles, both ragged) and three lattices added in lattice order; U = 9,
    T = 150, window 20, stride 7."""
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(9, 150, base_seed=7, p_absent=0.1)
    mu[40:75, 2], mv[40:75, 2] = np.nan, np.nan
    plan = fib_plan(native, engine, list(tcs), True)
    res = plan.spatial_user_divergence(mu=mu, mv=mv, window=20, stride=7)
    div, samples = do.fast(mu, mv, W, H, list(tcs), 20, 7)
    assert np.array_equal(res["samples"], samples) and (samples == 0).any()
    close(res["divergence"], div, atol_of(plan), f"tcs {tcs}")
    check_structure(res["divergence"], res["samples"])
    plan.close()


# ------------------------------------------------------------------------------------------- row chunks
@pytest.mark.parametrize("kind", ["weighted3", "unweighted"])
def test_row_chunks_do_not_change_a_bit(native, engine, kind):
    """U = 2B + 1, T = 60, window 20, stride 1 (41 rows): histograms built 1 and 7 rows at a time (41 and 6 chunks, the last one
    ragged) against the default (one chunk)."""
    from viewport_entropy_toolkit import _synthetic
    U = 2 * B + 1
    mu, mv = _synthetic.random_walk_video(U, 60, base_seed=61, p_absent=0.1)
    mu[10:45, 4], mv[10:45, 4] = np.nan, np.nan
    plan = fib_plan(native, engine, [50, 100, 200] if kind == "weighted3" else [50], kind != "unweighted")
    try:
        a = plan.spatial_user_divergence(mu=mu, mv=mv, window=20, stride=1)
        assert a["divergence"].shape == (41, U, U) and (a["samples"] == 0).any()
        check_structure(a["divergence"], a["samples"])
        for rows in (1, 7):
            engine.test_divergence_chunk_rows(rows)
            b = plan.spatial_user_divergence(mu=mu, mv=mv, window=20, stride=1)
            assert a["divergence"].tobytes() == b["divergence"].tobytes(), rows
            assert np.array_equal(a["samples"], b["samples"]), rows
    finally:
        engine.test_divergence_chunk_rows(0)
        plan.close()


# ------------------------------------------------------------------------------------------- properties
def masses(plan, kind, mu, mv, window, stride):
    """W[R][U] of lattice 0: the histogram totals vet_user_entropy reports (weighted), the samples (counts)."""
    if kind == "weighted":
        return np.abs(plan.spatial_per_user(mu=mu, mv=mv, window=window, stride=stride, want_weights=True)["weights"]).sum(axis=2).T
    return plan.spatial_per_user(mu=mu, mv=mv, window=window, stride=stride)["samples"].T.astype(np.float64)


@pytest.mark.parametrize("kind", ["weighted", "unweighted", "naive"])
def test_properties(native, engine, kind):
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(12, 90, base_seed=19, p_absent=0.15)
    mu[20:60, 1], mv[20:60, 1] = np.nan, np.nan
    mu[:, 7], mv[:, 7] = mu[:, 4], mv[:, 4]                          # viewer 7 is viewer 4's twin
    plan = naive_analyzer(False)._naive_plan() if kind == "naive" else fib_plan(native, engine, [50], kind == "weighted")
    atol = atol_of(plan)
    res = plan.spatial_user_divergence(mu=mu, mv=mv, window=20, stride=5)
    D = res["divergence"]
    check_structure(D, res["samples"])
    Wm = masses(plan, kind, mu, mv, 20, 5)
    with np.errstate(all="ignore"):
        bound = do.h2(Wm[:, :, None] / (Wm[:, :, None] + Wm[:, None, :]))
    ok = ~np.isnan(D)
    assert ok.any() and (D[ok] >= -atol).all() and (D[ok] <= bound[ok] + atol).all()
    print(kind, "min D", float(D[ok].min()), "max D - bound", float((D[ok] - bound[ok]).max()), "twin", float(np.nanmax(np.abs(D[:, 4, 7]))))
    twin = D[:, 4, 7]
    assert (~np.isnan(twin)).any() and (np.abs(twin[~np.isnan(twin)]) <= atol).all()   # a duplicated column against its twin
    third = np.delete(np.arange(12), [4, 7])                                           # ... and bit-equal against third viewers
    assert np.ascontiguousarray(D[:, 4][:, third]).tobytes() == np.ascontiguousarray(D[:, 7][:, third]).tobytes()
    if kind != "naive":
        plan.close()


@pytest.mark.parametrize("weighted", [True, False])
def test_antipodal_viewers_give_the_binary_entropy_of_their_masses(native, engine, weighted):
    """Two viewers held at antipodal pixels under a 30 degree field of view share no tile: D = H2(W_u / (W_u + W_v)); with
    equal sample counts on an unweighted plan that is 1.0."""
    T = 40
    mu = np.stack([np.full(T, 0.25), np.full(T, 0.75), np.full(T, 0.75)], axis=1)      # longitude -90 and +90 on the equator
    mv = np.full((T, 3), 0.5)
    mu[10:, 2], mv[10:, 2] = np.nan, np.nan                                            # viewer 2: 10 samples of viewer 1's 40
    plan = fib_plan(native, engine, [500], weighted, fov=30.0)
    atol = atol_of(plan)
    res = plan.spatial_user_divergence(mu=mu, mv=mv)
    D = res["divergence"][0]
    Wm = masses(plan, "weighted" if weighted else "unweighted", mu, mv, T, 1)[0]       # weighted: a direction's weights times its samples
    assert res["samples"][:, 0].tolist() == [40, 40, 10] and (Wm > 0).all()
    want = do.h2(Wm[:, None] / (Wm[:, None] + Wm[None, :]))
    print("weighted", weighted, "masses", Wm, "D01 - H2", D[0, 1] - want[0, 1], "D02 - H2", D[0, 2] - want[0, 2], "D12", D[1, 2])
    assert abs(D[0, 1] - want[0, 1]) <= atol and abs(D[0, 2] - want[0, 2]) <= atol    # disjoint tiles: H2 of the mass split
    assert abs(D[1, 2]) <= atol                                                        # the same place: the same proportions
    if not weighted:
        assert want[0, 1] == 1.0 and abs(D[0, 1] - 1.0) <= atol                        # equal sample counts: one bit
        assert abs(D[0, 2] - float(do.h2(0.2))) <= atol                                # 40 : 10
    plan.close()


# ------------------------------------------------------------------------------------------- purity
@pytest.mark.parametrize("kind", ["weighted", "weighted3", "unweighted", "naive"])
def test_pairs_are_pure_functions_of_the_two_viewers_samples(native, engine, kind):
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(9, 150, base_seed=7, p_absent=0.1)
    mu[40:75, 2], mv[40:75, 2] = np.nan, np.nan
    ids = ids_of(mu, mv)
    plan = (naive_analyzer(False)._naive_plan() if kind == "naive" else
            fib_plan(native, engine, [50, 100, 200] if kind == "weighted3" else [50], kind != "unweighted"))

    def same(x, y, msg):
        assert x["divergence"].tobytes() == y["divergence"].tobytes(), msg
        assert np.array_equal(x["samples"], y["samples"]), msg

    a = plan.spatial_user_divergence(mu=mu, mv=mv, window=20, stride=7)
    same(a, plan.spatial_user_divergence(mu=mu, mv=mv, window=20, stride=7), "run to run")
    one = plan.spatial_user_divergence(mu=mu, mv=mv, window=20, stride=1)
    same(a, dict(divergence=np.ascontiguousarray(one["divergence"][::7]), samples=one["samples"][:, ::7]),
         "the rows of the same frames at stride 1")
    if kind != "naive":
        same(a, plan.spatial_user_divergence(ids=ids, window=20, stride=7), "ids entry")
    for r in (0, 5, 7, a["divergence"].shape[0] - 1):              # a call that holds only the row's 20 frames
        cut = plan.spatial_user_divergence(mu=mu[7 * r:7 * r + 20], mv=mv[7 * r:7 * r + 20], window=20)
        same(dict(divergence=np.ascontiguousarray(a["divergence"][r:r + 1]), samples=a["samples"][:, r:r + 1]), cut, f"row {r} alone")
    pair = [3, 5]                                                  # whichever other viewers the call holds
    duo = plan.spatial_user_divergence(mu=mu[:, pair], mv=mv[:, pair], window=20, stride=7)
    same(dict(divergence=np.ascontiguousarray(a["divergence"][:, pair][:, :, pair]), samples=a["samples"][pair]), duo, "viewers 3 and 5 alone")
    if kind != "naive":
        plan.close()


# ------------------------------------------------------------------------------------------- quirks
def test_quirks(native, engine, golden_dir):
    mu = np.full((40, 2), np.nan)
    mv = np.full((40, 2), np.nan)
    mu[7, 0], mv[7, 0] = 0.3, 0.4                                   # one sample in the whole video
    mu[:, 1], mv[:, 1] = np.linspace(0.1, 0.9, 40), 0.5
    pu = fib_plan(native, engine, [50], False)
    a = pu.spatial_user_divergence(mu=mu, mv=mv)
    div, samples = do.fast(mu, mv, W, H, [50], 40, 1, use_weight_distribution=False)
    assert a["samples"][:, 0].tolist() == [1, 40] and not np.isnan(a["divergence"]).any()      # unnormalised bits: one sample is fine
    close(a["divergence"], div, atol_of(pu), "one sample against forty")
    bad = mu.copy()
    bad[3, 1] = 1.5
    r = pu.spatial_user_divergence(mu=bad, mv=mv, check=False)
    assert r["code"] == native.VET_ERR_RANGE and r["samples"][:, 0].tolist() == [1, 39]        # outputs still written
    assert not np.isnan(r["divergence"]).any() and r["divergence"][0, 0, 1] > 0
    with pytest.raises(native.NativeError):
        pu.spatial_user_divergence(mu=bad, mv=mv)
    for window, stride in ((0, 1), (4, 0), (41, 1), (-1, 1)):
        with pytest.raises(ValueError):
            pu.spatial_user_divergence(mu=mu, mv=mv, window=window, stride=stride)
        e = np.zeros(8)
        rc = pu.lib.vet_user_divergence_host(pu.handle, native._ptr(mu), native._ptr(mv), None, 2, 40, window, stride, native._ptr(e), None)
        assert rc == native.VET_ERR_INVALID and pu.lib.vet_last_error()
    pu.close()
    # golden G12's configuration (power factor 150: in-FoV weights underflow to 0.0 and stay keys): the reference's NaN on pooled rows
    g = np.load(golden_dir / "g12_underflow.npz")
    px, py = g["px"], g["py"]
    present = px >= 0
    gm = np.where(present, np.where(px == W, 1.0, (px + 0.5) / W), np.nan)
    gv = np.where(present, np.where(py == H, 1.0, (py + 0.5) / H), np.nan)
    T = len(gm)
    window = min(T, 5)
    plan = fib_plan(native, engine, [500], True, 120.0, 150.0)
    res = plan.spatial_user_divergence(mu=gm, mv=gv, window=window, stride=window)
    div, samples = do.fast(gm, gv, W, H, [500], window, window, fov_angle=120.0, power_factor=150.0)
    both = (samples.T[:, :, None] > 0) & (samples.T[:, None, :] > 0)
    assert np.isnan(div[both]).any(), "the configuration no longer produces the reference's NaN on a row with samples"
    assert (~np.isnan(div[both])).any()
    assert np.array_equal(res["samples"], samples)
    close(res["divergence"], div, atol_of(plan), "G12 pooled")
    plan.close()


# ------------------------------------------------------------------------------------------- vet_user_entropy does not move
@pytest.mark.parametrize("weighted", [True, False])
def test_user_entropy_is_the_same_before_and_after(native, engine, weighted):
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(9, 150, base_seed=7, p_absent=0.1)
    plan = fib_plan(native, engine, [50, 100] if weighted else [50], weighted)
    before = plan.spatial_per_user(mu=mu, mv=mv, window=20, stride=7, want_weights=True)
    plan.spatial_user_divergence(mu=mu, mv=mv, window=20, stride=7)
    after = plan.spatial_per_user(mu=mu, mv=mv, window=20, stride=7, want_weights=True)
    for k in ("entropy", "weights", "samples"):
        assert before[k].tobytes() == after[k].tobytes(), k
    ent, samples, _ = uo.fast(mu, mv, W, H, [50, 100] if weighted else [50], 20, 7, use_weight_distribution=weighted)
    np.testing.assert_allclose(after["entropy"], ent, rtol=1e-6, atol=0, equal_nan=True)
    assert np.array_equal(after["samples"], samples)
    plan.close()
