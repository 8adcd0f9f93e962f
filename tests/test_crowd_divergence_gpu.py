"""GPU: the viewer-to-crowd divergence through the C-ABI (Plan.spatial_crowd_divergence -> vet_crowd_divergence_host, the device
entry, both analyzers).  D(u, r) is the Kullback-Leibler divergence, in bits, of viewer u's tile histogram of frames
[r * stride, r * stride + window) from the row's pooled histogram; per row pooled = within + between.  The references are golden
G20 (the real reference's dicts, tools/gen_golden_crowd_divergence.py) and the numpy oracles of tests/_crowd_oracle.py (pinned
against G20 in tests/test_crowd_divergence_surface.py).

Tolerances: ABSOLUTE, from tests/_tol.py's W_RTOL (a histogram entry may differ from the oracle's by W_RTOL relative):
  D(u, r)                      2 * (log2(n_max) + log2(W_r / W_u)) * W_RTOL: the cross entropy -sum q log2 p is bounded by
                               log2(n_max) + log2(W_r / W_u) (p_t >= q_t W_u / W_r), the own entropy by log2(n_max);
  pooled, within, between      2 * (log2(n_max) + log2(U)) * W_RTOL.
No relative tolerance: D goes to 0 for a typical viewer.  Where NaN sits and the integer samples must match exactly.  Every
comparison prints its largest absolute error."""
import ctypes

import numpy as np
import pytest

from oracle import vet_oracle as vo
from tests import _crowd_oracle as co
from tests import _user_oracle as uo
from tests import _window_oracle as wo
from tests._tol import W_RTOL

pytestmark = pytest.mark.gpu

W, H = 100, 200
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
def g20(golden_dir):
    return np.load(golden_dir / "g20_crowd_divergence.npz")


def fib_plan(native, engine, tcs, weighted=True, fov=120.0, power=2.0):
    return native.Plan(engine, [vo.fibonacci_lattice(t) for t in tcs], fov, power, weighted, W, H)


def naive_analyzer(weighted=True):
    from viewport_entropy_toolkit import NaiveSpatialEntropyAnalyzer
    from viewport_entropy_toolkit.config import EntropyConfig, NaiveAnalyzerConfig
    return NaiveSpatialEntropyAnalyzer(NaiveAnalyzerConfig(tile_height=10, tile_width=20, video_width=W, video_height=H,
                                                           entropy_config=EntropyConfig(use_weight_distribution=weighted)))


def n_max_of(plan):
    return max(plan.n_tiles)


def close(got, want, atol, msg=""):
    print(msg, "max abs err", float(np.nanmax(np.abs(got - want), initial=0.0)), "atol", float(np.min(atol)), "..", float(np.max(atol)))
    assert got.shape == want.shape, msg
    assert np.array_equal(np.isnan(got), np.isnan(want)), (msg, np.argwhere(np.isnan(got) != np.isnan(want))[:10])
    ok = ~np.isnan(want)
    bad = ok & (np.abs(np.where(ok, got - want, 0.0)) > atol)
    assert not bad.any(), (msg, np.argwhere(bad)[:10], got[bad][:10], want[bad][:10])


def check_result(res, div, series, samples, ratio, n_max, msg, rows=None):
    """res against the oracle's (div, series, samples, log2(W_r / W_u)); ``rows`` picks res's rows first."""
    pick = slice(None) if rows is None else rows
    U = res["divergence"].shape[0]
    assert np.array_equal(res["samples"][:, pick], samples), msg
    close(res["divergence"][:, pick], div, co.atol_div(n_max, ratio, W_RTOL), msg + " D")
    close(res["rows"][:, pick], series, co.atol_rows(n_max, U, W_RTOL), msg + " rows")
    check_structure(res)


def check_structure(res):
    """What every result must have, whatever the reference: NaN for viewers without a sample, NaN rows only where D is NaN for
    every viewer or a present viewer's D is, pooled = within + between."""
    D, rows, samples = res["divergence"], res["rows"], res["samples"]
    U = D.shape[0]
    assert np.isnan(D[samples == 0]).all()
    empty = samples.sum(axis=0) == 0
    assert np.isnan(rows[:, empty]).all()
    assert np.array_equal(np.isnan(rows[1]), np.isnan(rows[2]))
    assert not (np.isnan(rows[0]) & ~np.isnan(rows[1])).any()                          # pooled NaN -> within, between NaN
    assert np.array_equal(np.isnan(rows[2]), np.isnan(np.where(samples > 0, D, 0.0)).any(axis=0) | empty)
    return U


def ids_of(mu, mv):
    return uo.direction_ids(mu, mv, W, H)[0].astype(np.int32)


def g20_cases():
    for w, s in SHAPES:
        for flag, tcs in ((True, (50,)), (True, (50, 100, 200)), (False, (50,))):
            yield f"{'w' if flag else 'u'}_tc{'_'.join(map(str, tcs))}_w{w}_s{s}", flag, tcs, w, s
        yield f"naive_h10_w20_w{w}_s{s}", True, None, w, s


def check_g20(g20, tag, res, n_max, msg):
    rows = g20[f"{tag}__rows"]
    with np.errstate(all="ignore"):
        ratio = np.log2(g20[f"{tag}__pooled_total"][:, :, None] / g20[f"{tag}__own_total"]).mean(axis=1).T      # [U][m]
    check_result(res, g20[f"{tag}__divergence"], g20[f"{tag}__series"], g20[f"{tag}__samples"], ratio, n_max, msg, rows=rows)
    w, s = int(tag.split("_")[-2][1:]), int(tag.split("_")[-1][1:])
    r = np.arange(res["samples"].shape[1])
    gone = (r * s >= 100) & (r * s + w <= 200)
    assert not res["samples"][ABSENT_USER][gone].any() and np.isnan(res["divergence"][ABSENT_USER][gone]).all()


# ------------------------------------------------------------------------------------------- the reference (golden G20)
def test_host_entry_vs_reference_golden(native, engine, g16, g20):
    """Plan.spatial_crowd_divergence (vet_crowd_divergence_host), the grid and the ids entry points, every stored case."""
    mu, mv = g16["mu"], g16["mv"]
    ids = ids_of(mu, mv)
    plans = {}
    for tag, flag, tcs, w, s in g20_cases():
        key = (tcs, flag)
        if key not in plans:
            plans[key] = naive_analyzer(flag)._naive_plan() if tcs is None else fib_plan(native, engine, tcs, flag)
        plan = plans[key]
        res = plan.spatial_crowd_divergence(mu=mu, mv=mv, window=None if w == 300 else w, stride=s)
        R = uo.n_rows(300, w, s)
        assert res["code"] == native.VET_OK and res["divergence"].shape == (8, R) and res["rows"].shape == (3, R), tag
        assert res["samples"].shape == (8, R), tag
        check_g20(g20, tag, res, n_max_of(plan), tag + " grid")
        if tcs is not None:                 # a naive plan has no ids entry of its own table
            res = plan.spatial_crowd_divergence(ids=ids, window=w, stride=s)
            check_g20(g20, tag, res, n_max_of(plan), tag + " ids")
    for key, p in plans.items():
        if key[0] is not None:
            p.close()


def test_device_entry_vs_reference_golden(native, engine, g16, g20):
    """vet_crowd_divergence / vet_crowd_divergence_ids on device buffers; d_status = {0, (row, viewer) slots without a sample},
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
        for tag, flag, tcs, w, s in g20_cases():
            if tcs is None:
                continue
            plan = plans.get((tcs, flag)) or plans.setdefault((tcs, flag), fib_plan(native, engine, tcs, flag))
            R = uo.n_rows(T, w, s)
            for entry in ("grid", "ids"):
                div, rows, smp = np.empty((U, R)), np.empty((3, R)), np.empty((U, R), np.int32)
                st = np.array([0, 1000], np.int32)
                d_div, d_rows, d_s, d_st = dev(div.nbytes), dev(rows.nbytes), dev(smp.nbytes), dev(8, st)
                plan.spatial_crowd_divergence_device(d_mu.value, d_mv.value, U, T, w, s, d_div.value, d_rows.value, d_s.value,
                                                     d_st.value, d_ids=d_ids.value if entry == "ids" else 0)
                for h, d in ((div, d_div), (rows, d_rows), (smp, d_s), (st, d_st)):
                    assert lib.vet_memcpy_d2h(engine.handle, native._ptr(h), d, h.nbytes) == 0
                check_g20(g20, tag, dict(divergence=div, rows=rows, samples=smp), n_max_of(plan), f"{tag} device {entry}")
                assert st.tolist() == [0, 1000 + int((smp == 0).sum())], tag
    finally:
        engine.synchronize()
        for p in bufs:
            lib.vet_free(engine.handle, p)
        for p in plans.values():
            p.close()


def test_analyzers_vs_reference_golden(native, g16, g20):
    from viewport_entropy_toolkit import SpatialEntropyAnalyzer
    from viewport_entropy_toolkit.config import AnalyzerConfig, EntropyConfig
    mu, mv = g16["mu"], g16["mv"]
    times = np.arange(300) * 0.1
    names = [f"viewer{u}" for u in range(8)]
    ans = {}
    for tag, flag, tcs, w, s in g20_cases():
        if (tcs, flag) not in ans:
            an = (naive_analyzer(flag) if tcs is None else
                  SpatialEntropyAnalyzer(AnalyzerConfig(tile_counts=list(tcs), entropy_config=EntropyConfig(use_weight_distribution=flag))))
            an.load_arrays(times, mu, mv, user_names=names)
            ans[(tcs, flag)] = an
        an = ans[(tcs, flag)]
        df = an.compute_crowd_divergence(None if w == 300 else w, s)
        R = uo.n_rows(300, w, s)
        assert list(df.columns) == ["user", "time", "time_end", "divergence", "samples"] and len(df) == 8 * R
        assert df.attrs["users"] == names and df["user"].tolist() == [n for n in names for _ in range(R)]
        first = np.arange(R) * s
        assert np.array_equal(df["time"], np.tile(times[first], 8)) and np.array_equal(df["time_end"], np.tile(times[first + w - 1], 8))
        rows = df.attrs["rows"]
        assert list(rows.columns) == ["time", "time_end", "samples", "pooled", "within", "between"] and len(rows) == R
        assert np.array_equal(rows["time"], times[first]) and np.array_equal(rows["time_end"], times[first + w - 1])
        res = dict(divergence=df["divergence"].to_numpy().reshape(8, R), samples=df["samples"].to_numpy().reshape(8, R),
                   rows=np.stack([rows["pooled"], rows["within"], rows["between"]]))
        assert np.array_equal(rows["samples"], res["samples"].sum(axis=0))
        n_max = max(an._naive_plan().n_tiles) if tcs is None else max(tcs) + 1
        check_g20(g20, tag, res, n_max, tag + " analyzer")


# ------------------------------------------------------------------------------------------- viewer edges of k_crowd_rows
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("U", [1, 2, 63, 64, 65, 129])
def test_viewer_edges(native, engine, U, weighted):
    """One viewer, two, a ragged wave of viewers, a full one, a full one plus one and two plus one in k_crowd_rows; T = 40, the
    whole video; one viewer never present."""
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(U, 40, base_seed=500 + U, p_absent=0.1)
    if U > 1:
        gone = min(2, U - 1)
        mu[:, gone], mv[:, gone] = np.nan, np.nan                    # a viewer who never shows up
    plan = fib_plan(native, engine, [50], weighted)
    res = plan.spatial_crowd_divergence(mu=mu, mv=mv)
    div, series, samples, ratio = co.fast(mu, mv, W, H, [50], 40, 1, use_weight_distribution=weighted, want_ratio=True)
    assert res["divergence"].shape == (U, 1) and res["rows"].shape == (3, 1)
    check_result(res, div, series, samples, ratio, n_max_of(plan), f"U{U} weighted {weighted}")
    if U == 1:                                                       # the crowd is the viewer
        atol = co.atol_rows(n_max_of(plan), 1, W_RTOL)
        assert abs(res["divergence"][0, 0]) <= atol and abs(res["rows"][2, 0]) <= atol
    else:
        assert np.isnan(res["divergence"][gone, 0]) and res["samples"][gone, 0] == 0
    plan.close()


# ------------------------------------------------------------------------------------------- tile and wave-split edges
@pytest.mark.parametrize("window", [20, 100, 150])
@pytest.mark.parametrize("tcs", [(200,), (1000,), (50, 100, 200)])
def test_tile_and_wave_split_edges(native, engine, tcs, window):
    """201 and 1001 tiles (lanes along t: ragged last pass) and three lattices added in lattice order, at windows of 20, 100 and
    150 frames (1, 2 and 4 waves per (row, viewer) workgroup); U = 9, T = 150, stride 7; a viewer absent over frames 40-75."""
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(9, 150, base_seed=7, p_absent=0.1)
    mu[40:75, 2], mv[40:75, 2] = np.nan, np.nan
    plan = fib_plan(native, engine, list(tcs), True)
    res = plan.spatial_crowd_divergence(mu=mu, mv=mv, window=window, stride=7)
    div, series, samples, ratio = co.fast(mu, mv, W, H, list(tcs), window, 7, want_ratio=True)
    assert (samples == 0).any() == (window == 20)
    check_result(res, div, series, samples, ratio, n_max_of(plan), f"tcs {tcs} window {window}")
    plan.close()


# ------------------------------------------------------------------------------------------- row chunks
@pytest.mark.parametrize("kind", ["weighted3", "unweighted"])
def test_row_chunks_do_not_change_a_bit(native, engine, kind):
    """U = 65, T = 60, window 20, stride 1 (41 rows): 1 and 7 rows at a time (41 and 6 chunks, the last one ragged) against the
    default (one chunk)."""
    from viewport_entropy_toolkit import _synthetic
    U = 65
    mu, mv = _synthetic.random_walk_video(U, 60, base_seed=61, p_absent=0.1)
    mu[10:45, 4], mv[10:45, 4] = np.nan, np.nan
    plan = fib_plan(native, engine, [50, 100, 200] if kind == "weighted3" else [50], kind != "unweighted")
    try:
        a = plan.spatial_crowd_divergence(mu=mu, mv=mv, window=20, stride=1)
        assert a["divergence"].shape == (U, 41) and (a["samples"] == 0).any()
        check_structure(a)
        assert not np.isnan(a["rows"]).any() and (a["rows"][2] > 0).all()
        for rows in (1, 7):
            engine.test_crowd_divergence_chunk_rows(rows)
            b = plan.spatial_crowd_divergence(mu=mu, mv=mv, window=20, stride=1)
            for k in ("divergence", "rows", "samples"):
                assert a[k].tobytes() == b[k].tobytes(), (rows, k)
    finally:
        engine.test_crowd_divergence_chunk_rows(0)
        plan.close()


# ------------------------------------------------------------------------------------------- purity
@pytest.mark.parametrize("kind", ["weighted", "weighted3", "unweighted", "naive"])
def test_values_are_pure_functions_of_the_rows_frames(native, engine, kind):
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(9, 150, base_seed=7, p_absent=0.1)
    mu[40:75, 2], mv[40:75, 2] = np.nan, np.nan
    ids = ids_of(mu, mv)
    plan = (naive_analyzer(False)._naive_plan() if kind == "naive" else
            fib_plan(native, engine, [50, 100, 200] if kind == "weighted3" else [50], kind != "unweighted"))

    def same(x, y, msg):
        for k in ("divergence", "rows", "samples"):
            assert np.ascontiguousarray(x[k]).tobytes() == np.ascontiguousarray(y[k]).tobytes(), (msg, k)

    def cols(x, pick):
        return {k: x[k][:, pick] for k in ("divergence", "rows", "samples")}

    a = plan.spatial_crowd_divergence(mu=mu, mv=mv, window=20, stride=7)
    same(a, plan.spatial_crowd_divergence(mu=mu, mv=mv, window=20, stride=7), "run to run")
    one = plan.spatial_crowd_divergence(mu=mu, mv=mv, window=20, stride=1)
    same(a, cols(one, slice(None, None, 7)), "the rows of the same frames at stride 1")
    if kind != "naive":
        same(a, plan.spatial_crowd_divergence(ids=ids, window=20, stride=7), "ids entry")
    for r in (0, 5, 7, a["divergence"].shape[1] - 1):              # a call that holds only the row's 20 frames
        cut = plan.spatial_crowd_divergence(mu=mu[7 * r:7 * r + 20], mv=mv[7 * r:7 * r + 20], window=20)
        same(cols(a, slice(r, r + 1)), cut, f"row {r} alone")
    if kind != "naive":
        plan.close()


# ------------------------------------------------------------------------------------------- properties
def bits_rows(weights):
    """S in bits of every row of dense weights [..., n] (include/vet.h's encoding: -0.0 = a key whose value is 0.0)."""
    keys = (weights != 0) | np.signbit(weights)
    h = np.abs(weights)
    with np.errstate(all="ignore"):
        Wt = h.sum(axis=-1)
        q = np.where(keys, h / Wt[..., None], 1.0)
        return -(q * np.log2(q)).sum(axis=-1), Wt


@pytest.mark.parametrize("kind", ["weighted", "unweighted", "naive"])
def test_properties(native, engine, kind):
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(12, 90, base_seed=19, p_absent=0.15)
    mu[20:60, 1], mv[20:60, 1] = np.nan, np.nan
    plan = naive_analyzer(False)._naive_plan() if kind == "naive" else fib_plan(native, engine, [50], kind == "weighted")
    n_max = n_max_of(plan)
    res = plan.spatial_crowd_divergence(mu=mu, mv=mv, window=20, stride=5)
    D, rows = res["divergence"], res["rows"]
    check_structure(res)
    own, Wu = bits_rows(plan.spatial_per_user(mu=mu, mv=mv, window=20, stride=5, want_weights=True)["weights"])      # [U][R]
    pooled, Wr = bits_rows(plan.spatial_windowed(mu=mu, mv=mv, window=20, stride=5, want_weights=True)["weights"])   # [R]
    with np.errstate(all="ignore"):
        bound = np.log2(Wr[None, :] / Wu)
    atol = co.atol_div(n_max, bound, W_RTOL)
    ok = ~np.isnan(D)
    assert ok.any() and np.array_equal(ok, res["samples"] > 0)
    assert (D[ok] >= -atol[ok]).all() and (D[ok] <= bound[ok] + atol[ok]).all()
    row_atol = co.atol_rows(n_max, 12, W_RTOL)
    print(kind, "min D", float(D[ok].min()), "max D - bound", float((D[ok] - bound[ok]).max()),
          "identity", float(np.abs(rows[0] - (rows[1] + rows[2])).max()),
          "pooled", float(np.abs(rows[0] - pooled).max()), "row atol", row_atol)
    assert not np.isnan(rows).any()
    assert (np.abs(rows[0] - (rows[1] + rows[2])) <= row_atol).all()
    assert (np.abs(rows[0] - pooled) <= row_atol).all()
    within = np.where(ok, Wu / Wr[None, :] * np.where(ok, own, 0.0), 0.0).sum(axis=0)
    print(kind, "within", float(np.abs(rows[1] - within).max()))
    assert (np.abs(rows[1] - within) <= row_atol).all()
    assert (rows[2] > 0.01).all()                                                      # these viewers do differ
    # an audience of identical columns: everybody is the crowd
    same_mu, same_mv = np.repeat(mu[:, 4:5], 12, axis=1), np.repeat(mv[:, 4:5], 12, axis=1)
    twin = plan.spatial_crowd_divergence(mu=same_mu, mv=same_mv, window=20, stride=5)
    tD, tok = twin["divergence"], ~np.isnan(twin["divergence"])
    print(kind, "identical columns: max |D|", float(np.abs(tD[tok]).max()), "max |between|", float(np.nanmax(np.abs(twin["rows"][2]))))
    assert tok.any() and (np.abs(tD[tok]) <= co.atol_div(n_max, np.log2(12.0), W_RTOL)).all()
    assert (np.abs(twin["rows"][2][~np.isnan(twin["rows"][2])]) <= row_atol).all()
    if kind != "naive":
        plan.close()


@pytest.mark.parametrize("weighted", [True, False])
def test_lone_viewer_gives_the_log_of_the_mass_ratio(native, engine, weighted):
    """One viewer held at longitude -90 under a 30 degree field of view shares no tile with the three held at +90:
    D = log2(W / W_0) for the lone one, log2(W / (W - W_0)) for the others (who share every tile in the same proportions)."""
    T = 40
    mu = np.stack([np.full(T, 0.25), np.full(T, 0.75), np.full(T, 0.75), np.full(T, 0.75)], axis=1)
    mv = np.full((T, 4), 0.5)
    mu[10:, 3], mv[10:, 3] = np.nan, np.nan                                            # viewer 3: 10 samples
    plan = fib_plan(native, engine, [500], weighted, fov=30.0)
    res = plan.spatial_crowd_divergence(mu=mu, mv=mv)
    D = res["divergence"][:, 0]
    assert res["samples"][:, 0].tolist() == [40, 40, 40, 10]
    if weighted:
        Wu = np.abs(plan.spatial_per_user(mu=mu, mv=mv, want_weights=True)["weights"]).sum(axis=2)[:, 0]
    else:
        Wu = res["samples"][:, 0].astype(np.float64)
    Wr = Wu.sum()
    ratio = np.log2(Wr / Wu)
    atol = co.atol_div(n_max_of(plan), ratio, W_RTOL)
    want = np.array([np.log2(Wr / Wu[0])] + [np.log2(Wr / (Wr - Wu[0]))] * 3)
    print("weighted", weighted, "masses", Wu, "D - want", D - want, "atol", atol)
    assert (np.abs(D - want) <= atol).all()
    if not weighted:
        assert want[0] == np.log2(130 / 40) and want[1] == np.log2(130 / 90)
    rows = res["rows"][:, 0]
    assert abs(rows[0] - (rows[1] + rows[2])) <= co.atol_rows(n_max_of(plan), 4, W_RTOL)
    plan.close()


# ------------------------------------------------------------------------------------------- quirks
def test_quirks(native, engine, golden_dir):
    mu = np.full((40, 2), np.nan)
    mv = np.full((40, 2), np.nan)
    mu[7, 0], mv[7, 0] = 0.3, 0.4                                   # one sample in the whole video
    mu[:, 1], mv[:, 1] = np.linspace(0.1, 0.9, 40), 0.5
    pu = fib_plan(native, engine, [50], False)
    a = pu.spatial_crowd_divergence(mu=mu, mv=mv)
    div, series, samples, ratio = co.fast(mu, mv, W, H, [50], 40, 1, use_weight_distribution=False, want_ratio=True)
    assert a["samples"][:, 0].tolist() == [1, 40] and not np.isnan(a["divergence"]).any()
    check_result(a, div, series, samples, ratio, n_max_of(pu), "one sample against forty")
    bad = mu.copy()
    bad[3, 1] = 1.5
    r = pu.spatial_crowd_divergence(mu=bad, mv=mv, check=False)
    assert r["code"] == native.VET_ERR_RANGE and r["samples"][:, 0].tolist() == [1, 39]        # outputs still written
    assert not np.isnan(r["divergence"]).any() and r["divergence"][0, 0] > 0 and not np.isnan(r["rows"]).any()
    with pytest.raises(native.NativeError):
        pu.spatial_crowd_divergence(mu=bad, mv=mv)
    for window, stride in ((0, 1), (4, 0), (41, 1), (-1, 1)):
        with pytest.raises(ValueError):
            pu.spatial_crowd_divergence(mu=mu, mv=mv, window=window, stride=stride)
        e = np.zeros(8)
        rc = pu.lib.vet_crowd_divergence_host(pu.handle, native._ptr(mu), native._ptr(mv), None, 2, 40, window, stride,
                                              native._ptr(e), None, None)
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
    res = plan.spatial_crowd_divergence(mu=gm, mv=gv, window=window, stride=window)
    div, series, samples, ratio = co.fast(gm, gv, W, H, [500], window, window, fov_angle=120.0, power_factor=150.0, want_ratio=True)
    has = samples > 0
    assert np.isnan(div[has]).any(), "the configuration no longer produces the reference's NaN on a slot with samples"
    assert (~np.isnan(div[has])).any()
    check_result(res, div, series, samples, ratio, n_max_of(plan), "G12 pooled")
    plan.close()


# ------------------------------------------------------------------------------------------- the neighbours do not move
@pytest.mark.parametrize("weighted", [True, False])
def test_neighbours_are_the_same_before_and_after(native, engine, weighted):
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(9, 150, base_seed=7, p_absent=0.1)
    plan = fib_plan(native, engine, [50, 100] if weighted else [50], weighted)

    def neighbours():
        return (plan.spatial_per_user(mu=mu, mv=mv, window=20, stride=7, want_weights=True),
                plan.spatial_windowed(mu=mu, mv=mv, window=20, stride=7, want_weights=True),
                plan.spatial_user_divergence(mu=mu, mv=mv, window=20, stride=7))

    before = neighbours()
    plan.spatial_crowd_divergence(mu=mu, mv=mv, window=20, stride=7)
    after = neighbours()
    for b, a in zip(before, after):
        for k in b:
            if isinstance(b[k], np.ndarray):
                assert b[k].tobytes() == a[k].tobytes(), k
    ent, samples, _ = uo.fast(mu, mv, W, H, [50, 100] if weighted else [50], 20, 7, use_weight_distribution=weighted)
    np.testing.assert_allclose(after[0]["entropy"], ent, rtol=1e-6, atol=0, equal_nan=True)
    went, wsamples, _ = wo.fast(mu, mv, W, H, [50, 100] if weighted else [50], 20, 7, use_weight_distribution=weighted)
    np.testing.assert_allclose(after[1]["entropy"], went, rtol=1e-6, atol=0, equal_nan=True)
    assert np.array_equal(after[0]["samples"], samples) and np.array_equal(after[1]["samples"], wsamples)
    plan.close()
