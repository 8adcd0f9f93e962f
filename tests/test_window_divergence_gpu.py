"""GPU: the window-to-window attention divergence through the C-ABI (Plan.spatial_window_divergence -> vet_window_divergence_host,
the device entries, both analyzers).  D(r, l) is the mass-weighted Jensen-Shannon divergence, in bits, of the pooled tile
histograms of rows r and r + l (frames [r * stride, r * stride + window) each); the references are golden G19 (the real
reference's dicts, tools/gen_golden_window_divergence.py) and the numpy oracles of tests/_window_divergence_oracle.py (pinned
against G19 in tests/test_window_divergence_surface.py).

Tolerance: ABSOLUTE, atol = 2 * log2(n_max) * W_RTOL (1.1e-8 bits at 51 tiles): a histogram entry may differ from the oracle's by
tests/_tol.py's W_RTOL relative, and D is a difference of entropies of at most log2(n) bits each.  No relative tolerance: D goes
to 0 for similar windows.  Where NaN sits and the integer samples must match exactly.  Every comparison prints its largest
absolute error."""
import ctypes

import numpy as np
import pytest

from oracle import vet_oracle as vo
from tests import _window_divergence_oracle as wdo
from tests import _window_oracle as wo
from tests._tol import W_RTOL

pytestmark = pytest.mark.gpu

W, H = 100, 200
# k_window_divergence's block shapes (rows RB x lags LB, tiles per LDS stage TC) and the largest max_lag each one serves
KERNEL_SHAPES = ((256, 1, 8), (32, 8, 32), (8, 32, 32))
SHAPE_MAX_LAG = (1, 8, None)
SHAPES = ((20, 20, 14), (20, 5, 8), (5, 1, 6), (1, 1, 3))          # golden G19: (window, stride, max_lag)
KINDS = ("weighted", "unweighted", "naive")


@pytest.fixture(scope="module")
def native():
    from viewport_entropy_toolkit import _native
    return _native


@pytest.fixture(scope="module")
def engine(native):
    return native.Engine.default()


@pytest.fixture(scope="module")
def g14(golden_dir):
    return np.load(golden_dir / "g14_windowed.npz")


@pytest.fixture(scope="module")
def g19(golden_dir):
    return np.load(golden_dir / "g19_window_divergence.npz")


def fib_plan(native, engine, tcs, weighted=True, fov=120.0, power=2.0):
    return native.Plan(engine, [vo.fibonacci_lattice(t) for t in tcs], fov, power, weighted, W, H)


def naive_analyzer(weighted=True):
    from viewport_entropy_toolkit import NaiveSpatialEntropyAnalyzer
    from viewport_entropy_toolkit.config import EntropyConfig, NaiveAnalyzerConfig
    return NaiveSpatialEntropyAnalyzer(NaiveAnalyzerConfig(tile_height=10, tile_width=20, video_width=W, video_height=H,
                                                           entropy_config=EntropyConfig(use_weight_distribution=weighted)))


def plan_of(native, engine, kind):
    if kind == "naive":
        return naive_analyzer(False)._naive_plan()
    return fib_plan(native, engine, [50, 100, 200] if kind == "weighted3" else [50], kind != "unweighted")


def done(plan, kind):
    if kind != "naive":
        plan.close()


def oracle_of(kind, mu, mv, w, s, L):
    if kind == "naive":
        return wdo.naive(mu, mv, W, H, 10, 20, w, s, L)
    return wdo.fast(mu, mv, W, H, [50, 100, 200] if kind == "weighted3" else [50], w, s, L,
                    use_weight_distribution=kind != "unweighted")


def atol_of(plan):
    return 2.0 * np.log2(max(plan.n_tiles)) * W_RTOL


def close(got, want, atol, msg=""):
    print(msg, "max abs err", float(np.nanmax(np.abs(got - want), initial=0.0)), "atol", atol)
    assert got.shape == want.shape, msg
    assert np.array_equal(np.isnan(got), np.isnan(want)), (msg, np.argwhere(np.isnan(got) != np.isnan(want))[:10])
    np.testing.assert_allclose(got, want, rtol=0, atol=atol, equal_nan=True, err_msg=msg)


def ids_of(mu, mv):
    return wo._ids(mu, mv, W, H)[0].astype(np.int32)


def structural(R, L):
    return np.arange(R)[:, None] + np.arange(1, L + 1)[None, :] >= R


def video(U, T, seed, p_absent=0.0):
    from viewport_entropy_toolkit import _synthetic
    return _synthetic.random_walk_video(U, T, base_seed=seed, p_absent=p_absent)


class Device:
    """Device buffers for the device entries; everything is freed by close()."""

    def __init__(self, native, engine):
        self.native, self.engine, self.lib, self.bufs = native, engine, engine.lib, []

    def put(self, nbytes, src=None):
        p = ctypes.c_void_p()
        assert self.lib.vet_malloc(self.engine.handle, nbytes, ctypes.byref(p)) == 0
        self.bufs.append(p)
        if src is not None:
            assert self.lib.vet_memcpy_h2d(self.engine.handle, p, self.native._ptr(src), nbytes) == 0
        return p

    def run(self, plan, U, T, w, s, L, d_mu=None, d_mv=None, d_ids=None, status0=(0, 1000)):
        R = wo.n_rows(T, w, s)
        div, smp, st = np.empty((R, L)), np.empty(R, np.int32), np.array(status0, np.int32)
        d_div, d_s, d_st = self.put(div.nbytes), self.put(smp.nbytes), self.put(8, st)
        plan.spatial_window_divergence_device(d_mu.value if d_mu else 0, d_mv.value if d_mv else 0, U, T, w, s, L, d_div.value,
                                              d_s.value, d_st.value, d_ids=d_ids.value if d_ids else 0)
        for h, d in ((div, d_div), (smp, d_s), (st, d_st)):
            assert self.lib.vet_memcpy_d2h(self.engine.handle, self.native._ptr(h), d, h.nbytes) == 0
        return div, smp, st

    def close(self):
        self.engine.synchronize()
        for p in self.bufs:
            self.lib.vet_free(self.engine.handle, p)


# ------------------------------------------------------------------------------------------- 1 the reference (golden G19)
def g19_cases():
    for w, s, L in SHAPES:
        for flag, tcs in ((True, (50,)), (True, (50, 100, 200)), (False, (50,))):
            yield f"{'w' if flag else 'u'}_tc{'_'.join(map(str, tcs))}_w{w}_s{s}_l{L}", flag, tcs, w, s, L
        yield f"naive_h10_w20_w{w}_s{s}_l{L}", True, None, w, s, L


def check_g19(g19, tag, div, samples, windowed_samples, atol, msg):
    rows = g19[f"{tag}__rows"]
    close(div[rows], g19[f"{tag}__divergence"], atol, msg)
    assert np.array_equal(samples[rows], g19[f"{tag}__samples"]), msg
    assert np.array_equal(samples, windowed_samples), msg
    assert np.array_equal(np.isnan(div), structural(*div.shape)), msg     # this dataset: NaN only where there is no partner row


def test_host_and_device_entries_vs_reference_golden(native, engine, g14, g19):
    """Plan.spatial_window_divergence (vet_window_divergence_host) and the device entries, grid and ids, every stored case;
    d_status = {0, rows without a sample}, added to."""
    mu, mv = np.ascontiguousarray(g14["mu_absent"]), np.ascontiguousarray(g14["mv_absent"])
    ids = ids_of(mu, mv)
    T, U = mu.shape
    dev = Device(native, engine)
    d_mu, d_mv, d_ids = dev.put(mu.nbytes, mu), dev.put(mv.nbytes, mv), dev.put(ids.nbytes, ids)
    plans = {}
    try:
        for tag, flag, tcs, w, s, L in g19_cases():
            key = (tcs, flag)
            if key not in plans:
                plans[key] = naive_analyzer(flag)._naive_plan() if tcs is None else fib_plan(native, engine, tcs, flag)
            plan = plans[key]
            R = wo.n_rows(T, w, s)
            ws = plan.spatial_windowed(mu=mu, mv=mv, window=w, stride=s)["samples"]
            res = plan.spatial_window_divergence(mu=mu, mv=mv, window=w, stride=s, max_lag=L)
            assert res["code"] == native.VET_OK and res["divergence"].shape == (R, L) and res["samples"].shape == (R,), tag
            check_g19(g19, tag, res["divergence"], res["samples"], ws, atol_of(plan), tag + " host grid")
            div, smp, st = dev.run(plan, U, T, w, s, L, d_mu=d_mu, d_mv=d_mv)
            check_g19(g19, tag, div, smp, ws, atol_of(plan), tag + " device grid")
            assert st.tolist() == [0, 1000] and div.tobytes() == res["divergence"].tobytes(), tag
            if tcs is not None:                 # a naive plan has no ids entry of its own table
                res = plan.spatial_window_divergence(ids=ids, window=w, stride=s, max_lag=L)
                check_g19(g19, tag, res["divergence"], res["samples"], ws, atol_of(plan), tag + " host ids")
                div, smp, st = dev.run(plan, U, T, w, s, L, d_ids=d_ids)
                check_g19(g19, tag, div, smp, ws, atol_of(plan), tag + " device ids")
                assert st.tolist() == [0, 1000], tag
    finally:
        dev.close()
        for key, p in plans.items():
            if key[0] is not None:
                p.close()


def test_analyzers_vs_reference_golden(native, g14, g19):
    from viewport_entropy_toolkit import SpatialEntropyAnalyzer
    from viewport_entropy_toolkit.config import AnalyzerConfig, EntropyConfig
    mu, mv = g14["mu_absent"], g14["mv_absent"]
    times = np.arange(300) * 0.1
    ans = {}
    for tag, flag, tcs, w, s, L in g19_cases():
        if (tcs, flag) not in ans:
            an = (naive_analyzer(flag) if tcs is None else
                  SpatialEntropyAnalyzer(AnalyzerConfig(tile_counts=list(tcs), entropy_config=EntropyConfig(use_weight_distribution=flag))))
            an.load_arrays(times, mu, mv)
            ans[(tcs, flag)] = an
        an = ans[(tcs, flag)]
        df = an.compute_window_divergence(w, s, L)
        R = wo.n_rows(300, w, s)
        assert list(df.columns) == ["time", "time_end", "samples", "shift", "divergence"] and len(df) == R
        assert df.attrs["lags"] == list(range(1, L + 1)) and df.attrs["lag_frames"] == [s * l for l in range(1, L + 1)]
        assert np.array_equal(df["time"], times[np.arange(R) * s]) and np.array_equal(df["time_end"], times[np.arange(R) * s + w - 1])
        whole = df["divergence"][0].base
        assert whole is not None and whole.shape == (R, L) and all(df["divergence"][r].base is whole for r in range(R))   # views into ONE array
        assert np.array_equal(df["shift"], whole[:, 0], equal_nan=True)
        n_max = max(an._naive_plan().n_tiles) if tcs is None else max(tcs) + 1
        ws = an.compute_windowed_entropy(w, s)["samples"].to_numpy()
        check_g19(g19, tag, whole, df["samples"].to_numpy(), ws, 2.0 * np.log2(n_max) * W_RTOL, tag + " analyzer")


# ------------------------------------------------------------------------------------------- 2 band and block edges
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", range(len(KERNEL_SHAPES)))
def test_band_and_block_edges(native, engine, kind, shape):
    """Per kernel shape: one pair, a ragged, a full, a full plus one and two-and-a-bit row blocks; lags 1, one short of a lag block,
    a full one, one more, and the whole band.  window = stride = 1, U = 4, T = R; no absences, so NaN is structural only."""
    RB, LB, _ = KERNEL_SHAPES[shape]
    lo = 1 if shape == 0 else SHAPE_MAX_LAG[shape - 1] + 1
    plan = plan_of(native, engine, kind)
    atol = atol_of(plan)
    for R in sorted({2, RB - 1, RB, RB + 1, 2 * RB + 1}):
        mu, mv = video(4, R, 900 + R)
        want, samples = oracle_of(kind, mu, mv, 1, 1, R - 1)
        assert (samples == 4).all()
        edges = {L for _, lb, _ in KERNEL_SHAPES for L in (lb - 1, lb, lb + 1)}          # every shape's lag-block edges
        lags = sorted(L for L in edges | {1, R - 1, lo} if 1 <= L <= R - 1)
        for L in lags:
            res = plan.spatial_window_divergence(mu=mu, mv=mv, window=1, stride=1, max_lag=L)
            close(res["divergence"], want[:, :L], atol, f"{kind} shape {KERNEL_SHAPES[shape]} R{R} L{L}")
            assert np.array_equal(np.isnan(res["divergence"]), structural(R, L))
            assert np.array_equal(res["samples"], samples)
    done(plan, kind)


# ------------------------------------------------------------------------------------------- 3 tile-chunk edges, several lattices
@pytest.mark.parametrize("tcs", [(200,), (1000,), (50, 100, 200)])
def test_tile_chunk_edges_and_several_lattices(native, engine, tcs):
    """201 and 1001 tiles (neither a multiple of a stage of 8 or 32 tiles, both more than one stage) and three lattices added in
    lattice order; U = 8, T = 150, window 20, stride 7 (19 rows), every kernel shape."""
    mu, mv = video(8, 150, 7, p_absent=0.1)
    plan = fib_plan(native, engine, list(tcs), True)
    want, samples = wdo.fast(mu, mv, W, H, list(tcs), 20, 7, 18)
    for _, LB, TC in KERNEL_SHAPES:
        assert all((t + 1) % TC and t + 1 > TC for t in tcs)
    for L in (1, 5, 18):
        res = plan.spatial_window_divergence(mu=mu, mv=mv, window=20, stride=7, max_lag=L)
        assert np.array_equal(res["samples"], samples)
        close(res["divergence"], want[:, :L], atol_of(plan), f"tcs {tcs} L{L}")
    plan.close()


# ------------------------------------------------------------------------------------------- 4 row chunks
@pytest.mark.parametrize("kind", ["weighted3", "unweighted"])
def test_row_chunks_do_not_change_a_bit(native, engine, kind):
    """U = 8, T = 60, window 20, stride 1 (41 rows): pair rows 1, 3 and 41 at a time against the default, with lags that reach
    across several chunks (the halo), one per kernel shape."""
    mu, mv = video(8, 60, 61, p_absent=0.1)
    mu[10:32], mv[10:32] = np.nan, np.nan                           # rows 10..12 have no sample
    plan = plan_of(native, engine, kind)
    dev = Device(native, engine)
    d_mu, d_mv = dev.put(mu.nbytes, mu), dev.put(mv.nbytes, mv)
    try:
        for L in (1, 5, 9):
            a = dev.run(plan, 8, 60, 20, 1, L, d_mu=d_mu, d_mv=d_mv)
            assert a[0].shape == (41, L) and (a[1] == 0).sum() == 3 and a[2].tolist() == [0, 1003]
            for rows in (1, 3, 41):
                engine.test_window_divergence_chunk_rows(rows)
                b = dev.run(plan, 8, 60, 20, 1, L, d_mu=d_mu, d_mv=d_mv)
                assert a[0].tobytes() == b[0].tobytes(), (L, rows)
                assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), (L, rows)      # every row booked once
            engine.test_window_divergence_chunk_rows(0)
    finally:
        engine.test_window_divergence_chunk_rows(0)
        dev.close()
        done(plan, kind)


# ------------------------------------------------------------------------------------------- 5 purity
@pytest.mark.parametrize("kind", ["weighted", "weighted3", "unweighted", "naive"])
def test_pairs_are_pure_functions_of_their_two_rows(native, engine, kind):
    mu, mv = video(8, 150, 7, p_absent=0.1)
    plan = plan_of(native, engine, kind)
    call = lambda m, v, w, s, L: plan.spatial_window_divergence(mu=m, mv=v, window=w, stride=s, max_lag=L)["divergence"]
    w, s = 10, 3                                                    # 47 rows, overlapping windows
    R = wo.n_rows(150, w, s)
    full = call(mu, mv, w, s, R - 1)
    assert full.tobytes() == call(mu, mv, w, s, R - 1).tobytes(), "run to run"
    for L in (1, 7, 8, 9, 20):                                      # the columns of a shorter band, across the kernel shapes
        short = call(mu, mv, w, s, L)
        ok = ~structural(R, L)
        assert short[ok].tobytes() == full[:, :L][ok].tobytes(), f"max_lag {L} against {R - 1}"
        assert np.isnan(short[~ok]).all()
    if kind != "naive":
        ids = ids_of(mu, mv)
        assert plan.spatial_window_divergence(ids=ids, window=w, stride=s, max_lag=9)["divergence"].tobytes() == call(mu, mv, w, s, 9).tobytes()
    rng = np.random.default_rng(5)                                  # frames outside rows r and r + l do not matter
    for r, l in ((0, 1), (5, 9), (20, 3), (30, 16)):
        m2, v2 = rng.random(mu.shape), rng.random(mv.shape)
        for f0 in (r * s, (r + l) * s):
            m2[f0:f0 + w], v2[f0:f0 + w] = mu[f0:f0 + w], mv[f0:f0 + w]
        other = call(m2, v2, w, s, 16)
        assert other[r, l - 1].tobytes() == full[r, l - 1].tobytes(), (r, l)
    for k in (1, 4):                                                # dropping the first k * stride frames shifts the rows by k
        cut = call(mu[k * s:], mv[k * s:], w, s, 9)
        ok = ~structural(R - k, 9)
        assert cut[ok].tobytes() == full[k:, :9][ok].tobytes(), k
    twice = call(mu, mv, w, 2 * s, 5)                               # stride 2 s at L = even rows and even lags of stride s at 2 L
    R2 = wo.n_rows(150, w, 2 * s)
    ok = ~structural(R2, 5)
    assert twice[ok].tobytes() == np.ascontiguousarray(full[::2, 1:10:2])[:R2][ok].tobytes()
    done(plan, kind)


# ------------------------------------------------------------------------------------------- 6 time reversal
@pytest.mark.parametrize("kind", KINDS)
def test_time_reversal(native, engine, kind):
    """The reversed video has the same windows in reverse order: D_rev[R - 1 - r - l][l - 1] = D[r][l - 1] — bit for bit on counts
    (exact, and every pair operation is commutative), within atol on weighted plans (the frame order of the FP64 sums changes)."""
    mu, mv = video(8, 146, 23, p_absent=0.1)                        # (146 - 20) % 7 == 0: the reversed rows are the same windows
    plan = plan_of(native, engine, kind)
    w, s, L = 20, 7, 11
    R = wo.n_rows(146, w, s)
    D = plan.spatial_window_divergence(mu=mu, mv=mv, window=w, stride=s, max_lag=L)["divergence"]
    Dr = plan.spatial_window_divergence(mu=mu[::-1].copy(), mv=mv[::-1].copy(), window=w, stride=s, max_lag=L)["divergence"]
    back = np.full_like(D, np.nan)
    for l in range(1, L + 1):
        back[:R - l, l - 1] = Dr[:R - l, l - 1][::-1]
    if kind == "weighted":
        close(back, D, atol_of(plan), "weighted reversal")
    else:
        assert back.tobytes() == D.tobytes(), kind
    done(plan, kind)


# ------------------------------------------------------------------------------------------- 7 properties
def masses(plan, mu, mv, w, s):
    """W[R] of lattice 0: the totals of the windowed call's pooled histograms."""
    return np.abs(plan.spatial_windowed(mu=mu, mv=mv, window=w, stride=s, want_weights=True)["weights"]).sum(axis=1)


def bound_of(Wm, L):
    R = len(Wm)
    out = np.full((R, L), np.nan)
    with np.errstate(all="ignore"):
        for l in range(1, L + 1):
            out[:R - l, l - 1] = wdo.h2(Wm[:R - l] / (Wm[:R - l] + Wm[l:]))
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_bounds_and_a_static_audience(native, engine, kind):
    mu, mv = video(8, 120, 19, p_absent=0.15)
    plan = plan_of(native, engine, kind)
    atol = atol_of(plan)
    D = plan.spatial_window_divergence(mu=mu, mv=mv, window=20, stride=5, max_lag=12)["divergence"]
    bound = bound_of(masses(plan, mu, mv, 20, 5), 12)
    ok = ~np.isnan(D)
    assert np.array_equal(ok, ~structural(*D.shape)) and (D[ok] >= -atol).all() and (D[ok] <= bound[ok] + atol).all()
    print(kind, "min D", float(D[ok].min()), "max D - bound", float((D[ok] - bound[ok]).max()))
    rng = np.random.default_rng(3)                                  # every viewer holds one direction: nothing ever moves
    mu, mv = np.repeat(rng.random((1, 8)), 60, axis=0), np.repeat(rng.random((1, 8)), 60, axis=0)
    for L in (1, 4, 11):
        D = plan.spatial_window_divergence(mu=mu, mv=mv, window=5, stride=5, max_lag=L)["divergence"]
        ok = ~structural(12, L)
        print(kind, "static audience, max |D|", float(np.abs(D[ok]).max()))
        assert not np.isnan(D[ok]).any() and (np.abs(D[ok]) <= atol).all()
    done(plan, kind)


@pytest.mark.parametrize("weighted", [True, False])
def test_a_jump_to_the_antipode_gives_the_binary_entropy_of_the_masses(native, engine, weighted):
    """Everyone on one point of the equator for the first half and on its antipode for the second, under a 30 degree field of
    view: the windows across the cut share no tile, D = H2(mass split) (1.0 for equal masses); within a half D = 0."""
    T, U, w = 40, 6, 5
    mu = np.full((T, U), 0.25)
    mu[T // 2:] = 0.75
    mv = np.full((T, U), 0.5)
    mu[30:35, :3], mv[30:35, :3] = np.nan, np.nan                   # row 6 has half the samples
    plan = fib_plan(native, engine, [500], weighted, fov=30.0)
    atol = atol_of(plan)
    res = plan.spatial_window_divergence(mu=mu, mv=mv, window=w, stride=w, max_lag=7)
    D = res["divergence"]
    assert res["samples"].tolist() == [30, 30, 30, 30, 30, 30, 15, 30]
    want = bound_of(masses(plan, mu, mv, w, w), 7)
    r, l = np.nonzero(~structural(8, 7))
    across = (r < 4) & (r + l + 1 >= 4)
    print("weighted", weighted, "max |D - H2| across", float(np.abs(D[r, l] - want[r, l])[across].max()), "max |D| within",
          float(np.abs(D[r, l])[~across].max()))
    assert (np.abs(D[r, l] - want[r, l])[across] <= atol).all() and (np.abs(D[r, l])[~across] <= atol).all()
    assert abs(D[0, 3] - 1.0) <= atol and abs(D[3, 0] - 1.0) <= atol                    # equal masses: one bit
    if not weighted:
        assert abs(D[3, 2] - float(wdo.h2(1 / 3))) <= atol                              # 30 : 15
    plan.close()


# ------------------------------------------------------------------------------------------- 8 consistency with the windowed entry
@pytest.mark.parametrize("kind", KINDS)
def test_band_of_the_windowed_entrys_own_histograms(native, engine, kind):
    """The pair stage alone: from_hists' arithmetic on vet_spatial_entropy_windowed's d_weights of the same call, 1e-12 absolute."""
    mu, mv = video(8, 150, 7, p_absent=0.1)
    plan = plan_of(native, engine, kind)
    for w, s, L in ((20, 7, 18), (5, 1, 8), (1, 1, 1)):
        wt = plan.spatial_windowed(mu=mu, mv=mv, window=w, stride=s, want_weights=True)
        res = plan.spatial_window_divergence(mu=mu, mv=mv, window=w, stride=s, max_lag=L)
        assert np.array_equal(res["samples"], wt["samples"])
        close(res["divergence"], wdo.band(np.abs(wt["weights"]), wo.keys_of(wt["weights"]), L), 1e-12, f"{kind} w{w} s{s} L{L}")
    done(plan, kind)


# ------------------------------------------------------------------------------------------- 9 quirks
@pytest.mark.parametrize("kind", KINDS)
def test_an_all_absent_stretch_is_data(native, engine, kind):
    mu, mv = video(8, 300, 31, p_absent=0.1)
    mu[100:140], mv[100:140] = np.nan, np.nan
    plan = plan_of(native, engine, kind)
    dev = Device(native, engine)
    d_mu, d_mv = dev.put(mu.nbytes, mu), dev.put(mv.nbytes, mv)
    try:
        for w, s, L in ((10, 10, 6), (5, 1, 1), (20, 5, 12)):
            R = wo.n_rows(300, w, s)
            div, smp, st = dev.run(plan, 8, 300, w, s, L, d_mu=d_mu, d_mv=d_mv, status0=(0, 0))
            r = np.arange(R)
            empty = (r * s >= 100) & (r * s + w <= 140)
            assert empty.any() and np.array_equal(smp == 0, empty) and st.tolist() == [0, int(empty.sum())]
            gone = structural(R, L) | empty[:, None]
            for l in range(1, L + 1):
                gone[:R - l, l - 1] |= empty[l:]
            assert np.array_equal(np.isnan(div), gone), (w, s, L)
            want, samples = oracle_of(kind, mu, mv, w, s, L)
            assert np.array_equal(smp, samples)
            close(div, want, atol_of(plan), f"{kind} absent stretch w{w} s{s} L{L}")
            host = plan.spatial_window_divergence(mu=mu, mv=mv, window=w, stride=s, max_lag=L)       # nothing raises
            assert host["code"] == native.VET_OK and host["divergence"].tobytes() == div.tobytes()
    finally:
        dev.close()
        done(plan, kind)


def test_quirks(native, engine, golden_dir):
    T = 40                                                          # window 1, a single present sample per row
    mu, mv = np.full((T, 3), np.nan), np.full((T, 3), np.nan)
    who = np.arange(T) % 3
    mu[np.arange(T), who], mv[np.arange(T), who] = np.linspace(0.1, 0.9, T), 0.5
    for weighted in (True, False):
        plan = fib_plan(native, engine, [50], weighted)
        res = plan.spatial_window_divergence(mu=mu, mv=mv, window=1, stride=1, max_lag=10)
        want, samples = wdo.fast(mu, mv, W, H, [50], 1, 1, 10, use_weight_distribution=weighted)
        assert (res["samples"] == 1).all() and np.array_equal(res["samples"], samples)
        close(res["divergence"], want, atol_of(plan), f"one sample per row, weighted {weighted}")
        assert np.array_equal(np.isnan(res["divergence"]), structural(T, 10))
        if not weighted:
            bad = mu.copy()
            bad[3, 0] = 1.5
            r = plan.spatial_window_divergence(mu=bad, mv=mv, window=1, stride=1, max_lag=2, check=False)
            assert r["code"] == native.VET_ERR_RANGE and r["samples"][3] == 0 and np.isnan(r["divergence"][3]).all()  # outputs still written
            with pytest.raises(native.NativeError):
                plan.spatial_window_divergence(mu=bad, mv=mv, window=1, stride=1, max_lag=2)
            for window, stride, L in ((0, 1, 1), (4, 0, 1), (41, 1, 1), (4, 4, 0), (4, 4, 10), (40, 1, 1), (None, 1, 1)):
                with pytest.raises(ValueError):
                    plan.spatial_window_divergence(mu=mu, mv=mv, window=window, stride=stride, max_lag=L)
            e = np.zeros(512)
            for window, stride, L in ((0, 1, 1), (4, 0, 1), (41, 1, 1), (4, 4, 0), (4, 4, 10), (40, 1, 1)):
                rc = plan.lib.vet_window_divergence_host(plan.handle, native._ptr(mu), native._ptr(mv), None, 3, 40, window, stride, L,
                                                         native._ptr(e), None)
                assert rc == native.VET_ERR_INVALID and plan.lib.vet_last_error()
        plan.close()
    # golden G12's configuration (power factor 150: in-FoV weights underflow to 0.0 and stay keys): the reference's NaN on pooled rows
    g = np.load(golden_dir / "g12_underflow.npz")
    px, py = g["px"], g["py"]
    present = px >= 0
    gm = np.where(present, np.where(px == W, 1.0, (px + 0.5) / W), np.nan)
    gv = np.where(present, np.where(py == H, 1.0, (py + 0.5) / H), np.nan)
    T = len(gm)
    window = 1 if T < 10 else 2
    L = min(4, wo.n_rows(T, window, window) - 1)
    plan = fib_plan(native, engine, [500], True, 120.0, 150.0)
    res = plan.spatial_window_divergence(mu=gm, mv=gv, window=window, stride=window, max_lag=L)
    want, samples, bits, _ = wdo.fast(gm, gv, W, H, [500], window, window, L, fov_angle=120.0, power_factor=150.0, want_terms=True)
    R = len(samples)
    valid = ~structural(R, L) & (samples[:, None] > 0)
    for l in range(1, L + 1):
        valid[:R - l, l - 1] &= samples[l:] > 0
    assert np.isnan(want[valid]).any(), "the configuration no longer produces the reference's NaN on a pair of rows with samples"
    own_nan = np.isnan(bits[:, 0, 0, 0]) & (samples > 0)            # a window whose own S is NaN: all its pairs are
    if own_nan[:R - 1].any():
        assert np.isnan(res["divergence"][:R - 1][own_nan[:R - 1]]).all()
    assert np.array_equal(res["samples"], samples)
    close(res["divergence"], want, atol_of(plan), "G12 pooled")
    plan.close()


# ------------------------------------------------------------------------------------------- 10 nothing else moved
@pytest.mark.parametrize("weighted", [True, False])
def test_the_calls_that_share_the_workspace_do_not_move(native, engine, weighted):
    mu, mv = video(9, 150, 7, p_absent=0.1)
    plan = fib_plan(native, engine, [50, 100] if weighted else [50], weighted)
    before_w = plan.spatial_windowed(mu=mu, mv=mv, window=20, stride=7, want_weights=True)
    before_u = plan.spatial_user_divergence(mu=mu, mv=mv, window=20, stride=7)
    for L in (1, 5, 18):
        plan.spatial_window_divergence(mu=mu, mv=mv, window=20, stride=7, max_lag=L)
    after_w = plan.spatial_windowed(mu=mu, mv=mv, window=20, stride=7, want_weights=True)
    after_u = plan.spatial_user_divergence(mu=mu, mv=mv, window=20, stride=7)
    for k in ("entropy", "weights", "samples"):
        assert before_w[k].tobytes() == after_w[k].tobytes(), k
    for k in ("divergence", "samples"):
        assert before_u[k].tobytes() == after_u[k].tobytes(), k
    ent, samples, _ = wo.fast(mu, mv, W, H, [50, 100] if weighted else [50], 20, 7, use_weight_distribution=weighted)
    np.testing.assert_allclose(after_w["entropy"], ent, rtol=1e-6, atol=0, equal_nan=True)
    assert np.array_equal(after_w["samples"], samples)
    plan.close()
