"""GPU: the attention coverage through the C-ABI (Plan.spatial_coverage -> vet_coverage_host, the device entries, both analyzers).
For every window (row) lattice 0's tiles are ranked by the row's pooled weight; tiles[r][i] is the smallest number of top-ranked
tiles whose running sum reaches fractions[i] of the row's mass, hit[r][l][i] the share of row r + l's mass on those tiles.  The
references are the engine's own histograms through tests/_coverage_oracle.py's ``from_hists`` (exact in tiles and order: the
summation order is part of the contract), and golden G23 (the real reference's histograms, tools/gen_golden_coverage.py).

Tolerances.  Against the engine's own histograms: tiles, order, samples exact; hit 1e-12 absolute (a share in [0, 1] of at most
2048 FP64 terms added in two different orders).  Against G23: a histogram entry differs from the reference's by tests/_tol.py's
W_RTOL relative, so hit (a ratio of two sums of such entries) holds to 2 * W_RTOL absolute; tiles is compared exactly except
where the oracle says the entry sits within 1e-13 W of changing (boundary gap or threshold margin positive and below 1e-13), at
most 1 % of the entries; order is compared exactly at every rank whose weight differs from both neighbours' by at least 1e-13 W or
not at all (a tie is broken by the index in both)."""
import ctypes

import numpy as np
import pytest

from oracle import vet_oracle as vo
from tests import _coverage_oracle as co
from tests import _window_oracle as wo
from tests._tol import W_RTOL

pytestmark = pytest.mark.gpu

W, H = 100, 200
FRACTIONS = (0.5, 0.8, 0.95)
G23_FRACTIONS = (0.5, 0.8, 0.95, 1.0)
G23_SHAPES = ((20, 20, 14), (5, 1, 6), (1, 1, 3))                   # (window, stride, max_lag)
T_SMALL, U_SMALL = 150, 8
# lattice 0 -> tiles n and the records P of the sort: a single tile, fewer than the 8-record minimum, just above a power of two
# (nearly all padding), just below one, and more than one pass of the 256 threads
PADDING = {1: (1, 8), 2: (3, 8), 50: (51, 64), 64: (65, 128), 500: (501, 512), 1000: (1001, 1024)}


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
def g23(golden_dir):
    return np.load(golden_dir / "g23_coverage.npz")


@pytest.fixture(scope="module")
def small():
    return video(U_SMALL, T_SMALL, 7, p_absent=0.1)


def video(U, T, seed, p_absent=0.0):
    from viewport_entropy_toolkit import _synthetic
    return _synthetic.random_walk_video(U, T, base_seed=seed, p_absent=p_absent)


def fib_plan(native, engine, tcs, weighted=True, fov=120.0, power=2.0):
    return native.Plan(engine, [vo.fibonacci_lattice(t) for t in tcs], fov, power, weighted, W, H)


def naive_analyzer(th=10, tw=20):
    from viewport_entropy_toolkit import NaiveSpatialEntropyAnalyzer
    from viewport_entropy_toolkit.config import NaiveAnalyzerConfig
    return NaiveSpatialEntropyAnalyzer(NaiveAnalyzerConfig(tile_height=th, tile_width=tw, video_width=W, video_height=H))


def plan_of(native, engine, kind):
    if kind == "naive":
        return naive_analyzer()._naive_plan()
    flag, tcs = kind[0] == "w", [int(t) for t in kind[1:].split("_")]
    return fib_plan(native, engine, tcs, flag)


def done(plan, kind):
    if kind != "naive":
        plan.close()


def ids_of(mu, mv):
    return wo._ids(mu, mv, W, H)[0].astype(np.int32)


def structural(R, L):
    return np.arange(R)[:, None] + np.arange(L + 1)[None, :] >= R


def close(got, want, atol, msg=""):
    print(msg, "max abs err", float(np.nanmax(np.abs(got - want), initial=0.0)), "atol", atol)
    assert got.shape == want.shape, msg
    assert np.array_equal(np.isnan(got), np.isnan(want)), (msg, np.argwhere(np.isnan(got) != np.isnan(want))[:10])
    np.testing.assert_allclose(got, want, rtol=0, atol=atol, equal_nan=True, err_msg=msg)


def same_bits(a, b, msg, keys=("tiles", "hit", "order", "samples")):
    for k in keys:
        if a.get(k) is not None and b.get(k) is not None:
            assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (msg, k)


def against_own_histograms(plan, mu, mv, w, s, L, fractions, msg, ids=None):
    """The call against from_hists of the windowed call's own weights: the whole contract short of the histogram itself."""
    src = dict(ids=ids) if ids is not None else dict(mu=mu, mv=mv)
    wt = plan.spatial_windowed(window=w, stride=s, want_weights=True, check=False, **src)
    res = plan.spatial_coverage(window=w, stride=s, max_lag=L, fractions=fractions, want_order=True, **src)
    R, n = wt["weights"].shape
    assert res["code"] == 0 and res["tiles"].shape == (R, len(fractions)) and res["tiles"].dtype == np.int32, msg
    assert res["hit"].shape == (R, L + 1, len(fractions)) and res["order"].shape == (R, n) and res["order"].dtype == np.int32, msg
    want = co.from_hists(np.abs(wt["weights"]), fractions, L)
    assert np.array_equal(res["samples"], wt["samples"]), msg
    assert np.array_equal(res["order"], want["order"]), (msg, np.argwhere(res["order"] != want["order"])[:10])
    assert np.array_equal(res["tiles"], want["tiles"]), (msg, np.argwhere(res["tiles"] != want["tiles"])[:10])
    close(res["hit"], want["hit"], 1e-12, msg)
    return res, want, wt


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

    def run(self, plan, U, T, w, s, L, fractions, d_mu=None, d_mv=None, d_ids=None, status0=(0, 1000), want_order=True):
        R, Q, n = wo.n_rows(T, w, s), len(fractions), plan.n_tiles[0]
        out = dict(tiles=np.empty((R, Q), np.int32), hit=np.empty((R, L + 1, Q)), order=np.empty((R, n), np.int32),
                   samples=np.empty(R, np.int32), status=np.array(status0, np.int32))
        d = {k: self.put(v.nbytes, v if k == "status" else None) for k, v in out.items()}
        plan.spatial_coverage_device(d_mu.value if d_mu else 0, d_mv.value if d_mv else 0, U, T, w, s, L, fractions, d["tiles"].value,
                                     d["hit"].value, d["order"].value if want_order else 0, d["samples"].value, d["status"].value,
                                     d_ids=d_ids.value if d_ids else 0)
        for k, v in out.items():
            if k != "order" or want_order:
                assert self.lib.vet_memcpy_d2h(self.engine.handle, self.native._ptr(v), d[k], v.nbytes) == 0
        if not want_order:
            out["order"] = None
        return out

    def close(self):
        self.engine.synchronize()
        for p in self.bufs:
            self.lib.vet_free(self.engine.handle, p)


# ------------------------------------------------------------------------------------------- 1 the engine's own histograms
@pytest.mark.parametrize("kind", ["w1", "w2", "w50", "w64", "w500", "w1000", "w50_100_200", "u50", "naive"])
def test_exact_against_the_engines_own_histograms(native, engine, small, kind):
    """(window, stride, max_lag) = (20, 20, R - 1), (5, 1, 6), (1, 1, 3) on 8 users x 150 frames (10 % absences)."""
    mu, mv = small
    plan = plan_of(native, engine, kind)
    n = plan.n_tiles[0]
    if kind[1:].isdigit():
        P = 8
        while P < n:
            P *= 2
        assert (n, P) == PADDING[int(kind[1:])], kind
    for w, s, L in ((20, 20, None), (5, 1, 6), (1, 1, 3)):
        R = wo.n_rows(T_SMALL, w, s)
        L = R - 1 if L is None else L
        res, want, wt = against_own_histograms(plan, mu, mv, w, s, L, FRACTIONS, f"{kind} w{w} s{s} L{L}")
        assert (res["samples"] > 0).all() and np.isnan(res["hit"][structural(R, L)]).all()
        if kind == "u50":                                           # counts: exact ties, broken by the tile index
            srt = np.take_along_axis(np.abs(wt["weights"]), res["order"].astype(np.int64), axis=1)
            ties = np.diff(srt, axis=1) == 0
            assert (ties & (srt[:, 1:] > 0)).any() and (np.diff(res["order"], axis=1)[ties] > 0).all()
    done(plan, kind)


# ------------------------------------------------------------------------------------------- 2 the reference (golden G23)
def g23_cases():
    for w, s, L in G23_SHAPES:
        for tag, kind in (("w_tc50", "w50"), ("w_tc50_100_200", "w50_100_200"), ("u_tc50", "u50"), ("naive_h10_w20", "naive")):
            yield f"{tag}_w{w}_s{s}_l{L}", kind, w, s, L


def check_g23(g23, tag, res, msg):
    """Returns (entries left out, entries)."""
    rows = g23[f"{tag}__rows"]
    ref = co.from_hists(g23[f"{tag}__weights"], G23_FRACTIONS, 0)       # per-row margins of the reference's own histograms
    assert np.array_equal(ref["tiles"], g23[f"{tag}__tiles"]) and np.array_equal(ref["order"], g23[f"{tag}__order"]), msg
    near = ((ref["gap"] > 0) & (ref["gap"] < 1e-13)) | ((ref["margin"] > 0) & (ref["margin"] < 1e-13))
    assert np.array_equal(res["samples"][rows], g23[f"{tag}__samples"]), msg
    tiles = res["tiles"][rows]
    assert np.array_equal(tiles[~near], g23[f"{tag}__tiles"][~near]), (msg, np.argwhere((tiles != g23[f"{tag}__tiles"]) & ~near)[:10])
    # order: every rank whose weight is at least 1e-13 W from both neighbours', or exactly equal to a neighbour's in a run of ties
    srt = np.take_along_axis(g23[f"{tag}__weights"], g23[f"{tag}__order"].astype(np.int64), axis=1)
    d = np.abs(np.diff(srt, axis=1)) / ref["mass"][:, None]
    loose = (d > 0) & (d < 1e-13)
    pinned = np.ones(srt.shape, dtype=bool)
    pinned[:, 1:] &= ~loose
    pinned[:, :-1] &= ~loose
    if "naive" in tag or tag.startswith("u_"):
        assert pinned.all(), msg                                     # counts are exact
    order = res["order"][rows]
    assert np.array_equal(order[pinned], g23[f"{tag}__order"][pinned]), (msg, np.argwhere((order != g23[f"{tag}__order"]) & pinned)[:10])
    hit, want = res["hit"][rows].copy(), g23[f"{tag}__hit"].copy()
    hit[np.repeat(near[:, None, :], hit.shape[1], axis=1)] = 0.0
    want[np.repeat(near[:, None, :], hit.shape[1], axis=1)] = 0.0
    close(hit, want, 2 * W_RTOL, msg)
    print(msg, "left out", int(near.sum()), "of", near.size, "entries; unpinned ranks", int((~pinned).sum()), "of", pinned.size)
    return int(near.sum()), near.size


def test_host_and_device_entries_vs_reference_golden(native, engine, g14, g23):
    mu, mv = np.ascontiguousarray(g14["mu_absent"]), np.ascontiguousarray(g14["mv_absent"])
    T, U = mu.shape
    dev = Device(native, engine)
    d_mu, d_mv = dev.put(mu.nbytes, mu), dev.put(mv.nbytes, mv)
    plans, out, total = {}, 0, 0
    try:
        for tag, kind, w, s, L in g23_cases():
            if kind not in plans:
                plans[kind] = plan_of(native, engine, kind)
            plan = plans[kind]
            res = plan.spatial_coverage(mu=mu, mv=mv, window=w, stride=s, max_lag=L, fractions=G23_FRACTIONS, want_order=True)
            a, b = check_g23(g23, tag, res, tag + " host")
            out, total = out + a, total + b
            got = dev.run(plan, U, T, w, s, L, G23_FRACTIONS, d_mu=d_mu, d_mv=d_mv)
            same_bits(got, res, tag + " device")
            assert got["status"].tolist() == [0, 1000], tag
    finally:
        dev.close()
        for kind, p in plans.items():
            done(p, kind)
    print("G23: left out", out, "of", total, "(row, fraction) entries")
    assert out <= 0.01 * total


# ------------------------------------------------------------------------------------------- 3 edges
@pytest.mark.parametrize("kind", ["w50", "u50", "naive"])
def test_frames_without_a_viewer_are_data(native, engine, kind):
    mu, mv = video(8, 120, 31, p_absent=0.1)
    mu[40:52], mv[40:52] = np.nan, np.nan
    plan = plan_of(native, engine, kind)
    dev = Device(native, engine)
    d_mu, d_mv = dev.put(mu.nbytes, mu), dev.put(mv.nbytes, mv)
    try:
        for w, s, L in ((1, 1, 3), (5, 1, 6), (4, 4, 5)):
            R = wo.n_rows(120, w, s)
            res, want, wt = against_own_histograms(plan, mu, mv, w, s, L, FRACTIONS, f"{kind} absent stretch w{w} s{s}")   # nothing raises
            r = np.arange(R)
            empty = (r * s >= 40) & (r * s + w <= 52)
            assert empty.any() and np.array_equal(res["samples"] == 0, empty)
            assert (res["tiles"][empty] == 0).all() and (res["tiles"][~empty] > 0).all()
            gone = structural(R, L) | empty[:, None]
            for l in range(L + 1):
                gone[:R - l, l] |= empty[l:]
            for i in range(len(FRACTIONS)):
                assert np.array_equal(np.isnan(res["hit"][..., i]), gone), (w, s, L, i)
            assert (np.sort(res["order"], axis=1) == np.arange(plan.n_tiles[0])).all()
            assert (res["order"][empty] == np.arange(plan.n_tiles[0])).all()          # all weights 0: index order
            got = dev.run(plan, 8, 120, w, s, L, FRACTIONS, d_mu=d_mu, d_mv=d_mv, status0=(0, 0))
            same_bits(got, res, "device entry")
            assert got["status"].tolist() == [0, int(empty.sum())]
    finally:
        dev.close()
        done(plan, kind)


def test_keys_of_weight_zero_and_rows_without_mass(native, engine, golden_dir):
    """power_factor 150 (golden G12's configuration): in-FoV weights underflow to 0.0 and stay keys — NaN rows in the sibling calls;
    coverage is defined from the values.  fov_angle 2 on 50 tiles: rows with samples none of whose tiles is inside a FoV: W = 0."""
    g = np.load(golden_dir / "g12_underflow.npz")
    px, py = g["px"], g["py"]
    present = px >= 0
    gm = np.where(present, np.where(px == W, 1.0, (px + 0.5) / W), np.nan)
    gv = np.where(present, np.where(py == H, 1.0, (py + 0.5) / H), np.nan)
    T = len(gm)
    window = 1 if T < 10 else 2
    L = min(4, wo.n_rows(T, window, window) - 1)
    plan = fib_plan(native, engine, [500], True, 120.0, 150.0)
    res, want, wt = against_own_histograms(plan, gm, gv, window, window, L, FRACTIONS, "G12")
    assert (np.signbit(wt["weights"]) & (wt["weights"] == 0)).any(), "the configuration no longer produces keys of weight 0.0"
    assert np.isnan(wt["entropy"][wt["samples"] > 0]).any()
    mass = np.abs(wt["weights"]).sum(axis=1) > 0
    assert ((res["tiles"] > 0) == mass[:, None]).all() and not np.isnan(res["hit"][mass, 0]).any()
    plan.close()
    mu, mv = video(8, 60, 5, p_absent=0.1)
    plan = fib_plan(native, engine, [50], True, 2.0, 2.0)
    res, want, wt = against_own_histograms(plan, mu, mv, 1, 1, 3, FRACTIONS, "fov 2")
    massless = (np.abs(wt["weights"]).sum(axis=1) == 0) & (wt["samples"] > 0)
    assert massless.any(), "no row with samples and W = 0: choose a smaller fov_angle"
    assert (res["tiles"][massless] == 0).all() and np.isnan(res["hit"][massless]).all()
    plan.close()


@pytest.mark.parametrize("kind", ["w50", "naive"])
def test_lag_and_fraction_edges(native, engine, small, kind):
    mu, mv = small
    plan = plan_of(native, engine, kind)
    R = wo.n_rows(T_SMALL, 10, 10)
    for L in (0, R - 1):
        res, _, _ = against_own_histograms(plan, mu, mv, 10, 10, L, FRACTIONS, f"{kind} max_lag {L}")
        assert res["hit"].shape == (R, L + 1, 3) and not np.isnan(res["hit"][:, 0]).any()
        assert (res["hit"][:, 0] >= np.asarray(FRACTIONS)[None, :] - 1e-12).all() and (np.diff(res["tiles"], axis=1) >= 0).all()
    for fractions in ((0.8,), (1.0,), tuple(np.linspace(0.125, 1.0, 8))):
        res, _, wt = against_own_histograms(plan, mu, mv, 10, 10, 2, fractions, f"{kind} fractions {fractions}")
        if fractions[-1] == 1.0:
            assert np.array_equal(res["tiles"][:, -1], (np.abs(wt["weights"]) > 0).sum(axis=1))
            np.testing.assert_allclose(res["hit"][:, 0, -1], 1.0, rtol=0, atol=1e-12)
    if kind != "naive":
        against_own_histograms(plan, None, None, 5, 3, 4, FRACTIONS, "ids", ids=ids_of(mu, mv))
    done(plan, kind)


# ------------------------------------------------------------------------------------------- 4 purity, bit for bit
@pytest.mark.parametrize("kind", ["w50", "u50", "naive"])
def test_row_chunks_do_not_change_a_bit(native, engine, kind):
    """41 rows, 1, 3 and the default number at a time, with lags that reach across several chunks (the halo)."""
    mu, mv = video(8, 60, 61, p_absent=0.1)
    mu[10:32], mv[10:32] = np.nan, np.nan                           # rows 10..12 have no sample
    plan = plan_of(native, engine, kind)
    dev = Device(native, engine)
    d_mu, d_mv = dev.put(mu.nbytes, mu), dev.put(mv.nbytes, mv)
    try:
        for L in (0, 1, 9):
            a = dev.run(plan, 8, 60, 20, 1, L, FRACTIONS, d_mu=d_mu, d_mv=d_mv)
            assert (a["samples"] == 0).sum() == 3 and a["status"].tolist() == [0, 1003]
            for rows in (1, 3):
                engine.test_coverage_chunk_rows(rows)
                b = dev.run(plan, 8, 60, 20, 1, L, FRACTIONS, d_mu=d_mu, d_mv=d_mv)
                same_bits(a, b, (L, rows), keys=("tiles", "hit", "order", "samples", "status"))      # every row booked once
            engine.test_coverage_chunk_rows(0)
    finally:
        engine.test_coverage_chunk_rows(0)
        dev.close()
        done(plan, kind)


@pytest.mark.parametrize("kind", ["w50", "u50", "naive"])
def test_entries_are_pure_functions_of_their_rows(native, engine, small, kind):
    mu, mv = small
    plan = plan_of(native, engine, kind)
    call = lambda w, s, L, f=FRACTIONS, **kw: plan.spatial_coverage(window=w, stride=s, max_lag=L, fractions=f, want_order=True,
                                                                     **(kw or dict(mu=mu, mv=mv)))
    w = 10
    full = call(w, 1, 6)
    R = wo.n_rows(T_SMALL, w, 1)
    same_bits(full, call(w, 1, 6), "run to run")
    short = call(w, 1, 2)                                           # max_lag 2 against 6 on the common lags
    same_bits(dict(short, hit=None), dict(full, hit=None), "max_lag 2 against 6")
    ok = ~structural(R, 2)
    assert short["hit"][ok].tobytes() == full["hit"][:, :3][ok].tobytes() and np.isnan(short["hit"][~ok]).all()
    five = call(w, 5, 1)                                            # stride 5 against stride 1: rows 0, 5, 10, ...; lag 1 there = lag 5 here
    R5 = wo.n_rows(T_SMALL, w, 5)
    for k in ("tiles", "order", "samples"):
        assert five[k].tobytes() == np.ascontiguousarray(full[k][::5][:R5]).tobytes(), k
    assert five["hit"][:, 0].tobytes() == np.ascontiguousarray(full["hit"][::5, 0][:R5]).tobytes()
    assert five["hit"][:R5 - 1, 1].tobytes() == np.ascontiguousarray(full["hit"][::5, 5][:R5 - 1]).tobytes()
    one = call(w, 1, 6, (0.8,))                                     # a fraction alone against the same fraction among others
    assert one["tiles"][:, 0].tobytes() == np.ascontiguousarray(full["tiles"][:, 1]).tobytes()
    assert one["hit"][:, :, 0].tobytes() == np.ascontiguousarray(full["hit"][:, :, 1]).tobytes()
    assert one["order"].tobytes() == full["order"].tobytes()
    cut = plan.spatial_coverage(mu=mu[4:], mv=mv[4:], window=w, stride=1, max_lag=6, want_order=True)       # n_frames
    ok = ~structural(R - 4, 6)
    assert cut["tiles"].tobytes() == full["tiles"][4:].tobytes() and cut["order"].tobytes() == full["order"][4:].tobytes()
    assert cut["hit"][ok].tobytes() == full["hit"][4:][ok].tobytes()
    # the entries: host, device (mu, mv), and the ids entries
    dev = Device(native, engine)
    try:
        d_mu, d_mv = dev.put(mu.nbytes, mu), dev.put(mv.nbytes, mv)
        same_bits(dev.run(plan, U_SMALL, T_SMALL, w, 1, 6, FRACTIONS, d_mu=d_mu, d_mv=d_mv), full, "device (mu, mv)")
        no_order = dev.run(plan, U_SMALL, T_SMALL, w, 1, 6, FRACTIONS, d_mu=d_mu, d_mv=d_mv, want_order=False)
        same_bits(no_order, full, "device, no order")
        if kind != "naive":
            ids = ids_of(mu, mv)
            same_bits(call(w, 1, 6, ids=ids), full, "host ids")
            same_bits(dev.run(plan, U_SMALL, T_SMALL, w, 1, 6, FRACTIONS, d_ids=dev.put(ids.nbytes, ids)), full, "device ids")
    finally:
        dev.close()
    rng = np.random.default_rng(5)                                  # frames outside rows r and r + l do not matter
    for r, l in ((0, 0), (5, 6), (40, 3)):
        m2, v2 = rng.random(mu.shape), rng.random(mv.shape)
        for f0 in (r, r + l):
            m2[f0:f0 + w], v2[f0:f0 + w] = mu[f0:f0 + w], mv[f0:f0 + w]
        other = plan.spatial_coverage(mu=m2, mv=v2, window=w, stride=1, max_lag=6, want_order=True)
        assert other["tiles"][r].tobytes() == full["tiles"][r].tobytes() and other["order"][r].tobytes() == full["order"][r].tobytes()
        assert other["hit"][r, l].tobytes() == full["hit"][r, l].tobytes() and other["hit"][r, 0].tobytes() == full["hit"][r, 0].tobytes()
    done(plan, kind)


def test_only_lattice_zero_takes_part(native, engine, small):
    mu, mv = small
    one, three = fib_plan(native, engine, [50]), fib_plan(native, engine, [50, 100, 200])
    for w, s, L in ((20, 20, 6), (5, 1, 6)):
        a = one.spatial_coverage(mu=mu, mv=mv, window=w, stride=s, max_lag=L, want_order=True)
        b = three.spatial_coverage(mu=mu, mv=mv, window=w, stride=s, max_lag=L, want_order=True)
        same_bits(a, b, f"[50, 100, 200] against [50], w{w} s{s}")
    one.close()
    three.close()


# ------------------------------------------------------------------------------------------- 5 refusals
def test_refusals(native, engine, small):
    mu, mv = small
    mu, mv = np.ascontiguousarray(mu[:40]), np.ascontiguousarray(mv[:40])
    plan = fib_plan(native, engine, [50], False)
    lib = plan.lib
    tiles, hit = np.full(40 * 8, -7, np.int32), np.full(40 * 40 * 8, -7.0)

    def host(p, fractions, Q, max_lag, window=4, stride=4):
        f = np.asarray(fractions, dtype=np.float64)
        return lib.vet_coverage_host(p.handle, native._ptr(mu), native._ptr(mv), None, U_SMALL, 40, window, stride, max_lag,
                                     native._ptr(f) if f.size else None, Q, native._ptr(tiles), native._ptr(hit), None, None)

    engine.profile_enable(True)
    engine.profile_reset()
    bad = [((0.8, 0.5), 2, 0), ((0.5, 0.5), 2, 0), ((0.0, 0.5), 2, 0), ((0.5, 1.5), 2, 0), ((-0.5,), 1, 0), ((float("nan"),), 1, 0),
           ((0.5,), 0, 0), (tuple(np.linspace(0.1, 0.9, 9)), 9, 0), ((0.5,), 1, -1), ((0.5,), 1, 10), ((), 1, 0)]
    for fractions, Q, max_lag in bad:                               # window = stride = 4: 10 rows, max_lag in 0..9
        assert host(plan, fractions, Q, max_lag) == native.VET_ERR_INVALID and lib.vet_last_error(), (fractions, Q, max_lag)
    assert host(plan, (0.5,), 1, 0, window=41) == native.VET_ERR_INVALID
    assert (tiles == -7).all() and (hit == -7.0).all()              # nothing was written
    for name in native.KERNEL_IDS:
        assert engine.profile_get(name)[1] == 0, name
    assert host(plan, (0.5,), 1, 9) == native.VET_OK and (tiles[:10] > 0).all()
    assert engine.profile_get("k_transition")[1] == 1 and engine.profile_get("k_wtab")[1] == 1      # the two coverage kernels
    engine.profile_reset()
    for fractions, max_lag in (((0.8, 0.5), 0), ((0.5,), 10), ((0.5,), -1), ((), 0)):
        with pytest.raises(ValueError):
            plan.spatial_coverage(mu=mu, mv=mv, window=4, stride=4, max_lag=max_lag, fractions=fractions)
    plan.close()
    # a naive 1 x 1 degree plan: 65 341 cells, more than the LDS sort holds
    fine = naive_analyzer(1, 1)._naive_plan()
    assert fine.n_tiles[0] == 65341
    engine.profile_reset()                                          # the plan's own tables are built by now
    tiles[:] = -7
    assert host(fine, (0.5,), 1, 0) == native.VET_ERR_UNSUPPORTED and b"2048" in lib.vet_last_error()
    assert (tiles == -7).all()
    with pytest.raises(native.NativeError) as e:
        fine.spatial_coverage(mu=mu, mv=mv, window=4, stride=4)
    assert e.value.code == native.VET_ERR_UNSUPPORTED
    for name in native.KERNEL_IDS:                                  # nothing was launched by any refused call
        assert engine.profile_get(name)[1] == 0, name
    engine.profile_enable(False)


# ------------------------------------------------------------------------------------------- 6 analyzers end to end
def test_analyzers_end_to_end(native, engine, small):
    from viewport_entropy_toolkit import SpatialEntropyAnalyzer
    from viewport_entropy_toolkit.config import AnalyzerConfig
    mu, mv = small
    times = np.arange(T_SMALL) * 0.1
    fractions = (0.5, 0.9)
    for an, kind in ((SpatialEntropyAnalyzer(AnalyzerConfig(tile_counts=[50, 100], video_width=W, video_height=H)), "w50_100"),
                     (naive_analyzer(), "naive")):
        an.load_arrays(times, mu, mv)
        plan = plan_of(native, engine, kind)
        for w, s, L, keep in ((20, 7, 5, True), (1, 1, 0, False)):
            df = an.compute_coverage(w, s, fractions, L, keep_order=keep)
            want = plan.spatial_coverage(mu=mu, mv=mv, window=w, stride=s, max_lag=L, fractions=fractions, want_order=keep)
            R, n = wo.n_rows(T_SMALL, w, s), plan.n_tiles[0]
            assert list(df.columns) == ["time", "time_end", "samples", "tiles", "share", "covered", "forecast"] + (["order"] if keep else [])
            assert len(df) == R and df.attrs == {"fractions": fractions, "lags": list(range(1, L + 1)),
                                                 "lag_frames": [s * l for l in range(1, L + 1)], "n_tiles": n}
            assert np.array_equal(df["time"], times[np.arange(R) * s]) and np.array_equal(df["time_end"], times[np.arange(R) * s + w - 1])
            assert np.array_equal(df["samples"].to_numpy(), want["samples"])
            assert np.stack(df["tiles"].to_list()).tobytes() == want["tiles"].tobytes()
            assert np.array_equal(np.stack(df["share"].to_list()), want["tiles"] / n)
            assert np.stack(df["covered"].to_list()).tobytes() == np.ascontiguousarray(want["hit"][:, 0]).tobytes()
            assert np.stack(df["forecast"].to_list()).tobytes() == np.ascontiguousarray(want["hit"][:, 1:]).tobytes()
            whole = df["covered"][0].base
            assert whole is not None and whole.shape == (R, L + 1, 2)                                           # views into ONE array
            assert all(np.shares_memory(df["covered"][r], whole) and (L == 0 or np.shares_memory(df["forecast"][r], whole))
                       for r in range(R))
            if keep:
                assert np.stack(df["order"].to_list()).tobytes() == want["order"].tobytes()
        done(plan, kind)
