"""GPU: windowed Markov transition statistics through the C-ABI (Plan.transition_markov -> vet_transition_markov_host, the device
entries through Plan.transition_markov_device).  Pair f is (frame f, frame f + lag); row r pools the (pair, user) samples of pairs
[r * stride, r * stride + window) present in both frames into integer counts per (source tile, destination tile).  The references
are golden G24 (the textbook forms on the real reference's tile pairs, tools/gen_golden_markov.py) and the numpy oracles of
tests/_markov_oracle.py (pinned against G24 in tests/test_markov_surface.py) — never the code under test.  ``samples`` and
``matrix`` are compared for equality, ``stats`` at 1e-12 bits absolute with NaN equal to NaN.

The 1e-12 is derived, not measured: a statistic is at most log2 N < 20 bits; each of its sums holds non-negative terms with at most
W / 256 + 16 sequential roundings (a thread's positions, the butterfly, the four waves); the worst case stays below 4e-13 at
W = 32768, and the chunked shape's sums over a matrix of n^2 <= 2^22 cells are no longer."""
import numpy as np
import pytest

from oracle import vet_oracle as vo
from tests import _markov_oracle as mo

pytestmark = pytest.mark.gpu

W, H = 100, 200
ATOL = 1e-12
LDS_SAMPLES = 32768                    # k_markov_rows holds up to this many candidate samples; beyond, the chunked shape


@pytest.fixture(scope="module")
def native():
    from viewport_entropy_toolkit import _native
    return _native


@pytest.fixture(scope="module")
def engine(native):
    return native.Engine.default()


@pytest.fixture(scope="module")
def plans(native, engine):
    """fibonacci plans by tile counts, built once"""
    made = {}

    def get(tcs):
        key = tuple(tcs)
        if key not in made:
            made[key] = native.Plan(engine, [vo.fibonacci_lattice(t) for t in key], 120.0, 2.0, True, W, H)
        return made[key]

    yield get
    for p in made.values():
        p.close()


def ids_of(mu, mv):
    px, py, present, _ = vo.sample_directions(mu, mv, W, H)
    return np.where(present, py * (W + 1) + px, -1).astype(np.int32)


def walk(U, T, p_absent, seed):
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(U, T, base_seed=seed, p_absent=p_absent)
    if p_absent:
        mu[8:31] = np.nan              # frames 8-30 without anybody: windows of up to 20 pairs fall inside
        mv[8:31] = np.nan
    return mu, mv


def check(res, want, msg, rows=None):
    """a result dict (or its rows ``rows``) against the oracle's (stats, samples, matrix)"""
    stats, samples, matrix = want
    got = res["stats"] if rows is None else res["stats"][:, rows]
    print(msg, "max abs err", float(np.nanmax(np.abs(got - stats), initial=0.0)))
    assert np.array_equal(np.isnan(got), np.isnan(stats)), msg
    np.testing.assert_allclose(got, stats, rtol=0, atol=ATOL, equal_nan=True, err_msg=msg)
    assert np.array_equal(res["samples"] if rows is None else res["samples"][rows], samples), msg
    if res["matrix"] is not None:
        assert res["matrix"].dtype == np.int32
        assert np.array_equal(res["matrix"] if rows is None else res["matrix"][rows], matrix), msg
    empty = samples == 0
    assert np.isnan(got[:, empty]).all() and not np.isnan(got[:, ~empty]).any(), msg


def same_bytes(a, b, msg, keys=("stats", "samples", "matrix")):
    for key in keys:
        if a[key] is None or b[key] is None:
            continue
        assert a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), (msg, key)


# ------------------------------------------------------------------------------------------- the reference's tile pairs (golden G24)
def test_vs_golden_grid_and_ids(plans, golden_dir):
    g = np.load(golden_dir / "g24_markov.npz")
    g15 = np.load(golden_dir / "g15_windowed_transition.npz")
    mu, mv = g15["mu"], g15["mv"]
    ids = ids_of(mu, mv)
    cases = sorted({k.rsplit("__", 1)[0] for k in g.files})
    assert len(cases) == 32
    for tag in cases:
        head, w, s, lag = tag.rsplit("_", 3)
        tcs, w, s, lag = [int(x) for x in head[2:].split("_")], int(w[1:]), int(s[1:]), int(lag[1:])
        rows = g[f"{tag}__rows"]
        want = (g[f"{tag}__stats"], g[f"{tag}__samples"], g[f"{tag}__matrix"])
        for kw in (dict(mu=mu, mv=mv), dict(ids=ids)):
            res = plans(tcs).transition_markov(window=w, stride=s, lag=lag, want_matrix=True, **kw)
            assert res["stats"].shape == (5, mo.n_rows(60, w, s, lag)) and res["code"] == 0
            check(res, want, tag, rows)
        if w == 60 - lag:                          # window=None is the whole video
            same_bytes(plans(tcs).transition_markov(mu=mu, mv=mv, stride=s, lag=lag, want_matrix=True), res, tag)


# ------------------------------------------------------------------------------------------- the numpy oracle, seeded walks
@pytest.mark.parametrize("p_absent", [0.0, 0.3], ids=["full", "absent"])
@pytest.mark.parametrize("tcs", [[50], [50, 100, 200]], ids=["tc50", "tc50_100_200"])
@pytest.mark.parametrize("U,T", [(1, 40), (7, 60), (64, 60), (512, 45)])
def test_vs_oracle(plans, U, T, tcs, p_absent):
    mu, mv = walk(U, T, p_absent, 700 + U)
    tiles = mo.tiles_of(mu, mv, W, H, tcs)
    plan, n0 = plans(tcs), 51
    kinds = set()
    for lag in (1, 3):
        for window in (1, 2, 20, None):
            w = T - lag if window is None else window
            for stride in sorted({1, 7, w}):
                msg = f"U={U} T={T} {tcs} absent={p_absent} window={window} stride={stride} lag={lag}"
                res = plan.transition_markov(mu=mu, mv=mv, window=window, stride=stride, lag=lag, want_matrix=True)
                want = mo.fast(mu, mv, W, H, tcs, w, stride, lag, tiles=tiles)
                assert res["stats"].shape == (5, mo.n_rows(T, w, stride, lag)) and res["matrix"].shape[1:] == (n0, n0), msg
                check(res, want, msg)
                N = res["samples"]
                assert np.array_equal(res["matrix"].sum(axis=(1, 2)), N), msg
                kinds |= {"empty"} if (N == 0).any() else set()
                kinds |= {"one"} if (N == 1).any() else set()
                kinds |= {"few"} if ((N > 1) & (N <= n0)).any() else set()
                kinds |= {"many"} if (N > n0).any() else set()
                one = N == 1                   # N = 1: all zero but stay, which is 0 or 1 per lattice
                assert (res["stats"][:4, one] == 0).all() and np.isin(res["stats"][4, one] * len(tcs), np.arange(len(tcs) + 1)).all(), msg
    # the cases cover an empty row, an N = 1 row, N <= n and N > n
    assert "few" in kinds or U > 51
    if p_absent:
        assert "empty" in kinds
    if U == 1:
        assert {"one", "few"} <= kinds
    if U >= 64:
        assert "many" in kinds


# ------------------------------------------------------------------------------------------- shape edges
@pytest.mark.parametrize("U,window,T,samples", [(32, 32, 40, 1024), (41, 25, 30, 1025), (512, 10, 13, 5120), (512, 64, 66, 32768),
                                                (331, 99, 101, 32769)])
def test_shape_thresholds(plans, U, window, T, samples):
    """W = 1024 / 1025: the first two LDS shapes (5120: the 8192 shape, which no other test here enters); W = 32768 / 32769: the
    last LDS shape and the smallest input of the chunked one."""
    assert U * window == samples
    mu, mv = walk(U, T, 0.0, 900 + U)
    mu[3, ::5] = np.nan
    mv[3, ::5] = np.nan
    for tcs in ([50], [50, 100, 200]):
        res = plans(tcs).transition_markov(mu=mu, mv=mv, window=window, stride=1, lag=1, want_matrix=True)
        check(res, mo.fast(mu, mv, W, H, tcs, window, 1, 1), f"W={samples} {tcs}")
        assert len(res["samples"]) == T - 1 - window + 1 >= 2


@pytest.mark.parametrize("tcs", [[50, 100, 200], [500]], ids=["tc50_100_200", "tc500"])
def test_whole_video_in_four_chunks(plans, tcs):
    """512 x 200: 199 pairs of 512 candidates, 101 888 > 3 * 32768.  [500]: a matrix row longer than the workgroup."""
    mu, mv = walk(512, 200, 0.3, 11)
    for lag in (1, 3):
        assert 3 * LDS_SAMPLES < (200 - lag) * 512 <= 4 * LDS_SAMPLES
        res = plans(tcs).transition_markov(mu=mu, mv=mv, lag=lag, want_matrix=True)
        check(res, mo.fast(mu, mv, W, H, tcs, None, 1, lag), f"whole {tcs} lag={lag}")
        assert res["samples"][0] > LDS_SAMPLES


def test_nearly_every_pair_distinct(plans):
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.uniform_sphere_video(512, 45, base_seed=5)
    for window, stride in ((20, 7), (None, 1)):
        res = plans([200]).transition_markov(mu=mu, mv=mv, window=window, stride=stride, want_matrix=True)
        check(res, mo.fast(mu, mv, W, H, [200], window, stride, 1), f"uniform window={window}")
        assert ((res["matrix"] > 0).sum(axis=(1, 2)) > 0.2 * res["samples"]).all()      # thousands of runs of one or two


def test_lattice_of_2001_tiles(plans):
    mu, mv = walk(64, 30, 0.0, 13)
    plan = plans([2000])
    assert plan.n_tiles[0] == 2001
    for window, lag in ((20, 1), (None, 3)):
        res = plan.transition_markov(mu=mu, mv=mv, window=window, stride=20, lag=lag, want_matrix=True)
        assert res["matrix"].shape == (1, 2001, 2001)
        check(res, mo.fast(mu, mv, W, H, [2000], window, 20, lag), f"2001 tiles window={window}")


# ------------------------------------------------------------------------------------------- exact statements
@pytest.mark.parametrize("tcs", [[50], [50, 100, 200]], ids=["tc50", "tc50_100_200"])
def test_nobody_moves(plans, tcs):
    rng = np.random.default_rng(3)
    mu, mv = np.tile(rng.random(40), (30, 1)), np.tile(rng.random(40), (30, 1))
    mu[::4, 7] = np.nan
    mv[::4, 7] = np.nan
    for window, lag in ((1, 1), (5, 3), (None, 1)):
        res = plans(tcs).transition_markov(mu=mu, mv=mv, window=window, stride=2, lag=lag)
        rate, stationary, dest, mutual, stay = res["stats"]
        assert rate.tobytes() == np.zeros_like(rate).tobytes()                 # +0.0, bit for bit
        assert stay.tobytes() == np.ones_like(stay).tobytes()
        np.testing.assert_allclose(mutual, stationary, rtol=0, atol=ATOL)
        assert (stationary > 3).all()                                          # 40 viewers over many tiles: not a trivial row


def test_periodic_deterministic_moves(plans):
    """Every viewer walks the same cycle of five far-apart directions from a phase of their own: a tile has one successor."""
    U, T, cycle = 12, 40, np.array([0.1, 0.3, 0.5, 0.7, 0.9])
    phase = (np.arange(T)[:, None] + np.arange(U)[None, :]) % 5
    mu, mv = cycle[phase], np.full((T, U), 0.5)
    for tcs in ([50], [50, 100, 200]):
        for window, lag in ((1, 1), (10, 1), (10, 3), (None, 2)):
            res = plans(tcs).transition_markov(mu=mu, mv=mv, window=window, stride=3, lag=lag, want_matrix=True)
            assert ((res["matrix"] > 0).sum(axis=2) <= 1).all() and ((res["matrix"] > 0).sum(axis=(1, 2)) == 5).all()
            assert res["stats"][0].tobytes() == np.zeros_like(res["stats"][0]).tobytes()
            assert (res["stats"][4] == 0).all()
            check(res, mo.fast(mu, mv, W, H, tcs, window, 3, lag), f"periodic {tcs} {window} {lag}")


def test_lag_1_agrees_with_the_other_transition_calls(plans):
    mu, mv = walk(64, 60, 0.3, 17)
    plan = plans([50, 100, 200])
    for window, stride in ((1, 1), (20, 7)):
        res = plan.transition_markov(mu=mu, mv=mv, window=window, stride=stride, lag=1, want_matrix=True)
        old = plan.transition_windowed(mu=mu, mv=mv, window=window, stride=stride, want_srccount=True, check=False)
        assert np.array_equal(res["matrix"].sum(axis=2), old["srccount"])
        assert np.array_equal(res["samples"], old["samples"])
    per_pair = plan.transition(mu=mu, mv=mv, want_pairs=False, check=False)
    assert np.array_equal(plan.transition_markov(mu=mu, mv=mv, window=1, lag=1)["samples"], per_pair["common"])


# ------------------------------------------------------------------------------------------- purity
@pytest.mark.parametrize("tcs", [[50], [50, 100, 200]], ids=["tc50", "tc50_100_200"])
def test_bits_depend_on_the_rows_frames_only(plans, tcs):
    mu, mv = walk(64, 60, 0.3, 19)
    ids = ids_of(mu, mv)
    plan = plans(tcs)
    for window, lag in ((1, 1), (20, 1), (20, 3)):
        a = plan.transition_markov(mu=mu, mv=mv, window=window, stride=1, lag=lag, want_matrix=True)
        same_bytes(plan.transition_markov(mu=mu, mv=mv, window=window, stride=1, lag=lag, want_matrix=True), a, "run to run")
        same_bytes(plan.transition_markov(ids=ids, window=window, stride=1, lag=lag, want_matrix=True), a, "ids entry")
        b = plan.transition_markov(mu=mu, mv=mv, window=window, stride=1, lag=lag)
        assert b["matrix"] is None
        same_bytes(b, a, "without the matrix")
        c = plan.transition_markov(mu=mu, mv=mv, window=window, stride=7, lag=lag, want_matrix=True)
        same_bytes(c, {k: np.ascontiguousarray(a[k][..., ::7] if k == "stats" else a[k][::7]) for k in ("stats", "samples", "matrix")},
                   "stride 7")
        d = plan.transition_markov(mu=mu[5:45], mv=mv[5:45], window=window, stride=1, lag=lag, want_matrix=True)
        R = d["stats"].shape[1]
        same_bytes(d, {k: np.ascontiguousarray(a[k][..., 5:5 + R] if k == "stats" else a[k][5:5 + R]) for k in ("stats", "samples", "matrix")},
                   "frame-shifted slice")


def test_device_entries_give_the_host_bytes(engine, plans):
    import torch
    mu, mv = walk(64, 60, 0.3, 23)
    ids = ids_of(mu, mv)
    plan = plans([50, 100, 200])
    U, T, window, stride, lag = 64, 60, 20, 3, 3
    host = plan.transition_markov(mu=mu, mv=mv, window=window, stride=stride, lag=lag, want_matrix=True)
    R = host["stats"].shape[1]
    dev = torch.device("cuda", 0)
    d_mu, d_mv, d_ids = (torch.from_numpy(a).to(dev) for a in (mu, mv, ids))
    for src in ("mu_mv", "ids"):
        stats = torch.full((5, R), -7.0, dtype=torch.float64, device=dev)
        matrix = torch.full((R, 51, 51), -7, dtype=torch.int32, device=dev)
        samples = torch.full((R,), -7, dtype=torch.int32, device=dev)
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        plan.transition_markov_device(d_mu.data_ptr(), d_mv.data_ptr(), U, T, window, stride, lag, stats.data_ptr(), matrix.data_ptr(),
                                      samples.data_ptr(), status.data_ptr(), **(dict(d_ids=d_ids.data_ptr()) if src == "ids" else {}))
        engine.synchronize()
        same_bytes(dict(stats=stats.cpu().numpy(), samples=samples.cpu().numpy(), matrix=matrix.cpu().numpy()), host, src)
        assert status.cpu().numpy().tolist() == [0, int((host["samples"] == 0).sum())]


def test_chunk_rows_do_not_change_a_bit(engine, plans):
    """The chunked shape (331 x 99 = 32769 candidates), five rows, in passes of one, three and all rows."""
    mu, mv = walk(331, 104, 0.3, 29)
    ids = ids_of(mu, mv)
    for tcs in ([50], [50, 100, 200]):
        plan = plans(tcs)
        try:
            runs = []
            for rows in (1, 3, 0):
                engine.test_markov_chunk_rows(rows)
                runs.append(plan.transition_markov(mu=mu, mv=mv, window=99, stride=1, lag=1, want_matrix=True))
                runs.append(plan.transition_markov(ids=ids, window=99, stride=1, lag=1, want_matrix=False))
        finally:
            engine.test_markov_chunk_rows(0)
        assert runs[0]["stats"].shape == (5, 5)
        for r in runs[1:]:
            same_bytes(r, runs[0], f"chunk rows {tcs}")
        check(runs[0], mo.fast(mu, mv, W, H, tcs, 99, 1, 1), f"chunked {tcs}")
        same_bytes(plan.transition_markov(mu=mu, mv=mv, window=99, stride=2, lag=1, want_matrix=True),
                   {k: np.ascontiguousarray(runs[0][k][..., ::2] if k == "stats" else runs[0][k][::2]) for k in ("stats", "samples", "matrix")},
                   "stride 2")


# ------------------------------------------------------------------------------------------- errors and limits
def test_invalid_arguments(native, plans):
    mu, mv = walk(4, 30, 0.0, 31)
    plan = plans([50])
    lib = native.load_library()
    stats = np.empty((5, 64))
    for window, stride, lag in ((0, 1, 1), (-1, 1, 1), (5, 0, 1), (5, -2, 1), (30, 1, 1), (28, 1, 3), (5, 1, 0), (5, 1, -1), (1, 1, 30),
                                (1, 1, 31)):
        with pytest.raises(ValueError):
            plan.transition_markov(mu=mu, mv=mv, window=window, stride=stride, lag=lag)
        rc = lib.vet_transition_markov_host(plan.handle, native._ptr(mu), native._ptr(mv), None, 4, 30, window, stride, lag,
                                            native._ptr(stats), None, None)
        assert rc == native.VET_ERR_INVALID, (window, stride, lag)
        with pytest.raises(native.NativeError) as e:          # the device entry refuses before it looks at a pointer
            plan.transition_markov_device(8, 8, 4, 30, window, stride, lag, 8)
        assert e.value.code == native.VET_ERR_INVALID
    # the longest legal window and lag
    assert plan.transition_markov(mu=mu, mv=mv, window=27, lag=3)["stats"].shape == (5, 1)
    assert plan.transition_markov(mu=mu, mv=mv, window=1, lag=29)["stats"].shape == (5, 1)
    assert lib.vet_transition_markov_host(plan.handle, native._ptr(mu), native._ptr(mv), None, 4, 30, 5, 1, 1, None, None, None) \
        == native.VET_ERR_INVALID


def test_unsupported_plans_and_outputs(native, engine, plans):
    mu, mv = walk(2, 8, 0.0, 37)
    lib = native.load_library()
    stats = np.empty((5, 8))
    # a lattice of 2049 tiles, wherever it stands in the plan
    for tcs in ([2048], [50, 2048]):
        big = native.Plan(engine, [vo.fibonacci_lattice(t) for t in tcs], 120.0, 2.0, True, W, H)
        assert max(big.n_tiles) == 2049
        with pytest.raises(native.NativeError) as e:
            big.transition_markov(mu=mu, mv=mv, window=2)
        assert e.value.code == native.VET_ERR_UNSUPPORTED and "2049" in str(e.value)
        assert lib.vet_transition_markov_host(big.handle, native._ptr(mu), native._ptr(mv), None, 2, 8, 2, 1, 1, native._ptr(stats),
                                              None, None) == native.VET_ERR_UNSUPPORTED
        big.close()
    # a matrix output of 2^31 cells or more: 537 rows of 2001 x 2001 (536 fit); refused before a pointer is looked at
    plan = plans([2000])
    dummy = np.empty(8, dtype=np.int32)
    rc = lib.vet_transition_markov_host(plan.handle, native._ptr(dummy), native._ptr(dummy), None, 1, 538, 1, 1, 1, native._ptr(stats),
                                        native._ptr(dummy), None)
    assert rc == native.VET_ERR_UNSUPPORTED and b"cells" in lib.vet_last_error()
    with pytest.raises(native.NativeError) as e:
        plan.transition_markov_device(8, 8, 1, 538, 1, 1, 1, 8, d_matrix=8)
    assert e.value.code == native.VET_ERR_UNSUPPORTED
    assert 536 * 2001 * 2001 <= 2**31 - 1 < 537 * 2001 * 2001


def test_sample_out_of_range(native, plans):
    mu, mv = walk(7, 40, 0.0, 41)
    bad_mu, gone_mu, gone_mv = mu.copy(), mu.copy(), mv.copy()
    bad_mu[12, 3] = 1.5
    gone_mu[12, 3] = gone_mv[12, 3] = np.nan
    plan = plans([50, 100, 200])
    with pytest.raises(native.NativeError) as e:
        plan.transition_markov(mu=bad_mu, mv=mv, window=5)
    assert e.value.code == native.VET_ERR_RANGE
    for window, lag in ((5, 1), (5, 3), (None, 1)):
        res = plan.transition_markov(mu=bad_mu, mv=mv, window=window, lag=lag, want_matrix=True, check=False)
        clean = plan.transition_markov(mu=mu, mv=mv, window=window, lag=lag)
        assert res["code"] == native.VET_ERR_RANGE and clean["code"] == native.VET_OK
        check(res, mo.fast(gone_mu, gone_mv, W, H, [50, 100, 200], window, 1, lag), "the sample counts as absent")
        w = 40 - lag if window is None else window
        # rows that pool pair 12 (the sample as source) or pair 12 - lag (as destination) lose exactly one sample each
        lost = np.array([sum(r <= f < r + w for f in (12, 12 - lag)) for r in range(len(res["samples"]))])
        assert np.array_equal(clean["samples"] - res["samples"], lost) and lost.any()


# ------------------------------------------------------------------------------------------- the analyzer
def test_analyzer_returns_the_markov_frame(tmp_path):
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
    df = an.compute_markov_entropy(window=20, stride=5, lag=3, keep_matrix=True)
    stats, samples, matrix = mo.fast(mu, mv, W, H, [50, 100], 20, 5, 3)                 # pooled counts: the user order does not matter
    assert list(df.columns) == ["time", "time_end", "samples", "rate", "stationary", "dest", "mutual", "stay", "matrix"]
    assert len(df) == mo.n_rows(T, 20, 5, 3) == 8
    later = an._samples()[1][3:]
    assert np.array_equal(df["time"], later[::5][:8]) and np.array_equal(df["time_end"], later[19::5][:8])
    for i, name in enumerate(mo.STATS):
        np.testing.assert_allclose(df[name].to_numpy(), stats[i], rtol=0, atol=ATOL, err_msg=name)
    assert np.array_equal(df["samples"], samples)
    assert all(np.array_equal(df["matrix"][r], matrix[r]) and df["matrix"][r].shape == (51, 51) for r in range(8))
    assert df["matrix"][1].base is not None and df["matrix"][1].base is df["matrix"][0].base          # views into one array
    assert df.attrs["lag"] == 3 and df.attrs["lag_frames"] == 3 and df.attrs["n_tiles"] == 51
    assert sorted(df.attrs["users"]) == [f"user{u:03d}" for u in range(U)] and df.attrs["users"] == list(an._samples()[4])
    assert an._entropy_results is per_pair and np.array_equal(per_pair["entropy"].to_numpy(), kept)    # left alone
    whole = an.compute_markov_entropy()
    assert list(whole.columns) == list(df.columns)[:-1] and len(whole) == 1 and whole.attrs["lag"] == 1
    assert whole["time"][0] == an._samples()[1][1] and whole["time_end"][0] == an._samples()[1][-1]
    np.testing.assert_allclose(whole["mutual"][0], mo.fast(mu, mv, W, H, [50, 100], None, 1, 1)[0][3, 0], rtol=0, atol=ATOL)
    with pytest.raises(ValueError):
        an.compute_markov_entropy(window=58, lag=3)
    # an empty window is NaN, not an exception
    a2 = TransitionEntropyAnalyzer(AnalyzerConfig(tile_counts=[50]))
    m2, v2 = mu.copy(), mv.copy()
    m2[10:40] = np.nan
    v2[10:40] = np.nan
    a2.load_arrays(times, m2, v2)
    df2 = a2.compute_markov_entropy(window=20, keep_matrix=True)
    gone = df2["samples"].to_numpy() == 0
    assert gone.any() and not gone.all()
    for name in mo.STATS:
        assert np.array_equal(np.isnan(df2[name].to_numpy()), gone), name
    assert all((df2["matrix"][r] == 0).all() for r in np.flatnonzero(gone))
    # a sample outside [0, 1] is the engine's refusal
    a2._dense[1][2, 0] = 1.5
    with pytest.raises(ValidationError, match="^Normalized coordinates must be between 0 and 1$"):
        a2.compute_markov_entropy(window=20)
