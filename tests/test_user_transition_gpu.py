"""GPU: per-viewer transition entropy through the C-ABI (Plan.transition_per_user -> vet_user_transition_entropy_host, the
device entry, the analyzer).  Row (u, r) pools user u's own transitions of frame pairs [r * stride, r * stride + window); the
references are golden G17 (the real reference on that viewer's dicts, tools/gen_golden_user_transition.py) and the numpy oracles
of tests/_user_transition_oracle.py (pinned against G17 in tests/test_user_transition_surface.py).  Entropy: the project's
contract, 1e-6 relative, NaN = NaN; samples and source counts exact.  Rows of up to 64 pairs run k_user_transition_wave, longer
ones k_user_transition; Engine.test_user_transition_hash sends the short ones through the second kernel too."""
import ctypes

import numpy as np
import pytest

from oracle import vet_oracle as vo
from tests import _user_transition_oracle as ut

pytestmark = pytest.mark.gpu

W, H = 100, 200
RTOL = 1e-6
SHAPES = ((299, 1), (20, 20), (20, 7), (64, 5), (65, 5), (2, 1))
TILE_COUNTS = ((50,), (50, 100, 200), (20,))
HASH_SLOTS = 8192          # k_user_transition's 1024-thread shape: a pass holds a bucket bound of 0.6 * 8192 - n (vet_transition.hpp)


@pytest.fixture(scope="module")
def native():
    from viewport_entropy_toolkit import _native
    return _native


@pytest.fixture(scope="module")
def engine(native):
    eng = native.Engine.default()
    eng.test_user_transition_hash(False)
    return eng


@pytest.fixture(scope="module")
def g17(golden_dir):
    g16 = np.load(golden_dir / "g16_user_entropy.npz")
    return g16["mu"], g16["mv"], np.load(golden_dir / "g17_user_transition.npz")


def fib_plan(native, engine, tcs):
    return native.Plan(engine, [vo.fibonacci_lattice(t) for t in tcs], 120.0, 2.0, True, W, H)


def close(got, want, msg="", rtol=RTOL):
    print(msg, "max rel err", float(np.nanmax(np.abs(got - want) / np.maximum(np.abs(want), 1e-300), initial=0.0)))
    assert np.array_equal(np.isnan(got), np.isnan(want)), (msg, np.argwhere(np.isnan(got) != np.isnan(want))[:10])
    np.testing.assert_allclose(got, want, rtol=rtol, atol=0, equal_nan=True, err_msg=msg)


def ids_of(mu, mv):
    px, py, present, _ = vo.sample_directions(mu, mv, W, H)
    return np.where(present, py * (W + 1) + px, -1).astype(np.int32)


def walk(U, T, p_absent, seed):
    from viewport_entropy_toolkit import _synthetic
    return _synthetic.random_walk_video(U, T, base_seed=seed, p_absent=p_absent)


def hashed(engine, fn):
    """fn() with rows of up to 64 pairs sent through the hash kernel"""
    engine.test_user_transition_hash(True)
    try:
        return fn()
    finally:
        engine.test_user_transition_hash(False)


def check_fast(res, mu, mv, tcs, window, stride, msg, tiles=None):
    """every row against the closed-form oracle"""
    ent, samples, src = ut.fast(mu, mv, W, H, tcs, window, stride, tiles=tiles)
    assert res["entropy"].shape == ent.shape, msg
    close(res["entropy"], ent, msg)
    assert np.array_equal(res["samples"], samples), msg
    if res.get("srccount") is not None:
        assert np.array_equal(res["srccount"], src), msg
    return samples


def g17_cases():
    for tcs in TILE_COUNTS:
        for w, s in SHAPES:
            yield f"tc{'_'.join(map(str, tcs))}_w{w}_s{s}", tcs, w, s


def check_g17(g, tag, res, msg):
    rows = g[f"{tag}__rows"]
    close(res["entropy"][:, rows], g[f"{tag}__entropy"], msg)
    assert np.array_equal(res["samples"][:, rows], g[f"{tag}__samples"]), msg
    if res.get("srccount") is not None:
        assert np.array_equal(res["srccount"][:, rows], g[f"{tag}__srccount"]), msg
    assert np.isnan(res["entropy"][res["samples"] <= 1]).all(), msg


# ------------------------------------------------------------------------------------------- 1. the reference (golden G17)
def test_host_entry_vs_reference_golden_grid_and_ids(native, engine, g17):
    mu, mv, g = g17
    ids = ids_of(mu, mv)
    plans = {}
    for tag, tcs, w, s in g17_cases():
        plan = plans.get(tcs) or plans.setdefault(tcs, fib_plan(native, engine, tcs))
        for kw in (dict(mu=mu, mv=mv), dict(ids=ids)):
            res = plan.transition_per_user(window=None if w == 299 else w, stride=s, want_srccount=True, **kw)
            assert res["code"] == native.VET_OK and res["entropy"].shape == (8, ut.n_rows(300, w, s)), tag    # empty rows: no error
            check_g17(g, tag, res, f"{tag} {'ids' if 'ids' in kw else 'grid'}")
    for p in plans.values():
        p.close()


def test_device_entry_vs_reference_golden(native, engine, g17):
    """vet_user_transition_entropy / _ids on device buffers; d_status = {0, rows without a common sample}, added to."""
    lib = engine.lib
    mu, mv, g = g17
    mu, mv = np.ascontiguousarray(mu), np.ascontiguousarray(mv)
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
        for tag, tcs, w, s in g17_cases():
            plan = plans.get(tcs) or plans.setdefault(tcs, fib_plan(native, engine, tcs))
            R = ut.n_rows(T, w, s)
            n0 = plan.n_tiles[0]
            for entry in ("grid", "ids"):
                ent, src, smp = np.empty((U, R)), np.empty((U, R, n0), np.int32), np.empty((U, R), np.int32)
                st = np.array([0, 1000], np.int32)
                d_ent, d_src, d_s, d_st = dev(ent.nbytes), dev(src.nbytes), dev(smp.nbytes), dev(8, st)
                if entry == "grid":
                    plan.transition_per_user_device(d_mu.value, d_mv.value, U, T, w, s, d_ent.value, d_src.value, d_s.value,
                                                    d_st.value)
                else:
                    native._check(lib, lib.vet_user_transition_entropy_ids(plan.handle, d_ids, U, T, w, s, d_ent, d_src, d_s,
                                                                           d_st, None))
                for h, d in ((ent, d_ent), (src, d_src), (smp, d_s), (st, d_st)):
                    assert lib.vet_memcpy_d2h(engine.handle, native._ptr(h), d, h.nbytes) == 0
                check_g17(g, tag, dict(entropy=ent, srccount=src, samples=smp), f"{tag} device {entry}")
                assert st.tolist() == [0, 1000 + int((smp == 0).sum())], tag
    finally:
        engine.synchronize()
        for p in bufs:
            lib.vet_free(engine.handle, p)
        for p in plans.values():
            p.close()


# ------------------------------------------------------------------------------------------- 2. the analyzer
def test_analyzer_on_a_csv_directory_vs_reference_golden(native, g17, golden_dir, tmp_path):
    """The dataset as CSV files through process_directory.  The ingest builds the reference's frame table: a time is appended
    when some user first shows it, so with absent samples the table is a permutation of the dataset's frames (and the CSV round
    trip moves a sample by a few ulps).  compute_user_entropy runs on the table as it is — checked against the oracle on the
    ingested arrays — and G17, which is in the dataset's frame order, is compared on the same ingested samples put back into
    time order (what tools/gen_golden_user_entropy.py does with the reference's own table)."""
    import pandas as pd
    from viewport_entropy_toolkit import TransitionEntropyAnalyzer
    from viewport_entropy_toolkit.config import AnalyzerConfig
    mu, mv, g = g17
    times = np.load(golden_dir / "g4_spatial.npz")["time_in"]                 # [U][T], the dataset's clock
    d = tmp_path / "video"
    d.mkdir()
    for u in range(8):
        keep = ~np.isnan(mu[:, u])
        pd.DataFrame({"time": times[u][keep], "2dmu": mu[keep, u], "2dmv": mv[keep, u]}).to_csv(d / f"user{u:03d}.csv", index=False)
    for tcs in TILE_COUNTS:
        an = TransitionEntropyAnalyzer(AnalyzerConfig(tile_counts=list(tcs), output_dir=tmp_path / "out"))
        an.process_directory(d)
        kind, t_an, a, b, names = an._samples()
        order = [int(name[4:]) for name in names]
        by_time = np.argsort(t_an, kind="stable")
        assert kind == "grid"
        # the ingest's frames are the dataset's: the CSV round trip moves a value by a few ulps, never to another pixel
        np.testing.assert_allclose(np.asarray(t_an)[by_time], times[0], rtol=1e-14, atol=0)
        assert np.array_equal(ids_of(a[by_time], b[by_time]), ids_of(mu[:, order], mv[:, order]))
        # ---- the table as ingested, against the oracle on the ingested arrays
        windowed_cols = list(an.compute_windowed_entropy(20, 20).columns)
        for w, s in ((20, 7), (64, 5)):
            df = an.compute_user_entropy(w, s)
            R = ut.n_rows(300, w, s)
            assert list(df.columns) == ["user"] + windowed_cols == ["user", "time", "time_end", "entropy", "samples", "tile_weights"]
            assert len(df) == 8 * R and list(df["user"]) == [n for n in names for _ in range(R)]
            pair_time = np.asarray(t_an)[1:]
            assert np.array_equal(df["time"], np.tile(pair_time[np.arange(R) * s], 8))
            assert np.array_equal(df["time_end"], np.tile(pair_time[np.arange(R) * s + w - 1], 8))
            ent, samples, src = ut.fast(a, b, W, H, list(tcs), w, s)
            close(df["entropy"].to_numpy().reshape(8, R), ent, f"{tcs} w{w} s{s} as ingested")
            assert np.array_equal(df["samples"].to_numpy().reshape(8, R), samples)
            assert (samples == 0).any() and np.isnan(ent[samples == 0]).all()             # a viewer's empty rows: NaN, samples 0
            tiles = an._fibonacci_vectors[tcs[0]]
            u, r = 5, R // 2
            cell = df["tile_weights"][u * R + r]
            assert {k: int(v) for k, v in dict(cell).items()} == {tiles[t]: int(src[u, r, t]) for t in np.flatnonzero(src[u, r])}
        assert an._entropy_results is None                                        # compute_entropy's results are left alone
        # ---- the same ingested samples in time order, against G17
        an.load_arrays(np.asarray(t_an)[by_time], a[by_time], b[by_time], user_names=names)
        inv = np.argsort(order)                                                   # dataset user -> analyzer row block
        for tag, tcs2, w, s in g17_cases():
            if tcs2 != tcs:
                continue
            df = an.compute_user_entropy(None if w == 299 else w, s)
            R = ut.n_rows(300, w, s)
            res = dict(entropy=df["entropy"].to_numpy().reshape(8, R)[inv], samples=df["samples"].to_numpy().reshape(8, R)[inv])
            check_g17(g, tag, res, tag + " analyzer")
            rows = g[f"{tag}__rows"]
            u, i = 5, len(rows) // 2
            cell = df["tile_weights"][int(inv[u]) * R + int(rows[i])]
            want = g[f"{tag}__srccount"][u, i]
            assert {k: int(v) for k, v in dict(cell).items()} == {tiles[t]: int(want[t]) for t in np.flatnonzero(want)}, tag


# ------------------------------------------------------------------------------------------- 3. wave kernel vs hash kernel
def _switch_T(window):
    spw = 64 // window
    R = 3 * spw + 1 if spw > 1 else 5             # R is no multiple of the rows a wave holds: a predicated tail segment
    return R + window


@pytest.mark.parametrize("U", [1, 5])
@pytest.mark.parametrize("window", [1, 2, 3, 20, 21, 22, 32, 33, 63, 64])
def test_wave_kernel_equals_hash_kernel(native, engine, window, U):
    tcs = [50, 100]
    plan = fib_plan(native, engine, tcs)
    for T, stride in ((_switch_T(window), 1), (_switch_T(window) + 7, 3)) + (((2, 1),) if window == 1 else ()):
        mu, mv = walk(U, T, 0.2, 100 * window + U)
        msg = f"w{window} U{U} T{T} s{stride}"
        a = plan.transition_per_user(mu=mu, mv=mv, window=window, stride=stride, want_srccount=True)
        b = hashed(engine, lambda: plan.transition_per_user(mu=mu, mv=mv, window=window, stride=stride, want_srccount=True))
        if stride == 1 and 64 // window > 1 and T > 2:
            assert a["entropy"].shape[1] % (64 // window) != 0
        close(a["entropy"], b["entropy"], msg + " wave vs hash", rtol=1e-12)
        assert np.array_equal(a["samples"], b["samples"]) and np.array_equal(a["srccount"], b["srccount"]), msg
        check_fast(a, mu, mv, tcs, window, stride, msg + " wave")
        check_fast(b, mu, mv, tcs, window, stride, msg + " hash")
    plan.close()


# ------------------------------------------------------------------------------------------- 4. the hash shapes
@pytest.mark.parametrize("p_absent", [0.0, 0.3], ids=["full", "absent"])
@pytest.mark.parametrize("tcs", [[50], [50, 100, 200]], ids=["tc50", "tc50_100_200"])
def test_hash_shapes_vs_oracle(native, engine, tcs, p_absent):
    """64 threads / 512 slots up to 256 pairs, 256 / 2048 up to 1024, 256 / 4096 up to 2048, 1024 / 8192 above: both sides of
    every threshold."""
    U, T = 3, 2051
    mu, mv = walk(U, T, p_absent, 41)
    tiles = ut.tiles_of(mu, mv, W, H, tcs)
    plan = fib_plan(native, engine, tcs)
    for window in (65, 256, 257, 1024, 1025, 2048, 2049):
        stride = 1 if window >= 2048 else 331
        res = plan.transition_per_user(mu=mu, mv=mv, window=window, stride=stride, want_srccount=True)
        check_fast(res, mu, mv, tcs, window, stride, f"w{window}", tiles=tiles)
    plan.close()


def test_uniform_on_sphere_takes_several_hash_passes(native, engine):
    from viewport_entropy_toolkit import _synthetic
    U, T, tc = 2, 6000, 1000
    window = T - 1
    n = len(vo.fibonacci_lattice(tc))
    mu, mv = _synthetic.uniform_sphere_video(U, T, base_seed=77)
    tiles = ut.tiles_of(mu, mv, W, H, [tc])
    for u in range(U):
        bound = ut.bucket_bound(tiles[0][:, u], 0, window, n)
        assert bound > HASH_SLOTS * 6 // 10 - n, bound             # the row is cut into more than one range of source tiles
    plan = fib_plan(native, engine, [tc])
    res = plan.transition_per_user(mu=mu, mv=mv, window=window, want_srccount=True)
    check_fast(res, mu, mv, [tc], window, 1, "uniform", tiles=tiles)
    plan.close()


# ------------------------------------------------------------------------------------------- 5. identity with the windowed call
@pytest.mark.parametrize("window", [20, 100])
def test_one_user_equals_the_windowed_call(native, engine, window):
    mu, mv = walk(1, 150, 0.2, 5)
    plan = fib_plan(native, engine, [50, 100, 200])
    for stride in (1, 7):
        a = plan.transition_per_user(mu=mu, mv=mv, window=window, stride=stride, want_srccount=True)
        b = plan.transition_windowed(mu=mu, mv=mv, window=window, stride=stride, want_srccount=True, check=False)
        close(a["entropy"][0], b["entropy"], f"w{window} s{stride}", rtol=1e-12)
        assert np.array_equal(a["samples"][0], b["samples"]) and np.array_equal(a["srccount"][0], b["srccount"])
    plan.close()


# ------------------------------------------------------------------------------------------- 6. purity
@pytest.mark.parametrize("window", [20, 64, 65])
def test_rows_are_pure_functions_of_their_own_frames(native, engine, window):
    mu, mv = walk(6, 200, 0.2, 7)
    mu[60:130, 2], mv[60:130, 2] = np.nan, np.nan
    ids = ids_of(mu, mv)
    plan = fib_plan(native, engine, [50, 100, 200])

    def same(x, y, msg):
        assert x["entropy"].tobytes() == y["entropy"].tobytes(), msg
        assert np.array_equal(x["samples"], y["samples"]) and np.array_equal(x["srccount"], y["srccount"]), msg

    def sel(x, f):
        return {k: (f(v) if k != "code" else v) for k, v in x.items()}

    def run(**kw):
        return plan.transition_per_user(window=window, want_srccount=True, **kw)

    a = run(mu=mu, mv=mv, stride=1)
    same(a, run(mu=mu, mv=mv, stride=1), "run to run")
    same(sel(a, lambda v: v[:, ::7]), run(mu=mu, mv=mv, stride=7), "whatever stride selected the row")
    same(sel(a, lambda v: v[:, 13:]), run(mu=mu[13:], mv=mv[13:], stride=1), "frames shifted by 13")
    same(sel(a, lambda v: v[3:4]), run(mu=mu[:, 3:4], mv=mv[:, 3:4], stride=1), "user 3 alone")
    perm = np.array([4, 0, 5, 2, 1, 3])
    same(sel(a, lambda v: v[perm]), run(mu=mu[:, perm], mv=mv[:, perm], stride=1), "users permuted")
    same(a, run(ids=ids, stride=1), "ids entry")
    plan.close()


# ------------------------------------------------------------------------------------------- 7. transpose and pair edges
@pytest.mark.parametrize("U,T", [(1, 2), (1, 66), (63, 65), (65, 130)])
def test_transpose_and_pair_edges(native, engine, U, T):
    rng = np.random.default_rng(1000 * U + T)
    mu, mv = rng.random((T, U)), rng.random((T, U))
    absent = rng.random((T, U)) < 0.15
    mu[absent] = np.nan
    mv[absent] = np.nan
    tiles = ut.tiles_of(mu, mv, W, H, [50])
    plan = fib_plan(native, engine, [50])
    both = ~absent[:-1] & ~absent[1:]
    for kw in (dict(mu=mu, mv=mv), dict(ids=ids_of(mu, mv))):
        one = plan.transition_per_user(window=1, want_srccount=True, **kw)          # every pair read back one by one
        assert np.array_equal(one["samples"], both.T.astype(np.int32)) and np.isnan(one["entropy"]).all()   # N = 1: 0 / 0
        onehot = (np.where(both, tiles[0][:-1], -1).T[:, :, None] == np.arange(one["srccount"].shape[-1])).astype(np.int32)
        assert np.array_equal(one["srccount"], onehot)
        whole = plan.transition_per_user(window=T - 1, want_srccount=True, **kw)
        check_fast(whole, mu, mv, [50], T - 1, 1, f"U{U} T{T} whole", tiles=tiles)
    plan.close()


# ------------------------------------------------------------------------------------------- 8. quirks and errors
def test_quirks(native, engine):
    mu, mv = walk(4, 120, 0.0, 11)
    mu[30:90, 1], mv[30:90, 1] = np.nan, np.nan                       # a viewer away for a stretch
    mu[1:, 2], mv[1:, 2] = np.nan, np.nan
    mu[50:52, 2], mv[50:52, 2] = 0.4, 0.6                             # a viewer with one pair in the whole video
    plan = fib_plan(native, engine, [50])
    for on in (False, True):
        engine.test_user_transition_hash(on)
        try:
            res = plan.transition_per_user(mu=mu, mv=mv, window=20, stride=3, want_srccount=True)
        finally:
            engine.test_user_transition_hash(False)
        assert res["code"] == native.VET_OK                            # rows without a common sample are data
        samples = check_fast(res, mu, mv, [50], 20, 3, f"quirks hash={on}")
        empty = samples == 0
        assert empty[1].any() and empty[2].any() and not empty[0].any()
        assert np.isnan(res["entropy"][empty]).all() and (res["srccount"][empty] == 0).all()
        assert (samples[2] == 1).any() and np.isnan(res["entropy"][2]).all()      # N = 1: the reference's 0 / 0
    # status[1] counts the rows without a common sample and only those
    lib = engine.lib
    T, U = mu.shape
    R = ut.n_rows(T, 20, 3)
    bufs = []

    def dev(nbytes, src=None):
        p = ctypes.c_void_p()
        assert lib.vet_malloc(engine.handle, nbytes, ctypes.byref(p)) == 0
        bufs.append(p)
        if src is not None:
            assert lib.vet_memcpy_h2d(engine.handle, p, native._ptr(src), nbytes) == 0
        return p
    try:
        mu_c, mv_c = np.ascontiguousarray(mu), np.ascontiguousarray(mv)
        st = np.zeros(2, np.int32)
        d_mu, d_mv, d_ent, d_st = dev(mu_c.nbytes, mu_c), dev(mv_c.nbytes, mv_c), dev(U * R * 8), dev(8, st)
        plan.transition_per_user_device(d_mu.value, d_mv.value, U, T, 20, 3, d_ent.value, 0, 0, d_st.value)
        assert lib.vet_memcpy_d2h(engine.handle, native._ptr(st), d_st, 8) == 0
        assert st.tolist() == [0, int(empty.sum())]
    finally:
        engine.synchronize()
        for p in bufs:
            lib.vet_free(engine.handle, p)
    # a sample outside [0, 1]: VET_ERR_RANGE, the outputs still written (the sample counts as absent)
    bad = mu.copy()
    bad[5, 0] = 1.5
    r = plan.transition_per_user(mu=bad, mv=mv, window=4, check=False)
    assert r["code"] == native.VET_ERR_RANGE
    ok = plan.transition_per_user(mu=mu, mv=mv, window=4)
    covers = np.zeros_like(ok["samples"])
    covers[0, 1:6] = 1                                  # pairs 4 and 5 hold frame 5: rows 1..5 lose one sample each ...
    covers[0, 2:5] = 2                                  # ... rows 2..4 hold both pairs
    assert np.array_equal(r["samples"], ok["samples"] - covers)
    with pytest.raises(native.NativeError):
        plan.transition_per_user(mu=bad, mv=mv, window=4)
    plan.close()


def test_refusals_launch_and_allocate_nothing(native, engine):
    lib = engine.lib
    mu, mv = walk(16, 30, 0.0, 9)
    plan = fib_plan(native, engine, [50])
    plan.transition_per_user(mu=mu, mv=mv, window=4)                  # tables built, workspace and staging grown
    hip = ctypes.CDLL(native.HIP_RUNTIME_PRELOADED or "libamdhip64.so")

    def free_bytes():
        engine.synchronize()
        free, total = ctypes.c_size_t(), ctypes.c_size_t()
        assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value

    def launches():
        return sum(engine.profile_get(k)[1] for k in native.KERNEL_IDS)

    engine.profile_enable(True)
    engine.profile_reset()
    try:
        before = free_bytes()
        ent = np.zeros(64 * 16)
        for window, stride in ((0, 1), (4, 0), (30, 1), (-1, 1)):
            with pytest.raises(ValueError):
                plan.transition_per_user(mu=mu, mv=mv, window=window, stride=stride)
            rc = lib.vet_user_transition_entropy_host(plan.handle, native._ptr(mu), native._ptr(mv), None, 16, 30, window, stride,
                                                      native._ptr(ent), None, None)
            assert rc == native.VET_ERR_INVALID and lib.vet_last_error()
        one = np.full((1, 16), 0.5)
        assert lib.vet_user_transition_entropy_host(plan.handle, native._ptr(one), native._ptr(one), None, 16, 1, 1, 1,
                                                    native._ptr(ent), None, None) == native.VET_ERR_INVALID       # n_frames < 2
        # U * R >= 2^31: refused from the shape alone, before a sample is read, staged or a byte of the 8 GiB of direction ids
        # is allocated; the host entry and the device entry, a short window (wave kernel) and a long one alike
        # (no sample array is passed: a call that got past the refusal would stop at VET_ERR_INVALID for the NULL samples)
        U, T = 1 << 16, (1 << 15) + 300
        for window in (1, 200):
            assert ut.n_rows(T, window, 1) * U >= 1 << 31
            assert lib.vet_user_transition_entropy_host(plan.handle, None, None, None, U, T, window, 1,
                                                        native._ptr(ent), None, None) == native.VET_ERR_UNSUPPORTED
            assert lib.vet_user_transition_entropy(plan.handle, None, None, U, T, window, 1,
                                                   native._ptr(ent), None, None, None, None) == native.VET_ERR_UNSUPPORTED
        # window >= 2^19
        assert lib.vet_user_transition_entropy_host(plan.handle, None, None, None, 1, (1 << 19) + 1, 1 << 19, 1,
                                                    native._ptr(ent), None, None) == native.VET_ERR_UNSUPPORTED
        # nothing launched.  Free memory: the U * R shapes would have grown the workspace by 8 GiB; what the other refusals would
        # grow is far smaller than the slack allowed here, so for them the launch count alone is the evidence
        assert launches() == 0 and before - free_bytes() < 64 << 20
        # a lattice above TRANS_BIG_MAX_TILES, whatever the window
        big = fib_plan(native, engine, [50, 2900])
        engine.profile_reset()                                         # the plan's own set-up kernels are not the call's
        before_big = free_bytes()
        for window in (4, 20, 29):
            with pytest.raises(native.NativeError) as e:
                big.transition_per_user(mu=mu, mv=mv, window=window)
            assert e.value.code == native.VET_ERR_UNSUPPORTED
        assert launches() == 0 and before_big - free_bytes() < 64 << 20   # nothing launched (the evidence here), no growth
        big.close()
    finally:
        engine.profile_enable(False)
    plan.close()
