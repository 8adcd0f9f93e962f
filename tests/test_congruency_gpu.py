"""GPU: the viewer congruency through the C-ABI (Plan.congruency -> vet_congruency_host, the device entries through
Plan.congruency_device, the analyzers' compute_congruency).  The reference is the numpy oracle of tests/_congruency_oracle.py
(written from the definition in include/vet.h on top of the saliency oracle; its Q_u is the direct double sum, not the library's
split) — never the code under test.

Tolerances.  Counts, ``scored`` and the status words: equality; NaN, +inf and -inf in the same places.  Finite values: 1e-10 relative +
1e-10 absolute, the saliency-similarity suite's tolerance; a numpy prototype of these values on golden G15 agrees with its own
longdouble evaluation to 4.5e-14.  The tests print the largest deviations they saw.

Largest deviations seen on an MI355X over all tests of this file, relative to 1 + |value|: lift 2.1e-15, info_gain 6.3e-15,
nss 4.4e-14; the row means lift 1.0e-15, info_gain 2.7e-15, nss 1.6e-14."""
import functools

import numpy as np
import pytest

from tests import _congruency_oracle as co
from tests import _saliency_oracle as so

pytestmark = pytest.mark.gpu

W, H = 100, 200
KEYS = ("stats", "counts", "rows")
# (sigma in degrees, window) on golden G15
SETTINGS = [(5.0, 5), (2.0, 1), (10.0, 60), (1.0, 5), (5.0, 20), (30.0, 20)]


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
    assert np.array_equal(p.read_dirs(), grid())                 # the plan's own direction table: the Vectors the oracle works on
    yield p
    p.close()


@functools.lru_cache(maxsize=None)
def grid():
    return so.grid_table(W, H)


@functools.lru_cache(maxsize=None)
def oracle():
    return co.Oracle(grid())


@functools.lru_cache(maxsize=None)
def g15():
    """(mu, mv, ids) of golden G15's video moved off the centre: 8 viewers x 60 frames; shared, never written to"""
    from pathlib import Path
    g = np.load(Path(__file__).resolve().parent / "golden" / "g15_windowed_transition.npz")
    mu, mv = so.off_centre(g["mu"], g["mv"])
    ids = so.ids_of(mu, mv, W, H)
    for a in (mu, mv, ids):
        a.setflags(write=False)
    return mu, mv, ids


@functools.lru_cache(maxsize=None)
def sphere(U, T, seed):
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.uniform_sphere_video(U, T, base_seed=seed)
    ids = so.ids_of(mu, mv, W, H)
    for a in (mu, mv, ids):
        a.setflags(write=False)
    return mu, mv, ids


def rad(deg):
    return min(float(np.radians(deg)), float(np.pi))


def check(res, ids, sigma_deg, window, stride, msg, nss=True, only=None):
    """a result dict against the oracle at the module's tolerances; returns the oracle's rows"""
    T, U = ids.shape
    w = T if window is None else window
    R = (T - w) // stride + 1
    assert res["code"] == 0 and res["stats"].shape == (3, U, R) and res["counts"].shape == (3, U, R) and res["rows"].shape == (4, R), msg
    assert res["stats"].dtype == np.float64 and res["counts"].dtype == np.int64 and res["rows"].dtype == np.float64, msg
    want = oracle().rows(ids, w, stride, rad(sigma_deg), nss=nss, only=only)
    rs = np.arange(R) if only is None else np.asarray(only)
    stats, counts, rows = res["stats"][:, :, rs], res["counts"][:, :, rs], res["rows"][:, rs]
    assert np.array_equal(counts, want["counts"]), msg
    assert np.array_equal(rows[0], want["rows"][0]), msg
    scored = (counts[0] > 0) & (counts[2] > 0)
    assert np.isnan(stats[:2][:, ~scored]).all() and not np.isnan(stats[:2][:, scored]).any(), msg
    if not nss:
        assert np.isnan(stats[2]).all() and np.isnan(rows[3]).all(), msg
    dev = {}
    for name, got, ref in [(n, stats[k], want["stats"][k]) for k, n in enumerate(co.STATS)] + \
                          [("row " + n, rows[1 + k], want["rows"][1 + k]) for k, n in enumerate(co.STATS)]:
        assert np.array_equal(np.isnan(got), np.isnan(ref)), (msg, name)
        assert np.array_equal(np.isposinf(got), np.isposinf(ref)), (msg, name)
        assert np.array_equal(np.isneginf(got), np.isneginf(ref)), (msg, name)
        fin = np.isfinite(ref)
        dev[name] = float((np.abs(got[fin] - ref[fin]) / (1.0 + np.abs(ref[fin]))).max(initial=0.0))
    print(msg, "largest deviations over 1 + |value|", dev, "finite share", float(np.isfinite(stats[:2]).mean()),
          "-inf:", int(np.isneginf(stats).sum()))
    for k, name in enumerate(co.STATS):
        fin = np.isfinite(want["stats"][k])
        np.testing.assert_allclose(stats[k][fin], want["stats"][k][fin], rtol=1e-10, atol=1e-10, err_msg=f"{msg} {name}")
        fin = np.isfinite(want["rows"][1 + k])
        np.testing.assert_allclose(rows[1 + k][fin], want["rows"][1 + k][fin], rtol=1e-10, atol=1e-10, err_msg=f"{msg} row {name}")
    return want


def same_bytes(a, b, msg, keys=KEYS):
    for key in keys:
        assert a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), (msg, key)


def take_rows(res, sel):
    """the rows ``sel`` (a slice) of a result dict, contiguous"""
    return {key: np.ascontiguousarray(res[key][..., sel]) for key in KEYS}


def take_users(res, users):
    """the per-viewer outputs of the viewers ``users``"""
    return {key: np.ascontiguousarray(res[key][:, users]) for key in ("stats", "counts")}


def device_call(plan, U, T, window, stride, sigma, nss, wanted, d_mu=0, d_mv=0, d_ids=0):
    """the device entry into fresh buffers: (dict of numpy results for ``wanted``, status [2])"""
    import torch
    dev = torch.device("cuda", 0)
    R = (T - window) // stride + 1
    shapes = dict(stats=((3, U, R), torch.float64), counts=((3, U, R), torch.int64), rows=((4, R), torch.float64))
    bufs = {k: torch.full(shapes[k][0], -7, dtype=shapes[k][1], device=dev) for k in wanted}
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    plan.congruency_device(d_mu, d_mv, U, T, window, stride, sigma, nss, d_status=status.data_ptr(), d_ids=d_ids,
                           **{"d_" + k: b.data_ptr() for k, b in bufs.items()})
    torch.cuda.synchronize()
    return {k: b.cpu().numpy() for k, b in bufs.items()}, status.cpu().tolist()


# ------------------------------------------------------------------------------------------- 1. the numpy oracle
@pytest.mark.parametrize("sigma,window", SETTINGS)
def test_vs_oracle(plan, sigma, window):
    mu, mv, ids = g15()
    for n, stride in enumerate((1, window)):
        kw = dict(ids=ids) if n else dict(mu=mu, mv=mv)          # both entries
        res = plan.congruency(window=window, stride=stride, sigma_deg=sigma, **kw)
        check(res, ids, sigma, window, stride, f"sigma={sigma} window={window} stride={stride}")
        nan = int(np.isnan(res["stats"][0]).sum())
        # NaN only where the oracle has it: the 16 absent samples of G15 at window 1, none at windows of five frames and more
        assert nan == (16 if window == 1 else 0), nan
        assert (~np.isnan(res["stats"])).mean() >= 0.96            # a kernel that answers NaN everywhere cannot pass
        assert np.isfinite(res["stats"][0]).mean() >= 0.96 and np.isfinite(res["stats"][2]).mean() >= 0.96


# ------------------------------------------------------------------------------------------- 2. seams
def test_more_than_a_workgroup_of_queries(plan):
    """40 viewers x 12 frames, one row: 480 query slots, two workgroups of k_congruency_points"""
    mu, mv, ids = sphere(40, 12, 21)
    res = plan.congruency(mu=mu, mv=mv, window=12, sigma_deg=10.0)
    check(res, ids, 10.0, 12, 1, "40 x 12")
    assert (res["counts"][0] == 12).all() and res["rows"][0, 0] == 40.0


def test_pooled_list_beyond_an_lds_tile_and_a_block(engine, plan):
    """300 viewers x 8 frames, one row: about 2 250 distinct directions — three LDS tiles of the pooled list, three 1024-blocks of the
    rule behind Q, two blocks of viewers behind the row means; the tile switch puts matches on a tile's first and last entry"""
    mu, mv, ids = sphere(300, 8, 22)
    kw = dict(window=8, sigma_deg=10.0)
    res = plan.congruency(mu=mu, mv=mv, **kw)
    check(res, ids, 10.0, 8, 1, "300 x 8")
    assert res["counts"][1].sum() > 2048 and res["rows"][0, 0] == 300.0
    try:
        for tile in (3, 100, 0):
            engine.test_saliency_tile(tile)
            same_bytes(plan.congruency(ids=ids, **kw), res, f"tiles of {tile}")
    finally:
        engine.test_saliency_tile(0)


def test_pooled_long_rows_take_the_counting_path(plan):
    """600 viewers x 8 frames: 4 800 pooled positions, beyond the 4 096 of the LDS sort; the viewers' own lists stay sorted.  With the
    last frame empty, a row of 6 frames (3 600 positions: sorted) and the row of 8 hold the same lists: the same bytes"""
    mu, mv, ids = sphere(600, 8, 23)
    res = plan.congruency(mu=mu, mv=mv, window=8, sigma_deg=10.0, nss=False)
    check(res, ids, 10.0, 8, 1, "600 x 8", nss=False)
    gone = np.array(ids)
    gone[6:] = -1
    a = plan.congruency(ids=gone, window=6, stride=2, sigma_deg=10.0, nss=False)
    b = plan.congruency(ids=gone, window=8, sigma_deg=10.0, nss=False)
    same_bytes(take_rows(a, slice(0, 1)), b, "sorted against counted pooled lists")


def test_per_viewer_long_rows_take_the_counting_path(plan):
    """2 viewers x 4 200 frames, the whole video: both layouts beyond the LDS sort, about 3 800 distinct directions per viewer — own
    lists beyond a block of the rule"""
    mu, mv, ids = sphere(2, 4200, 24)
    res = plan.congruency(mu=mu, mv=mv, window=None, sigma_deg=10.0)
    check(res, ids, 10.0, None, 1, "2 x 4200")
    assert (res["counts"][1] > 3000).all()
    gone = np.array(ids)
    gone[4000:] = -1
    a = plan.congruency(ids=gone, window=4000, stride=200, sigma_deg=10.0)
    b = plan.congruency(ids=gone, window=4200, sigma_deg=10.0)
    same_bytes(take_rows(a, slice(0, 1)), b, "sorted against counted lists")


# ------------------------------------------------------------------------------------------- 3. edges
def test_edge_rows(plan):
    """frame 3: nobody; frame 4: viewer 0 alone; viewer 5 never present; frames 7 and 8: everyone on one pixel; viewers 1 and 2 are
    identical columns"""
    _, _, walk = g15()
    ids = np.array(walk[:20, :6])
    ids[3] = -1
    ids[4, 1:] = -1
    ids[:, 5] = -1
    ids[:, 2] = ids[:, 1]
    ids[7, :5] = ids[8, :5] = 77 * 101 + 31
    for window, stride in ((1, 1), (2, 1), (4, 3), (None, 1)):
        res = plan.congruency(ids=ids, window=window, stride=stride, sigma_deg=5.0)
        check(res, ids, 5.0, window, stride, f"edge rows window={window}")
        assert res["stats"][:, 1].tobytes() == res["stats"][:, 2].tobytes() and res["counts"][:, 1].tobytes() == res["counts"][:, 2].tobytes()
        assert np.isnan(res["stats"][:, 5]).all() and (res["counts"][:2, 5] == 0).all()
        if window == 1:
            assert np.isnan(res["stats"][:, :, 3]).all() and (res["counts"][:, :, 3] == 0).all() and res["rows"][0, 3] == 0.0
            assert np.isnan(res["rows"][1:, 3]).all()
            assert res["counts"][:, 0, 4].tolist() == [1, 1, 0] and np.isnan(res["stats"][:, 0, 4]).all() and res["rows"][0, 4] == 0.0
            assert res["counts"][2, 5, 4] == 1                    # the absent viewer's others are everyone
            kappa = 1.0 / rad(5.0) ** 2
            C = kappa / (2.0 * np.pi * (1.0 - np.exp(-2.0 * kappa)))
            np.testing.assert_allclose(res["stats"][0, :5, 7], 4.0 * np.pi * C, rtol=4.0 * kappa * 2.0 ** -53)
            assert res["counts"][:, :5, 7].tolist() == [[1] * 5, [1] * 5, [4] * 5]
    whole = plan.congruency(ids=ids, window=None, sigma_deg=5.0)
    same_bytes(whole, plan.congruency(ids=ids, window=20, sigma_deg=5.0), "window=None is window = T")


def test_far_pair_at_a_narrow_kernel(plan):
    """two viewers 90 degrees apart at sigma 1 degree: the other's density underflows at the viewer's sample"""
    ids = np.array([[100 * 101 + 50, 100 * 101 + 25]], dtype=np.int32)            # the equator, a quarter of the width apart
    res = plan.congruency(ids=ids, window=1, sigma_deg=1.0)
    check(res, ids, 1.0, 1, 1, "far pair")
    assert (res["stats"][0] == 0.0).all() and np.isneginf(res["stats"][1]).all()
    assert np.isfinite(res["stats"][2]).all() and (res["stats"][2] < 0).all()
    assert res["rows"][:, 0].tolist()[:2] == [2.0, 0.0] and np.isneginf(res["rows"][2, 0]) and res["rows"][3, 0] < 0


# ------------------------------------------------------------------------------------------- 4. bit invariance
def test_bits_do_not_depend_on_stride_length_entry_or_outputs(plan):
    import torch
    mu_long, mv_long, ids_long = g15()
    T, U = 25, 8
    mu, mv, ids = mu_long[:T], mv_long[:T], ids_long[:T]
    kw = dict(window=5, sigma_deg=5.0)
    s1 = plan.congruency(mu=mu, mv=mv, stride=1, **kw)
    s5 = plan.congruency(mu=mu, mv=mv, stride=5, **kw)
    same_bytes(take_rows(s1, slice(0, None, 5)), s5, "stride 1 against stride 5")
    long = plan.congruency(mu=mu_long, mv=mv_long, stride=1, **kw)                  # the rows wholly inside the prefix
    same_bytes(take_rows(long, slice(0, T - 5 + 1)), s1, "a prefix of the video")
    few = plan.congruency(mu=mu[3:9], mv=mv[3:9], stride=1, **kw)                   # two rows of the same frames
    same_bytes(few, take_rows(s1, slice(3, 5)), "the number of rows")
    same_bytes(plan.congruency(ids=ids, stride=1, **kw), s1, "ids against (mu, mv)")
    off = plan.congruency(ids=ids, stride=1, nss=False, **kw)
    assert np.isnan(off["stats"][2]).all() and np.isnan(off["rows"][3]).all()
    assert off["stats"][:2].tobytes() == s1["stats"][:2].tobytes() and off["rows"][:3].tobytes() == s1["rows"][:3].tobytes()
    assert off["counts"].tobytes() == s1["counts"].tobytes()
    # the device entries, every output and one output at a time (a NULL output is not written)
    dev = torch.device("cuda", 0)
    d_mu, d_mv, d_ids = (torch.from_numpy(np.array(a)).to(dev) for a in (mu, mv, ids))
    for src in ("mu_mv", "ids"):
        samples = dict(d_ids=d_ids.data_ptr()) if src == "ids" else dict(d_mu=d_mu.data_ptr(), d_mv=d_mv.data_ptr())
        for wanted in (KEYS, ("stats",), ("counts",), ("rows",), ("stats", "counts"), ()):
            got, status = device_call(plan, U, T, 5, 1, 5.0, True, wanted, **samples)
            for k, b in got.items():
                assert b.tobytes() == s1[k].tobytes(), (src, wanted, k)
            assert status == [0, 0], (src, wanted)
    got, status = device_call(plan, U, T, 5, 1, 5.0, False, KEYS, d_ids=d_ids.data_ptr())
    same_bytes(got, off, "the device entry without nss")


def test_a_viewers_bits_do_not_depend_on_the_other_columns_order(plan):
    _, _, ids_long = g15()
    ids = ids_long[:25]
    kw = dict(window=5, sigma_deg=5.0)
    s1 = plan.congruency(ids=ids, **kw)
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])                   # viewer perm[k] moves to column k
    p = plan.congruency(ids=np.ascontiguousarray(ids[:, perm]), **kw)
    for key in ("stats", "counts"):
        assert p[key].tobytes() == np.ascontiguousarray(s1[key][:, perm]).tobytes(), key
    assert p["rows"][0].tobytes() == s1["rows"][0].tobytes()
    np.testing.assert_allclose(p["rows"], s1["rows"], rtol=1e-13)            # the row means run over the viewer index
    # an all-absent column more: nobody's values move, the newcomer is NaN with everyone as its others
    more = np.concatenate([ids, np.full((25, 1), -1, dtype=np.int32)], axis=1)
    m = plan.congruency(ids=more, **kw)
    same_bytes(take_users(m, slice(0, 8)), take_users(s1, slice(0, 8)), "an absent column more", keys=("stats", "counts"))
    assert m["rows"].tobytes() == s1["rows"].tobytes()
    assert np.isnan(m["stats"][:, 8]).all() and (m["counts"][:2, 8] == 0).all()
    assert np.array_equal(m["counts"][2, 8], s1["counts"][0].sum(axis=0))


def test_passes_do_not_change_a_bit(plan):
    """100 viewers x 8 100 frames at window 6: a row of a pass takes 33 616 B (the pooled list of 600 slots, its T, 100 own lists of
    6 slots with their lengths and counts, 24 B a query slot, four sums a viewer), so a pass holds 7 985 rows under the 256 MB budget
    and the 8 095 rows take two (0-7984, 7985-8094).  The rows on both sides of the seam keep the bytes they have in a call of their
    own."""
    mu, mv, ids = sphere(100, 8100, 25)
    res = plan.congruency(ids=ids, window=6, sigma_deg=10.0)
    assert res["rows"].shape == (4, 8095) and (res["rows"][0] == 100.0).all() and not np.isnan(res["stats"]).any()
    for r0 in (0, 7980, 8084):
        one = plan.congruency(ids=ids[r0:r0 + 16], window=6, sigma_deg=10.0)
        same_bytes(take_rows(res, slice(r0, r0 + 11)), one, f"rows from {r0}")
    check(dict(take_rows(res, slice(7984, 7986)), code=0), ids[7984:7991], 10.0, 6, 1, "the rows on either side of the seam")


# ------------------------------------------------------------------------------------------- 5. refusals and the analyzers
def test_illegal_arguments_are_refused_before_anything_runs(native, plan):
    mu, mv, _ = g15()
    mu, mv = np.ascontiguousarray(mu[:30, :4]), np.ascontiguousarray(mv[:30, :4])
    lib = native.load_library()
    stats = np.empty((3, 4, 64))
    good = dict(U=4, window=5, stride=1, sigma=0.1)
    for change in (dict(U=1), dict(window=0), dict(window=31), dict(stride=0), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")),
                   dict(sigma=float("inf")), dict(sigma=3.2)):
        a = dict(good, **change)
        rc = lib.vet_congruency_host(plan.handle, native._ptr(mu), native._ptr(mv), None, a["U"], 30, a["window"], a["stride"],
                                     a["sigma"], 1, native._ptr(stats), None, None)
        assert rc == native.VET_ERR_INVALID, change
    with pytest.raises(native.NativeError) as err:                # the device entry refuses before it looks at a pointer
        plan.congruency_device(8, 8, 4, 30, 31, 1, d_stats=8)
    assert err.value.code == native.VET_ERR_INVALID
    with pytest.raises(native.NativeError) as err:
        plan.congruency_device(8, 8, 1, 30, 5, 1, d_stats=8)
    assert err.value.code == native.VET_ERR_INVALID
    for kw in (dict(window=31), dict(sigma_deg=0.0), dict(sigma_deg=181.0)):
        with pytest.raises(ValueError):
            plan.congruency(**dict(dict(mu=mu, mv=mv), **kw))
    with pytest.raises(native.NativeError):
        plan.congruency(mu=mu[:, :1], mv=mv[:, :1], window=5)
    assert plan.congruency(mu=mu, mv=mv)["stats"].shape == (3, 4, 1)               # window=None: the whole video
    bad = mu.copy()
    bad[7, 2] = 1.5
    with pytest.raises(native.NativeError) as err:
        plan.congruency(mu=bad, mv=mv, window=5)
    assert err.value.code == native.VET_ERR_RANGE
    gone_mu, gone_mv = mu.copy(), mv.copy()
    gone_mu[7, 2] = gone_mv[7, 2] = np.nan
    res = plan.congruency(mu=bad, mv=mv, window=5, check=False)
    assert res["code"] == native.VET_ERR_RANGE                    # the outputs are still written: the sample counts as absent
    same_bytes(res, plan.congruency(mu=gone_mu, mv=gone_mv, window=5), "a sample out of range")


def test_analyzers_return_the_oracle_columns():
    from viewport_entropy_toolkit import SpatialEntropyAnalyzer, TransitionEntropyAnalyzer
    from viewport_entropy_toolkit.analyzers import NaiveSpatialEntropyAnalyzer
    from viewport_entropy_toolkit.config import AnalyzerConfig, NaiveAnalyzerConfig
    mu, mv, ids = g15()
    times = np.arange(60) / 30.0
    frames = []
    for cls in (SpatialEntropyAnalyzer, NaiveSpatialEntropyAnalyzer, TransitionEntropyAnalyzer):
        an = cls(NaiveAnalyzerConfig(tile_height=10, tile_width=20, video_width=W, video_height=H)) \
            if cls is NaiveSpatialEntropyAnalyzer else cls(AnalyzerConfig(tile_counts=[20], video_width=W, video_height=H))
        an.load_arrays(times, mu.copy(), mv.copy())
        frames.append(an.compute_congruency(window=5, stride=5, sigma_deg=5.0))
        plain = an.compute_congruency(window=5, stride=5, nss=False)
        assert np.isnan(plain["nss"]).all() and plain["lift"].to_numpy().tobytes() == frames[-1]["lift"].to_numpy().tobytes()
        whole = an.compute_congruency()
        assert len(whole) == 8 and whole["time_end"][0] == times[-1] and whole.attrs["window"] == 60 and len(whole.attrs["rows"]) == 1
    df = frames[0]
    cols = ["user", "time", "time_end", "samples", "distinct", "others"] + list(co.STATS)
    row_cols = ["time", "time_end", "scored"] + list(co.STATS)
    assert list(df.columns) == cols and list(df.attrs["rows"].columns) == row_cols and len(df) == 8 * 12
    for other in frames[1:]:                                     # the call is lattice-independent: three analyzers, the same values
        for c in cols[1:]:
            assert df[c].to_numpy().tobytes() == other[c].to_numpy().tobytes(), c
        for c in row_cols:
            assert df.attrs["rows"][c].to_numpy().tobytes() == other.attrs["rows"][c].to_numpy().tobytes(), c
    per_row = df.attrs["rows"]
    res = dict(code=0, stats=np.stack([df[c].to_numpy().reshape(8, 12) for c in co.STATS]),
               counts=np.stack([df[c].to_numpy().reshape(8, 12) for c in ("samples", "distinct", "others")]).astype(np.int64),
               rows=np.stack([per_row[c].to_numpy().astype(np.float64) for c in ("scored",) + co.STATS]))
    check(res, ids, 5.0, 5, 5, "the analyzers' DataFrame")
    assert df["user"].tolist() == [u for u in df.attrs["users"] for _ in range(12)] and len(df.attrs["users"]) == 8
    assert df.attrs["sigma_deg"] == 5.0 and df.attrs["kappa"] == 1.0 / rad(5.0) ** 2
    assert df.attrs["window"] == 5 and df.attrs["stride"] == 5
    assert df["time"].tolist() == times[0::5].tolist() * 8 and df["time_end"].tolist() == times[4::5].tolist() * 8
    assert per_row["time"].tolist() == times[0::5].tolist() and per_row["scored"].tolist() == [8] * 12
