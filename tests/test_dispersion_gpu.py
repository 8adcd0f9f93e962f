"""GPU: audience dispersion through the C-ABI (Plan.dispersion -> vet_dispersion_host, the device entries through
Plan.dispersion_device, the analyzers' compute_dispersion).  A pair sample is two viewers present in one frame, its angle the
reference's vector_angle_distance of their Vectors, +0.0 where the two Vectors are the same.  The references are golden G26 (the real
reference's angles, tools/gen_golden_dispersion.py) and the numpy oracle of tests/_dispersion_oracle.py (pinned against G26 in
tests/test_dispersion_surface.py) — never the code under test.

``counts`` and ``hist`` are compared for equality on every row; for ``hist`` the test asserts on the ORACLE's angles that none lies
within 1e-9 relative of an edge, so a last-bit difference of an angle cannot move a count.

Tolerance of ``stats``, derived, not measured: tests/_tol.py's W_RTOL = 1e-9 relative plus 4e-16 absolute (the ulp of arccos), NaN
equal to NaN.  The oracle evaluates the definition's fused dot with one rounding per fma (exact integer arithmetic), so the angles
differ by the two arccos implementations only: an ulp or two of the angle.  The sums add non-negative terms with chains far below
1e6 roundings (1e-10 relative); the minimum and the maximum are 1-Lipschitz in the values.  ``centroid`` sums signed terms: its
absolute bound is 1.2e-16 * present^2, the worst case of any order of `present` unit components.  The tests print the largest
error they saw."""
import functools
import warnings

import numpy as np
import pytest

from tests import _dispersion_oracle as do
from tests._tol import W_RTOL

pytestmark = pytest.mark.gpu

W, H = 100, 200
ATOL = 4e-16
EDGES = np.radians([0.0, 1.0, 5.0, 15.0, 30.0, 60.0, 90.0, 120.0, 180.0])
WIDE = np.radians([0.0, 0.5, 1.0, 2.0, 5.0, 10.0, 15.0, 30.0, 45.0, 60.0, 90.0, 120.0, 180.0])     # 12 bins: beyond the 8 kept in registers
MOST = np.linspace(0.0, np.pi, 65)                               # 64 bins: the most the call takes, its largest LDS footprint
KEYS = ("stats", "centroid", "hist", "counts")
WALKS = {"walk70": (70, 40, 11, 0.2), "walk257": (257, 6, 12, 0.1), "walk8": (8, 60, 13, 0.3), "sphere40": (40, 12, 23, None)}


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


@functools.lru_cache(maxsize=None)
def grid():
    return do.grid_table(W, H)


@pytest.fixture(scope="module")
def table(plan):
    """the plan's own direction table: the Vectors the oracle works on"""
    assert np.array_equal(plan.read_dirs(), grid())
    return grid()


@functools.lru_cache(maxsize=None)
def video(name):
    """(mu, mv, ids, angles) of a named input: computed once, shared, never written to"""
    from viewport_entropy_toolkit import _synthetic
    U, T, seed, p_absent = WALKS[name]
    if p_absent is None:
        mu, mv = _synthetic.uniform_sphere_video(U, T, base_seed=seed)
    else:
        mu, mv = _synthetic.random_walk_video(U, T, base_seed=seed, p_absent=p_absent)
    ids = do.ids_of(mu, mv, W, H)
    ang, same = do.frame_angles(grid(), ids)
    for a in (mu, mv, ids, ang, same):
        a.setflags(write=False)
    return mu, mv, ids, ang, same


def walk_ids(U, T, seed, p_absent=0.2):
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(U, T, base_seed=seed, p_absent=p_absent)
    return mu, mv, do.ids_of(mu, mv, W, H)


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


def close_centroid(got, want, present, msg):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and not np.isnan(got).any(), msg
    err = np.abs(got - want).max(axis=-1)
    print(msg, "max abs err", float(err.max(initial=0.0)), "of present up to", int(np.max(present, initial=0)))
    assert (err <= 1.2e-16 * np.asarray(present, dtype=np.float64) ** 2).all(), msg
    zero = got[np.asarray(present) == 0]
    assert (zero == 0.0).all() and not np.signbit(zero).any(), msg


def kept(R):
    return np.unique([0, R // 2, max(R - 2, 0), R - 1])


def check(res, ang, ids, table, window, stride, per_user, msg, edges=EDGES):
    """a result dict against the oracle: the integers of every row, the FP outputs of the kept rows (and viewers)"""
    T, U = ids.shape
    w = T if window is None else window
    R = (T - w) // stride + 1
    lead = (U, R) if per_user else (R,)
    assert res["code"] == 0 and res["stats"].shape == (3,) + lead and res["counts"].shape == (4,) + lead, msg
    assert res["centroid"].shape == lead + (3,) and res["counts"].dtype == np.int64, msg
    counts = do.counts(ang, ids, w, stride, per_user)
    assert np.array_equal(res["counts"], counts), msg
    empty = counts[0] == 0
    assert np.isnan(res["stats"][:, empty]).all() and not np.isnan(res["stats"][:, ~empty]).any(), msg
    assert (counts[2][empty] == 0).all() and (counts[1] <= counts[0]).all(), msg
    rows, users = kept(R), (np.unique([0, 1, U // 2, U - 2, U - 1]) if U > 8 else np.arange(U))
    if per_user:
        want = do.rows(ang, ids, table, w, stride, True, only=rows, users=users)
        close(res["stats"][:, users][:, :, rows], want["stats"], msg + " stats")
        close_centroid(res["centroid"][users][:, rows], want["centroid"], counts[3][users][:, rows], msg + " centroid")
        assert res["hist"] is None, msg
    else:
        want = do.rows(ang, ids, table, w, stride, False, edges=edges)          # every row: the histogram is an integer
        close(res["stats"][:, rows], want["stats"][:, rows], msg + " stats")
        close_centroid(res["centroid"], want["centroid"], counts[3], msg + " centroid")
        assert np.array_equal(want["counts"], counts), msg
        if edges is not None:
            assert res["hist"].dtype == np.int64 and np.array_equal(res["hist"], want["hist"]), msg
            assert (res["hist"].sum(axis=-1) <= counts[0]).all() and (res["hist"][..., 0] >= counts[1]).all(), msg
    return counts


def same_bytes(a, b, msg, keys=KEYS):
    for key in keys:
        if a[key] is None or b[key] is None:
            continue
        assert a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), (msg, key)


def take_rows(res, sel, per_user):
    """the rows ``sel`` (a slice) of a result dict, contiguous"""
    out = {}
    for key in KEYS:
        a = res[key]
        if a is None:
            out[key] = None
        elif key in ("stats", "counts"):
            out[key] = np.ascontiguousarray(a[..., sel])
        else:
            out[key] = np.ascontiguousarray(a[:, sel] if per_user else a[sel])
    return out


# ------------------------------------------------------------------------------------------- the reference's angles (golden G26)
def test_vs_golden_angles(plan, golden_dir):
    g = np.load(golden_dir / "g26_dispersion.npz")
    g15 = np.load(golden_dir / "g15_windowed_transition.npz")
    mu, mv = g15["mu"], g15["mv"]
    ids = do.ids_of(mu, mv, W, H)
    want = np.where(g["same"], 0.0, g["angles"])                  # the stated departure: the same Vector is +0.0
    has = ~np.isnan(want).all(axis=-1)                            # [60][8]: a partner in the frame
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # all-NaN slices: no partner
        w_mean, w_max, w_min = np.nanmean(want, axis=-1).T, np.nanmax(want, axis=-1).T, np.nanmin(want, axis=-1).T
    upper = np.triu(np.ones((8, 8), dtype=bool), 1)
    for kw in (dict(mu=mu, mv=mv), dict(ids=ids)):
        per = plan.dispersion(window=1, per_user=True, **kw)      # row (u, f): viewer u's partners in frame f
        assert per["stats"].shape == (3, 8, 60) and np.array_equal(per["counts"][2], has.T.astype(np.int64))
        close(per["stats"][0], w_mean, "G26 per viewer mean")
        close(per["stats"][1], w_max, "G26 per viewer max")
        close(per["stats"][2], w_min, "G26 per viewer nearest")
        assert np.array_equal(per["counts"][0], (~np.isnan(want)).sum(axis=-1).T)
        assert np.array_equal(per["counts"][1], g["same"].sum(axis=-1).T)
        pooled = plan.dispersion(window=1, **kw)
        tri = want[:, upper]                                      # [60][28]
        n = (~np.isnan(tri)).sum(axis=-1)
        assert np.array_equal(pooled["counts"][0], n) and np.array_equal(pooled["counts"][1], g["same"][:, upper].sum(axis=-1))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            close(pooled["stats"][0], np.nanmean(tri, axis=-1), "G26 pooled mean")
            close(pooled["stats"][1], np.nanmax(tri, axis=-1), "G26 pooled max")
    for a, b in ((0, 1), (2, 5), (3, 7), (6, 4)):                 # two viewers selected: `mean` is the reference's angle
        two = plan.dispersion(mu=mu[:, [a, b]], mv=mv[:, [a, b]], window=1)
        close(two["stats"][0], want[:, a, b], f"G26 viewers {a}, {b}")
        assert two["stats"][1].tobytes() == two["stats"][0].tobytes() == two["stats"][2].tobytes()      # one pair: mean = max = nearest
        assert np.array_equal(two["counts"][1], g["same"][:, a, b].astype(np.int64))


# ------------------------------------------------------------------------------------------- the numpy oracle
@pytest.mark.parametrize("name", sorted(WALKS))
def test_vs_oracle(plan, table, name):
    mu, mv, ids, ang, same = video(name)
    T, U = ids.shape
    assert clear_of_edges(ang) and clear_of_edges(ang, WIDE)
    if name == "sphere40":
        assert do.rows(ang, ids, table, None, 1, edges=EDGES)["hist"][0, -1] > 0        # the bins above 120 degrees fill
    else:
        assert same.any()                                        # same-Vector pairs
    n = 0
    for window, stride in ((1, 1), (20, 7), (None, 1)):
        if window is not None and window > T:
            continue
        for per_user in (False, True):
            msg = f"{name} window={window} stride={stride} per_user={per_user}"
            kw = dict(ids=ids) if n % 2 else dict(mu=mu, mv=mv)   # both entries
            n += 1
            res = plan.dispersion(window=window, stride=stride, per_user=per_user, edges=None if per_user else EDGES, **kw)
            counts = check(res, ang, ids, table, window, stride, per_user, msg)
            if not per_user:                                     # 12 bins take the kernel's other histogram path
                wide = plan.dispersion(window=window, stride=stride, edges=WIDE, **kw)
                check(wide, ang, ids, table, window, stride, False, msg + " 12 bins", edges=WIDE)
                same_bytes(wide, res, msg + " 12 bins", keys=("stats", "centroid", "counts"))
            if not per_user and window is None and name != "sphere40":
                assert counts[0][0] == (~np.isnan(ang)).sum() // 2 and counts[1][0] == same.sum() // 2


@pytest.mark.parametrize("name", ["walk70", "walk257"])
def test_sixty_four_bins(engine, plan, table, name):
    """B = 64: 64 KB of histogram columns beside the 32 KB tile of viewers; against the oracle, and in tiles of 32 viewers"""
    mu, mv, ids, ang, _ = video(name)
    assert clear_of_edges(ang, MOST)
    eight = plan.dispersion(ids=ids, window=None, edges=EDGES)
    for window, stride in ((1, 1), (None, 1)):
        res = plan.dispersion(mu=mu, mv=mv, window=window, stride=stride, edges=MOST)
        check(res, ang, ids, table, window, stride, False, f"{name} 64 bins window={window}", edges=MOST)
        assert res["hist"].shape[-1] == 64
    same_bytes(res, eight, f"{name} 64 bins against 8", keys=("stats", "centroid", "counts"))
    engine.test_dispersion_tile(32)
    try:
        same_bytes(plan.dispersion(ids=ids, window=None, edges=MOST), res, f"{name} 64 bins, tiles of 32")
    finally:
        engine.test_dispersion_tile(0)


@pytest.mark.parametrize("U", [1, 2, 3, 63, 64, 65])
def test_small_audiences(plan, table, U):
    mu, mv, ids = walk_ids(U, 9, 300 + U, p_absent=0.25)
    ang, _ = do.frame_angles(table, ids)
    assert clear_of_edges(ang)
    for window, stride in ((1, 1), (4, 2), (None, 1)):
        for per_user in (False, True):
            res = plan.dispersion(ids=ids, window=window, stride=stride, per_user=per_user, edges=None if per_user else EDGES)
            counts = check(res, ang, ids, table, window, stride, per_user, f"U={U} window={window} per_user={per_user}")
            if U == 1:                                           # legal: every row has N = 0
                assert (counts[:3] == 0).all() and np.isnan(res["stats"]).all()
    one = plan.dispersion(mu=mu[:1], mv=mv[:1], window=1, edges=EDGES)           # T = 1
    check(one, ang[:1], ids[:1], table, 1, 1, False, f"U={U} T=1")
    check(plan.dispersion(ids=ids[:1], window=None, per_user=True), ang[:1], ids[:1], table, None, 1, True, f"U={U} T=1 per viewer")


def empty_video():
    """ids [30][5]: frames 4-9 with nobody, frames 10-15 with viewer 2 alone, frame 16 with two, then a walk of four; viewer 4 never"""
    _, _, walk = walk_ids(4, 30, 91, p_absent=0.0)
    ids = np.full((30, 5), -1, dtype=np.int32)
    ids[:4, :4] = walk[:4]
    ids[10:16, 2] = walk[10:16, 2]
    ids[16, [1, 3]] = walk[16, [1, 3]]
    ids[17:, :4] = walk[17:]
    return ids


def test_frames_with_nobody_and_with_one_viewer(plan, table):
    import torch
    ids = empty_video()
    ang, _ = do.frame_angles(table, ids)
    assert clear_of_edges(ang)
    for window, stride in ((1, 1), (3, 1), (6, 2), (None, 1)):
        pooled = plan.dispersion(ids=ids, window=window, stride=stride, edges=EDGES)
        counts = check(pooled, ang, ids, table, window, stride, False, f"empty frames window={window}")
        per = plan.dispersion(ids=ids, window=window, stride=stride, per_user=True)
        check(per, ang, ids, table, window, stride, True, f"empty frames per viewer window={window}")
        if window == 3:
            assert (counts[:, 4:8] == 0).all()                    # rows 4-7: nobody at all; +0.0 centroid
            assert (counts[0, 10:14] == 0).all() and (counts[3, 10:14] == 3).all()          # one viewer: present, never a pair
            assert not np.isnan(pooled["centroid"]).any() and (np.abs(pooled["centroid"][10:14]).sum(axis=-1) > 0).all()
            assert np.isnan(pooled["stats"][:, 4:14]).all() and (pooled["hist"][4:14] == 0).all()
            assert counts[0, 14] == 1 and counts[2, 14] == 2      # frames 14-16: the one pair of frame 16
        assert (per["counts"][:, 4] == 0).all() and np.isnan(per["stats"][:, 4]).all() and (per["centroid"][4] == 0.0).all()
    # status[1]: the rows with N = 0, through the device entry
    dev = torch.device("cuda", 0)
    d_ids = torch.from_numpy(ids).to(dev)
    for per_user in (False, True):
        host = plan.dispersion(ids=ids, window=3, per_user=per_user)
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        counts = torch.zeros(host["counts"].shape, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        plan.dispersion_device(0, 0, 5, 30, 3, 1, per_user, None, d_counts=counts.data_ptr(), d_status=status.data_ptr(),
                               d_ids=d_ids.data_ptr())
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [0, int((host["counts"][0] == 0).sum())] and status[1].item() > 0
        assert counts.cpu().numpy().tobytes() == host["counts"].tobytes()


# ------------------------------------------------------------------------------------------- bit invariance
@pytest.mark.parametrize("name,tiles", [("walk70", (32, 1, 69)), ("walk257", (32, 100, 256))])
def test_lds_tile_does_not_change_a_bit(engine, plan, name, tiles):
    """vet_test_dispersion_tile: U = 70 (257) viewers in tiles of 32 run 3 (9) tiles; the default stages the frame at once"""
    mu, mv, ids, ang, _ = video(name)
    T = ids.shape[0]
    shapes = [(1, 1, False), (min(20, T), 7, False), (None, 1, False), (None, 1, True), (1, 1, True)]
    default = [plan.dispersion(mu=mu, mv=mv, window=w, stride=s, per_user=pu, edges=None if pu else EDGES) for w, s, pu in shapes]
    wide = plan.dispersion(ids=ids, window=None, edges=WIDE)
    try:
        for n in tiles:
            engine.test_dispersion_tile(n)
            for (w, s, pu), ref in zip(shapes, default):
                kw = dict(ids=ids) if n == 32 else dict(mu=mu, mv=mv)
                res = plan.dispersion(window=w, stride=s, per_user=pu, edges=None if pu else EDGES, **kw)
                same_bytes(res, ref, f"{name} tile {n}: window={w} stride={s} per_user={pu}")
            same_bytes(plan.dispersion(ids=ids, window=None, edges=WIDE), wide, f"{name} tile {n}: 12 bins")
    finally:
        engine.test_dispersion_tile(0)


def test_bits_do_not_depend_on_stride_length_entry_or_outputs(plan):
    import torch
    mu_long, mv_long, ids_long, _, _ = video("walk70")
    T = 25
    mu, mv, ids = mu_long[:T], mv_long[:T], ids_long[:T]
    other = np.radians([0.0, 2.0, 45.0, 170.0])
    dev = torch.device("cuda", 0)
    for per_user in (False, True):
        e = None if per_user else EDGES
        kw = dict(window=5, per_user=per_user, edges=e)
        s1 = plan.dispersion(mu=mu, mv=mv, stride=1, **kw)
        s3 = plan.dispersion(mu=mu, mv=mv, stride=3, **kw)
        same_bytes(take_rows(s1, slice(0, None, 3), per_user), s3, f"stride 1 against stride 3, per_user={per_user}")
        long = plan.dispersion(mu=mu_long, mv=mv_long, stride=1, **kw)          # the rows wholly inside the truncated video
        same_bytes(take_rows(long, slice(0, T - 5 + 1), per_user), s1, f"a truncated video, per_user={per_user}")
        few = plan.dispersion(mu=mu[3:9], mv=mv[3:9], stride=1, **kw)           # two rows of the same frames
        same_bytes(few, take_rows(s1, slice(3, 5), per_user), f"the number of rows, per_user={per_user}")
        whole = plan.dispersion(mu=mu, mv=mv, window=None, per_user=per_user, edges=e)
        same_bytes(whole, plan.dispersion(mu=mu, mv=mv, window=T, stride=4, per_user=per_user, edges=e), "window=None is window = T")
        same_bytes(plan.dispersion(ids=ids, stride=1, **kw), s1, f"ids against (mu, mv), per_user={per_user}")
        if not per_user:                                         # other edges, no edges: the other outputs keep their bytes
            for edges in (other, None):
                res = plan.dispersion(mu=mu, mv=mv, window=5, stride=1, edges=edges)
                same_bytes(res, s1, "other edges", keys=("stats", "centroid", "counts"))
            assert plan.dispersion(mu=mu, mv=mv, window=5, edges=None)["hist"] is None
        # the device entries, every output and one output at a time
        U, rows = 70, s1["counts"][0].size
        d_mu, d_mv, d_ids = (torch.from_numpy(np.array(a)).to(dev) for a in (mu, mv, ids))          # writable copies
        shapes = dict(stats=((3, rows), torch.float64), centroid=((rows, 3), torch.float64),
                      hist=((rows, len(EDGES) - 1), torch.int64), counts=((4, rows), torch.int64))
        for src in ("mu_mv", "ids"):
            extra = dict(d_ids=d_ids.data_ptr()) if src == "ids" else {}
            for wanted in (KEYS, ("stats",), ("centroid",), ("hist",), ("counts",), ()):
                wanted = [k for k in wanted if not (per_user and k == "hist")]
                bufs = {k: torch.full(shapes[k][0], -7, dtype=shapes[k][1], device=dev) for k in wanted}
                status = torch.zeros(2, dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                plan.dispersion_device(d_mu.data_ptr(), d_mv.data_ptr(), U, T, 5, 1, per_user, e if "hist" in wanted else None,
                                       d_status=status.data_ptr(), **{"d_" + k: b.data_ptr() for k, b in bufs.items()}, **extra)
                torch.cuda.synchronize()
                for k, b in bufs.items():
                    assert b.cpu().numpy().tobytes() == s1[k].tobytes(), (per_user, src, wanted, k)
                assert status.cpu().tolist() == [0, int((s1["counts"][0] == 0).sum())]


# ------------------------------------------------------------------------------------------- consistency, permutation, closed forms
@pytest.mark.parametrize("name", ["walk70", "walk257", "walk8"])
def test_pooled_and_per_viewer_rows_agree(plan, name):
    mu, mv, ids, _, _ = video(name)
    T = ids.shape[0]
    for window, stride in ((1, 1), (min(20, T), 7), (None, 1)):
        pooled = plan.dispersion(ids=ids, window=window, stride=stride, edges=EDGES)
        per = plan.dispersion(ids=ids, window=window, stride=stride, per_user=True)
        assert np.array_equal(per["counts"][:2].sum(axis=1), 2 * pooled["counts"][:2])           # samples, same: exact
        assert np.array_equal(per["counts"][2:].sum(axis=1), pooled["counts"][2:])               # slots, present
        with np.errstate(invalid="ignore"):
            top = np.fmax.reduce(per["stats"][1], axis=0)        # NaN where no viewer has a partner
        assert top.tobytes() == pooled["stats"][1].tobytes()     # the maximum of the per-viewer maxima, bit for bit
        assert (pooled["hist"].sum(axis=-1) == pooled["counts"][0]).all()      # the edges span [0, pi]: every pair in a bin
        assert (pooled["hist"][:, 0] >= pooled["counts"][1]).all()


def test_permuting_the_viewers(plan):
    mu, mv, ids, _, _ = video("walk70")
    perm = np.random.default_rng(3).permutation(70)
    for window, stride in ((1, 1), (20, 7)):
        a = plan.dispersion(ids=ids, window=window, stride=stride, edges=EDGES)
        b = plan.dispersion(ids=np.ascontiguousarray(ids[:, perm]), window=window, stride=stride, edges=EDGES)
        assert np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["hist"], b["hist"])
        assert a["stats"][1].tobytes() == b["stats"][1].tobytes()           # the maximum is order-free
        close(b["stats"], a["stats"], "permuted viewers, pooled stats")
        pa = plan.dispersion(ids=ids, window=window, stride=stride, per_user=True)
        pb = plan.dispersion(ids=np.ascontiguousarray(ids[:, perm]), window=window, stride=stride, per_user=True)
        assert np.array_equal(pa["counts"][:, perm], pb["counts"])
        assert pa["stats"][1][perm].tobytes() == pb["stats"][1].tobytes() and pa["stats"][2][perm].tobytes() == pb["stats"][2].tobytes()
        assert pa["centroid"][perm].tobytes() == pb["centroid"].tobytes()   # a viewer's own vectors in frame order
        close(pb["stats"][0], pa["stats"][0][perm], "permuted viewers, per-viewer mean")


def test_closed_forms(plan):
    T, U = 7, 130
    ids = np.full((T, U), 77 * (W + 1) + 31, dtype=np.int32)      # every viewer on one pixel
    ids[2, 5:9] = -1
    for per_user in (False, True):
        res = plan.dispersion(ids=ids, window=3, stride=2, per_user=per_user, edges=None if per_user else EDGES)
        assert (res["counts"][1] == res["counts"][0]).all() and (res["counts"][0] > 0).all()      # same = N
        for k in (0, 1, 2):
            assert (res["stats"][k] == 0.0).all() and not np.signbit(res["stats"][k]).any()        # +0.0 exactly
        length = np.sqrt((res["centroid"] ** 2).sum(axis=-1)) / res["counts"][3]
        assert (np.abs(length - 1.0) <= 1e-15).all()
        if not per_user:
            present = np.array([(ids[r * 2:r * 2 + 3] >= 0).sum(axis=1) for r in range(3)])
            assert np.array_equal(res["counts"][0], (present * (present - 1) // 2).sum(axis=1))
            assert np.array_equal(res["hist"][:, 0], res["counts"][0]) and (res["hist"][:, 1:] == 0).all()
    pole = np.array([[3, 90], [0, 100], [17, 17]], dtype=np.int32)            # py = 0: every pixel of the row is the pole
    res = plan.dispersion(ids=pole, window=1)
    assert res["counts"][0].tolist() == [1, 1, 1] and res["counts"][1].tolist() == [1, 1, 1]       # different ids, one Vector
    assert (res["stats"] == 0.0).all() and not np.signbit(res["stats"]).any()
    off = plan.dispersion(ids=np.array([[3, (W + 1) + 90]], dtype=np.int32), window=1)             # the next row: not the pole
    assert off["counts"][1].tolist() == [0] and off["stats"][0, 0] > 0


# ------------------------------------------------------------------------------------------- refusals, range, the analyzers
def test_illegal_arguments_are_refused_before_anything_runs(native, plan):
    mu, mv, _ = walk_ids(4, 30, 33, p_absent=0.0)
    lib = native.load_library()
    stats = np.empty((3, 64))
    e = np.array([0.0, 0.1, 0.2])
    good = dict(window=5, stride=1, per_user=0, B=2, e=e)
    bad = [dict(window=0), dict(window=31), dict(stride=0), dict(B=65), dict(B=-1), dict(e=np.array([0.0, 0.2, 0.1])),
           dict(e=np.array([0.0, 0.1, 0.1])), dict(e=np.array([0.0, np.inf, 0.2])), dict(e=np.array([0.0, np.nan, 0.2])),
           dict(per_user=1)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.vet_dispersion_host(plan.handle, native._ptr(mu), native._ptr(mv), None, 4, 30, a["window"], a["stride"], a["per_user"],
                                     native._ptr(a["e"]), a["B"], native._ptr(stats), None, None, None)
        assert rc == native.VET_ERR_INVALID, change
    with pytest.raises(native.NativeError) as err:                # the device entry refuses before it looks at a pointer
        plan.dispersion_device(8, 8, 4, 30, 31, 1, False, None, 8)
    assert err.value.code == native.VET_ERR_INVALID
    with pytest.raises(native.NativeError) as err:                # a frame's pair count must fit 31 bits
        plan.dispersion_device(8, 8, 65536, 2, 1, 1, False, None, 8)
    assert err.value.code == native.VET_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        plan.dispersion(mu=mu, mv=mv, window=31)
    with pytest.raises(ValueError):
        plan.dispersion(mu=mu, mv=mv, per_user=True, edges=e)
    assert plan.dispersion(mu=mu, mv=mv, window=30)["stats"].shape == (3, 1)


def test_sample_out_of_range(native, plan):
    mu, mv, _ = walk_ids(7, 20, 41, p_absent=0.0)
    bad_mu, gone_mu, gone_mv = mu.copy(), mu.copy(), mv.copy()
    bad_mu[19, 3] = 1.5
    gone_mu[19, 3] = gone_mv[19, 3] = np.nan
    with pytest.raises(native.NativeError) as e:
        plan.dispersion(mu=bad_mu, mv=mv, window=5)
    assert e.value.code == native.VET_ERR_RANGE
    for per_user in (False, True):
        res = plan.dispersion(mu=bad_mu, mv=mv, window=5, per_user=per_user, check=False)
        assert res["code"] == native.VET_ERR_RANGE                # the outputs are still written: the sample counts as absent
        same_bytes(res, plan.dispersion(mu=gone_mu, mv=gone_mv, window=5, per_user=per_user), "range")


def test_analyzers_return_degrees(plan, table):
    from viewport_entropy_toolkit import SpatialEntropyAnalyzer, TransitionEntropyAnalyzer
    from viewport_entropy_toolkit.analyzers import NaiveSpatialEntropyAnalyzer
    from viewport_entropy_toolkit.config import AnalyzerConfig, NaiveAnalyzerConfig
    mu, mv, ids, ang, _ = video("walk8")
    times = np.arange(60) / 30.0
    bins = (0.0, 1.0, 5.0, 15.0, 30.0, 60.0, 90.0, 120.0, 180.0)
    frames = []
    for cls in (SpatialEntropyAnalyzer, TransitionEntropyAnalyzer, NaiveSpatialEntropyAnalyzer):
        an = cls(NaiveAnalyzerConfig(tile_height=10, tile_width=20, video_width=W, video_height=H)) \
            if cls is NaiveSpatialEntropyAnalyzer else cls(AnalyzerConfig(tile_counts=[20], video_width=W, video_height=H))
        an.load_arrays(times, mu.copy(), mv.copy())
        frames.append(an.compute_dispersion(window=20, stride=7, bins_deg=bins))
        per = an.compute_dispersion(window=20, stride=7, per_user=True)
        assert list(per.columns)[0] == "user" and len(per) == 8 * len(frames[-1]) and "hist" not in per.columns
        whole = an.compute_dispersion(window=None)
        assert len(whole) == 1 and whole["time_end"][0] == times[-1] and len(an.compute_dispersion()) == 60
    df = frames[0]
    assert list(df.columns) == ["time", "time_end", "samples", "same", "same_share", "mean", "max", "nearest", "present", "resultant",
                                "center", "hist"]
    for c in df.columns:                                         # the call is lattice-independent: three analyzers, the same values
        for other in frames[1:]:
            a, b = (np.stack(list(f[c])) if c in ("center", "hist") else f[c].to_numpy() for f in (df, other))
            assert a.tobytes() == b.tobytes(), c
    want = do.rows(ang, ids, table, 20, 7, False, edges=np.radians(bins))
    close(np.array([df["mean"], df["max"], df["nearest"]]), np.degrees(want["stats"]), "analyzer stats in degrees")
    assert np.array_equal(df["samples"], want["counts"][0]) and np.array_equal(df["same"], want["counts"][1])
    assert np.array_equal(np.stack(list(df["hist"])), want["hist"]) and np.array_equal(df["present"], want["counts"][3])
    assert ((df["resultant"] >= 0) & (df["resultant"] <= 1)).all()
    norm = np.sqrt((np.stack(list(df["center"])) ** 2).sum(axis=1))
    assert (np.abs(norm - 1.0) < 1e-12).all()
    assert df.attrs == dict(bins_deg=bins, users=df.attrs["users"], window=20, stride=7) and len(df.attrs["users"]) == 8
    assert df["time"].tolist() == times[0::7][:len(df)].tolist() and df["time_end"].tolist() == times[19::7][:len(df)].tolist()
