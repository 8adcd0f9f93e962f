"""GPU: saliency maps through the C-ABI (Plan.saliency -> vet_saliency_host, the device entries through Plan.saliency_device, the
analyzers' compute_saliency).  The reference is the numpy oracle of tests/_saliency_oracle.py (written from the definition in
include/vet.h, pinned against the real reference's cell directions and angles by golden G27 in tests/test_saliency_surface.py) —
never the code under test.

Tolerances, derived, not measured.  ``samples``, ``distinct`` and the status words: equality.  The map: rtol 1e-12, atol 2**-1000 —
the argument of exp is bit-identical (the fused dot is specified, the cell directions are products of the same sines and cosines),
two exp implementations are within 2 ulp, and a sum of n <= 2048 positive terms in any order is within (n - 1) * 2**-53 = 2.3e-13
relative (the lists here hold at most 4600 entries, 5.1e-13); subnormal terms carry no relative guarantee.  ``mass`` and ``peak``:
rtol 1e-12.  ``entropy``: 1e-10 bits absolute, four orders above the 6.3e-15 the CPU measured between summation orders
(test_saliency_surface.py), because its terms cancel.  ``area``: rtol 1e-10.  ``peak_index``: the oracle's on the rows whose largest
oracle value exceeds the second largest by more than 1e-9 relative (at least 90 % of the rows, asserted), and on every row the
argmax of the GPU's own map with ``peak`` its value.  The tests print the largest deviations they saw."""
import functools

import numpy as np
import pytest

from tests import _saliency_oracle as so

pytestmark = pytest.mark.gpu

W, H = 100, 200
RTOL, ATOL = 1e-12, 2.0 ** -1000
KEYS = ("map", "stats", "peak", "counts")
SCALES = {"none": 0, "mean": 1, "density": 2}
# (map width, map height, sigma in degrees, window): 648, 162 and 703 pixels — partial workgroups and an odd width
SETTINGS = [(36, 18, 5.0, 5), (36, 18, 2.0, 1), (18, 9, 10.0, 60), (37, 19, 1.0, 5)]


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
def oracle(mw, mh):
    return so.Oracle(grid(), mw, mh)


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


def check(res, ids, mw, mh, sigma_deg, scale, window, stride, per_user, msg, only=None, users=None):
    """a result dict against the oracle: counts of every evaluated row for equality, the map and the statistics at the module's
    tolerances; returns the oracle's rows"""
    T, U = ids.shape
    w = T if window is None else window
    R = (T - w) // stride + 1
    lead = (U, R) if per_user else (R,)
    assert res["code"] == 0 and res["stats"].shape == (4,) + lead and res["counts"].shape == (2,) + lead, msg
    assert res["peak"].shape == lead and res["peak"].dtype == np.int32 and res["counts"].dtype == np.int64, msg
    assert res["map"] is None or res["map"].shape == lead + (mh, mw), msg
    want = oracle(mw, mh).rows(ids, w, stride, rad(sigma_deg), SCALES[scale], per_user, only=only, users=users)
    rs = np.arange(R) if only is None else np.asarray(only)
    us = np.arange(U) if users is None else np.asarray(users)
    pick = (lambda a: a[..., us[:, None], rs[None, :]]) if per_user else (lambda a: a[..., rs])
    counts, stats, peak = pick(res["counts"]), pick(res["stats"]), pick(res["peak"])
    assert np.array_equal(counts, want["counts"]), msg
    empty = want["counts"][0] == 0
    assert np.isnan(stats[:, empty]).all() and not np.isnan(stats[:, ~empty]).any() and (peak[empty] == -1).all(), msg
    dev = {}
    if res["map"] is not None:
        m = res["map"][us[:, None], rs[None, :]] if per_user else res["map"][rs]
        assert (m[empty] == 0.0).all() and not np.signbit(m[empty]).any(), msg
        with np.errstate(invalid="ignore", divide="ignore"):
            big = want["map"] > 2.0 ** -900
            dev["map"] = float(np.max(np.abs(m - want["map"])[big] / want["map"][big], initial=0.0))
        np.testing.assert_allclose(m, want["map"], rtol=RTOL, atol=ATOL, err_msg=msg + " map")
        flat = m.reshape(-1, mh * mw)                            # the GPU's own map: peak is its largest value, at the first index
        own = np.where(empty.reshape(-1), -1, flat.argmax(axis=1))
        assert np.array_equal(own, peak.reshape(-1)), msg
        assert flat[~empty.reshape(-1)].max(axis=1).tobytes() == np.ascontiguousarray(stats[1].reshape(-1)[~empty.reshape(-1)]).tobytes(), msg
    ok = ~empty
    with np.errstate(invalid="ignore", divide="ignore"):
        for k, name in ((0, "mass"), (1, "peak"), (3, "area")):
            dev[name] = float(np.max(np.abs(stats[k][ok] - want["stats"][k][ok]) / want["stats"][k][ok], initial=0.0))
        dev["entropy"] = float(np.max(np.abs(stats[2][ok] - want["stats"][2][ok]), initial=0.0))
    print(msg, "largest deviations", dev)
    np.testing.assert_allclose(stats[0], want["stats"][0], rtol=RTOL, atol=0, equal_nan=True, err_msg=msg + " mass")
    np.testing.assert_allclose(stats[1], want["stats"][1], rtol=RTOL, atol=0, equal_nan=True, err_msg=msg + " peak")
    np.testing.assert_allclose(stats[2], want["stats"][2], rtol=0, atol=1e-10, equal_nan=True, err_msg=msg + " entropy")
    np.testing.assert_allclose(stats[3], want["stats"][3], rtol=1e-10, atol=0, equal_nan=True, err_msg=msg + " area")
    assert (stats[2][ok] <= 1e-10).all() and (stats[3][ok] <= 1.0 + 1e-10).all(), msg
    margin = so.peak_margin(want["map"])
    clear = ok & (margin > 1e-9)
    assert clear.sum() >= 0.9 * ok.sum(), (msg, "the peak margin condition holds for too few rows")
    assert np.array_equal(peak[clear], want["peak"][clear]), msg
    return want


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


# ------------------------------------------------------------------------------------------- the numpy oracle
@pytest.mark.parametrize("mw,mh,sigma,window", SETTINGS)
@pytest.mark.parametrize("per_user", [False, True])
def test_vs_oracle(plan, mw, mh, sigma, window, per_user):
    mu, mv, ids = g15()
    for n, stride in enumerate((1, 5)):
        kw = dict(ids=ids) if n else dict(mu=mu, mv=mv)          # both entries
        res = plan.saliency(window=window, stride=stride, per_user=per_user, sigma_deg=sigma, width=mw, height=mh, **kw)
        check(res, ids, mw, mh, sigma, "density", window, stride, per_user,
              f"{mw}x{mh} sigma={sigma} window={window} stride={stride} per_user={per_user}")
    if window == 60:
        whole = plan.saliency(mu=mu, mv=mv, window=None, per_user=per_user, sigma_deg=sigma, width=mw, height=mh)
        same_bytes(whole, res, "window=None is window = T")


def edge_video():
    """ids [20][5] on the 100 x 200 grid: frame 3 with nobody, pole-row ids that share one Vector, repeated ids, viewer 4 never"""
    _, _, walk = g15()
    ids = np.array(walk[:20, :5])
    ids[3] = -1
    ids[:, 4] = -1
    ids[5] = [3, 90, 60 * 101 + 30, 60 * 101 + 30, -1]            # py = 0: every pixel of the row is the north pole; another id twice
    ids[6] = [200 * 101 + 7, 200 * 101 + 7, 40 * 101 + 20, 40 * 101 + 20, -1]           # the last pixel row: one id twice
    ids[7, :4] = ids[8, :4] = 77 * 101 + 31                       # eight samples on one pixel
    return ids


@pytest.mark.parametrize("per_user", [False, True])
def test_edge_rows(plan, per_user):
    import torch
    ids = edge_video()
    for window, stride in ((1, 1), (2, 1), (4, 3), (None, 1)):
        for scale in ("density", "none"):
            res = plan.saliency(ids=ids, window=window, stride=stride, per_user=per_user, sigma_deg=5.0, width=36, height=18, scale=scale)
            check(res, ids, 36, 18, 5.0, scale, window, stride, per_user, f"edge rows window={window} per_user={per_user} {scale}")
        if window == 1 and not per_user:
            assert res["counts"][:, 3].tolist() == [0, 0] and res["peak"][3] == -1 and np.isnan(res["stats"][:, 3]).all()
            assert res["counts"][:, 5].tolist() == [4, 3] and res["counts"][:, 6].tolist() == [4, 2]         # entries with m = 2
            assert res["counts"][:, 7].tolist() == [4, 1]
        if window == 1 and per_user:
            assert res["peak"][0, 5] // 36 == 0 and res["peak"][1, 5] // 36 == 0                            # the north pole: the top row
    # status[1]: the rows with N = 0, through the device entry
    dev = torch.device("cuda", 0)
    d_ids = torch.from_numpy(ids).to(dev)
    host = plan.saliency(ids=ids, window=1, per_user=per_user, width=36, height=18, want_map=False)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    counts = torch.zeros(host["counts"].shape, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    plan.saliency_device(0, 0, 5, 20, 1, 1, per_user, width=36, height=18, d_counts=counts.data_ptr(), d_status=status.data_ptr(),
                         d_ids=d_ids.data_ptr())
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, int((host["counts"][0] == 0).sum())] and status[1].item() > 0
    assert counts.cpu().numpy().tobytes() == host["counts"].tobytes()


def test_one_viewer(plan):
    mu, mv, ids = g15()
    one = np.ascontiguousarray(ids[:, 2:3])
    for per_user in (False, True):
        for window in (1, 5, None):
            res = plan.saliency(ids=one, window=window, per_user=per_user, sigma_deg=5.0, width=36, height=18)
            check(res, one, 36, 18, 5.0, "density", window, 1, per_user, f"U=1 window={window} per_user={per_user}")
    a = plan.saliency(ids=one, window=5, sigma_deg=5.0, width=36, height=18)
    b = plan.saliency(ids=one, window=5, per_user=True, sigma_deg=5.0, width=36, height=18)
    same_bytes(a, {k: v[0] if k in ("map", "peak") else v[:, 0] for k, v in b.items() if k != "code"}, "U = 1: pooled is per viewer")
    t1 = plan.saliency(mu=mu[:1], mv=mv[:1], window=1, sigma_deg=5.0, width=36, height=18)           # T = 1
    check(t1, ids[:1], 36, 18, 5.0, "density", 1, 1, False, "T=1")


@pytest.mark.parametrize("sigma", [1.0, 0.5, 180.0])
def test_narrow_and_wide_kernels(plan, sigma):
    """sigma 1 and 0.5 degrees: far terms underflow to 0.0 and some land in the subnormals; sigma 180: kappa = 1 / pi^2"""
    _, _, ids = g15()
    for per_user in (False, True):
        res = plan.saliency(ids=ids, window=5, stride=5, per_user=per_user, sigma_deg=sigma, width=36, height=18)
        want = check(res, ids, 36, 18, sigma, "density", 5, 5, per_user, f"sigma={sigma} per_user={per_user}")
    if sigma < 180.0:
        none = plan.saliency(ids=ids, window=5, stride=5, sigma_deg=sigma, width=36, height=18, scale="none")
        want = check(none, ids, 36, 18, sigma, "none", 5, 5, False, f"sigma={sigma} sums")
        assert (want["map"] == 0.0).any(), "no term underflowed to zero"
        if sigma == 0.5:
            assert ((want["map"] > 0) & (want["map"] < 2.0 ** -1022)).any(), "no value among the subnormals"
    else:
        assert res["stats"][3].min() > 0.9                        # nearly uniform: the effective area is nearly the sphere


def test_two_thousand_directions_cross_the_lds_tile(engine, plan):
    """64 viewers x 40 frames, uniform on the sphere: about 2 500 distinct directions in the whole-video row, three LDS tiles"""
    mu, mv, ids = sphere(64, 40, 5)
    res = plan.saliency(mu=mu, mv=mv, window=None, sigma_deg=10.0, width=12, height=6)
    check(res, ids, 12, 6, 10.0, "density", None, 1, False, "64 x 40 whole video")
    assert 2000 <= res["counts"][1, 0] <= 2560 and res["counts"][0, 0] <= 2560
    engine.test_saliency_tile(100)
    try:
        same_bytes(plan.saliency(ids=ids, window=None, sigma_deg=10.0, width=12, height=6), res, "tiles of 100")
    finally:
        engine.test_saliency_tile(0)


def test_long_rows_take_the_counting_path(plan):
    """128 viewers x 40 frames: the whole-video row has 5 120 positions, beyond the 4 096 of the LDS sort; window 32 (4 096) is the
    largest sorted row, window 33 the smallest counted one: the same frames give the same bytes through both"""
    mu, mv, ids = sphere(128, 40, 6)
    res = plan.saliency(ids=ids, window=None, sigma_deg=10.0, width=12, height=6)
    check(res, ids, 12, 6, 10.0, "density", None, 1, False, "128 x 40 whole video")
    assert res["counts"][0, 0] > 4096 and res["counts"][1, 0] > 4000
    for window in (32, 33):
        r = plan.saliency(mu=mu, mv=mv, window=window, stride=4, sigma_deg=10.0, width=12, height=6)
        check(r, ids, 12, 6, 10.0, "density", window, 4, False, f"128 x 40 window={window}", only=[0, 1])
    gone = np.array(ids)
    gone[32] = -1                                                 # frame 32 empty: rows of 33 frames hold the lists of 32 frames
    a = plan.saliency(ids=gone, window=32, stride=8, sigma_deg=10.0, width=12, height=6)
    b = plan.saliency(ids=gone, window=33, stride=8, sigma_deg=10.0, width=12, height=6)
    same_bytes(take_rows(a, slice(0, 1), False), b, "sorted against counted list")


def test_long_rows_on_a_direction_table_beyond_the_lds_counts(native, engine):
    """a 300 x 200 pixel grid has 60 501 directions, more than the 32 768 that the counting path holds in LDS: 64 viewers x 70 frames,
    4 480 positions in the whole-video row, counted by global integer atomics"""
    from oracle import vet_oracle as vo
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.uniform_sphere_video(64, 70, base_seed=8)
    ids = so.ids_of(mu, mv, 300, 200)
    big = native.Plan(engine, [vo.fibonacci_lattice(50)], 120.0, 2.0, True, 300, 200)
    try:
        table = so.grid_table(300, 200)
        assert np.array_equal(big.read_dirs(), table) and len(table) == 60501
        res = big.saliency(mu=mu, mv=mv, window=None, sigma_deg=10.0, width=12, height=6)
        want = so.Oracle(table, 12, 6).rows(ids, 70, 1, rad(10.0), 2)
        assert np.array_equal(res["counts"], want["counts"]) and res["counts"][0, 0] == 4480 and res["counts"][1, 0] > 4096
        np.testing.assert_allclose(res["map"], want["map"], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(res["stats"][:2], want["stats"][:2], rtol=RTOL)
        np.testing.assert_allclose(res["stats"][2], want["stats"][2], rtol=0, atol=1e-10)
        np.testing.assert_allclose(res["stats"][3], want["stats"][3], rtol=1e-10)
        assert so.peak_margin(want["map"])[0] > 1e-9 and res["peak"][0] == want["peak"][0]
        a = big.saliency(ids=ids, window=64, stride=6, sigma_deg=10.0, width=12, height=6)          # 4 096 positions: the sorted list
        gone = np.array(ids)
        gone[64] = -1
        b = big.saliency(ids=gone, window=65, stride=5, sigma_deg=10.0, width=12, height=6)          # 4 160: counted; frame 64 is empty
        same_bytes(take_rows(a, slice(0, 1), False), take_rows(b, slice(0, 1), False), "sorted against counted list")
    finally:
        big.close()


# ------------------------------------------------------------------------------------------- bit invariance
def test_scales_are_one_multiply(plan):
    _, _, ids = g15()
    for per_user in (False, True):
        kw = dict(ids=ids, window=5, stride=5, per_user=per_user, sigma_deg=5.0, width=37, height=19)
        S = plan.saliency(scale="none", **kw)
        want = oracle(37, 19).rows(ids, 5, 5, rad(5.0), 0, per_user)
        np.testing.assert_allclose(S["map"], want["S"], rtol=RTOL, atol=ATOL)
        N = S["counts"][0].astype(np.float64)[..., None, None]
        kappa = 1.0 / rad(5.0) ** 2
        C = kappa / (2.0 * np.pi * (1.0 - np.exp(-2.0 * kappa)))
        with np.errstate(divide="ignore", invalid="ignore"):
            for scale, g in (("mean", 1.0 / N), ("density", C / N)):
                got = plan.saliency(scale=scale, **kw)
                assert got["map"].tobytes() == np.where(N == 0, 0.0, S["map"] * g).tobytes(), (scale, per_user)
                same_bytes(got, S, scale, keys=("counts", "peak"))


def test_bits_do_not_depend_on_stride_length_entry_or_outputs(plan):
    import torch
    mu_long, mv_long, ids_long = g15()
    T, U = 25, 8
    mu, mv, ids = mu_long[:T], mv_long[:T], ids_long[:T]
    dev = torch.device("cuda", 0)
    for per_user in (False, True):
        kw = dict(window=5, per_user=per_user, sigma_deg=5.0, width=37, height=19)
        s1 = plan.saliency(mu=mu, mv=mv, stride=1, **kw)
        s3 = plan.saliency(mu=mu, mv=mv, stride=3, **kw)
        same_bytes(take_rows(s1, slice(0, None, 3), per_user), s3, f"stride 1 against stride 3, per_user={per_user}")
        long = plan.saliency(mu=mu_long, mv=mv_long, stride=1, **kw)             # the rows wholly inside the truncated video
        same_bytes(take_rows(long, slice(0, T - 5 + 1), per_user), s1, f"a truncated video, per_user={per_user}")
        few = plan.saliency(mu=mu[3:9], mv=mv[3:9], stride=1, **kw)              # two rows of the same frames
        same_bytes(few, take_rows(s1, slice(3, 5), per_user), f"the number of rows, per_user={per_user}")
        same_bytes(plan.saliency(ids=ids, stride=1, **kw), s1, f"ids against (mu, mv), per_user={per_user}")
        same_bytes(plan.saliency(ids=ids, stride=1, want_map=False, **kw), s1, f"without the map, per_user={per_user}")
        # the device entries, every output and one output at a time
        rows = s1["peak"].size
        d_mu, d_mv, d_ids = (torch.from_numpy(np.array(a)).to(dev) for a in (mu, mv, ids))          # writable copies
        shapes = dict(map=((rows, 19, 37), torch.float64), stats=((4, rows), torch.float64), peak=((rows,), torch.int32),
                      counts=((2, rows), torch.int64))
        for src in ("mu_mv", "ids"):
            extra = dict(d_ids=d_ids.data_ptr()) if src == "ids" else {}
            for wanted in (KEYS, ("map",), ("stats",), ("peak",), ("counts",), ("stats", "peak"), ()):
                bufs = {k: torch.full(shapes[k][0], -7, dtype=shapes[k][1], device=dev) for k in wanted}
                status = torch.zeros(2, dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                plan.saliency_device(d_mu.data_ptr(), d_mv.data_ptr(), U, T, 5, 1, per_user, 5.0, 37, 19, "density",
                                     d_status=status.data_ptr(), **{"d_" + k: b.data_ptr() for k, b in bufs.items()}, **extra)
                torch.cuda.synchronize()
                for k, b in bufs.items():
                    assert b.cpu().numpy().tobytes() == s1[k].tobytes(), (per_user, src, wanted, k)
                assert status.cpu().tolist() == [0, int((s1["counts"][0] == 0).sum())]


@pytest.mark.parametrize("tile", [4, 1])
def test_lds_tile_does_not_change_a_bit(engine, plan, tile):
    mu, mv, ids = g15()
    shapes = [(1, 1, False), (5, 5, False), (None, 1, False), (None, 1, True), (5, 5, True)]
    default = [plan.saliency(mu=mu, mv=mv, window=w, stride=s, per_user=pu, sigma_deg=5.0, width=36, height=18) for w, s, pu in shapes]
    try:
        engine.test_saliency_tile(tile)
        for (w, s, pu), ref in zip(shapes, default):
            kw = dict(ids=ids) if tile == 4 else dict(mu=mu, mv=mv)
            res = plan.saliency(window=w, stride=s, per_user=pu, sigma_deg=5.0, width=36, height=18, **kw)
            same_bytes(res, ref, f"tile {tile}: window={w} stride={s} per_user={pu}")
    finally:
        engine.test_saliency_tile(0)


def test_row_chunks_do_not_change_a_bit(plan):
    """A 1024 x 512 map is 4 MB a row: without d_map a pass holds 63 rows (their lists too) under the 256 MB budget, so 70 rows take
    two passes; the rows on both sides of the seam keep the bytes they have in calls of their own.  The mass: the midpoint rule on
    cells of 0.35 degrees under a kernel of sigma 3 degrees is within h^2 / (24 sigma^2) = 6e-4 of the integral, 4 pi * mass = 1."""
    rng = np.random.default_rng(9)
    ids = rng.integers(0, 101 * 201, size=(70, 3)).astype(np.int32)
    kw = dict(window=1, sigma_deg=3.0, width=1024, height=512, want_map=False)
    res = plan.saliency(ids=ids, **kw)
    assert res["map"] is None and (res["counts"][0] == 3).all() and not np.isnan(res["stats"]).any()
    for r in (0, 62, 63, 64, 69):
        one = plan.saliency(ids=ids[r:r + 1], **kw)
        same_bytes(take_rows(res, slice(r, r + 1), False), one, f"row {r}", keys=("stats", "peak", "counts"))
    np.testing.assert_allclose(4.0 * np.pi * res["stats"][0], 1.0, rtol=1e-3)     # the grid resolves sigma: the density integrates to 1
    full = plan.saliency(ids=ids[63:65], window=1, sigma_deg=3.0, width=1024, height=512)             # with the maps
    same_bytes(take_rows(res, slice(63, 65), False), full, "with d_map", keys=("stats", "peak", "counts"))


# ------------------------------------------------------------------------------------------- per viewer, refusals, the analyzers
def test_per_viewer_rows_add_up_to_the_pooled_row(plan):
    _, _, ids = g15()
    for window, stride in ((1, 1), (5, 5), (None, 1)):
        kw = dict(ids=ids, window=window, stride=stride, sigma_deg=5.0, width=36, height=18, scale="none")
        pooled, per = plan.saliency(**kw), plan.saliency(per_user=True, **kw)
        assert np.array_equal(per["counts"][0].sum(axis=0), pooled["counts"][0])
        assert (per["counts"][1].sum(axis=0) >= pooled["counts"][1]).all()
        np.testing.assert_allclose(per["map"].sum(axis=0), pooled["map"], rtol=RTOL, atol=ATOL)


def test_illegal_arguments_are_refused_before_anything_runs(native, plan):
    mu, mv, _ = g15()
    mu, mv = np.ascontiguousarray(mu[:30, :4]), np.ascontiguousarray(mv[:30, :4])
    lib = native.load_library()
    stats = np.empty((4, 64))
    good = dict(window=5, stride=1, sigma=0.1, W=36, H=18, scale=2)
    bad = [dict(window=0), dict(window=31), dict(stride=0), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")),
           dict(sigma=float("inf")), dict(sigma=3.2), dict(W=1), dict(W=4097), dict(H=0), dict(H=2049), dict(scale=-1), dict(scale=3)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.vet_saliency_host(plan.handle, native._ptr(mu), native._ptr(mv), None, 4, 30, a["window"], a["stride"], 0,
                                   a["sigma"], a["W"], a["H"], a["scale"], None, native._ptr(stats), None, None)
        assert rc == native.VET_ERR_INVALID, change
    with pytest.raises(native.NativeError) as err:                # the device entry refuses before it looks at a pointer
        plan.saliency_device(8, 8, 4, 30, 31, 1, False, d_stats=8)
    assert err.value.code == native.VET_ERR_INVALID
    with pytest.raises(native.NativeError) as err:                # per viewer: k_user_dirs' grid holds 65535 * 64 frames
        plan.saliency_device(8, 8, 1, 65535 * 64 + 1, 1, 1, True, d_stats=8)
    assert err.value.code == native.VET_ERR_UNSUPPORTED
    for kw in (dict(window=31), dict(sigma_deg=0.0), dict(sigma_deg=181.0), dict(width=1), dict(height=2049), dict(scale="max")):
        with pytest.raises(ValueError):
            plan.saliency(mu=mu, mv=mv, **kw)
    assert plan.saliency(mu=mu, mv=mv, window=30, width=36, height=18)["stats"].shape == (4, 1)


def test_sample_out_of_range(native, plan):
    mu, mv, _ = g15()
    mu, mv = np.array(mu[:20]), np.array(mv[:20])
    mu[np.isnan(mu)] = 0.5
    mv[np.isnan(mv)] = 0.5
    bad_mu, gone_mu, gone_mv = mu.copy(), mu.copy(), mv.copy()
    bad_mu[19, 3] = 1.5
    gone_mu[19, 3] = gone_mv[19, 3] = np.nan
    with pytest.raises(native.NativeError) as e:
        plan.saliency(mu=bad_mu, mv=mv, window=5, width=36, height=18)
    assert e.value.code == native.VET_ERR_RANGE
    for per_user in (False, True):
        res = plan.saliency(mu=bad_mu, mv=mv, window=5, per_user=per_user, width=36, height=18, check=False)
        assert res["code"] == native.VET_ERR_RANGE                # the outputs are still written: the sample counts as absent
        same_bytes(res, plan.saliency(mu=gone_mu, mv=gone_mv, window=5, per_user=per_user, width=36, height=18), "range")


def test_analyzers_return_the_oracle_columns():
    from viewport_entropy_toolkit import SpatialEntropyAnalyzer
    from viewport_entropy_toolkit.analyzers import NaiveSpatialEntropyAnalyzer
    from viewport_entropy_toolkit.config import AnalyzerConfig, NaiveAnalyzerConfig
    mu, mv, ids = g15()
    times = np.arange(60) / 30.0
    frames = []
    for cls in (SpatialEntropyAnalyzer, NaiveSpatialEntropyAnalyzer):
        an = cls(NaiveAnalyzerConfig(tile_height=10, tile_width=20, video_width=W, video_height=H)) \
            if cls is NaiveSpatialEntropyAnalyzer else cls(AnalyzerConfig(tile_counts=[20], video_width=W, video_height=H))
        an.load_arrays(times, mu.copy(), mv.copy())
        frames.append(an.compute_saliency(window=5, stride=5, sigma_deg=5.0, width=36, height=18))
        per = an.compute_saliency(window=5, stride=5, width=36, height=18, per_user=True, keep_maps=False)
        assert list(per.columns)[0] == "user" and len(per) == 8 * len(frames[-1]) and "map" not in per.columns
        whole = an.compute_saliency(window=None, width=36, height=18, normalize="mean")
        assert len(whole) == 1 and whole["time_end"][0] == times[-1] and whole.attrs["normalize"] == "mean"
    df = frames[0]
    assert list(df.columns) == ["time", "time_end", "samples", "distinct", "mass", "peak", "peak_lon", "peak_lat", "entropy", "area", "map"]
    for c in df.columns:                                         # the call is lattice-independent: two analyzers, the same values
        a, b = (np.stack(list(f[c])) if c == "map" else f[c].to_numpy() for f in (df, frames[1]))
        assert a.tobytes() == b.tobytes(), c
    o = oracle(36, 18)
    want = o.rows(ids, 5, 5, rad(5.0), 2)
    assert np.array_equal(df["samples"], want["counts"][0]) and np.array_equal(df["distinct"], want["counts"][1])
    np.testing.assert_allclose(np.stack(list(df["map"])), want["map"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(df["mass"], want["stats"][0], rtol=RTOL)
    np.testing.assert_allclose(df["peak"], want["stats"][1], rtol=RTOL)
    np.testing.assert_allclose(df["entropy"], want["stats"][2], rtol=0, atol=1e-10)
    np.testing.assert_allclose(df["area"], want["stats"][3], rtol=1e-10)
    clear = so.peak_margin(want["map"]) > 1e-9
    assert clear.all()
    assert np.array_equal(df["peak_lon"], o.lon[want["peak"] % 36]) and np.array_equal(df["peak_lat"], o.lat[want["peak"] // 36])
    base = df["map"][0].base
    assert base is not None and all(np.shares_memory(m, base) for m in df["map"]) and df["map"][0].shape == (18, 36)     # views, no copy
    assert df.attrs["sigma_deg"] == 5.0 and df.attrs["width"] == 36 and df.attrs["height"] == 18 and df.attrs["normalize"] == "density"
    assert df.attrs["window"] == 5 and df.attrs["stride"] == 5 and len(df.attrs["users"]) == 8 and df.attrs["kappa"] == 1.0 / rad(5.0) ** 2
    assert df["time"].tolist() == times[0::5][:len(df)].tolist() and df["time_end"].tolist() == times[4::5][:len(df)].tolist()
