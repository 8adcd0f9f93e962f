"""GPU: scoring a predicted saliency map against where the audience looked, through the C-ABI (Plan.saliency_score ->
vet_saliency_score_host, the device entries through Plan.saliency_score_device, the analyzers' compute_saliency_score).  The
reference is the numpy oracle of tests/_saliency_score_oracle.py (written from the definition in include/vet.h on top of the
saliency and similarity oracles) — never the code under test.

Tolerances.  Counts and status words: equality; +inf, -inf and NaN in the same places.  The audience's map: the saliency suite's
rtol 1e-12, atol 2**-1000.  Finite statistics: the similarity suite's 1e-10 — absolute for ``auc``, ``cc``, ``sim`` and ``jsd``,
1e-10 relative + 1e-10 absolute for ``nss``, ``info_gain``, ``kl``, ``mass`` and ``mass_pred``.  ``auc`` additionally at 1e-12
absolute: its counts are integers, and every comparison first asserts the oracle's own ``auc_gap >= 1e-9`` — no interpolated value
within rounding of an unequal cell value, a condition on the inputs, not a tolerance; what remains is the rounding of v_i where it
ties nothing and the order of the sums.  The tests print the largest deviations they saw.

Largest deviations seen on an MI355X over all tests of this file: auc 3.3e-16, cc 4.4e-16, sim 4.4e-16, jsd 2.2e-16 absolute;
nss 3.9e-14, info_gain 2.0e-14, kl 8.1e-16, mass 3.9e-17, mass_pred 1.1e-16 relative to 1 + |value|; the smallest ``auc_gap`` of
the inputs 1.1e-8; audience A scored by the similarity call's map of audience B against that call's cc, sim, jsd, kl_ab: 0.0."""
import functools
import math

import numpy as np
import pytest

from tests import _saliency_oracle as so
from tests import _saliency_score_oracle as sco
from tests import _saliency_similarity_oracle as sso

pytestmark = pytest.mark.gpu

W, H = 100, 200
KEYS = ("map", "stats", "counts")
ABS = (0, 3, 4, 5)               # auc, cc, sim, jsd: absolute 1e-10
LOC = [0, 1, 2, 8]               # the location metrics and mass_pred
# (map width, map height, sigma in degrees, window): the issue's four settings
SETTINGS = [(36, 18, 5.0, 5), (37, 19, 2.0, 1), (18, 9, 10.0, 60), (50, 25, 5.0, 20)]


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
    return sco.Oracle(grid(), mw, mh)


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


@functools.lru_cache(maxsize=None)
def g15_map(mw, mh, sigma, seed, n=None):
    """the issue's construction on G15: the video's whole-video density + a quarter of its mean, 5 % noise; shared, never written to"""
    m = sco.density_map(oracle(mw, mh), g15()[2], rad(sigma), seed, n)
    m.setflags(write=False)
    return m


def noise_map(mw, mh, seed, n=None):
    """a map of independent uniform values in [0.5, 1.5): every value distinct, nothing smooth — for the seams of the AUC walk"""
    return np.random.default_rng(seed).uniform(0.5, 1.5, size=(mh, mw) if n is None else (n, mh, mw))


def rad(deg):
    return min(float(np.radians(deg)), float(np.pi))


def check(res, ids, maps, sigma_deg, window, stride, msg, distribution=True, only=None):
    """a result dict against the oracle at the module's tolerances; returns the oracle's rows"""
    T, U = ids.shape
    mh, mw = maps.shape[-2:]
    w = T if window is None else window
    R = (T - w) // stride + 1
    assert res["code"] == 0 and res["stats"].shape == (9, R) and res["counts"].shape == (2, R), msg
    assert res["stats"].dtype == np.float64 and res["counts"].dtype == np.int64, msg
    assert res["map"] is None or res["map"].shape == (R, mh, mw), msg
    want = oracle(mw, mh).rows(ids, maps, w, stride, rad(sigma_deg), distribution, only=only)
    assert want["gap"] >= sco.GAP_MIN, (msg, "the inputs do not meet the gap condition", want["gap"])
    rs = np.arange(R) if only is None else np.asarray(only)
    stats, counts = res["stats"][:, rs], res["counts"][:, rs]
    assert np.array_equal(counts, want["counts"]), msg
    empty = counts[0] == 0
    assert np.isnan(stats[:8, empty]).all() and not np.isnan(stats[8]).any(), msg
    if not distribution:
        assert np.isnan(stats[3:8]).all(), msg
    assert np.array_equal(np.isnan(stats), np.isnan(want["stats"])), (msg, stats, want["stats"])
    assert np.array_equal(np.isposinf(stats), np.isposinf(want["stats"])), msg
    assert np.array_equal(np.isneginf(stats), np.isneginf(want["stats"])), msg
    dev = {}
    for k, name in enumerate(sco.STATS):
        fin = np.isfinite(want["stats"][k])
        d = np.abs(stats[k][fin] - want["stats"][k][fin])
        if k not in ABS:
            d = d / (1.0 + np.abs(want["stats"][k][fin]))
        dev[name] = float(d.max(initial=0.0))
    print(msg, "gap", want["gap"], "largest deviations (auc, cc, sim, jsd absolute; the others over 1 + |value|)", dev,
          "inf:", int(np.isinf(stats).sum()))
    for k, name in enumerate(sco.STATS):
        fin = np.isfinite(want["stats"][k])
        np.testing.assert_allclose(stats[k][fin], want["stats"][k][fin], rtol=0 if k in ABS else 1e-10, atol=1e-10, err_msg=f"{msg} {name}")
    fin = np.isfinite(want["stats"][0])
    np.testing.assert_allclose(stats[0][fin], want["stats"][0][fin], rtol=0, atol=1e-12, err_msg=f"{msg} auc at 1e-12")
    if res["map"] is not None and distribution:
        np.testing.assert_allclose(res["map"][rs], want["map"], rtol=1e-12, atol=2.0 ** -1000, err_msg=msg + " map")
    return want


def same_bytes(a, b, msg, keys=KEYS):
    for key in keys:
        if a[key] is None or b[key] is None:
            continue
        assert a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), (msg, key)


def take_rows(res, sel):
    """the rows ``sel`` (a slice) of a result dict, contiguous"""
    return dict(map=None if res["map"] is None else np.ascontiguousarray(res["map"][sel]),
                stats=np.ascontiguousarray(res["stats"][:, sel]), counts=np.ascontiguousarray(res["counts"][:, sel]))


def device_call(plan, pred, U, T, window, stride, sigma, wanted, distribution=True, d_mu=0, d_mv=0, d_ids=0):
    """the device entry into fresh buffers: (dict of numpy results for ``wanted``, status [2]); the predicted map is read in place"""
    import torch
    dev = torch.device("cuda", 0)
    R = (T - window) // stride + 1
    mh, mw = pred.shape[-2:]
    d_pred = torch.from_numpy(np.array(pred)).to(dev)
    shapes = dict(map=((R, mh, mw), torch.float64), stats=((9, R), torch.float64), counts=((2, R), torch.int64))
    bufs = {k: torch.full(shapes[k][0], -7, dtype=shapes[k][1], device=dev) for k in wanted}
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    plan.saliency_score_device(d_mu, d_mv, U, T, window, stride, d_pred.data_ptr(), 1 if pred.ndim == 2 else pred.shape[0], mw, mh, sigma,
                               distribution, d_status=status.data_ptr(), d_ids=d_ids, **{"d_" + k: b.data_ptr() for k, b in bufs.items()})
    torch.cuda.synchronize()
    assert d_pred.cpu().numpy().tobytes() == np.ascontiguousarray(pred).tobytes()
    return {k: b.cpu().numpy() for k, b in bufs.items()}, status.cpu().tolist()


# ------------------------------------------------------------------------------------------- 1. the numpy oracle
@pytest.mark.parametrize("mw,mh,sigma,window", SETTINGS)
def test_vs_oracle(plan, mw, mh, sigma, window):
    import torch
    mu, mv, ids = g15()
    for n, stride in enumerate((1, window) if window > 1 else (1,)):
        R = (60 - window) // stride + 1
        only = None if R <= 20 or window == 1 else sorted(set(range(0, R, 5)) | {R - 1})      # the oracle's time, not the library's
        per_row = g15_map(mw, mh, sigma, 7, (60 - window) + 1)[::stride]
        for maps, what in ((np.ascontiguousarray(per_row), "per-row maps"), (g15_map(mw, mh, sigma, 7), "a static map")):
            kw = dict(ids=ids) if n else dict(mu=mu, mv=mv)      # both entries
            res = plan.saliency_score(maps=maps, window=window, stride=stride, sigma_deg=sigma, want_map=True, **kw)
            check(res, ids, maps, sigma, window, stride, f"{mw}x{mh} sigma={sigma} window={window} stride={stride} {what}", only=only)
            if window == 1:
                n_empty = int((res["counts"][0] == 0).sum())
                d_ids = torch.from_numpy(np.array(ids)).to(torch.device("cuda", 0))
                got, status = device_call(plan, maps, 8, 60, 1, 1, sigma, ("stats", "counts"), d_ids=d_ids.data_ptr())
                assert status == [0, n_empty]
                same_bytes(dict(got, map=None), res, "the device entry")


# ------------------------------------------------------------------------------------------- 2. seams of the sort and of the walk
@pytest.mark.parametrize("mw,mh", [(100, 50), (128, 33), (37, 19), (4096, 2), (36, 1), (2, 1)])
def test_map_shapes_location_only(plan, mw, mh):
    """100 x 50: the sorted rows take two LDS tiles of 40 map rows; 128 x 33: a power-of-two width, no padding of the sort, and a last
    tile of one row; 37 x 19: padding to 64; 4096 x 2: the widest sort, one map row per tile; one map row; the smallest map"""
    _, _, ids = g15()
    for maps, what in ((noise_map(mw, mh, 21), "static"), (noise_map(mw, mh, 22, 12), "per row")):
        res = plan.saliency_score(ids=ids, maps=maps, window=5, stride=5, distribution=False)
        check(res, ids, maps, 5.0, 5, 5, f"{mw}x{mh} {what} location only", distribution=False)
        assert res["map"] is None


def test_lists_beyond_a_workgroup_and_a_block(plan):
    """40 viewers x 64 frames, uniform on the sphere, the whole video: 2 560 positions and more than 1 024 distinct directions — several
    workgroups per list in k_score_points and more than one 1 024-block of the rule over v_i and u_i"""
    mu, mv, ids = sphere(40, 64, 11)
    maps = noise_map(36, 18, 23)
    res = plan.saliency_score(mu=mu, mv=mv, maps=maps, window=64, distribution=False)
    check(res, ids, maps, 5.0, 64, 1, "40 x 64 whole video", distribution=False)
    assert res["counts"][0, 0] == 2560 and 1024 < res["counts"][1, 0] <= 2560


def test_long_rows_take_the_counting_path(plan):
    """80 viewers x 64 frames: a row of 64 frames has 5 120 positions, beyond the 4 096 of the LDS sort.  With the last 13 frames empty,
    a row of 51 frames (4 080 positions: sorted) and the row of 64 frames (counted) hold the same lists: the same bytes"""
    mu, mv, ids = sphere(80, 64, 12)
    maps = noise_map(36, 18, 24)
    res = plan.saliency_score(mu=mu, mv=mv, maps=maps, window=64, distribution=False)
    check(res, ids, maps, 5.0, 64, 1, "80 x 64 whole video", distribution=False)
    assert res["counts"][0, 0] == 5120 and res["counts"][1, 0] > 2000
    gone = np.array(ids)
    gone[51:] = -1
    for dist in (False, True):
        a = plan.saliency_score(ids=gone, maps=maps, window=51, stride=13, sigma_deg=10.0, distribution=dist, want_map=dist)
        b = plan.saliency_score(ids=gone, maps=maps, window=64, sigma_deg=10.0, distribution=dist, want_map=dist)
        assert a["stats"].shape == (9, 2)
        same_bytes(take_rows(a, slice(0, 1)), b, "sorted against counted lists")


# ------------------------------------------------------------------------------------------- 3. edges
def edge_video():
    """ids [20][6] on the 100 x 200 grid: frame 3 with nobody, viewer 5 never present, a pole direction, both sides of the antimeridian,
    samples above the first and below the last cell-centre latitude of an 18-row map, repeated ids"""
    _, _, walk = g15()
    ids = np.array(walk[:20, :6])
    ids[3] = -1
    ids[:, 5] = -1
    ids[5] = [3, 90, 60 * 101 + 30, 60 * 101 + 30, 7, -1]            # py = 0: every pixel of the row is the north pole
    ids[6] = [77 * 101 + 0, 77 * 101 + 100, 77 * 101 + 1, 77 * 101 + 99, 120 * 101 + 0, -1]       # lon -180 and +180: both column wraps
    ids[7] = [2 * 101 + 40, 3 * 101 + 70, 198 * 101 + 10, 197 * 101 + 55, 199 * 101 + 99, -1]     # within 5 degrees of the poles
    ids[8, :5] = ids[9, :5] = 77 * 101 + 31                        # ten samples on one pixel
    return ids


def cell_of(idx, mw, mh):
    """(y0, c0): the top-left corner of the bilinear cell of direction ``idx``, by the definition's arithmetic"""
    x, y, z = so.unit_rows(grid())[idx]
    lon = 0.0 if x == 0 and y == 0 else math.atan2(y, x)
    fy = min(max(math.acos(min(max(z, -1.0), 1.0)) / math.pi * mh - 0.5, 0.0), mh - 1.0)
    return int(math.floor(fy)), int(math.floor((lon + math.pi) / (2 * math.pi) * mw - 0.5)) % mw


def test_edge_rows(plan):
    ids = edge_video()
    mw, mh = 36, 18
    maps = np.array(g15_map(mw, mh, 5.0, 9))
    y0, c0 = cell_of(60 * 101 + 30, mw, mh)                         # a zero region under the two samples of frame 5
    for dy in range(-1, 3):
        for dx in range(-1, 3):
            maps[min(max(y0 + dy, 0), mh - 1), (c0 + dx) % mw] = 0.0
    for window, stride in ((1, 1), (2, 1), (4, 3), (None, 1)):
        res = plan.saliency_score(ids=ids, maps=maps, window=window, stride=stride, sigma_deg=5.0, want_map=True)
        check(res, ids, maps, 5.0, window, stride, f"edge rows window={window}")
        assert np.isneginf(res["stats"][2]).any() and np.isposinf(res["stats"][6]).any()      # info_gain -inf, kl +inf: data
        if window == 1:
            assert res["counts"][:, 3].tolist() == [0, 0] and np.isnan(res["stats"][:8, 3]).all() and res["stats"][8, 3] > 0
            assert (res["map"][3] == 0.0).all() and not np.signbit(res["map"][3]).any()
            assert res["counts"][:, 5].tolist() == [5, 4] and res["counts"][:, 8].tolist() == [5, 1]
            assert np.isneginf(res["stats"][2, 5]) and np.isposinf(res["stats"][6, 5]) and np.isfinite(res["stats"][[0, 1, 3, 4, 5], 5]).all()
    import torch
    d_ids = torch.from_numpy(ids).to(torch.device("cuda", 0))
    got, status = device_call(plan, maps, 6, 20, 1, 1, 5.0, ("counts",), d_ids=d_ids.data_ptr())
    assert status == [0, 1] and got["counts"][:, 3].tolist() == [0, 0]                      # status[1]: the rows without a sample
    whole = plan.saliency_score(ids=ids, maps=maps, window=None, want_map=True)
    same_bytes(whole, plan.saliency_score(ids=ids, maps=maps, window=20, want_map=True), "window=None is window = T")


def test_all_zero_and_constant_maps(plan):
    """Nothing is special-cased.  An all-zero map: every value ties, auc is 0.5 * sum a_p; mass_pred is 0.0, so nss, info_gain, cc, jsd
    and kl are 0 / 0 = NaN and sim is the audience's own total (fmin drops the NaN): the oracle's expressions give the same.  A
    constant map on 4 x 2 cells, where every a_p is exactly 0.125: mass_pred is the constant, var_pred 0.0, nss and cc NaN, info_gain
    log2(1) = 0, in the library's order of summation as in numpy's"""
    _, _, ids = g15()
    zero = np.zeros((18, 36))
    res = plan.saliency_score(ids=ids, maps=zero, window=5, stride=5)
    check(res, ids, zero, 5.0, 5, 5, "an all-zero map")
    # 0.5 up to the rounding of sum a_p (648 terms near 1 / 648) and of the mean over at most 40 list entries: 1e-14
    assert np.abs(res["stats"][0] - 0.5).max() <= 1e-14 and (res["stats"][8] == 0.0).all() and np.isnan(res["stats"][[1, 2, 3, 5, 6]]).all()
    const = np.full((2, 4), 3.0)
    res = plan.saliency_score(ids=ids, maps=const, window=5, stride=5)
    check(res, ids, const, 5.0, 5, 5, "a constant map")
    assert np.abs(res["stats"][0] - 0.5).max() <= 1e-15 and (res["stats"][8] == 3.0).all() and (res["stats"][2] == 0.0).all()
    assert np.isnan(res["stats"][[1, 3]]).all() and np.isfinite(res["stats"][[4, 5, 6, 7]]).all()
    wide = plan.saliency_score(ids=ids, maps=np.full((18, 36), 0.25), window=5, stride=5, distribution=False)
    assert np.abs(wide["stats"][0] - 0.5).max() <= 1e-14 and np.abs(wide["stats"][2]).max() <= 1e-14


# ------------------------------------------------------------------------------------------- 4. bit invariance
def test_bits_do_not_depend_on_stride_length_entry_outputs_or_column_order(engine, plan):
    import torch
    mu_long, mv_long, ids_long = g15()
    T, U = 25, 8
    mu, mv, ids = mu_long[:T], mv_long[:T], ids_long[:T]
    per_row = np.ascontiguousarray(g15_map(37, 19, 5.0, 13, 56))    # one map per row of the long video at stride 1
    for maps_long, what in ((per_row, "per-row"), (g15_map(37, 19, 5.0, 13), "static")):
        static = maps_long.ndim == 2
        cut = (lambda sel: maps_long) if static else (lambda sel: np.ascontiguousarray(maps_long[sel]))
        kw = dict(window=5, sigma_deg=5.0, want_map=True)
        s1 = plan.saliency_score(mu=mu, mv=mv, maps=cut(slice(0, 21)), stride=1, **kw)
        s5 = plan.saliency_score(mu=mu, mv=mv, maps=cut(slice(0, 21, 5)), stride=5, **kw)
        same_bytes(take_rows(s1, slice(0, None, 5)), s5, f"{what}: stride 1 against stride 5")
        long = plan.saliency_score(mu=mu_long, mv=mv_long, maps=cut(slice(0, 56)), stride=1, **kw)      # the rows wholly inside the prefix
        same_bytes(take_rows(long, slice(0, 21)), s1, f"{what}: a prefix of the video")
        few = plan.saliency_score(mu=mu[3:9], mv=mv[3:9], maps=cut(slice(3, 5)), stride=1, **kw)       # two rows of the same frames
        same_bytes(few, take_rows(s1, slice(3, 5)), f"{what}: the number of rows")
        maps = cut(slice(0, 21))
        same_bytes(plan.saliency_score(ids=ids, maps=maps, stride=1, **kw), s1, f"{what}: ids against (mu, mv)")
        same_bytes(plan.saliency_score(ids=ids, maps=maps, stride=1, **dict(kw, want_map=False)), s1, f"{what}: without the map")
        loc = plan.saliency_score(ids=ids, maps=maps, stride=1, **dict(kw, distribution=False))        # the map is still built when asked for
        assert loc["stats"][LOC].tobytes() == s1["stats"][LOC].tobytes() and np.isnan(loc["stats"][3:8]).all(), what
        assert loc["map"].tobytes() == s1["map"].tobytes() and loc["counts"].tobytes() == s1["counts"].tobytes(), what
        bare = plan.saliency_score(ids=ids, maps=maps, stride=1, **dict(kw, distribution=False, want_map=False))
        assert bare["map"] is None and bare["stats"].tobytes() == loc["stats"].tobytes(), what
        perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
        same_bytes(plan.saliency_score(ids=np.ascontiguousarray(ids[:, perm]), maps=maps, stride=1, **kw), s1, f"{what}: a permutation of the viewers")
        more = np.concatenate([ids, np.full((T, 1), -1, dtype=np.int32)], axis=1)
        same_bytes(plan.saliency_score(ids=np.ascontiguousarray(more), maps=maps, stride=1, **kw), s1, f"{what}: an all-absent column")
        if static:
            copies = np.ascontiguousarray(np.broadcast_to(maps, (21,) + maps.shape))
            same_bytes(plan.saliency_score(ids=ids, maps=copies, stride=1, **kw), s1, "a static map against R copies of it")
        for k in (-20, 20):                                       # everything but mass_pred, which scales exactly
            sc = plan.saliency_score(ids=ids, maps=maps * 2.0 ** k, stride=1, **kw)
            assert sc["stats"][:8].tobytes() == s1["stats"][:8].tobytes() and sc["map"].tobytes() == s1["map"].tobytes(), (what, k)
            assert sc["stats"][8].tobytes() == (s1["stats"][8] * 2.0 ** k).tobytes(), (what, k)
        try:
            for tile in (3, 100, 0):
                engine.test_saliency_tile(tile)
                same_bytes(plan.saliency_score(ids=ids, maps=maps, stride=1, **kw), s1, f"{what}: tiles of {tile}")
        finally:
            engine.test_saliency_tile(0)
        # the device entries, every output and one output at a time, with and without the distribution metrics
        dev = torch.device("cuda", 0)
        d_mu, d_mv, d_ids = (torch.from_numpy(np.array(a)).to(dev) for a in (mu, mv, ids))
        n_empty = int((s1["counts"][0] == 0).sum())
        for src in ("mu_mv", "ids"):
            samples = dict(d_ids=d_ids.data_ptr()) if src == "ids" else dict(d_mu=d_mu.data_ptr(), d_mv=d_mv.data_ptr())
            for wanted in (KEYS, ("map",), ("stats",), ("counts",), ("stats", "counts"), ()):
                got, status = device_call(plan, maps, U, T, 5, 1, 5.0, wanted, **samples)
                for k, b in got.items():
                    assert b.tobytes() == s1[k].tobytes(), (what, src, wanted, k)
                assert status == [0, n_empty], (what, src, wanted)
            got, status = device_call(plan, maps, U, T, 5, 1, 5.0, ("stats",), distribution=False, **samples)
            assert got["stats"].tobytes() == loc["stats"].tobytes() and status == [0, n_empty], (what, src)


def test_passes_do_not_change_a_bit(plan):
    """A 1024 x 512 map is 4 MB: per-row maps, location only, keep one sorted copy per row of a pass, so a pass holds 63 rows under the
    256 MB budget and 70 rows take two passes; the rows on both sides of the seam keep the bytes they have in calls of their own"""
    rng = np.random.default_rng(9)
    ids = rng.integers(0, 101 * 201, size=(70, 3)).astype(np.int32)
    maps = rng.uniform(0.5, 1.5, size=(70, 512, 1024))
    res = plan.saliency_score(ids=ids, maps=maps, window=1, distribution=False)
    assert res["map"] is None and (res["counts"][0] == 3).all() and not np.isnan(res["stats"][LOC]).any() and np.isnan(res["stats"][3:8]).all()
    assert ((res["stats"][0] > 0) & (res["stats"][0] < 1)).all()
    np.testing.assert_allclose(res["stats"][8], 1.0, rtol=1e-2)
    for r in (0, 61, 62, 63, 64, 69):
        one = plan.saliency_score(ids=ids[r:r + 1], maps=maps[r:r + 1], window=1, distribution=False)
        same_bytes(take_rows(res, slice(r, r + 1)), one, f"row {r}", keys=("stats", "counts"))


# ------------------------------------------------------------------------------------------- 5. against merged code
def test_against_the_saliency_and_similarity_calls(plan):
    _, _, ids = g15()
    halves = np.array([0, 0, 0, 0, 1, 1, 1, 1], dtype=np.int8)
    for window, stride, mw, mh, sigma in ((5, 5, 37, 19, 5.0), (1, 1, 36, 18, 5.0), (None, 1, 50, 25, 2.0)):
        kw = dict(window=window, stride=stride, sigma_deg=sigma)
        own = plan.saliency(ids=ids, width=mw, height=mh, scale="density", **kw)
        res = plan.saliency_score(ids=ids, maps=g15_map(mw, mh, sigma, 5), want_map=True, **kw)
        assert res["map"].tobytes() == own["map"].tobytes() and res["stats"][7].tobytes() == own["stats"][0].tobytes()
        assert np.array_equal(res["counts"], own["counts"])
        # the audience's own maps as the prediction
        me = plan.saliency_score(ids=ids, maps=own["map"], **kw)
        ok = me["counts"][0] > 0
        assert ok.sum() >= 1 and np.isnan(me["stats"][:8, ~ok]).all()
        jsd, kl = me["stats"][5][ok], me["stats"][6][ok]
        assert (jsd == 0.0).all() and not np.signbit(jsd).any() and (kl == 0.0).all()
        assert np.abs(me["stats"][3][ok] - 1.0).max() <= 1e-14 and np.abs(me["stats"][4][ok] - 1.0).max() <= 1e-14
        assert me["stats"][7][ok].tobytes() == me["stats"][8][ok].tobytes()
        # audience A scored by audience B's maps: the similarity call's cc, sim, jsd and kl_ab
        sim = plan.saliency_similarity(ids=ids, groups=halves, width=mw, height=mh, want_maps=True, **kw)
        both = (sim["counts"][0] > 0) & (sim["counts"][1] > 0)
        ab = plan.saliency_score(ids=sso.masked(ids, halves, 0), maps=sim["maps"][1], **kw)
        assert both.sum() >= 1
        np.testing.assert_allclose(ab["stats"][3:7][:, both], sim["stats"][:4][:, both], rtol=1e-12, atol=1e-12)
        assert ab["stats"][7][both].tobytes() == sim["stats"][7][both].tobytes() and ab["stats"][8][both].tobytes() == sim["stats"][8][both].tobytes()
        fin = np.isfinite(sim["stats"][:4][:, both])
        print("against the similarity call", mw, mh, "largest difference",
              float(np.abs(ab["stats"][3:7][:, both][fin] - sim["stats"][:4][:, both][fin]).max(initial=0.0)))


# ------------------------------------------------------------------------------------------- 6. refusals and the range error
def test_illegal_arguments_are_refused_before_anything_runs(native, plan):
    mu, mv, _ = g15()
    mu, mv = np.ascontiguousarray(mu[:30, :4]), np.ascontiguousarray(mv[:30, :4])
    lib = native.load_library()
    stats = np.empty((9, 64))
    pred = noise_map(36, 18, 1, 26)
    good = dict(window=5, stride=1, sigma=0.1, W=36, H=18, pred=pred, n_pred=26)
    bad = [dict(window=0), dict(window=31), dict(stride=0), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")),
           dict(sigma=float("inf")), dict(sigma=3.2), dict(W=1), dict(W=4097), dict(H=0), dict(H=2049), dict(pred=None),
           dict(n_pred=0), dict(n_pred=2), dict(n_pred=25), dict(n_pred=27), dict(n_pred=-1)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.vet_saliency_score_host(plan.handle, native._ptr(mu), native._ptr(mv), None, 4, 30, a["window"], a["stride"], a["sigma"],
                                         a["W"], a["H"], native._ptr(a["pred"]), a["n_pred"], 1, None, native._ptr(stats), None)
        assert rc == native.VET_ERR_INVALID, change
    for n_pred in (1, 26):
        rc = lib.vet_saliency_score_host(plan.handle, native._ptr(mu), native._ptr(mv), None, 4, 30, 5, 1, 0.1, 36, 18, native._ptr(pred),
                                         n_pred, 0, None, native._ptr(stats), None)
        assert rc == native.VET_OK
    with pytest.raises(native.NativeError) as err:                # the device entries refuse before they look at a pointer
        plan.saliency_score_device(8, 8, 4, 30, 31, 1, 8, 1, 36, 18, d_stats=8)
    assert err.value.code == native.VET_ERR_INVALID
    for kw in (dict(d_pred=0), dict(n_pred=2)):
        with pytest.raises(native.NativeError) as err:
            plan.saliency_score_device(8, 8, 4, 30, 5, 1, **dict(dict(d_pred=8, n_pred=1, width=36, height=18), **kw), d_stats=8)
        assert err.value.code == native.VET_ERR_INVALID
    for kw in (dict(window=31), dict(sigma_deg=0.0), dict(sigma_deg=181.0), dict(maps=pred[:3]), dict(maps=pred.astype(np.float32)),
               dict(maps=-pred[0]), dict(maps=np.ones((18, 1)))):
        with pytest.raises(ValueError):
            plan.saliency_score(**dict(dict(mu=mu, mv=mv, maps=pred[0], window=5), **kw))
    assert plan.saliency_score(mu=mu, mv=mv, maps=pred[0], window=30)["stats"].shape == (9, 1)


def test_sample_out_of_range(native, plan):
    mu, mv, _ = g15()
    mu, mv = np.array(mu[:20]), np.array(mv[:20])
    mu[np.isnan(mu)] = 0.5
    mv[np.isnan(mv)] = 0.5
    kw = dict(maps=g15_map(36, 18, 5.0, 5), window=5, want_map=True)
    bad_mu, gone_mu, gone_mv = mu.copy(), mu.copy(), mv.copy()
    bad_mu[19, 2] = 1.5
    gone_mu[19, 2] = gone_mv[19, 2] = np.nan
    with pytest.raises(native.NativeError) as e:
        plan.saliency_score(mu=bad_mu, mv=mv, **kw)
    assert e.value.code == native.VET_ERR_RANGE
    res = plan.saliency_score(mu=bad_mu, mv=mv, check=False, **kw)
    assert res["code"] == native.VET_ERR_RANGE                    # the outputs are still written: the sample counts as absent
    same_bytes(res, plan.saliency_score(mu=gone_mu, mv=gone_mv, **kw), "range")


# ------------------------------------------------------------------------------------------- 7. the analyzers
def test_analyzers_return_the_oracle_columns():
    from viewport_entropy_toolkit import SpatialEntropyAnalyzer, TransitionEntropyAnalyzer
    from viewport_entropy_toolkit.analyzers import NaiveSpatialEntropyAnalyzer
    from viewport_entropy_toolkit.config import AnalyzerConfig, NaiveAnalyzerConfig
    mu, mv, ids = g15()
    times = np.arange(60) / 30.0
    maps = np.ascontiguousarray(g15_map(36, 18, 5.0, 7, 56)[::5])
    frames = []
    for cls in (SpatialEntropyAnalyzer, NaiveSpatialEntropyAnalyzer, TransitionEntropyAnalyzer):
        an = cls(NaiveAnalyzerConfig(tile_height=10, tile_width=20, video_width=W, video_height=H)) \
            if cls is NaiveSpatialEntropyAnalyzer else cls(AnalyzerConfig(tile_counts=[20], video_width=W, video_height=H))
        an.load_arrays(times, mu.copy(), mv.copy())
        frames.append(an.compute_saliency_score(maps, window=5, stride=5, sigma_deg=5.0, keep_maps=True))
        plain = an.compute_saliency_score(maps, window=5, stride=5)
        assert "map" not in plain.columns and plain["auc"].to_numpy().tobytes() == frames[-1]["auc"].to_numpy().tobytes()
        loc = an.compute_saliency_score(maps, window=5, stride=5, distribution=False)
        assert loc["nss"].to_numpy().tobytes() == plain["nss"].to_numpy().tobytes() and loc["cc"].isna().all() and not loc.attrs["distribution"]
        whole = an.compute_saliency_score(maps[0], window=None)
        assert len(whole) == 1 and whole["time_end"][0] == times[-1] and whole.attrs["window"] == 60 and whole.attrs["static"]
    df = frames[0]
    cols = ["time", "time_end", "samples", "distinct"] + list(sco.STATS) + ["map"]
    assert list(df.columns) == cols
    for other in frames[1:]:                                     # the call is lattice-independent: three analyzers, the same values
        for c in cols:
            a, b = (np.stack(list(f[c])) if c == "map" else f[c].to_numpy() for f in (df, other))
            assert a.tobytes() == b.tobytes(), c
    res = dict(code=0, map=np.stack(list(df["map"])), stats=np.stack([df[c].to_numpy() for c in sco.STATS]),
               counts=np.stack([df[c].to_numpy() for c in ("samples", "distinct")]).astype(np.int64))
    check(res, ids, maps, 5.0, 5, 5, "the analyzers' DataFrame")
    base = df["map"][0].base
    assert base is not None and all(np.shares_memory(m, base) for m in df["map"]) and df["map"][0].shape == (18, 36)      # views, no copy
    assert df.attrs["sigma_deg"] == 5.0 and df.attrs["width"] == 36 and df.attrs["height"] == 18 and df.attrs["kappa"] == 1.0 / rad(5.0) ** 2
    assert df.attrs["window"] == 5 and df.attrs["stride"] == 5 and len(df.attrs["users"]) == 8
    assert df.attrs["static"] is False and df.attrs["distribution"] is True
    assert df["time"].tolist() == times[0::5][:len(df)].tolist() and df["time_end"].tolist() == times[4::5][:len(df)].tolist()
