"""GPU: the saliency similarity of two audiences through the C-ABI (Plan.saliency_similarity -> vet_saliency_similarity_host, the
device entries through Plan.saliency_similarity_device, the analyzers' compute_saliency_similarity).  The reference is the numpy
oracle of tests/_saliency_similarity_oracle.py (written from the definition in include/vet.h on top of the saliency oracle, whose
directions and fused dot golden G27 pins against the real reference) — never the code under test.

Tolerances.  Counts and status words: equality; +inf, -inf and NaN in the same places.  The maps: the saliency suite's rtol 1e-12,
atol 2**-1000.  Finite values: 1e-10 — absolute for ``cc``, ``sim`` and ``jsd``, 1e-10 relative + 1e-10 absolute for ``kl_*``,
``nss_*`` and ``mass_*`` — the saliency suite's tolerance for its log2 sums; a numpy prototype of these metrics on these inputs
agrees with its own longdouble evaluation to 6e-14.  The tests print the largest deviations they saw.

Largest deviations seen on an MI355X over all tests of this file: cc 6.7e-16, sim 3.3e-16, jsd 4.4e-16 absolute; kl 7.6e-16,
nss 8.7e-15, mass 3.8e-17 relative to 1 + |value|."""
import functools

import numpy as np
import pytest

from tests import _saliency_oracle as so
from tests import _saliency_similarity_oracle as sso

pytestmark = pytest.mark.gpu

W, H = 100, 200
KEYS = ("maps", "stats", "counts")
ABS = (0, 1, 2)                  # cc, sim, jsd: absolute 1e-10
# (map width, map height, sigma in degrees, window): 648, 162, 703 and 1250 pixels — partial workgroups, an odd width, and a map that
# crosses the 1024-pixel block of the summation rule
SETTINGS = [(36, 18, 5.0, 5), (36, 18, 2.0, 1), (18, 9, 10.0, 60), (37, 19, 1.0, 5), (50, 25, 5.0, 20)]
HALVES = np.array([0, 0, 0, 0, 1, 1, 1, 1], dtype=np.int8)


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
    return sso.Oracle(grid(), mw, mh)


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


def check(res, ids, code, mw, mh, sigma_deg, window, stride, msg, only=None):
    """a result dict against the oracle at the module's tolerances; returns the oracle's rows"""
    T, U = ids.shape
    w = T if window is None else window
    R = (T - w) // stride + 1
    assert res["code"] == 0 and res["stats"].shape == (9, R) and res["counts"].shape == (4, R), msg
    assert res["stats"].dtype == np.float64 and res["counts"].dtype == np.int64, msg
    assert res["maps"] is None or res["maps"].shape == (2, R, mh, mw), msg
    want = oracle(mw, mh).rows(ids, code, w, stride, rad(sigma_deg), only=only)
    rs = np.arange(R) if only is None else np.asarray(only)
    stats, counts = res["stats"][:, rs], res["counts"][:, rs]
    assert np.array_equal(counts, want["counts"]), msg
    empty = (counts[0] == 0) | (counts[1] == 0)
    assert np.isnan(stats[:7, empty]).all() and not np.isnan(stats[:7, ~empty]).any(), msg
    assert np.array_equal(np.isnan(stats[7]), counts[0] == 0) and np.array_equal(np.isnan(stats[8]), counts[1] == 0), msg
    assert np.array_equal(np.isnan(stats), np.isnan(want["stats"])), msg
    assert np.array_equal(np.isposinf(stats), np.isposinf(want["stats"])), msg
    assert np.array_equal(np.isneginf(stats), np.isneginf(want["stats"])), msg
    dev = {}
    for k, name in enumerate(sso.STATS):
        fin = np.isfinite(want["stats"][k])
        d = np.abs(stats[k][fin] - want["stats"][k][fin])
        if k not in ABS:
            d = d / (1.0 + np.abs(want["stats"][k][fin]))
        dev[name] = float(d.max(initial=0.0))
    print(msg, "largest deviations (cc, sim, jsd absolute; the others over 1 + |value|)", dev,
          "inf:", int(np.isinf(stats).sum()), "largest |value|", float(np.abs(stats[np.isfinite(stats)]).max(initial=0.0)))
    for k, name in enumerate(sso.STATS):
        fin = np.isfinite(want["stats"][k])
        np.testing.assert_allclose(stats[k][fin], want["stats"][k][fin], rtol=0 if k in ABS else 1e-10, atol=1e-10, err_msg=f"{msg} {name}")
    if res["maps"] is not None:
        np.testing.assert_allclose(res["maps"][:, rs], want["maps"], rtol=1e-12, atol=2.0 ** -1000, err_msg=msg + " maps")
    return want


def same_bytes(a, b, msg, keys=KEYS):
    for key in keys:
        if a[key] is None or b[key] is None:
            continue
        assert a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), (msg, key)


def take_rows(res, sel):
    """the rows ``sel`` (a slice) of a result dict, contiguous"""
    return {key: None if res[key] is None else np.ascontiguousarray(res[key][:, sel]) for key in KEYS}


def device_call(plan, code, U, T, window, stride, sigma, mw, mh, wanted, d_mu=0, d_mv=0, d_ids=0):
    """the device entry into fresh buffers: (dict of numpy results for ``wanted``, status [2])"""
    import torch
    dev = torch.device("cuda", 0)
    R = (T - window) // stride + 1
    shapes = dict(maps=((2, R, mh, mw), torch.float64), stats=((9, R), torch.float64), counts=((4, R), torch.int64))
    bufs = {k: torch.full(shapes[k][0], -7, dtype=shapes[k][1], device=dev) for k in wanted}
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    plan.saliency_similarity_device(d_mu, d_mv, U, T, window, stride, code, sigma, mw, mh, d_status=status.data_ptr(), d_ids=d_ids,
                                    **{"d_" + k: b.data_ptr() for k, b in bufs.items()})
    torch.cuda.synchronize()
    return {k: b.cpu().numpy() for k, b in bufs.items()}, status.cpu().tolist()


# ------------------------------------------------------------------------------------------- 1. the numpy oracle
@pytest.mark.parametrize("mw,mh,sigma,window", SETTINGS)
def test_vs_oracle(plan, mw, mh, sigma, window):
    import torch
    mu, mv, ids = g15()
    for n, stride in enumerate((1, 5)):
        kw = dict(ids=ids) if n else dict(mu=mu, mv=mv)          # both entries
        res = plan.saliency_similarity(groups=HALVES, window=window, stride=stride, sigma_deg=sigma, width=mw, height=mh,
                                       want_maps=True, **kw)
        check(res, ids, HALVES, mw, mh, sigma, window, stride, f"{mw}x{mh} sigma={sigma} window={window} stride={stride}")
        if window == 1 and stride == 1:
            # frame 30 of this split has an empty audience: its values are NaN, the other audience keeps its mass and its counts
            c30, s30 = res["counts"][:, 30], res["stats"][:, 30]
            assert (c30[0] == 0) != (c30[1] == 0), c30.tolist()
            g = 0 if c30[0] == 0 else 1                            # the empty audience
            assert np.isnan(s30[:7]).all() and np.isnan(s30[7 + g]) and s30[8 - g] > 0 and c30[2 + g] == 0 and c30[3 - g] > 0
            assert (res["maps"][g, 30] == 0.0).all() and not np.signbit(res["maps"][g, 30]).any()
            n_empty = int(((res["counts"][0] == 0) | (res["counts"][1] == 0)).sum())
            d_ids = torch.from_numpy(np.array(ids)).to(torch.device("cuda", 0))
            got, status = device_call(plan, HALVES, 8, 60, 1, 1, sigma, mw, mh, ("stats", "counts"), d_ids=d_ids.data_ptr())
            assert status == [0, n_empty] and n_empty >= 1
            same_bytes(dict(got, maps=None), res, "the device entry")


# ------------------------------------------------------------------------------------------- 2. the maps are vet_saliency's
@pytest.mark.parametrize("window,stride", [(1, 1), (5, 5), (None, 1)])
def test_maps_masses_and_counts_are_the_saliency_calls_on_masked_ids(plan, window, stride):
    _, _, ids = g15()
    res = plan.saliency_similarity(ids=ids, groups=HALVES, window=window, stride=stride, sigma_deg=5.0, width=37, height=19, want_maps=True)
    for g in (0, 1):
        own = plan.saliency(ids=sso.masked(ids, HALVES, g), window=window, stride=stride, sigma_deg=5.0, width=37, height=19,
                            scale="density")
        assert res["maps"][g].tobytes() == own["map"].tobytes(), (g, "map")
        assert res["stats"][7 + g].tobytes() == own["stats"][0].tobytes(), (g, "mass")
        assert np.array_equal(res["counts"][g], own["counts"][0]) and np.array_equal(res["counts"][2 + g], own["counts"][1]), g


# ------------------------------------------------------------------------------------------- 3. exact identities
def swapped(res):
    """what exchanging the two labels must return, byte for byte"""
    return dict(maps=None if res["maps"] is None else np.ascontiguousarray(res["maps"][::-1]),
                stats=np.ascontiguousarray(res["stats"][[0, 1, 2, 4, 3, 6, 5, 8, 7]]),
                counts=np.ascontiguousarray(res["counts"][[1, 0, 3, 2]]))


@pytest.mark.parametrize("mw,mh,sigma,window", [(36, 18, 5.0, 5), (37, 19, 1.0, 5), (50, 25, 5.0, 20)])
def test_exchanging_the_labels_exchanges_the_values(plan, mw, mh, sigma, window):
    _, _, ids = g15()
    kw = dict(ids=ids, window=window, stride=3, sigma_deg=sigma, width=mw, height=mh, want_maps=True)
    ab = plan.saliency_similarity(groups=HALVES, **kw)
    ba = plan.saliency_similarity(groups=1 - HALVES, **kw)
    same_bytes(ba, swapped(ab), f"labels exchanged {mw}x{mh} sigma={sigma}")
    uneven = np.array([0, 1, 1, -1, 0, 1, 0, 1], dtype=np.int8)
    flipped = np.where(uneven < 0, -1, 1 - uneven).astype(np.int8)
    same_bytes(plan.saliency_similarity(groups=flipped, **kw), swapped(plan.saliency_similarity(groups=uneven, **kw)), "uneven labels")


def test_an_audience_compared_with_its_copy(plan):
    _, _, walk = g15()
    ids = np.ascontiguousarray(np.concatenate([walk[:, :4], walk[:, :4]], axis=1))            # B a column copy of A
    code = HALVES
    for mw, mh, sigma, window in ((36, 18, 5.0, 5), (50, 25, 2.0, 20)):
        res = plan.saliency_similarity(ids=ids, groups=code, window=window, stride=5, sigma_deg=sigma, width=mw, height=mh, want_maps=True)
        ok = res["counts"][0] > 0
        assert ok.sum() >= 8 and np.array_equal(res["counts"][0], res["counts"][1])
        assert res["maps"][0].tobytes() == res["maps"][1].tobytes()
        jsd, kl_ab, kl_ba = res["stats"][2][ok], res["stats"][3][ok], res["stats"][4][ok]
        assert (jsd == 0.0).all() and not np.signbit(jsd).any() and (kl_ab == 0.0).all() and (kl_ba == 0.0).all()
        assert np.abs(res["stats"][0][ok] - 1.0).max() <= 1e-14 and np.abs(res["stats"][1][ok] - 1.0).max() <= 1e-14
        assert res["stats"][5][ok].tobytes() == res["stats"][6][ok].tobytes() and (res["stats"][5][ok] > 0).all()
        assert res["stats"][7].tobytes() == res["stats"][8].tobytes()


# ------------------------------------------------------------------------------------------- 4. edges
def edge_video():
    """ids [20][6] on the 100 x 200 grid: frame 3 with nobody, frame 4 without audience B, pole-row ids that share one Vector,
    repeated ids within and across the audiences, viewer 5 never present"""
    _, _, walk = g15()
    ids = np.array(walk[:20, :6])
    ids[3] = -1
    ids[4, 3:] = -1
    ids[:, 5] = -1
    ids[5] = [3, 90, 60 * 101 + 30, 60 * 101 + 30, 7, -1]            # py = 0: every pixel of the row is the north pole
    ids[6] = [200 * 101 + 7, 200 * 101 + 7, 40 * 101 + 20, 40 * 101 + 20, 200 * 101 + 9, -1]           # the last pixel row
    ids[7, :5] = ids[8, :5] = 77 * 101 + 31                        # ten samples on one pixel: both audiences the same direction
    return ids


def test_edge_rows(plan):
    ids = edge_video()
    code = np.array([0, 0, 0, 1, 1, 1], dtype=np.int8)
    for window, stride in ((1, 1), (2, 1), (4, 3), (None, 1)):
        res = plan.saliency_similarity(ids=ids, groups=code, window=window, stride=stride, sigma_deg=5.0, width=36, height=18, want_maps=True)
        check(res, ids, code, 36, 18, 5.0, window, stride, f"edge rows window={window}")
        if window == 1:
            assert res["counts"][:, 3].tolist() == [0, 0, 0, 0] and np.isnan(res["stats"][:, 3]).all()        # both audiences empty
            assert res["counts"][:, 4].tolist()[1::2] == [0, 0] and res["counts"][0, 4] > 0 and np.isnan(res["stats"][:7, 4]).all()
            assert not np.isnan(res["stats"][7, 4]) and np.isnan(res["stats"][8, 4])
            assert res["counts"][:, 5].tolist() == [3, 2, 3, 2] and res["counts"][:, 6].tolist() == [3, 2, 2, 2]
            assert res["counts"][:, 7].tolist() == [3, 2, 1, 1]
            # the same direction three times against twice: one density up to the rounding of (3 k) * (C / 3) against (2 k) * (C / 2)
            assert np.abs(res["stats"][2:5, 7]).max() <= 1e-13 and abs(res["stats"][0, 7] - 1.0) <= 1e-13 and abs(res["stats"][1, 7] - 1.0) <= 1e-13
    whole = plan.saliency_similarity(ids=ids, groups=code, window=None, sigma_deg=5.0, width=36, height=18, want_maps=True)
    same_bytes(whole, plan.saliency_similarity(ids=ids, groups=code, window=20, sigma_deg=5.0, width=36, height=18, want_maps=True),
               "window=None is window = T")


def test_excluded_viewers_and_an_audience_of_one(plan):
    _, _, walk = g15()
    code = np.array([0, -1, 1, 0, -1, 1, 1, 0], dtype=np.int8)
    kw = dict(groups=code, window=5, stride=5, sigma_deg=5.0, width=36, height=18, want_maps=True)
    res = plan.saliency_similarity(ids=walk, **kw)
    check(res, walk, code, 36, 18, 5.0, 5, 5, "two viewers excluded")
    other = np.array(walk)
    rng = np.random.default_rng(4)
    other[:, code < 0] = rng.integers(-1, 101 * 201, size=(60, 2))                 # the excluded viewers look elsewhere, or away
    same_bytes(plan.saliency_similarity(ids=other, **kw), res, "the excluded viewers' samples")
    one = np.array([-1, -1, 1, 0, -1, -1, -1, -1], dtype=np.int8)                 # one viewer against one viewer
    for window in (1, 5, None):
        r = plan.saliency_similarity(ids=walk, groups=one, window=window, sigma_deg=5.0, width=36, height=18, want_maps=True)
        check(r, walk, one, 36, 18, 5.0, window, 1, f"one viewer each, window={window}")
    lone = np.array([0, 1, 1, 1, 1, 1, 1, 1], dtype=np.int8)                       # one viewer against the rest
    check(plan.saliency_similarity(ids=walk, groups=lone, window=5, stride=5, sigma_deg=5.0, width=36, height=18), walk, lone, 36, 18,
          5.0, 5, 5, "one viewer against seven")


# ------------------------------------------------------------------------------------------- 5. list seams of the points kernel
def test_lists_beyond_a_workgroup_a_block_and_an_lds_tile(engine, plan):
    """40 viewers x 70 frames, uniform on the sphere, 20 per audience, the whole video: about 1 350 distinct directions per audience —
    six workgroups per list in k_saliency_points, two 1024-blocks of the rule over the v_i, two LDS tiles of the other list"""
    mu, mv, ids = sphere(40, 70, 11)
    code = (np.arange(40) % 2).astype(np.int8)
    kw = dict(groups=code, window=70, sigma_deg=10.0, width=18, height=9, want_maps=True)
    res = plan.saliency_similarity(mu=mu, mv=mv, **kw)
    check(res, ids, code, 18, 9, 10.0, 70, 1, "40 x 70 whole video")
    assert (res["counts"][:2, 0] == 1400).all() and (res["counts"][2:, 0] > 1024).all() and (res["counts"][2:, 0] <= 1400).all()
    try:
        for tile in (3, 100, 0):
            engine.test_saliency_tile(tile)
            same_bytes(plan.saliency_similarity(ids=ids, **kw), res, f"tiles of {tile}")
    finally:
        engine.test_saliency_tile(0)


# ------------------------------------------------------------------------------------------- 6. the long-row path
def test_long_rows_take_the_counting_path(plan):
    """70 viewers x 64 frames: a row of 64 frames has 4 480 positions, beyond the 4 096 of the LDS sort.  With the last six frames
    empty, a row of 58 frames (4 060 positions: sorted) and the row of 64 frames (counted) hold the same lists: the same bytes"""
    mu, mv, ids = sphere(70, 64, 12)
    code = (np.arange(70) % 2).astype(np.int8)
    kw = dict(groups=code, sigma_deg=10.0, width=18, height=9, want_maps=True)
    res = plan.saliency_similarity(mu=mu, mv=mv, window=64, **kw)
    check(res, ids, code, 18, 9, 10.0, 64, 1, "70 x 64 whole video")
    assert res["counts"][:2, 0].sum() == 4480 and (res["counts"][2:, 0] > 2000).all()
    gone = np.array(ids)
    gone[58:] = -1
    a = plan.saliency_similarity(ids=gone, window=58, stride=6, **kw)
    b = plan.saliency_similarity(ids=gone, window=64, **kw)
    assert a["stats"].shape == (9, 2)
    same_bytes(take_rows(a, slice(0, 1)), b, "sorted against counted lists")


# ------------------------------------------------------------------------------------------- 7. pass seams
def test_passes_do_not_change_a_bit(plan):
    """A 1024 x 512 map is 4 MB: with two maps per row and without d_maps a pass holds 31 rows under the 256 MB budget, so 70 rows take
    three passes (rows 0-30, 31-61, 62-69); the rows on both sides of each seam keep the bytes they have in calls of their own.  The
    mass: the midpoint rule on cells of 0.35 degrees under a kernel of sigma 3 degrees is within h^2 / (24 sigma^2) = 6e-4 of the
    integral, 4 pi * mass = 1."""
    rng = np.random.default_rng(9)
    ids = rng.integers(0, 101 * 201, size=(70, 3)).astype(np.int32)
    code = np.array([0, 1, 0], dtype=np.int8)
    kw = dict(groups=code, window=1, sigma_deg=3.0, width=1024, height=512)
    res = plan.saliency_similarity(ids=ids, **kw)
    assert res["maps"] is None and (res["counts"][0] == 2).all() and (res["counts"][1] == 1).all() and not np.isnan(res["stats"]).any()
    for r in (0, 30, 31, 61, 62, 69):
        one = plan.saliency_similarity(ids=ids[r:r + 1], **kw)
        same_bytes(take_rows(res, slice(r, r + 1)), one, f"row {r}", keys=("stats", "counts"))
    np.testing.assert_allclose(4.0 * np.pi * res["stats"][7:], 1.0, rtol=1e-3)
    full = plan.saliency_similarity(ids=ids[30:32], want_maps=True, **kw)                  # with the maps
    same_bytes(take_rows(res, slice(30, 32)), full, "with d_maps", keys=("stats", "counts"))


# ------------------------------------------------------------------------------------------- 8. bit invariance
def test_bits_do_not_depend_on_stride_length_entry_outputs_or_column_order(plan):
    import torch
    mu_long, mv_long, ids_long = g15()
    T, U = 25, 8
    mu, mv, ids = mu_long[:T], mv_long[:T], ids_long[:T]
    code = np.array([0, 1, 1, 0, -1, 1, 0, 0], dtype=np.int8)
    kw = dict(groups=code, window=5, sigma_deg=5.0, width=37, height=19, want_maps=True)
    s1 = plan.saliency_similarity(mu=mu, mv=mv, stride=1, **kw)
    s5 = plan.saliency_similarity(mu=mu, mv=mv, stride=5, **kw)
    same_bytes(take_rows(s1, slice(0, None, 5)), s5, "stride 1 against stride 5")
    long = plan.saliency_similarity(mu=mu_long, mv=mv_long, stride=1, **kw)             # the rows wholly inside the prefix
    same_bytes(take_rows(long, slice(0, T - 5 + 1)), s1, "a prefix of the video")
    few = plan.saliency_similarity(mu=mu[3:9], mv=mv[3:9], stride=1, **kw)              # two rows of the same frames
    same_bytes(few, take_rows(s1, slice(3, 5)), "the number of rows")
    same_bytes(plan.saliency_similarity(ids=ids, stride=1, **kw), s1, "ids against (mu, mv)")
    same_bytes(plan.saliency_similarity(ids=ids, stride=1, **dict(kw, want_maps=False)), s1, "without the maps")
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])                   # the viewer columns permuted together with their labels
    same_bytes(plan.saliency_similarity(ids=np.ascontiguousarray(ids[:, perm]), stride=1, **dict(kw, groups=code[perm])), s1,
               "a permutation of the viewers")
    # the device entries, every output and one output at a time
    dev = torch.device("cuda", 0)
    d_mu, d_mv, d_ids = (torch.from_numpy(np.array(a)).to(dev) for a in (mu, mv, ids))
    n_empty = int(((s1["counts"][0] == 0) | (s1["counts"][1] == 0)).sum())
    for src in ("mu_mv", "ids"):
        samples = dict(d_ids=d_ids.data_ptr()) if src == "ids" else dict(d_mu=d_mu.data_ptr(), d_mv=d_mv.data_ptr())
        for wanted in (KEYS, ("maps",), ("stats",), ("counts",), ("stats", "counts"), ()):
            got, status = device_call(plan, code, U, T, 5, 1, 5.0, 37, 19, wanted, **samples)
            for k, b in got.items():
                assert b.tobytes() == s1[k].tobytes(), (src, wanted, k)
            assert status == [0, n_empty], (src, wanted)


# ------------------------------------------------------------------------------------------- 9. refusals and the range error
def test_illegal_arguments_are_refused_before_anything_runs(native, plan):
    mu, mv, _ = g15()
    mu, mv = np.ascontiguousarray(mu[:30, :4]), np.ascontiguousarray(mv[:30, :4])
    lib = native.load_library()
    stats = np.empty((9, 64))
    ok_groups = np.array([0, 1, -1, 0], dtype=np.int8)
    good = dict(window=5, stride=1, groups=ok_groups, sigma=0.1, W=36, H=18)
    bad = [dict(window=0), dict(window=31), dict(stride=0), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")),
           dict(sigma=float("inf")), dict(sigma=3.2), dict(W=1), dict(W=4097), dict(H=0), dict(H=2049), dict(groups=None),
           dict(groups=np.array([0, 0, -1, 0], dtype=np.int8)), dict(groups=np.array([1, 1, 1, 2], dtype=np.int8)),
           dict(groups=np.array([-1, 2, 3, 4], dtype=np.int8))]
    for change in bad:
        a = dict(good, **change)
        rc = lib.vet_saliency_similarity_host(plan.handle, native._ptr(mu), native._ptr(mv), None, 4, 30, a["window"], a["stride"],
                                              native._ptr(a["groups"]), a["sigma"], a["W"], a["H"], None, native._ptr(stats), None)
        assert rc == native.VET_ERR_INVALID, change
    other = np.array([0, 5, 1, -3], dtype=np.int8)               # any other value is an excluded viewer
    rc = lib.vet_saliency_similarity_host(plan.handle, native._ptr(mu), native._ptr(mv), None, 4, 30, 5, 1, native._ptr(other), 0.1, 36, 18,
                                          None, native._ptr(stats), None)
    assert rc == native.VET_OK
    with pytest.raises(native.NativeError) as err:                # the device entry refuses before it looks at a pointer
        plan.saliency_similarity_device(8, 8, 4, 30, 31, 1, ok_groups, d_stats=8)
    assert err.value.code == native.VET_ERR_INVALID
    for kw in (dict(window=31), dict(sigma_deg=0.0), dict(sigma_deg=181.0), dict(width=1), dict(height=2049), dict(groups=[0, 0, 0, 0]),
               dict(groups=[0, 1, 0])):
        with pytest.raises(ValueError):
            plan.saliency_similarity(**dict(dict(mu=mu, mv=mv, groups=ok_groups), **kw))
    assert plan.saliency_similarity(mu=mu, mv=mv, groups=ok_groups, window=30, width=36, height=18)["stats"].shape == (9, 1)


def test_sample_out_of_range(native, plan):
    mu, mv, _ = g15()
    mu, mv = np.array(mu[:20]), np.array(mv[:20])
    mu[np.isnan(mu)] = 0.5
    mv[np.isnan(mv)] = 0.5
    code = np.array([0, 1, 1, -1, 0, 1, 0, 0], dtype=np.int8)
    kw = dict(groups=code, window=5, width=36, height=18, want_maps=True)
    for u in (2, 3):                                             # a viewer of audience B, and an excluded one: stage 0 sees both
        bad_mu, gone_mu, gone_mv = mu.copy(), mu.copy(), mv.copy()
        bad_mu[19, u] = 1.5
        gone_mu[19, u] = gone_mv[19, u] = np.nan
        with pytest.raises(native.NativeError) as e:
            plan.saliency_similarity(mu=bad_mu, mv=mv, **kw)
        assert e.value.code == native.VET_ERR_RANGE
        res = plan.saliency_similarity(mu=bad_mu, mv=mv, check=False, **kw)
        assert res["code"] == native.VET_ERR_RANGE                # the outputs are still written: the sample counts as absent
        same_bytes(res, plan.saliency_similarity(mu=gone_mu, mv=gone_mv, **kw), f"range, viewer {u}")


# ------------------------------------------------------------------------------------------- 10. the analyzers
def test_analyzers_return_the_oracle_columns():
    from viewport_entropy_toolkit import SpatialEntropyAnalyzer, TransitionEntropyAnalyzer
    from viewport_entropy_toolkit.analyzers import NaiveSpatialEntropyAnalyzer
    from viewport_entropy_toolkit.config import AnalyzerConfig, NaiveAnalyzerConfig
    mu, mv, ids = g15()
    times = np.arange(60) / 30.0
    labels = ["hmd", "screen", "screen", None, "hmd", "screen", "hmd", float("nan")]
    code = np.array([0, 1, 1, -1, 0, 1, 0, -1], dtype=np.int8)
    frames = []
    for cls in (SpatialEntropyAnalyzer, NaiveSpatialEntropyAnalyzer, TransitionEntropyAnalyzer):
        an = cls(NaiveAnalyzerConfig(tile_height=10, tile_width=20, video_width=W, video_height=H)) \
            if cls is NaiveSpatialEntropyAnalyzer else cls(AnalyzerConfig(tile_counts=[20], video_width=W, video_height=H))
        an.load_arrays(times, mu.copy(), mv.copy())
        frames.append(an.compute_saliency_similarity(labels, window=5, stride=5, sigma_deg=5.0, width=36, height=18, keep_maps=True))
        plain = an.compute_saliency_similarity(labels, window=5, stride=5, width=36, height=18)
        assert "map_a" not in plain.columns and plain["cc"].to_numpy().tobytes() == frames[-1]["cc"].to_numpy().tobytes()
        whole = an.compute_saliency_similarity(labels, window=None, width=36, height=18)
        assert len(whole) == 1 and whole["time_end"][0] == times[-1] and whole.attrs["window"] == 60
    df = frames[0]
    cols = ["time", "time_end", "samples_a", "samples_b", "distinct_a", "distinct_b"] + list(sso.STATS) + ["map_a", "map_b"]
    assert list(df.columns) == cols
    for other in frames[1:]:                                     # the call is lattice-independent: three analyzers, the same values
        for c in cols:
            a, b = (np.stack(list(f[c])) if c.startswith("map_") else f[c].to_numpy() for f in (df, other))
            assert a.tobytes() == b.tobytes(), c
    res = dict(code=0, maps=np.stack([np.stack(list(df["map_a"])), np.stack(list(df["map_b"]))]),
               stats=np.stack([df[c].to_numpy() for c in sso.STATS]),
               counts=np.stack([df[c].to_numpy() for c in ("samples_a", "samples_b", "distinct_a", "distinct_b")]).astype(np.int64))
    check(res, ids, code, 36, 18, 5.0, 5, 5, "the analyzers' DataFrame")
    base = df["map_a"][0].base
    assert base is not None and all(np.shares_memory(m, base) for m in list(df["map_a"]) + list(df["map_b"]))      # views, no copy
    assert df["map_b"][0].shape == (18, 36)
    assert df.attrs["groups"] == ("hmd", "screen") and df.attrs["sizes"] == (3, 3)
    users = df.attrs["users"]
    assert len(users[0]) == 3 and len(users[1]) == 3 and not set(users[0]) & set(users[1])
    assert df.attrs["sigma_deg"] == 5.0 and df.attrs["width"] == 36 and df.attrs["height"] == 18 and df.attrs["kappa"] == 1.0 / rad(5.0) ** 2
    assert df.attrs["window"] == 5 and df.attrs["stride"] == 5
    assert df["time"].tolist() == times[0::5][:len(df)].tolist() and df["time_end"].tolist() == times[4::5][:len(df)].tolist()
