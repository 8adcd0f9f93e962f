"""GPU: viewer clusters through the C-ABI (Plan.viewer_clusters -> vet_viewer_clusters_host, the device entries through
Plan.viewer_clusters_device, the analyzers' compute_viewer_clusters).  The reference is the numpy oracle of tests/_cluster_oracle.py
(written from the definition in include/vet.h, checked on hand-made cases in tests/test_viewer_clusters_surface.py) — never the
code under test.

The partition is an exact integer result: ``labels``, ``sizes``, ``counts``, ``top`` and ``links`` are compared for equality.  Every
input places its NEAR decisions with margin: the tests assert, on the ORACLE's cosines, that none lies within 1e-9 of cos_threshold
(a condition on the inputs, not a tolerance; the oracle's fused dot and the kernel's differ by the unit vectors' last bits at most).
``stats`` at 1e-12 and ``centroids`` at 1e-12 relative to 1 + |value|: the entropy sum has at most U terms of one sign (log2 of two
libms, an ulp each), and the centroids are sums of the same unit vectors in the same order (their last bits may differ) — the
centroid inputs stay below 500 samples per cluster, 500 * 1.1e-16 * 500 < 3e-11 in the worst case of every rounding aligned and
some 1e-14 in practice; the tests print the largest error they saw.

The plan's grid is 200 columns of 1.8 degrees by 100 rows.  Synthetic viewers sit on or near the equator: 5 columns apart is 9
degrees (near at threshold_deg = 10), 7 columns apart is 12.6 degrees (not)."""
import functools
import math

import numpy as np
import pytest

from tests import _cluster_oracle as co

pytestmark = pytest.mark.gpu

W, H = 200, 100
COS10 = math.cos(math.radians(10.0))
FRACTIONS = (0.5, 0.8, 0.95)
INTS = ("labels", "sizes", "counts", "top", "links")
KEYS = INTS + ("stats", "centroids")


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
    assert np.array_equal(p.read_dirs(), grid())               # the Vectors the oracle works on
    yield p
    engine.test_cluster_tile(0, 0)
    p.close()


@functools.lru_cache(maxsize=None)
def grid():
    t = co.grid_table(W, H)
    t.setflags(write=False)
    return t


def pixel_ids(px, py, present=None):
    """direction ids of pixels (px, py); absent where ``present`` is False"""
    ids = (np.asarray(py) * (W + 1) + np.asarray(px)).astype(np.int32)
    return ids if present is None else np.where(present, ids, -1).astype(np.int32)


def samples_of(ids):
    """(mu, mv) that the quantiser turns into ``ids``: the pixel centres, NaN where absent"""
    py, px = np.divmod(np.maximum(ids, 0), W + 1)
    mu, mv = (px + 0.5) / W, (py + 0.5) / H
    return np.where(ids >= 0, mu, np.nan), np.where(ids >= 0, mv, np.nan)


@functools.lru_cache(maxsize=None)
def g15():
    """ids of golden G15's video on this grid, moved off the centre as the saliency tests move it: 8 viewers x 60 frames"""
    from pathlib import Path
    from tests._saliency_oracle import off_centre
    g = np.load(Path(__file__).resolve().parent / "golden" / "g15_windowed_transition.npz")
    mu, mv = off_centre(g["mu"], g["mv"])
    ids = co.ids_of(mu, mv, W, H)
    for a in (mu, mv, ids):
        a.setflags(write=False)
    return mu, mv, ids


@functools.lru_cache(maxsize=None)
def scattered(U, T, seed, distinct=None, p_absent=0.15):
    """ids [T][U]: viewers scattered over the band of rows 30 .. 70 (``distinct``: over that many random pixels only, which keeps
    the oracle's pair list short for a large audience), each absent with probability p_absent"""
    rng = np.random.default_rng(seed)
    if distinct:
        pool = np.stack([rng.integers(1, W, distinct), rng.integers(30, 71, distinct)], axis=1)
        pick = pool[rng.integers(0, distinct, (T, U))]
        px, py = pick[..., 0], pick[..., 1]
    else:
        px, py = rng.integers(1, W, (T, U)), rng.integers(30, 71, (T, U))
    ids = pixel_ids(px, py, rng.random((T, U)) >= p_absent)
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def walkers(U, T, seed, p_absent=0.15):
    """ids [T][U]: viewers who start scattered over the band and drift by up to two pixels a frame"""
    rng = np.random.default_rng(seed)
    px = np.clip(rng.integers(1, W, U)[None] + np.cumsum(rng.integers(-2, 3, (T, U)), axis=0), 1, W - 1)
    py = np.clip(rng.integers(35, 66, U)[None] + np.cumsum(rng.integers(-1, 2, (T, U)), axis=0), 20, 80)
    ids = pixel_ids(px, py, rng.random((T, U)) >= p_absent)
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def near_of(key, cos_threshold):
    """(near, c) of a cached input, computed once per threshold, with the margin condition checked on the CPU"""
    ids = key[0](*key[1:])
    ids = ids[2] if isinstance(ids, tuple) else ids
    near, c = co.frame_near(grid(), ids, cos_threshold)
    assert co.margin(c, cos_threshold) > 1e-9, (key, cos_threshold)
    near.setflags(write=False)
    return near


def want_of(ids, near, window, stride, min_share=1.0, fractions=FRACTIONS, only=None):
    return co.rows(near, ids, grid(), window, stride, min_share, fractions, only=only)


def run(plan, ids, window=1, stride=1, cos_threshold=COS10, min_share=1.0, fractions=FRACTIONS, samples=False, **kw):
    kw.setdefault("want_centroids", True)
    kw.setdefault("want_links", True)
    src = dict(zip(("mu", "mv"), samples_of(ids))) if samples else dict(ids=ids)
    res = plan.viewer_clusters(window=window, stride=stride, cos_threshold=cos_threshold, min_share=min_share, fractions=fractions,
                               **src, **kw)
    assert res["code"] == 0
    return res


def compare(res, want, msg, rows=None):
    """the integers for equality, stats at 1e-12, centroids at 1e-12 relative to 1 + |value|"""
    pick = (lambda k, a: a) if rows is None else (lambda k, a: a[:, rows] if k in ("counts", "stats") else a[rows])
    for k in INTS:
        got = pick(k, res[k])
        assert got.shape == want[k].shape and got.dtype == want[k].dtype, (msg, k, got.shape, want[k].shape, got.dtype)
        assert np.array_equal(got, want[k]), (msg, k)
    got, ref = pick("stats", res["stats"]), want["stats"]
    assert np.array_equal(np.isnan(got), np.isnan(ref)), msg
    err = np.nanmax(np.abs(got - ref), initial=0.0)
    cen = np.abs(pick("centroids", res["centroids"]) - want["centroids"]) / (1.0 + np.abs(want["centroids"]))
    print(msg, "stats max abs err", float(err), "centroids max rel err", float(cen.max(initial=0.0)))
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12, equal_nan=True, err_msg=msg)
    assert (cen <= 1e-12).all(), msg


def same_bytes(a, b, msg, keys=KEYS):
    for k in keys:
        assert (a[k] is None) == (b[k] is None), (msg, k)
        if a[k] is not None:
            assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (msg, k)


def take(res, rows):
    return {k: (None if res[k] is None else res[k][:, rows] if k in ("counts", "stats") else res[k][rows]) for k in KEYS}


# ------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("window,stride", [(1, 1), (4, 1), (4, 4), (60, 1)])
@pytest.mark.parametrize("threshold_deg,min_share", [(10.0, 1.0), (30.0, 0.5), (30.0, 0.05)])
def test_g15_against_the_oracle(plan, window, stride, threshold_deg, min_share):
    _, _, ids = g15()
    c = math.cos(math.radians(threshold_deg))
    near = near_of((g15,), c)
    res = run(plan, ids, window, stride, c, min_share)
    compare(res, want_of(ids, near, window, stride, min_share), f"g15 w={window} s={stride} {threshold_deg} deg share {min_share}")
    assert res["cos_threshold"] == c


@pytest.mark.parametrize("window,stride", [(1, 1), (4, 1), (4, 4), (60, 1), (60, 4), (64, 1), (33, 31)])
def test_windows_of_a_drifting_audience(plan, window, stride):
    """T = 64: windows below, at and beyond the 32 frames staged at a time, and the whole video"""
    ids = walkers(24, 64, 5)
    near = near_of((walkers, 24, 64, 5), COS10)
    for share in (1.0, 0.5):
        compare(run(plan, ids, window, stride, min_share=share), want_of(ids, near, window, stride, share),
                f"walkers w={window} s={stride} share {share}")


@pytest.mark.parametrize("U", [1, 2, 63, 64, 65, 130, 257, 300, 1100])
def test_audience_sizes_and_the_seams(engine, plan, U):
    """word boundaries (63, 64, 65, 130), two blocks of 256 viewers (257, 300), 1100; with the partner tile at 3 and 100 and the
    rows per pass at 1 and 3 the same bytes"""
    key = (scattered, U, 4, 100 + U, 60 if U > 300 else None)
    ids = scattered(*key[1:])
    near = near_of(key, COS10)
    try:
        first = run(plan, ids, 1, 1)
        compare(first, want_of(ids, near, 1, 1), f"U={U} window 1")
        pooled = run(plan, ids, 2, 1)
        compare(pooled, want_of(ids, near, 2, 1), f"U={U} window 2")
        for rows, tile in ((1, 3), (3, 100), (1, 0), (0, 3)):
            engine.test_cluster_tile(rows, tile)
            same_bytes(run(plan, ids, 1, 1), first, f"U={U} rows per pass {rows}, tile {tile}")
            same_bytes(run(plan, ids, 2, 1), pooled, f"U={U} window 2, rows per pass {rows}, tile {tile}")
    finally:
        engine.test_cluster_tile(0, 0)
    assert (first["links"] >> np.uint64(U % 64) == 0)[..., -1].all() if U % 64 else True      # no bit at or beyond U


# ------------------------------------------------------------------------------------------- convergence
def chain_ids(U, gap=None):
    """T = 8 frames, window 8: viewers i and i + 1 are in one frame together only in frame i % 8, 9 degrees apart, every pair of
    a frame at a place of its own (12 columns or 7 rows, 12.6 degrees, from the next): a path of U viewers, diameter U - 1.
    ``gap``: viewer gap + 1 misses the frame it shares with viewer gap"""
    ids = np.full((8, U), -1, dtype=np.int32)
    for i in range(U - 1):
        f, slot = i % 8, i // 8
        py, px = (43, 50, 57)[slot // 16], 1 + 12 * (slot % 16)
        ids[f, i] = pixel_ids(px, py)
        if i != gap:
            ids[f, i + 1] = pixel_ids(px + 5, py)
    return ids


@pytest.mark.parametrize("order", ["index", "reverse", "shuffled"])
def test_a_chain_of_300_viewers_is_one_cluster(plan, order):
    U = 300
    perm = {"index": np.arange(U), "reverse": np.arange(U)[::-1], "shuffled": np.random.default_rng(7).permutation(U)}[order]
    for gap in (None, 149):
        ids = np.ascontiguousarray(chain_ids(U, gap)[:, perm])          # column j holds chain position perm[j]
        near, c = co.frame_near(grid(), ids, COS10)
        assert co.margin(c, COS10) > 1e-9
        want = want_of(ids, near, 8, 1)
        assert want["counts"][:, 0].tolist() == ([U, 1, U, 0, U - 1] if gap is None else [U, 2, 150, 0, U - 2])
        res = run(plan, ids, 8, 1, want_centroids=False)
        for k in INTS:
            assert np.array_equal(res[k], want[k]), (order, gap, k)
        np.testing.assert_allclose(res["stats"], want["stats"], rtol=1e-12, atol=1e-12)
        most, total = plan.viewer_clusters_sweeps()
        print(f"chain of {U} in {order} order, gap {gap}: {most} sweeps")
        assert 1 <= most == total <= U


def test_a_star_and_everyone_on_one_direction(plan):
    U, T = 65, 32                      # the centre with two leaves a frame, 18 degrees from each other and 9 from the centre
    ids = np.full((T, U), -1, dtype=np.int32)
    ids[:, 0] = pixel_ids(100, 50)
    for leaf in range(1, U):
        ids[(leaf - 1) // 2, leaf] = pixel_ids(95 if leaf % 2 else 105, 50)
    near, c = co.frame_near(grid(), ids, COS10)
    assert co.margin(c, COS10) > 1e-9
    want = want_of(ids, near, T, 1)
    assert want["counts"][:, 0].tolist() == [U, 1, U, 0, U - 1]
    compare(run(plan, ids, T, 1), want, "star")
    U = 300
    ids = np.full((1, U), pixel_ids(77, 41), dtype=np.int32)
    near, _ = co.frame_near(grid(), ids, COS10)
    want = want_of(ids, near, 1, 1)
    assert want["counts"][:, 0].tolist() == [U, 1, U, 0, U * (U - 1) // 2]
    compare(run(plan, ids, 1, 1), want, "one direction")


def test_the_largest_audience_against_a_closed_form(plan):
    """8192 viewers, the most the call takes (the labels of a row fill its LDS): 16 places 12 columns apart, everyone at one of them —
    the clusters are the places, numbered by their first viewer; no oracle is needed"""
    U = 8192
    place = np.random.default_rng(21).integers(0, 16, U)
    ids = pixel_ids(1 + 12 * place, 50)[None]
    _, first = np.unique(place, return_index=True)
    rank = np.empty(16, dtype=np.int64)
    rank[np.argsort(first)] = np.arange(16)
    sizes = np.bincount(rank[place], minlength=16)
    res = run(plan, ids, 1, 1, want_centroids=False)
    assert np.array_equal(res["labels"][0], rank[place]) and np.array_equal(res["sizes"][0, :16], sizes) and not res["sizes"][0, 16:].any()
    assert res["counts"][:, 0].tolist() == [U, 16, sizes.max(), 0, int((sizes * (sizes - 1) // 2).sum())]
    bits = np.unpackbits(res["links"][0].view(np.uint8), axis=1, bitorder="little")[:, :U].astype(bool)
    assert np.array_equal(bits, (place[:, None] == place[None, :]) & ~np.eye(U, dtype=bool))
    want_h = math.log2(U) - float((sizes * np.log2(sizes)).sum()) / U
    np.testing.assert_allclose(res["stats"][:, 0], [want_h, want_h / math.log2(U), sizes.max() / U], rtol=1e-12)


# ------------------------------------------------------------------------------------------- edges
def test_absent_lonely_and_never_co_present_viewers(plan):
    a, b, far = pixel_ids(11, 50), pixel_ids(16, 50), pixel_ids(120, 50)
    ids = np.array([[a, -1, -1, -1, a, -1],        # viewer 1 is absent throughout; viewer 2 is only in a frame where nobody else is
                    [a, -1, -1, b, -1, -1],
                    [-1, -1, a, -1, -1, -1],
                    [-1, -1, -1, -1, -1, -1],       # a frame with nobody
                    [-1, -1, -1, -1, -1, far]], dtype=np.int32)
    near, c = co.frame_near(grid(), ids, COS10)
    assert co.margin(c, COS10) > 1e-9
    res = run(plan, ids, 3, 1)
    compare(res, want_of(ids, near, 3, 1), "edges, window 3")
    assert res["labels"][0].tolist() == [0, -1, 1, 0, 0, -1] and (res["links"][:, 1] == 0).all()
    per_frame = run(plan, ids, 1, 1)
    compare(per_frame, want_of(ids, near, 1, 1), "edges, window 1")
    assert per_frame["labels"][3].tolist() == [-1] * 6 and (per_frame["counts"][:, 3] == 0).all()
    assert np.isnan(per_frame["stats"][:, 3]).all() and per_frame["stats"][:, 2].tolist()[0] == 0.0
    whole = run(plan, ids, 5, 1)                   # viewers 0 and 4 share frame 0 on one direction; 2 never meets anybody
    compare(whole, want_of(ids, near, 5, 1), "edges, whole video")
    assert whole["labels"][0].tolist() == [0, -1, 1, 0, 0, 2]
    never = np.array([[a, -1], [-1, a]], dtype=np.int32)          # one direction, never in one frame: not linked
    res = run(plan, never, 2, 1)
    assert res["labels"].tolist() == [[0, 1]] and res["counts"][:, 0].tolist() == [2, 2, 1, 2, 0]


def test_the_pole_and_the_extreme_thresholds(plan):
    pole = np.array([[pixel_ids(3, 0), pixel_ids(90, 0), pixel_ids(3, 1)]], dtype=np.int32)       # one Vector under two ids
    assert np.array_equal(grid()[pole[0, 0]], grid()[pole[0, 1]]) and pole[0, 0] != pole[0, 1]
    for c_thr in (COS10, 1.0):
        near, c = co.frame_near(grid(), pole, c_thr)
        assert co.margin(c, c_thr) > 1e-9 and near[0, 0, 1]
        res = run(plan, pole, 1, 1, c_thr)
        compare(res, want_of(pole, near, 1, 1), f"pole at {c_thr}")
    assert res["labels"].tolist() == [[0, 0, 1]]                  # cos_threshold 1.0: only the equal Vectors link
    ids = np.array(scattered(40, 6, 3, 12))                       # 12 directions for 40 viewers: many share one
    for c_thr, share in ((1.0, 1.0), (-1.0, 1.0), (-1.0, 0.05)):
        near, c = co.frame_near(grid(), ids, c_thr)
        assert co.margin(c, c_thr) > 1e-9
        res = run(plan, ids, 3, 1, c_thr, share)
        compare(res, want_of(ids, near, 3, 1, share), f"threshold {c_thr}")
    both = (ids[:3, :, None] >= 0) & (ids[:3, None, :] >= 0)
    assert res["counts"][4, 0] == (np.triu(both.any(axis=0), 1)).sum()     # cos_threshold -1: everybody who meets links


# ------------------------------------------------------------------------------------------- byte for byte
def test_bits_do_not_depend_on_stride_length_entry_or_outputs(plan):
    import torch
    mu_long, mv_long, ids_long = g15()
    T, U, w = 40, 8, 5
    mu, mv, ids = mu_long[:T], mv_long[:T], ids_long[:T]
    kw = dict(window=w, cos_threshold=COS10, min_share=0.5, fractions=FRACTIONS, want_centroids=True, want_links=True)
    s1 = plan.viewer_clusters(mu=mu, mv=mv, stride=1, **kw)
    same_bytes(plan.viewer_clusters(mu=mu, mv=mv, stride=1, **kw), s1, "two runs of one call")
    same_bytes(take(s1, slice(0, None, 3)), plan.viewer_clusters(mu=mu, mv=mv, stride=3, **kw), "stride 1 against stride 3")
    long = plan.viewer_clusters(mu=mu_long, mv=mv_long, stride=1, **kw)
    same_bytes(take(long, slice(0, T - w + 1)), s1, "a longer video's prefix")
    same_bytes(plan.viewer_clusters(ids=ids, stride=1, **kw), s1, "ids against (mu, mv)")
    other = plan.viewer_clusters(mu=mu, mv=mv, stride=1, **dict(kw, fractions=(0.3, 0.5, 1.0)))
    same_bytes(other, s1, "other fractions", keys=[k for k in KEYS if k != "top"])
    assert np.array_equal(other["top"][:, 1], s1["top"][:, 0])
    for wanted in ((), ("labels",), ("centroids",), ("links",)):
        res = plan.viewer_clusters(mu=mu, mv=mv, stride=1, **dict(kw, fractions=FRACTIONS if wanted else (), want_labels="labels" in wanted,
                                                                 want_centroids="centroids" in wanted, want_links="links" in wanted))
        assert [k for k in KEYS if res[k] is not None] == [k for k in KEYS if k in ("counts", "stats") or k in wanted
                                                          or (k == "sizes" and "labels" in wanted) or (k == "top" and wanted)]
        same_bytes(res, s1, f"outputs {wanted}", keys=[k for k in KEYS if res[k] is not None])
    # the device entries, every output and one output at a time
    dev = torch.device("cuda", 0)
    R, words = s1["counts"].shape[1], 1
    d_mu, d_mv, d_ids = (torch.from_numpy(np.array(a)).to(dev) for a in (mu, mv, ids))
    shapes = dict(labels=((R, U), torch.int32), sizes=((R, U), torch.int32), counts=((5, R), torch.int64), top=((R, 3), torch.int32),
                  stats=((3, R), torch.float64), centroids=((R, U, 3), torch.float64), links=((R, U, words), torch.int64))
    for src in ("mu_mv", "ids"):
        extra = dict(d_ids=d_ids.data_ptr()) if src == "ids" else {}
        for wanted in (KEYS,) + tuple((k,) for k in KEYS) + ((),):
            bufs = {k: torch.full(shapes[k][0], -7, dtype=shapes[k][1], device=dev) for k in wanted}
            status = torch.zeros(2, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            plan.viewer_clusters_device(d_mu.data_ptr(), d_mv.data_ptr(), U, T, w, 1, COS10, 0.5, FRACTIONS if "top" in wanted else None,
                                        d_status=status.data_ptr(), **{"d_" + k: b.data_ptr() for k, b in bufs.items()}, **extra)
            torch.cuda.synchronize()
            for k, b in bufs.items():
                assert b.cpu().numpy().tobytes() == s1[k].tobytes(), (src, wanted, k)
            assert status.cpu().tolist() == [0, int((s1["counts"][0] == 0).sum())]


def test_permuting_the_viewers(plan):
    """A permutation of the viewer columns permutes labels and links accordingly and leaves counts, top and the sorted sizes alone.
    stats[2] = largest / P is a quotient of two integers.  stats[1] follows the entropy sum, whose positions are the cluster labels,
    and a permutation moves those: the sum keeps its bits where every term s log2 s is exact, which is so for sizes that are powers of
    two — the clusters of this audience have 1, 2, 4 and 8 members — and agrees to rounding on G15's, whose sizes are whatever they
    are."""
    rng = np.random.default_rng(11)
    groups = [8, 1, 4, 2, 8, 4, 1, 2, 2, 16, 1, 4]              # clusters of co-located viewers, the groups 12 columns apart
    cols = np.concatenate([np.full(n, 1 + 12 * g) for g, n in enumerate(groups)])
    T, U = 3, len(cols)
    ids = np.tile(pixel_ids(cols, 50), (T, 1))
    ids[1, rng.random(U) < 0.2] = -1                            # absences in the middle frame only: everybody is in both rows
    for name, ids, exact in (("powers of two", ids, True), ("g15", np.array(g15()[2][:30]), False)):
        U = ids.shape[1]
        near, c = co.frame_near(grid(), ids, COS10)
        assert co.margin(c, COS10) > 1e-9
        if exact:
            sizes = want_of(ids, near, 2, 1)["sizes"]
            assert np.isin(sizes, [0, 1, 2, 4, 8, 16]).all()
        perm = rng.permutation(U)
        a = run(plan, ids, 2, 1)
        b = run(plan, np.ascontiguousarray(ids[:, perm]), 2, 1)
        for k in ("counts", "top"):
            assert a[k].tobytes() == b[k].tobytes(), (name, k)
        assert np.array_equal(np.sort(a["sizes"], axis=1), np.sort(b["sizes"], axis=1)), name
        assert a["stats"][2].tobytes() == b["stats"][2].tobytes(), name
        if exact:
            assert a["stats"][1].tobytes() == b["stats"][1].tobytes(), name
        np.testing.assert_allclose(a["stats"], b["stats"], rtol=1e-12, atol=1e-12, equal_nan=True)
        for r in range(a["labels"].shape[0]):                    # the same partition: b's viewer j is a's viewer perm[j]
            la, lb = a["labels"][r][perm], b["labels"][r]
            assert np.array_equal(la < 0, lb < 0) and np.array_equal(la[:, None] == la[None, :], lb[:, None] == lb[None, :]), (name, r)
            bits_a = ((a["links"][r][:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).reshape(U, -1)[:, :U].astype(bool)
            bits_b = ((b["links"][r][:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).reshape(U, -1)[:, :U].astype(bool)
            assert np.array_equal(bits_a[np.ix_(perm, perm)], bits_b) and np.array_equal(bits_b, bits_b.T), (name, r)


# ------------------------------------------------------------------------------------------- against merged code
def test_links_of_a_frame_are_the_dispersion_pairs_within_the_threshold(plan):
    """window = 1: a frame's links are its pair samples whose Plan.dispersion angle is <= radians(threshold_deg): the one-bin histogram
    [0, theta] with the upper edge moved up by an ulp, which closes the bin"""
    mu, mv, ids = g15()
    for deg in (10.0, 30.0):
        theta = math.radians(deg)
        near_of((g15,), math.cos(theta))                         # the margin condition
        links = plan.viewer_clusters(mu=mu, mv=mv, window=1, threshold_deg=deg)["counts"][4]
        hist = plan.dispersion(mu=mu, mv=mv, window=1, edges=[0.0, math.nextafter(theta, math.inf)])["hist"][:, 0]
        assert np.array_equal(links, hist) and links.sum() > 0, deg


# ------------------------------------------------------------------------------------------- refusals, the range code, the analyzers
def test_illegal_arguments_are_refused_before_anything_runs(native, plan):
    ids = np.array(g15()[2][:30])
    T, U = ids.shape
    f = np.array(FRACTIONS)
    good = dict(U=U, T=T, window=5, stride=1, cos=COS10, share=1.0, f=f.ctypes.data, Q=3)
    counts = np.empty((5, 26), dtype=np.int64)

    def call(**change):
        a = dict(good, **change)
        return plan.lib.vet_viewer_clusters_host(plan.handle, None, None, ids.ctypes.data, a["U"], a["T"], a["window"], a["stride"],
                                                 a["cos"], a["share"], a["f"], a["Q"], None, None, counts.ctypes.data, None, None, None,
                                                 None)
    assert call() == native.VET_OK
    bad_f = [np.array(v) for v in ([0.0, 0.5, 0.9], [0.5, 1.5, 0.9], [0.5, float("nan"), 0.9], [0.5, float("inf"), 0.9])]
    for change in (dict(window=0), dict(window=T + 1), dict(stride=0), dict(Q=-1), dict(Q=17), dict(share=0.0), dict(share=1.5),
                   dict(share=float("nan")), dict(cos=1.5), dict(cos=-1.5), dict(cos=float("nan")), dict(f=None),
                   *(dict(f=v.ctypes.data) for v in bad_f)):
        assert call(**change) == native.VET_ERR_INVALID, change
    assert call(U=8193) == native.VET_ERR_UNSUPPORTED             # refused before the samples are read
    with pytest.raises(native.NativeError) as err:                # the device entry refuses before it looks at a pointer
        plan.viewer_clusters_device(8, 8, 4, 30, 31, 1, COS10, 1.0, None, 8)
    assert err.value.code == native.VET_ERR_INVALID
    with pytest.raises(native.NativeError) as err:
        plan.viewer_clusters_device(8, 8, 8193, 2, 1, 1, COS10, 1.0, None, 8)
    assert err.value.code == native.VET_ERR_UNSUPPORTED
    for bad in (dict(threshold_deg=-1.0), dict(min_share=0.0), dict(fractions=(0.0,)), dict(window=0), dict(stride=0)):
        with pytest.raises(ValueError):
            plan.viewer_clusters(ids=ids, **bad)


def test_sample_out_of_range(native, plan):
    mu, mv, ids = (np.array(a[:10]) for a in g15())
    mu[3, 2] = 1.5
    with pytest.raises(native.NativeError) as e:
        plan.viewer_clusters(mu=mu, mv=mv)
    assert e.value.code == native.VET_ERR_RANGE
    res = plan.viewer_clusters(mu=mu, mv=mv, threshold_deg=10.0, check=False)
    assert res["code"] == native.VET_ERR_RANGE                    # the outputs are still written: the sample counts as absent
    ids[3, 2] = -1
    assert np.array_equal(res["labels"], plan.viewer_clusters(ids=ids, threshold_deg=10.0)["labels"]) and res["labels"][3, 2] == -1


def test_analyzers_return_the_frame():
    from viewport_entropy_toolkit import SpatialEntropyAnalyzer, TransitionEntropyAnalyzer
    from viewport_entropy_toolkit.analyzers import NaiveSpatialEntropyAnalyzer
    from viewport_entropy_toolkit.config import AnalyzerConfig, NaiveAnalyzerConfig
    mu, mv, ids = g15()
    times = np.arange(60) / 30.0
    frames = []
    for cls in (SpatialEntropyAnalyzer, TransitionEntropyAnalyzer, NaiveSpatialEntropyAnalyzer):
        an = cls(NaiveAnalyzerConfig(tile_height=10, tile_width=20, video_width=W, video_height=H)) \
            if cls is NaiveSpatialEntropyAnalyzer else cls(AnalyzerConfig(tile_counts=[20], video_width=W, video_height=H))
        an.load_arrays(times, mu.copy(), mv.copy())
        frames.append(an.compute_viewer_clusters(window=4, stride=2, threshold_deg=10.0, keep_centroids=True, keep_links=True))
        slim = an.compute_viewer_clusters(window=None, keep_labels=False)
        assert len(slim) == 1 and list(slim.columns)[-1] == "streams" and slim["time_end"][0] == times[-1]
        assert len(an.compute_viewer_clusters()) == 60 and slim.attrs["threshold_deg"] == 30.0
        with pytest.raises(ValueError):
            an.compute_viewer_clusters(threshold_deg=200.0)
        with pytest.raises(ValueError):
            an.compute_viewer_clusters(fractions=(0.5, 2.0))
        with pytest.raises(ValueError):
            an.compute_viewer_clusters(window=61)
    df = frames[0]
    assert list(df.columns) == ["time", "time_end", "viewers", "clusters", "largest", "largest_share", "singletons", "links", "entropy",
                                "entropy_norm", "streams", "labels", "sizes", "centroids", "links_bits"]
    views = ("streams", "labels", "sizes", "centroids", "links_bits")
    for c in df.columns:                                         # the call is lattice-independent: three analyzers, the same values
        for other in frames[1:]:
            a, b = (np.stack(list(f[c])) if c in views else f[c].to_numpy() for f in (df, other))
            assert a.tobytes() == b.tobytes(), c
    near = near_of((g15,), COS10)
    want = want_of(ids, near, 4, 2)
    assert len(df) == 29 and df["clusters"].tolist() == want["counts"][1].tolist() and df["links"].tolist() == want["counts"][4].tolist()
    assert df["viewers"].tolist() == want["counts"][0].tolist() and df["singletons"].tolist() == want["counts"][3].tolist()
    assert all(np.array_equal(df["labels"][r], want["labels"][r]) and np.array_equal(df["streams"][r], want["top"][r]) and
               np.array_equal(df["links_bits"][r], want["links"][r]) for r in range(29))
    np.testing.assert_allclose(df["entropy"], want["stats"][0], rtol=1e-12, atol=1e-12)
    assert df.attrs == dict(threshold_deg=10.0, cos_threshold=COS10, min_share=1.0, fractions=FRACTIONS, window=4, stride=2,
                            users=df.attrs["users"]) and len(df.attrs["users"]) == 8
    assert df["time"].tolist() == times[0::2][:29].tolist() and df["time_end"].tolist() == times[3::2][:29].tolist()
