"""GPU: fixation and tile-dwell events through the C-ABI (Plan.fixations -> vet_fixations_host, the device entries through
Plan.fixations_device, the analyzers' compute_fixations).  The pair (f, f + 1) of a viewer HOLDS when the viewer is present in both
frames and the two directions are within max_step_deg (decided on the cosine) or on one tile; a run is a maximal stretch of holding
frames, an event a run of at least min_frames frames, counted in the row of its start.  The reference is the oracle of
tests/_fixation_oracle.py (plain loops from the definition; pinned against golden G25 in tests/test_fixations_surface.py) — never the
code under test — and, for the large periodic input, formulas written in the test.

Every integer output is compared for EQUALITY.  Every input first asserts, on the ORACLE's cosines, that none lies within 1e-9 of
the threshold, so a last-bit difference of a dot product cannot move a decision.  Centroids: 1e-12 relative to 1 + |value| — the
oracle adds the same unit vectors in the same order with the same plain adds; the unit vectors themselves may differ by an ulp of
the division or the root (2.2e-16 each), and a sum of at most 2049 of them by 2049 * 2.2e-16 = 4.5e-13."""
import math

import numpy as np
import pytest

from tests import _fixation_oracle as fo

pytestmark = pytest.mark.gpu

W, H = 100, 200
EDGES = (1, 2, 3, 5, 9, 4000)
INT_KEYS = ("counts", "hist", "labels", "offsets", "events")
MARGIN = 1e-9


def cos_of(deg):
    return min(1.0, max(-1.0, math.cos(math.radians(deg))))


@pytest.fixture(scope="module")
def native():
    from viewport_entropy_toolkit import _native
    return _native


@pytest.fixture(scope="module")
def engine(native):
    e = native.Engine.default()
    yield e
    e.test_fixation_chunk(0)


@pytest.fixture(scope="module")
def plan(native, engine):
    from oracle import vet_oracle as vo
    p = native.Plan(engine, [vo.fibonacci_lattice(50)], 120.0, 2.0, True, W, H)
    yield p
    p.close()


@pytest.fixture(scope="module")
def table(plan):
    t = plan.read_dirs()
    assert np.array_equal(t, fo.grid_table(W, H))
    return t


@pytest.fixture(scope="module")
def nearest(plan):
    return plan.read_nearest(0)


@pytest.fixture(scope="module")
def g15(golden_dir):
    g = np.load(golden_dir / "g15_windowed_transition.npz")
    mu, mv = np.array(g["mu"]), np.array(g["mv"])
    return mu, mv, fo.ids_of(mu, mv, W, H)


_HOLDS = {}


def hold_of(ids, by, deg, table, nearest):
    """the oracle's HOLD of an input (cached by the array's bytes), after the margin condition on its cosines"""
    key = (ids.tobytes(), ids.shape, by, deg)
    if key not in _HOLDS:
        if by == "tile":
            _HOLDS[key] = fo.hold_tile(nearest, 50, ids)
        else:
            hold, c = fo.hold_angle(table, ids, cos_of(deg))
            assert fo.margin(c, cos_of(deg)) >= MARGIN, (deg, fo.margin(c, cos_of(deg)))
            _HOLDS[key] = hold
    return _HOLDS[key]


def same(res, want, msg, keys=INT_KEYS + ("centroids",)):
    for k in keys:
        if want.get(k) is None:
            continue
        got = res[k]
        assert got is not None and got.shape == want[k].shape, (msg, k, None if got is None else got.shape, want[k].shape)
        if k == "centroids":
            err = np.abs(got - want[k]) / (1.0 + np.abs(want[k]))
            assert (err <= 1e-12).all(), (msg, k, float(err.max(initial=0.0)))
        else:
            assert np.array_equal(got, want[k]), (msg, k)


def same_bytes(a, b, msg, keys=INT_KEYS + ("centroids",)):
    for k in keys:
        assert (a[k] is None) == (b[k] is None), (msg, k)
        if a[k] is not None:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (msg, k)


def full(plan, ids=None, **kw):
    kw = dict(dict(edges=EDGES, keep_labels=True, keep_events=True, keep_centroids=True), **kw)
    return plan.fixations(ids=ids, **kw) if ids is not None else plan.fixations(**kw)


# ------------------------------------------------------------------------------------------- the oracle, golden G15's inputs
@pytest.mark.parametrize("per_user", [False, True])
@pytest.mark.parametrize("by", ["angle", "tile"])
def test_g15_against_the_oracle(plan, table, nearest, g15, by, per_user):
    mu, mv, ids = g15
    T, U = ids.shape
    n_events = set()
    for deg in ((1.0, 2.0, 5.0, 10.0) if by == "angle" else (2.0,)):
        hold = hold_of(ids, by, deg, table, nearest)
        for m in (1, 2, 3, 5):
            for window in (1, 7, 20, 60):
                for stride in sorted({1, window}):
                    want = fo.result(ids, hold, window, stride, m, per_user, EDGES, table)
                    msg = f"{by} {deg} min {m} w {window} s {stride} per_user {per_user}"
                    res = full(plan, mu=mu, mv=mv, window=window, stride=stride, by=by, max_step_deg=deg, min_frames=m,
                               per_user=per_user)
                    assert res["code"] == 0 and res["cos_threshold"] == cos_of(deg), msg
                    assert res["counts"].dtype == np.int64 and res["hist"].dtype == res["labels"].dtype == np.int32, msg
                    same(res, want, msg)
                    n_events.add(len(want["events"]))
            # without the optional outputs the counts are the same bytes
            slim = plan.fixations(mu=mu, mv=mv, window=7, stride=1, by=by, max_step_deg=deg, min_frames=m, per_user=per_user)
            assert all(slim[k] is None for k in ("hist", "labels", "offsets", "events", "centroids"))
            assert slim["counts"].tobytes() == fo.result(ids, hold, 7, 1, m, per_user)["counts"].tobytes()
    assert len(n_events) >= 3 and max(n_events) > 2 * min(n_events)               # the cases differ


def test_g15_event_counts_of_the_issue(plan, g15):
    mu, mv, _ = g15
    for m, n in ((2, 91), (3, 28), (5, 4)):
        res = plan.fixations(mu=mu, mv=mv, max_step_deg=2.0, min_frames=m, keep_events=True)
        assert int(res["offsets"][-1]) == n == len(res["events"]) == int(res["counts"][2, 0])


def device_run(plan, torch, U, T, window, stride, by, cos, m, per_user, edges, max_events, wanted, d_mu=None, d_mv=None, d_ids=None):
    """one call of a device entry; returns the wanted outputs as numpy arrays, and the status words"""
    dev = torch.device("cuda", 0)
    R = (T - window) // stride + 1
    lead = (U, R) if per_user else (R,)
    B = len(edges) - 1 if edges is not None else 0
    shapes = dict(counts=((5,) + lead, torch.int64), hist=(lead + (B,), torch.int32), labels=((U, T), torch.int32),
                  offsets=((U + 1,), torch.int64), events=((max_events, 4), torch.int32), centroids=((max_events, 3), torch.float64))
    bufs = {k: torch.full(shapes[k][0], -7, dtype=shapes[k][1], device=dev) for k in wanted}
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    extra = dict(d_ids=d_ids.data_ptr()) if d_ids is not None else {}
    plan.fixations_device(0 if d_mu is None else d_mu.data_ptr(), 0 if d_mv is None else d_mv.data_ptr(), U, T, window, stride, by, cos,
                          m, per_user, edges if "hist" in wanted else None, max_events=max_events, d_status=status.data_ptr(),
                          **{"d_" + k: b.data_ptr() for k, b in bufs.items()}, **extra)
    torch.cuda.synchronize()
    return {k: b.cpu().numpy() for k, b in bufs.items()}, status.cpu().tolist()


def test_entry_points_null_outputs_and_max_events(plan, g15):
    """(mu, mv) and ids, host and device: the same bytes; every output alone; a short event list is the prefix of the full one"""
    torch = pytest.importorskip("torch")
    mu, mv, ids = g15
    T, U = ids.shape
    dev = torch.device("cuda", 0)
    d_mu, d_mv, d_ids = (torch.from_numpy(np.array(a)).to(dev) for a in (mu, mv, ids))
    keys = INT_KEYS + ("centroids",)
    for by in ("angle", "tile"):
        for per_user in (False, True):
            kw = dict(window=7, stride=3, by=by, max_step_deg=2.0, min_frames=2, per_user=per_user)
            ref = full(plan, mu=mu, mv=mv, **kw)
            same_bytes(full(plan, ids=ids, **kw), ref, f"host ids {by} {per_user}")
            N = int(ref["offsets"][-1])
            assert N > 20
            empty = int((ref["counts"][0] == 0).sum())
            for src in (dict(d_mu=d_mu, d_mv=d_mv), dict(d_ids=d_ids)):
                for wanted in (keys, ("counts",), ("hist",), ("labels",), ("offsets",), ("events",), ("events", "centroids"), ()):
                    got, status = device_run(plan, torch, U, T, 7, 3, by, cos_of(2.0), 2, per_user, EDGES, N, wanted, **src)
                    for k in wanted:
                        assert got[k].tobytes() == ref[k].tobytes(), (by, per_user, sorted(src), wanted, k)
                    assert status == [0, empty], (by, per_user, wanted)
                # fewer slots than events: the prefix, the untouched tail, the same offsets
                for cap in (0, N // 2, N - 1):
                    short, _ = device_run(plan, torch, U, T, 7, 3, by, cos_of(2.0), 2, per_user, None, cap,
                                          ("offsets", "events", "centroids"), **src)
                    assert short["offsets"].tobytes() == ref["offsets"].tobytes()
                    assert short["events"].tobytes() == ref["events"][:cap].tobytes()
                    assert short["centroids"].tobytes() == ref["centroids"][:cap].tobytes()


# ------------------------------------------------------------------------------------------- seams
FAR = [(30, 20), (100, 70), (170, 10), (60, 50), (140, 90)]       # (py, px) of pixels tens of degrees apart


def run_ids(lengths, first=0):
    """one viewer's ids from run lengths (a negative length: that many absent frames): run j sits on pixel FAR[j % 5] and moves
    between it and the pixel below (0.9 degrees apart: holds at 2 degrees); two consecutive runs are tens of degrees apart"""
    out, j = [], first
    for L in lengths:
        if L < 0:
            out += [-1] * -L
            continue
        py, px = FAR[j % len(FAR)]
        base = py * (W + 1) + px
        out += [base + (W + 1) * (k & 1) * (j & 1) for k in range(L)]        # odd runs alternate two pixels, even runs stay
        j += 1
    return out


def random_lengths(T, rng, p_absent=0.15):
    out, left = [], T
    while left > 0:
        L = int(min(left, rng.choice([1, 1, 2, 3, 4, 5, 7, 11, 40])))
        out.append(-L if rng.random() < p_absent else L)
        left -= L
    return out


def stack(viewers, T):
    assert all(len(v) == T for v in viewers), [len(v) for v in viewers]
    return np.ascontiguousarray(np.array(viewers, dtype=np.int32).T)


def seam_check(plan, engine, table, nearest, ids, chunks, msg, min_frames=3, window=None, stride=1):
    T, U = ids.shape
    window = min(T, 5) if window is None else window
    for by in ("angle", "tile"):
        hold = hold_of(ids, by, 2.0, table, nearest)
        for per_user in (False, True):
            want = fo.result(ids, hold, window, stride, min_frames, per_user, EDGES, table)
            ref = None
            for chunk in chunks:
                engine.test_fixation_chunk(chunk)
                res = full(plan, ids=ids, window=window, stride=stride, by=by, max_step_deg=2.0, min_frames=min_frames, per_user=per_user)
                same(res, want, f"{msg} {by} per_user {per_user} chunk {chunk}")
                if ref is not None:
                    same_bytes(res, ref, f"{msg} {by} per_user {per_user} chunk {chunk} against chunk {chunks[0]}")
                ref = ref or res
    engine.test_fixation_chunk(0)


@pytest.mark.parametrize("chunk", [8, 16, 64])
def test_seams_at_small_chunks(plan, engine, table, nearest, chunk):
    C, T = chunk, 4 * chunk + 5
    rng = np.random.default_rng(chunk)
    viewers = [
        run_ids([C - 3, 5, T - C - 2]),                          # a run that crosses one chunk edge
        run_ids([C - 2, 2 * C + 3, T - 3 * C - 1]),              # a run that spans three chunks (and touches a fourth)
        run_ids([T]),                                            # a run that is the whole video
        run_ids([C - 1, 2, T - C - 1]),                          # starts on a chunk's last frame, ends on the next one's first
        run_ids([T - 3 - 4, -4, 3]),                             # a run of exactly min_frames ending at T - 1
        run_ids([-T]),                                           # an all-absent viewer
        run_ids([1] * T),                                        # every frame a run of its own
        run_ids(random_lengths(T, rng)),
    ]
    ids = stack(viewers, T)
    ids[2 * C + 1, [0, 3, 5, 6, 7]] = -1                         # holes next to a seam
    seam_check(plan, engine, table, nearest, ids, (chunk, 4, 0, 1024), f"chunk {chunk}")
    blank = np.array(ids)
    blank[C] = -1                                                # an all-absent frame, on a chunk's first frame
    seam_check(plan, engine, table, nearest, blank, (chunk, 0), f"chunk {chunk} blank frame", window=C, stride=C)


@pytest.mark.parametrize("T", [1023, 1024, 1025, 2049])
def test_seams_at_the_default_chunk(plan, engine, table, nearest, T):
    rng = np.random.default_rng(T)
    viewers = [run_ids([T]),                                     # the whole video
               run_ids([1020, 6, T - 1026] if T > 1026 else [1023, 2] if T == 1025 else [T - 2, 2]),      # over the chunk's edge
               run_ids(random_lengths(T, rng))]
    ids = stack(viewers, T)
    seam_check(plan, engine, table, nearest, ids, (0, 512, 64), f"T {T}", window=256, stride=255)


@pytest.mark.parametrize("U", [1, 63, 65, 130])
def test_audiences_around_the_transpose_tile(plan, engine, table, nearest, U):
    rng = np.random.default_rng(U)
    T = 70
    ids = stack([run_ids(random_lengths(T, rng), first=u) for u in range(U)], T)
    seam_check(plan, engine, table, nearest, ids, (0, 16), f"U {U}", min_frames=2, window=9, stride=4)


def test_videos_of_one_and_two_frames(plan, engine, table, nearest):
    py, px = FAR[0]
    a, far = py * (W + 1) + px, FAR[1][0] * (W + 1) + FAR[1][1]
    one = np.array([[a, -1, far]], dtype=np.int32)
    two = np.array([[a, -1, far, a, -1], [a + W + 1, a, a, -1, -1]], dtype=np.int32)    # holds, starts late, jumps, leaves, never there
    for ids in (one, two):
        for m in (1, 2):
            seam_check(plan, engine, table, nearest, ids, (0, 4), f"T {len(ids)} min {m}", min_frames=m, window=1)
            seam_check(plan, engine, table, nearest, ids, (0,), f"T {len(ids)} min {m} whole", min_frames=m, window=len(ids))
    res = plan.fixations(ids=two, min_frames=2, keep_events=True)
    assert res["counts"][:, 0].tolist() == [6, 2, 1, 2, 2] and res["events"].tolist() == [[0, 0, 2, a]]


# ------------------------------------------------------------------------------------------- closed form, no oracle
def test_periodic_pattern_in_closed_form(plan):
    """300 viewers x 5000 frames: viewer u holds one pixel for K frames, then jumps, with phase u mod K — its runs start at
    j K - phase (the first is cut at frame 0, the last at T).  Events, sum_len, max_len, fix_frames and the histogram of every row
    follow from that arithmetic."""
    U, T, K, M = 300, 5000, 7, 3
    u = np.arange(U)
    phase = u % K
    f = np.arange(T)
    block = (f[:, None] + phase[None, :]) // K                   # [T][U]
    pix = np.array([py * (W + 1) + px for py, px in FAR[:2]], dtype=np.int32)
    ids = np.ascontiguousarray(pix[(block + u[None, :]) % 2])
    edges = (1, M, K, K + 1)
    J = T // K + 2
    first = np.arange(J)[None, :] * K - phase[:, None]            # [U][J]: where run j of viewer u would start
    start, end = np.maximum(first, 0), np.minimum(first + K, T)
    L = np.where(end > start, end - start, 0)
    event = L >= M
    run_len = np.take_along_axis(L, (f[None, :] + phase[:, None]) // K, axis=1)       # [U][T]: the length of the frame's run
    start_len = np.zeros((U, T), dtype=np.int64)                  # L at the first frame of every event
    uu, jj = np.nonzero(event)
    start_len[uu, start[uu, jj]] = L[uu, jj]
    for per_user, window, stride in ((False, 50, 25), (True, 50, 25), (False, T, 1), (True, 1000, 1000), (False, 20, 20)):
        a = np.arange((T - window) // stride + 1) * stride

        def rows(x):                                             # [U][R]: the sum of x over the frames of each row
            cs = np.concatenate([np.zeros((U, 1), dtype=np.int64), np.cumsum(x, axis=1, dtype=np.int64)], axis=1)
            return cs[:, a + window] - cs[:, a]
        of_len = {v: rows(start_len == v) for v in range(1, K + 1)}          # the row's events of length v
        per = np.stack([np.full((U, len(a)), window), rows(run_len >= M), rows(start_len > 0), rows(start_len),
                        np.max([v * (of_len[v] > 0) for v in of_len], axis=0)])
        hist = np.stack([sum(of_len[v] for v in of_len if edges[b] <= v < edges[b + 1]) for b in range(3)], axis=-1)    # [U][R][3]
        want_counts = per if per_user else np.concatenate([per[:4].sum(axis=1), per[4:].max(axis=1)])
        want_hist = hist if per_user else hist.sum(axis=0)
        for by in ("angle", "tile"):
            res = plan.fixations(ids=ids, window=window, stride=stride, by=by, max_step_deg=2.0, min_frames=M, per_user=per_user,
                                 edges=edges, keep_events=True)
            assert np.array_equal(res["counts"], want_counts), (by, per_user, window)
            assert np.array_equal(res["hist"], want_hist) and (res["hist"][..., 0] == 0).sum() > 0, (by, per_user, window)
            assert np.array_equal(res["offsets"], np.concatenate([[0], np.cumsum(event.sum(axis=1))]))
            assert np.array_equal(res["events"][:, :3], np.stack([uu, start[uu, jj], L[uu, jj]], axis=1))
    assert event.sum() > 200000 and (L[event] < K).sum() > 300


# ------------------------------------------------------------------------------------------- byte for byte
def test_stride_permutation_extra_column_and_continuation(plan, engine, table, nearest):
    rng = np.random.default_rng(5)
    T, U = 90, 9
    ids = stack([run_ids(random_lengths(T, rng), first=u) for u in range(U)], T)
    for by in ("angle", "tile"):
        hold_of(ids, by, 2.0, table, nearest)                    # the margin condition
        for per_user in (False, True):
            kw = dict(window=8, by=by, max_step_deg=2.0, min_frames=2, per_user=per_user)
            s1 = full(plan, ids=ids, stride=1, **kw)
            for stride in (3, 8):                                # the shared rows
                s = full(plan, ids=ids, stride=stride, **kw)
                assert s["counts"].tobytes() == np.ascontiguousarray(s1["counts"][..., ::stride]).tobytes(), (by, per_user, stride)
                assert s["hist"].tobytes() == np.ascontiguousarray(s1["hist"][..., ::stride, :]).tobytes(), (by, per_user, stride)
                same_bytes(s, s1, f"stride {stride}", keys=("labels", "offsets", "events", "centroids"))
            # a permutation of the viewer columns: pooled rows equal, per-viewer rows, labels and events permute
            perm = rng.permutation(U)
            p = full(plan, ids=np.ascontiguousarray(ids[:, perm]), stride=1, **kw)
            if per_user:
                assert np.array_equal(p["counts"], s1["counts"][:, perm]) and np.array_equal(p["hist"], s1["hist"][perm])
            else:
                assert p["counts"].tobytes() == s1["counts"].tobytes() and p["hist"].tobytes() == s1["hist"].tobytes()
            assert np.array_equal(p["labels"], s1["labels"][perm])
            for new, old in enumerate(perm):
                mine, theirs = p["events"][:, 0] == new, s1["events"][:, 0] == old
                assert np.array_equal(p["events"][mine][:, 1:], s1["events"][theirs][:, 1:])
                assert p["centroids"][mine].tobytes() == s1["centroids"][theirs].tobytes()
            # an added all-absent column
            wide = np.concatenate([ids, np.full((T, 1), -1, dtype=np.int32)], axis=1)
            x = full(plan, ids=wide, stride=1, **kw)
            if per_user:
                assert np.array_equal(x["counts"][:, :U], s1["counts"]) and (x["counts"][:, U] == 0).all() and (x["hist"][U] == 0).all()
            else:
                assert x["counts"].tobytes() == s1["counts"].tobytes() and x["hist"].tobytes() == s1["hist"].tobytes()
            assert np.array_equal(x["labels"][:U], s1["labels"]) and (x["labels"][U] == -1).all()
            assert x["events"].tobytes() == s1["events"].tobytes() and x["offsets"].tolist() == s1["offsets"].tolist() + [s1["offsets"][-1]]
            # the video and its continuation behind an all-absent frame: the rows before the barrier
            more = stack([run_ids(random_lengths(40, rng), first=u + 2) for u in range(U)], 40)
            longer = np.concatenate([ids, np.full((1, U), -1, dtype=np.int32), more])
            hold_of(longer, by, 2.0, table, nearest)
            y = full(plan, ids=longer, stride=1, **kw)
            R = s1["counts"].shape[-1]
            assert np.array_equal(y["counts"][..., :R], s1["counts"]) and np.array_equal(y["hist"][..., :R, :], s1["hist"])
            assert np.array_equal(y["labels"][:, :T], s1["labels"]) and (y["labels"][:, T] == -1).all()
            early = y["events"][:, 1] < T
            assert np.array_equal(y["events"][early], s1["events"]) and y["centroids"][early].tobytes() == s1["centroids"].tobytes()


# ------------------------------------------------------------------------------------------- merged code
def test_agreement_with_head_motion_markov_and_saliency(plan, table, nearest, g15):
    from viewport_entropy_toolkit import _synthetic
    mu, mv, _ = g15
    walk = _synthetic.random_walk_video(40, 300, base_seed=11, p_absent=0.1)
    for a, b in ((mu, mv), walk):
        for deg in (0.0, 2.0):
            hold_of(fo.ids_of(a, b, W, H), "angle", deg, table, nearest)     # the margin condition
        res = plan.fixations(mu=a, mv=b, min_frames=1, max_step_deg=0.0)
        still = plan.head_motion(mu=a, mv=b, lag=1, quantiles=None)["still"]
        assert int(res["counts"][3, 0] - res["counts"][2, 0]) == int(still[0]) > 0
        res = plan.fixations(mu=a, mv=b, min_frames=1, by="tile")
        matrix = plan.transition_markov(mu=a, mv=b, lag=1, want_matrix=True)["matrix"]
        assert int(res["counts"][3, 0] - res["counts"][2, 0]) == int(np.trace(matrix[0])) > 0
        # fixation-based saliency: the masked ids run, and a row's samples are its fix_frames
        ids = fo.ids_of(a, b, W, H)
        for per_user in (False, True):
            fx = plan.fixations(mu=a, mv=b, window=10, stride=5, max_step_deg=2.0, min_frames=3, per_user=per_user, keep_labels=True)
            masked = np.where(fx["labels"].T > 0, ids, -1).astype(np.int32)
            sal = plan.saliency(ids=masked, window=10, stride=5, per_user=per_user, want_map=False)
            assert np.array_equal(sal["counts"][0], fx["counts"][1]) and fx["counts"][1].sum() > 0
            again = plan.fixations(ids=masked, window=10, stride=5, max_step_deg=2.0, min_frames=3, per_user=per_user)
            assert np.array_equal(again["counts"][0], again["counts"][1])


# ------------------------------------------------------------------------------------------- refusals, the range code, the analyzers
def test_illegal_arguments_are_refused_before_anything_runs(native, engine, plan, g15):
    ids = np.array(g15[2][:30])
    T, U = ids.shape
    e = np.array(EDGES, dtype=np.int32)
    good = dict(U=U, T=T, window=5, stride=1, mode=0, cos=cos_of(2.0), m=3, e=e.ctypes.data, B=len(EDGES) - 1, cap=0, events=None,
                centroids=None)
    counts = np.empty((5, 26), dtype=np.int64)
    hist = np.empty((26, len(EDGES) - 1), dtype=np.int32)
    buf = np.empty((64, 4), dtype=np.int32)

    def call(**change):
        a = dict(good, **change)
        return plan.lib.vet_fixations_host(plan.handle, None, None, ids.ctypes.data, a["U"], a["T"], a["window"], a["stride"], a["mode"],
                                           a["cos"], a["m"], 0, a["e"], a["B"], a["cap"], counts.ctypes.data, hist.ctypes.data, None, None,
                                           a["events"], a["centroids"])
    assert call() == native.VET_OK
    bad_e = [np.array(v, dtype=np.int32) for v in ([0, 2, 3, 5, 9, 4000], [1, 2, 2, 5, 9, 4000], [1, 2, 3, 5, 9, 8], [-1, 2, 3, 5, 9, 10])]
    for change in (dict(window=0), dict(window=T + 1), dict(stride=0), dict(m=0), dict(m=-3), dict(mode=2), dict(mode=-1),
                   dict(cos=float("nan")), dict(B=-1), dict(B=65), dict(e=None), dict(cap=-1),
                   dict(centroids=buf.ctypes.data, cap=4), *(dict(e=v.ctypes.data) for v in bad_e)):
        assert call(**change) == native.VET_ERR_INVALID, change
    assert call(cos=2.0) == call(cos=-3.0) == native.VET_OK      # only NaN is refused: the cosine is compared, never inverted
    # refused before the samples are read: the shapes below are far beyond the array
    assert call(U=60000, T=40000, window=40000) == native.VET_ERR_UNSUPPORTED
    assert call(U=1, T=65535 * 64 + 1, window=1) == native.VET_ERR_UNSUPPORTED
    for args in ((8, 8, 4, 30, 31, 1, "angle", 0.5, 3, False), (8, 8, 4, 30, 5, 1, "angle", 0.5, 0, False),
                 (8, 8, 4, 30, 5, 1, "angle", float("nan"), 3, True)):
        with pytest.raises(native.NativeError) as err:           # the device entries refuse before they look at a pointer
            plan.fixations_device(*args, d_counts=8)
        assert err.value.code == native.VET_ERR_INVALID
    with pytest.raises(native.NativeError) as err:
        plan.fixations_device(8, 8, 60000, 40000, 40000, 1, "tile", 0.5, 3, False, d_counts=8)
    assert err.value.code == native.VET_ERR_UNSUPPORTED
    for bad in (dict(max_step_deg=-1.0), dict(min_frames=0), dict(edges=(0, 1)), dict(by="gaze"), dict(window=0), dict(stride=0),
                dict(keep_centroids=True)):
        with pytest.raises(ValueError):
            plan.fixations(ids=ids, **bad)
    assert engine.lib.vet_test_fixation_chunk(engine.handle, 6) == native.VET_ERR_INVALID         # not a multiple of 4
    assert engine.lib.vet_test_fixation_chunk(engine.handle, -4) == native.VET_ERR_INVALID


def test_sample_out_of_range(native, plan, g15):
    mu, mv, ids = (np.array(a[:20]) for a in g15)
    mu[3, 2] = 1.5
    with pytest.raises(native.NativeError) as e:
        plan.fixations(mu=mu, mv=mv)
    assert e.value.code == native.VET_ERR_RANGE
    res = plan.fixations(mu=mu, mv=mv, min_frames=2, keep_labels=True, keep_events=True, check=False)
    assert res["code"] == native.VET_ERR_RANGE                    # the outputs are still written: the sample counts as absent
    ids[3, 2] = -1
    same_bytes(res, plan.fixations(ids=ids, min_frames=2, keep_labels=True, keep_events=True), "range", keys=INT_KEYS)
    assert res["labels"][2, 3] == -1


def test_analyzers_against_the_plan_call(g15):
    from viewport_entropy_toolkit import SpatialEntropyAnalyzer, TransitionEntropyAnalyzer, ValidationError
    from viewport_entropy_toolkit.analyzers import NaiveSpatialEntropyAnalyzer
    from viewport_entropy_toolkit.config import AnalyzerConfig, NaiveAnalyzerConfig
    mu, mv, ids = g15
    T, U = ids.shape
    times = np.arange(T) / 30.0
    bins = (1, 2, 4, 8, 61)
    for cls in (SpatialEntropyAnalyzer, TransitionEntropyAnalyzer, NaiveSpatialEntropyAnalyzer):
        an = cls(NaiveAnalyzerConfig(tile_height=10, tile_width=20, video_width=W, video_height=H)) \
            if cls is NaiveSpatialEntropyAnalyzer else cls(AnalyzerConfig(tile_counts=[50], video_width=W, video_height=H))
        an.load_arrays(times, mu.copy(), mv.copy())
        for by in ("angle", "tile"):
            for per_user in (False, True):
                df = an.compute_fixations(window=7, stride=3, by=by, min_frames=2, per_user=per_user, bins_frames=bins,
                                          keep_labels=True, keep_events=True)
                ref = an._grid_plan().fixations(mu=mu, mv=mv, window=7, stride=3, by=by, max_step_deg=2.0, min_frames=2,
                                                per_user=per_user, edges=bins, keep_labels=True, keep_events=True, keep_centroids=True)
                counts = ref["counts"].reshape(5, -1)
                assert len(df) == counts.shape[1] == (18 * U if per_user else 18)
                for col, k in (("samples", 0), ("fix_frames", 1), ("events", 2), ("max_frames", 4)):
                    assert np.array_equal(df[col].to_numpy(), counts[k]), (cls.__name__, by, per_user, col)
                has = counts[2] > 0
                assert np.array_equal(df["mean_frames"].to_numpy()[has], counts[3][has] / counts[2][has])
                assert np.isnan(df["mean_frames"].to_numpy()[~has]).all()
                assert np.array_equal(np.stack(list(df["hist"])), ref["hist"].reshape(-1, 4))
                assert np.array_equal(df.attrs["labels"], ref["labels"].T) and df.attrs["labels"].shape == (T, U)
                ev = df.attrs["events"]
                assert np.array_equal(ev["frame"].to_numpy(), ref["events"][:, 1]) and np.array_equal(ev["dir"].to_numpy(), ref["events"][:, 3])
                assert len(ev) == int(ref["offsets"][-1]) > 0 and ev["lat"].between(-90, 90).all() and ev["lon"].between(-180, 180).all()
                assert df.attrs["by"] == by and df.attrs["cos_threshold"] == cos_of(2.0) and df.attrs["min_frames"] == 2
                assert (df["time"].to_numpy()[:18] == times[::3][:18]).all() and df.attrs["frame_seconds"] == float(np.median(np.diff(times)))
        # seconds: 60 degrees per second at 30 frames per second is 2 degrees per frame, as far as the product rounds
        by_rate = an.compute_fixations(velocity_deg_s=60.0, min_seconds=0.1)
        assert by_rate.attrs["min_frames"] == math.ceil(0.1 / df.attrs["frame_seconds"]) and abs(by_rate.attrs["max_step_deg"] - 2.0) < 1e-12
        whole = an.compute_fixations()
        assert len(whole) == 1 and whole["time_end"][0] == times[-1] and whole.attrs["max_step_deg"] == 2.0 and whole.attrs["min_frames"] == 5
        assert "hist" not in whole and "labels" not in whole.attrs and "events" not in whole.attrs and whole["events"][0] == 4
        bad = mu.copy()
        bad[5, 1] = -0.25
        with pytest.raises(ValidationError):                     # samples outside [0, 1] never reach the engine
            an.load_arrays(times, bad, mv.copy())
