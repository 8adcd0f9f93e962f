"""The capped table kernels of one, two and three blocks (k_spatial_lut<NB>, csrc/vet_spatial.hip: lut_kernel) on plans that
cap at 64, 128 and 192 entries (tests/_cap_plans.py; test_row_cap_plans.py shows on the CPU why these plans cap there).

Every call is held against two references:
  * the FP64 oracle (oracle/vet_oracle.py, the reference's arithmetic in numpy): assignments and present counts equal, entropy
    at the table formulations' contract (rtol 1e-6), and, from the weights pass, tile weights within tests/_tol.py;
  * the uncapped layout of the same plan (vet_test_no_row_cap: whole rows of stride cap + 64 through the NB == 0 kernel), bit
    for bit: entropy bytes, assignments, present counts and the table's own histogram.  Integer adds commute.
The first catches an error that both layouts share, the second a single wrong entry below the entropy tolerance.

Which kernel served a call is read from Plan.last_table_kernel(), never inferred from the shape; the last test of the module
holds the set of capped kernels it has seen against the 24 that lut_kernel can return.

Shown to bite: with the main walk of walk_rows<NB == 3> stopped one block early (fewer loads, nothing out of bounds; never
committed) every test of the two 192-cap plans that runs samples failed, the oracle comparison (entropy off by 3-10 %) and
the bit comparison each on their own, and the 64- and 128-cap plans passed."""
import numpy as np
import pytest

from oracle import vet_oracle as vo
from tests import _cap_plans as cp
from tests._tol import W_RTOL, w_atol

pytestmark = pytest.mark.gpu

W, H, N_DIRS, POWER = cp.W, cp.H, cp.N_DIRS, cp.POWER
RTOL = 1e-6                                     # the table formulations' contract (test_rec32.check_against_oracle, smoke())

# what a capped launch must report per form; nb, il, occ8, fp_table, fused and from_ids are checked for every form
FORMS = {
    "rec8": dict(rec32=False, bucketed=False, dedup=False, batch=False),                 # fewer than 128 users: no set
    "rec8_set": dict(rec32=False, bucketed=False, dedup=True, batch=False),              # vet_test_rec8, 128 users or more
    "bucketed": dict(rec32=True, bucketed=True, dedup=True, batch=False, chunked=False, fpw=1),
    "chunked": dict(rec32=True, bucketed=False, dedup=True, batch=False, chunked=True),
    "batch": dict(rec32=True, bucketed=False, dedup=True, batch=True),
    "fpw": dict(rec32=True, bucketed=False, dedup=True, batch=False, chunked=False),     # and fpw >= 2, asserted by its test
}
# (nb, rec32, bucketed, dedup, from_ids) of every capped launch of this module that passed both comparisons
SEEN = set()


@pytest.fixture(scope="module")
def native():
    from viewport_entropy_toolkit import _native
    return _native


@pytest.fixture(scope="module")
def engines(native):
    """(capped, uncapped): the switch belongs to the engine and is read when a plan builds its table"""
    capped, whole = native.Engine(0), native.Engine(0)
    whole.test_no_row_cap(True)
    yield capped, whole
    whole.close()
    capped.close()


class Ctx:
    """one plan in both layouts, with what the tests share: the oracle's tables and every direction as a one-user frame"""

    def __init__(self, native, engines, key):
        self.key, (self.tc, self.fov), self.cap = key, key, cp.CAPPED_PLANS[key]
        self.nb = self.cap // 64
        self.eng = engines[0]
        self.tiles = vo.fibonacci_lattice(self.tc)
        self.n = len(self.tiles)
        self.flat = vo.direction_grid(W, H).reshape(-1, 3)
        self.near = vo.nearest_tile(self.flat, self.tiles)
        self.a, self.b = (self.make(native, e) for e in engines)
        self.maxdev, self.calls = 0.0, []
        one = np.arange(N_DIRS, dtype=np.int32).reshape(N_DIRS, 1)
        self.one = one
        self.ra = self.a.spatial(ids=one, want_weights=True)
        self.da = self.a.last_table_kernel()
        self.rb = self.b.spatial(ids=one, want_weights=True)
        self.db = self.b.last_table_kernel()
        # a direction's row = the non-zero slots of its one-user frame (every in-FoV tile has a mantissa >= 1)
        self.per_dir = np.count_nonzero(self.rb["weights"], axis=1)
        self.ovf_dirs = np.flatnonzero(self.per_dir > self.cap).astype(np.int32)
        self.one_ent = None

    def make(self, native, engine):
        plan = native.Plan(engine, [self.tiles], self.fov, POWER, True, W, H)
        plan.set_table_policy(1)
        plan.set_raw_weights(True)            # the table's own histogram: what the two layouts are compared on
        return plan

    def close(self):
        self.a.close()
        self.b.close()


@pytest.fixture(scope="module", params=sorted(cp.CAPPED_PLANS), ids=lambda p: f"{p[0]}@{p[1]:g}")
def P(request, native, engines):
    ctx = Ctx(native, engines, request.param)
    yield ctx
    ctx.close()


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def walk_video(U, T, seed, p_absent=0.1):
    rng = np.random.default_rng(seed)
    mu = np.mod(0.5 + np.cumsum(rng.normal(0, 0.02, (T, U)), axis=0) + rng.random((1, U)), 1.0)
    mv = np.clip(0.5 + np.cumsum(rng.normal(0, 0.01, (T, U)), axis=0) + rng.normal(0, 0.2, (1, U)), 0.0, 1.0)
    gone = rng.random((T, U)) < p_absent
    gone[np.arange(T), rng.integers(0, U, T)] = False
    mu[gone] = np.nan
    mv[gone] = np.nan
    return mu, mv


def ids_of(mu, mv):
    """direction ids as the reference forms them (truncation of mu * W, mv * H), -1 = absent"""
    px, py, present, _ = vo.sample_directions(mu, mv, W, H)
    return np.where(present, py * (W + 1) + px, -1).astype(np.int32)


def uv_of(ids):
    """a point inside the pixel of every direction id (the last column and row: the edge itself), NaN = absent"""
    d = np.maximum(ids, 0)
    mu = np.minimum((d % (W + 1) + 0.25) / W, 1.0)
    mv = np.minimum((d // (W + 1) + 0.25) / H, 1.0)
    gone = ids < 0
    mu[gone] = np.nan
    mv[gone] = np.nan
    return mu, mv


def overflow_frames(P, U, T, rng):
    """frames of overflow directions only, 5 % of the users absent, a multiplicity above 1 in every frame"""
    ids = P.ovf_dirs[rng.integers(0, P.ovf_dirs.size, (T, U))]
    if U > 1:
        ids[rng.random((T, U)) < 0.05] = -1
        ids[:, 0] = ids[:, 1] = P.ovf_dirs[0]
    return ids


# ---- the two references ---------------------------------------------------------------------------------------------------
def oracle(P, ids, frames, with_weights=False):
    """(entropy, tile weights or None) of frames `frames` of ids [T, U] as the reference computes them: the users' weight rows
    added in column order; NaN for a frame without users"""
    ent = np.full(len(frames), np.nan)
    weights = np.zeros((len(frames), P.n)) if with_weights else None
    group, held = [], 0

    def flush():
        if not group:
            return
        every = np.concatenate([ids[t][ids[t] >= 0] for _, t in group])
        rows, keys = vo.tile_weight_rows(P.flat[every], P.tiles, P.fov, POWER, True, return_keys=True)
        at = 0
        for i, t in group:
            m = int((ids[t] >= 0).sum())
            hist = np.zeros(P.n)
            for r in rows[at:at + m]:
                hist += r
            touched = keys[at:at + m].any(axis=0)
            ent[i] = vo.spatial_entropy_from_hist(hist, touched, P.n, True)
            if with_weights:
                weights[i] = np.where(touched & (hist == 0), -0.0, hist)
            at += m
        group.clear()

    for i, t in enumerate(frames):
        m = int((ids[t] >= 0).sum())
        if m == 0:
            continue
        if held + m > 4096:
            flush()
            held = 0
        group.append((i, t))
        held += m
    flush()
    return ent, weights


def against_oracle(P, res, ids, frames=None, want=None, with_weights=False):
    """assignments, present counts, entropy at the contract; returns the oracle's (entropy, weights) for reuse"""
    T = ids.shape[0]
    frames = list(range(T)) if frames is None else list(frames)
    assert np.array_equal(res["assign"], np.where(ids >= 0, P.near[np.maximum(ids, 0)], -1))
    assert np.array_equal(res["present"], (ids >= 0).sum(axis=1))
    ent, weights = oracle(P, ids, frames, with_weights) if want is None else want
    got = res["entropy"][frames]
    assert np.array_equal(np.isnan(got), np.isnan(ent)), "NaN exactly where the frame has no user"
    ok = ~np.isnan(ent)
    if ok.any():
        P.maxdev = max(P.maxdev, float(np.max(np.abs(got[ok] - ent[ok]) / np.abs(ent[ok]).clip(1e-300))))
    np.testing.assert_allclose(got, ent, rtol=RTOL, equal_nan=True)
    return ent, weights


def same_bits(x, y):
    assert x["code"] == y["code"]
    assert x["entropy"].tobytes() == y["entropy"].tobytes()
    assert np.array_equal(x["assign"], y["assign"])
    assert np.array_equal(x["present"], y["present"])
    if x.get("weights") is not None:
        assert x["weights"].tobytes() == y["weights"].tobytes()


def both_references(P, x, y, ids, frames=None, want=None, with_weights=False):
    """x against the oracle and against y, the uncapped layout's result: both comparisons run, and a failure names each that
    failed (so that either is seen to catch an error on its own); returns the oracle's values for reuse"""
    failed = []
    try:
        want = against_oracle(P, x, ids, frames, want, with_weights)
    except AssertionError as e:
        failed.append(f"against the oracle: {str(e).strip()[:400]}")
    try:
        same_bits(x, y)
    except AssertionError as e:
        failed.append(f"against the uncapped layout: {str(e).strip()[:400]}")
    assert not failed, f"{P.key}: " + " | ".join(failed)
    return want


def expect(P, form, d, from_ids, shape):
    """the descriptor of a capped launch of this form"""
    want = dict(FORMS[form], nb=P.nb, il=True, occ8=True, fp_table=False, fused=False, narrow=False, from_ids=from_ids)
    got = {k: d.get(k) for k in want}
    P.calls.append((form, shape, d))
    print(f"{P.key} cap {P.cap} {form} {shape}: {tag(d)}")
    assert got == want, (P.key, form, shape, d)


def expect_whole(P, d, from_ids, users, batch=False):
    """the uncapped layout runs the class-dealt kernel over whole rows"""
    want = dict(nb=0, rec32=False, bucketed=False, il=True, occ8=True, fp_table=False, fused=False, dedup=users >= 128,
                from_ids=from_ids, batch=batch)
    assert {k: d.get(k) for k in want} == want, (P.key, d)


def tag(d):
    return " ".join(f"{k}={int(v)}" for k, v in d.items())


def seen(P, form, from_ids):
    f = FORMS[form]
    SEEN.add((P.nb, f["rec32"], f["bucketed"], f["dedup"], from_ids))


def case(P, form, ids, uv=None, entries=("ids", "uv"), frames=None, weights=False, want=None):
    """one input through both entry points: each against the uncapped layout bit for bit and against the oracle"""
    T, U = ids.shape
    first = None
    P.eng.test_rec8(form == "rec8_set")
    try:
        for entry in entries:
            kw = dict(ids=ids) if entry == "ids" else dict(zip(("mu", "mv"), uv if uv is not None else uv_of(ids)))
            x = P.a.spatial(want_weights=True, check=False, **kw)
            assert P.a.last_formulation(0) == "table"
            expect(P, form, P.a.last_table_kernel(), entry == "ids", (U, T))
            y = P.b.spatial(want_weights=True, check=False, **kw)
            assert P.b.last_formulation(0) == "table"
            expect_whole(P, P.b.last_table_kernel(), entry == "ids", U)
            want = both_references(P, x, y, ids, frames, want, weights)
            if weights:
                P.a.set_raw_weights(False)
                try:
                    z = P.a.spatial(want_weights=True, check=False, **kw)
                finally:
                    P.a.set_raw_weights(True)
                assert z["entropy"].tobytes() == x["entropy"].tobytes()
                sel = list(range(T)) if frames is None else list(frames)
                np.testing.assert_allclose(z["weights"][sel], want[1], rtol=W_RTOL, atol=w_atol(U, POWER))
            if first is not None:                               # the two entry points: the same samples, the same bits
                same_bits(first, x)
            first = x
            seen(P, form, entry == "ids")
    finally:
        P.eng.test_rec8(False)
    return first, want


def form_of(U):
    return "rec8" if U < 128 else "bucketed" if U <= 2048 else "chunked"


# ---- the plans ------------------------------------------------------------------------------------------------------------
def test_the_plan_caps_at_the_expected_block_count(P):
    assert P.a.last_formulation(0) == P.b.last_formulation(0) == "table"
    cap, n_ovf = P.a.table_cap(0)
    rows = P.a.table_rows()
    print(f"{P.key}: {P.n} tiles, cap {cap}, {n_ovf} overflow rows of {rows}, {P.ovf_dirs.size} overflow directions "
          f"(longest row {P.per_dir.max()}); uncapped stride {P.b.table_stride(0)}")
    assert cap == P.cap and P.a.table_stride(0) == P.cap
    assert 1 <= n_ovf <= rows // 32
    assert P.a.record_bytes() == 4
    assert P.b.table_cap(0) == (P.cap + 64, 0) and P.b.table_stride(0) == P.cap + 64 and P.b.record_bytes() == 8
    assert n_ovf <= P.ovf_dirs.size <= N_DIRS // 32 + 1 and P.per_dir.max() <= P.cap + 64
    assert P.ovf_dirs.size > n_ovf, "mirrored partners share a row: both are among the overflow directions"
    assert np.array_equal(P.per_dir, cp.row_lengths(P.tc, P.fov)), "the rows are the oracle's in-FoV tile sets"


def test_the_table_is_the_uncapped_one_cut_at_the_cap(P):
    """main plus overflow entries of every row are the uncapped row; the side table is numbered densely in row order; meta
    bit 15 marks exactly the overflow rows; the shift is unchanged; the last side-table row is all zero"""
    cap, n_ovf = P.a.table_cap(0)
    ta, tb = P.a.read_table(0), P.b.read_table(0)
    rows = P.a.table_rows()
    assert ta["w"].shape == (rows + 1, cap) and tb["w"].shape == (rows + 1, cap + 64)
    assert ta["ovf_w"].shape == (n_ovf + 1, 64) and not ta["ovf_w"][n_ovf].any()
    assert not ta["w"][rows].any() and not tb["w"][rows].any()
    ovf_of_row = ta["ovf_of_row"]
    has = ovf_of_row != 0xFFFFFFFF
    assert np.array_equal(ovf_of_row[has], np.arange(n_ovf, dtype=np.uint32)), "numbered densely, in row order"
    assert np.array_equal((ta["meta"][:rows] >> 15) & 1, has.astype(np.uint32))
    assert np.array_equal(ta["meta"][:rows] >> 16, tb["meta"][:rows] >> 16), "the row shift is unchanged"
    len_a, len_b = ta["meta"][:rows] & 0xFFF, tb["meta"][:rows] & 0xFFF
    assert np.array_equal(has, len_b > cap)
    assert np.array_equal(len_a, np.minimum(len_b, cap))
    assert ta["tile"].max() < P.n and tb["tile"].max() < P.n and ta["ovf_tile"].max() < P.n

    def dense(w, t, at):
        """[rows, tiles] mantissa of every (row, tile); a tile occurs once per row"""
        out = np.zeros((rows, P.n), dtype=np.int64)
        np.add.at(out, (np.broadcast_to(at[:, None], w.shape), t), w)
        count = np.zeros(rows, dtype=np.int64)
        np.add.at(count, at, np.count_nonzero(w, axis=1))
        return out, count
    every = np.arange(rows)
    whole, n_whole = dense(tb["w"][:rows], tb["tile"][:rows], every)
    main, n_main = dense(ta["w"][:rows], ta["tile"][:rows], every)
    tail, n_tail = dense(ta["ovf_w"][:n_ovf], ta["ovf_tile"][:n_ovf], np.flatnonzero(has))
    assert np.array_equal(n_whole, len_b) and np.array_equal(np.count_nonzero(whole, axis=1), len_b)
    assert np.array_equal(n_main, len_a) and np.array_equal(n_tail, len_b - len_a)
    assert not ((main != 0) & (tail != 0)).any(), "an entry is in the main row or in the side table, not in both"
    assert np.array_equal(main + tail, whole)


# ---- inputs that walk every row -------------------------------------------------------------------------------------------
def test_every_direction_as_a_one_user_frame(P):
    """all 20 301 directions, each a frame of one user: every row and every overflow row walked once, alone"""
    expect(P, "rec8", P.da, True, (1, N_DIRS))
    expect_whole(P, P.db, True, 1)
    P.one_ent = both_references(P, dict(P.ra, code=0), dict(P.rb, code=0), P.one)
    seen(P, "rec8", True)
    # the histogram of a one-user frame is the direction's row: as many non-zero slots as the oracle has tiles in the FoV
    assert np.array_equal(np.count_nonzero(P.ra["weights"], axis=1), P.per_dir)
    uv = uv_of(P.one)
    x = P.a.spatial(mu=uv[0], mv=uv[1], want_weights=True)
    expect(P, "rec8", P.a.last_table_kernel(), False, (1, N_DIRS))
    same_bits(x, P.ra)
    seen(P, "rec8", False)


def test_every_direction_through_the_kernels_with_the_set(P):
    """each direction the only present user of a 128-user frame (compact record, several frames per workgroup), and all of
    them once in 20 frames of 1 024 users (bucket-ordered lists; the 8-byte record with the set)"""
    if P.one_ent is None:
        P.one_ent = oracle(P, P.one, list(range(N_DIRS)))
    ids = np.full((N_DIRS, 128), -1, dtype=np.int32)
    ids[np.arange(N_DIRS), np.arange(N_DIRS) % 128] = np.arange(N_DIRS)
    x, _ = case(P, "fpw", ids, entries=("ids",), want=P.one_ent)
    assert x["entropy"].tobytes() == P.ra["entropy"].tobytes() and x["weights"].tobytes() == P.ra["weights"].tobytes()
    packed = np.full(20 * 1024, -1, dtype=np.int32)
    packed[:N_DIRS] = np.random.default_rng(1).permutation(N_DIRS)
    packed = packed.reshape(20, 1024)
    _, want = case(P, "bucketed", packed)
    case(P, "rec8_set", packed, want=want)


def test_frames_of_overflow_directions(P):
    """every user in a direction whose row continues in the side table: the overflow list of a frame filled to its bound"""
    rng = np.random.default_rng(5)
    print(f"{P.key}: {P.ovf_dirs.size} overflow directions")
    for U, T in ((1, P.ovf_dirs.size), (64, 10), (256, 8), (1024, 4), (3000, 3)):
        ids = overflow_frames(P, U, T, rng) if U > 1 else P.ovf_dirs.reshape(T, 1).copy()
        x, want = case(P, form_of(U), ids)
        assert np.isfinite(x["entropy"]).all()
        if U >= 128:
            case(P, "rec8_set", ids, want=want)


def test_overflow_directions_among_others(P):
    """half and half"""
    rng = np.random.default_rng(6)
    for U, T in ((100, 8), (512, 12), (3000, 3)):
        ids = rng.integers(0, N_DIRS, (T, U)).astype(np.int32)
        ids[:, ::2] = P.ovf_dirs[rng.integers(0, P.ovf_dirs.size, (T, (U + 1) // 2))]
        _, want = case(P, form_of(U), ids)
        if U >= 128:
            case(P, "rec8_set", ids, want=want)


# ---- every kernel form on a random-walk video -----------------------------------------------------------------------------
@pytest.mark.parametrize("form,U,T", [("rec8", 100, 12), ("rec8_set", 300, 8), ("bucketed", 700, 10), ("chunked", 3000, 3)])
def test_random_walk_video(P, form, U, T):
    """absent users; both entry points; entropy, assignments and (weights pass) tile weights against the oracle"""
    mu, mv = walk_video(U, T, seed=1000 + U)
    x, _ = case(P, form, ids_of(mu, mv), uv=(mu, mv), weights=True)
    assert np.isfinite(x["entropy"]).all()


def test_random_walk_videos_in_one_batch_launch(P):
    vids = [walk_video(160, 6, seed=31), walk_video(60, 9, seed=32), walk_video(3, 11, seed=33, p_absent=0.3)]
    xs = P.a.spatial_batch(vids, want_assign=True, check=False)
    expect(P, "batch", P.a.last_table_kernel(), False, [v[0].shape[::-1] for v in vids])
    assert P.a.last_formulation(0) == "table"
    ys = P.b.spatial_batch(vids, want_assign=True, check=False)
    expect_whole(P, P.b.last_table_kernel(), False, 160, batch=True)
    for x, y, (mu, mv) in zip(xs, ys, vids):
        both_references(P, dict(x, code=0), dict(y, code=0), ids_of(mu, mv))
    seen(P, "batch", False)


def test_frames_with_one_user_and_with_none(P, native):
    """the reference's NaN row: a frame without users is NaN on every path, and does not disturb its neighbours"""
    for form, U, T in (("rec8", 100, 6), ("bucketed", 300, 6), ("rec8_set", 300, 6), ("chunked", 3000, 4)):
        ids = ids_of(*walk_video(U, T, seed=50 + U))
        ids[1] = -1
        ids[1, U // 2] = int(P.ovf_dirs[0])                # one present user, in an overflow direction
        ids[2] = -1                                        # none
        x, _ = case(P, form, ids)
        assert x["code"] == native.VET_ERR_EMPTY
        assert np.isnan(x["entropy"][2]) and x["present"][2] == 0 and (x["assign"][2] == -1).all()
        assert x["present"][1] == 1 and np.isfinite(np.delete(x["entropy"], 2)).all()
        assert x["entropy"][1].tobytes() == P.ra["entropy"][P.ovf_dirs[0]].tobytes()


def test_several_frames_per_workgroup(P):
    """2 560 frames of 128 users: two frames per workgroup on a 256-CU device (lut_frames_per_wg).  Every frame against the
    uncapped layout, every 16th against the oracle (frames are independent)."""
    mu, mv = walk_video(128, 2560, seed=77)
    ids = ids_of(mu, mv)
    case(P, "fpw", ids, uv=(mu, mv), frames=range(0, 2560, 16))
    d = P.calls[-1][2]
    assert d["fpw"] >= 2, f"{P.key}: 2560 frames x 128 users ran {d['fpw']} frame(s) per workgroup: {tag(d)}"


def test_report(P):
    print(f"{P.key}: cap {P.cap}, overflow rows {P.a.table_cap(0)[1]}, {len(P.calls)} capped launches checked, "
          f"largest entropy deviation from the oracle {P.maxdev:.3e} (contract {RTOL:g})")
    assert P.calls and P.maxdev <= RTOL


def test_all_capped_kernels_were_reached():
    """lut_kernel's capped instantiations: per block count and entry point the 8-byte record without and with the set of
    distinct rows, the compact record, and the compact record with bucket-ordered lists"""
    want = {(nb, rec32, bucketed, dedup, from_ids)
            for nb in (1, 2, 3) for from_ids in (False, True)
            for rec32, bucketed, dedup in ((False, False, False), (False, False, True), (True, False, True), (True, True, True))}
    assert len(want) == 24
    assert SEEN == want, f"missing {sorted(want - SEEN)}, unexpected {sorted(SEEN - want)}"


# ---- what the other table kernels run -------------------------------------------------------------------------------------
def census_oracle(res, mu, mv, tcs, fov):
    ent, assign = vo.spatial_series(mu, mv, W, H, tcs, fov_angle=fov, power_factor=POWER)[:2]
    assert np.array_equal(res["assign"], assign)
    np.testing.assert_allclose(res["entropy"], ent, rtol=RTOL)


def test_census_of_the_other_table_kernels(native, engines):
    """The dispatch rules of launch_lut / launch_lut_fused on a default engine: which kernel a small call of each kind runs."""
    eng = engines[0]
    eng.test_rec8(False)
    base = dict(nb=0, rec32=False, bucketed=False, batch=False, chunked=False)
    # (tile counts, fov, users, frames) -> descriptor
    # Fused rows (tiles of all lattices inside fov / 2 of a direction, counted with the oracle's geometry): [20, 50] 14..22,
    # [50, 100] 33..43, [50, 100, 200] 81..94, the reference's defaults 344..366.  8-lane groups (narrow) for rows of 17..32
    # and 65..96 entries, 16-lane groups beyond; class-dealt blocks (il) from 24 resp. 48 entries on (ensure_fused).
    narrow = dict(base, fused=True, narrow=True, il=True, fp_table=False)
    wide = dict(base, fused=True, narrow=False, il=True, occ8=False, fp_table=False)
    calls = [
        ([20, 50], 120.0, 100, 8, dict(narrow, il=False, dedup=False, occ8=False)),
        ([20, 50], 120.0, 300, 8, dict(narrow, il=False, dedup=True, occ8=True)),
        ([50, 100], 120.0, 100, 8, dict(wide, il=False, dedup=False)),
        ([50, 100], 120.0, 300, 8, dict(wide, il=False, dedup=True)),
        ([50, 100, 200], 120.0, 100, 8, dict(narrow, dedup=False, occ8=False)),
        ([50, 100, 200], 120.0, 300, 8, dict(narrow, dedup=True, occ8=True)),
        ([20, 50, 100, 250, 1000], 120.0, 100, 4, dict(wide, dedup=False)),
        ([20, 50, 100, 250, 1000], 120.0, 256, 4, dict(wide, dedup=True)),
        ([500], 10.0, 200, 6, dict(base, fused=False, narrow=False, fp_table=True, occ8=False, il=False, dedup=True)),
        ([500], 10.0, 60, 6, dict(base, fused=False, narrow=False, fp_table=True, occ8=False, il=False, dedup=False)),
        # [500] at fov 122: two thirds of the rows are longer than 128 entries, so no cap qualifies (test_row_cap_plans.py)
        ([500], 122.0, 300, 6, dict(base, fused=False, narrow=False, fp_table=False, occ8=True, il=True, dedup=True)),
        ([500], 122.0, 100, 6, dict(base, fused=False, narrow=False, fp_table=False, occ8=True, il=True, dedup=False)),
        ([50], 120.0, 200, 6, dict(base, fused=False, narrow=False, fp_table=False, occ8=True, il=False, dedup=True)),
        ([50], 120.0, 60, 6, dict(base, fused=False, narrow=False, fp_table=False, occ8=True, il=False, dedup=False)),
    ]
    plans = {}
    try:
        for tcs, fov, U, T, want in calls:
            key = (tuple(tcs), fov)
            if key not in plans:
                plans[key] = native.Plan(eng, [vo.fibonacci_lattice(tc) for tc in tcs], fov, POWER, True, W, H)
                plans[key].set_table_policy(1)
                assert plans[key].last_table_kernel() == {}, "empty before any table launch"
            plan = plans[key]
            mu, mv = walk_video(U, T, seed=U + T)
            for from_ids in (False, True):
                res = plan.spatial(ids=ids_of(mu, mv)) if from_ids else plan.spatial(mu=mu, mv=mv)
                d = plan.last_table_kernel()
                print(f"{tcs} fov {fov:g} {U} x {T}: {plan.last_formulation(0)} {tag(d)}")
                assert plan.last_formulation(0) == ("ftable" if want["fp_table"] else "table")
                assert {k: d[k] for k in want} == want and d["from_ids"] == from_ids and d["fpw"] == 1, (tcs, fov, U, d)
                census_oracle(res, mu, mv, tcs, fov)
        # a batch over the fused table, and one over a lattice's own whole rows
        vids = [walk_video(160, 5, seed=41), walk_video(40, 7, seed=42)]
        for key, want in ((((50, 100, 200), 120.0), dict(narrow, dedup=True, occ8=False, batch=True)),
                          (((20, 50), 120.0), dict(narrow, il=False, dedup=True, occ8=False, batch=True)),
                          (((50,), 120.0), dict(base, fused=False, fp_table=False, occ8=True, il=False, dedup=True, batch=True))):
            plan = plans[key]
            out = plan.spatial_batch(vids, want_assign=True)
            d = plan.last_table_kernel()
            print(f"{key} batch: {tag(d)}")
            assert {k: d[k] for k in want} == want and not d["from_ids"] and d["fpw"] == 0, (key, d)
            for res, (mu, mv) in zip(out, vids):
                census_oracle(res, mu, mv, list(key[0]), key[1])
    finally:
        for plan in plans.values():
            plan.close()
