"""The compact-record table kernel's way to its row walk.  Its young phases (sample loads, record gathers, set inserts, the
slot-number -> walk-word pass) run at a raised wave priority, the walk at priority 0; the shapes below are those at which a
reordered prologue can go wrong, and they were chosen for the variants measured beside the priority raise as well (first round
of sample loads ahead of the LDS initialisation, one barrier for the first chunk, histogram beside the set:
tools/experiments/early_walk_variants.patch).  Nothing of this changes what is added, and integer adds commute: entropy,
assignments, present counts and the table's own histogram must equal the forced 8-byte-record kernel (vet_test_rec8), which
keeps the earlier prologue, as bytes.  One case is also held against the numpy oracle, so the file does not rest on the
sibling kernel alone.

User counts: 128 (the smallest frame that keeps the set), 129, 1 024 (exactly one round of four samples per thread), 1 025 (a
second round of one sample), 2 048 (the largest single chunk), 2 049 and 4 096 (two chunks: histogram and set apart by
construction, the second chunk must not clear the histogram).  Frame counts 1, 3 and 7."""
import numpy as np
import pytest

from oracle import vet_oracle as vo

pytestmark = pytest.mark.gpu

W, H = 100, 200
N_DIRS = (W + 1) * (H + 1)
USERS = (128, 129, 1024, 1025, 2048, 2049, 4096)
FRAMES = (1, 3, 7)
SET_MIN_USERS = 128          # vet_layout.hpp: DEDUP_MIN_USERS, also the least number of slots of a frame's overflow list


@pytest.fixture(scope="module")
def native():
    from viewport_entropy_toolkit import _native
    return _native


@pytest.fixture(scope="module")
def engine(native):
    e = native.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def plan(native, engine):
    """the config-3 plan shape (the fixtures of tests/test_rec32.py), its table built"""
    p = native.Plan(engine, [vo.fibonacci_lattice(500)], 120.0, 2.0, True, W, H)
    p.set_table_policy(1)
    p.set_raw_weights(True)
    p.spatial(mu=np.full((1, 1), 0.5), mv=np.full((1, 1), 0.5))
    yield p
    p.close()


@pytest.fixture(scope="module")
def overflow(plan):
    """directions whose row continues in the side table, found as tests/test_row_cap.py finds them: the one-user frame of such
    a direction has more non-zero slots than a main row holds.  Computed once; (directions, their set keys row | mirrored << 15)"""
    cap, n_ovf = plan.table_cap(0)
    one = np.arange(N_DIRS, dtype=np.int32).reshape(N_DIRS, 1)
    per_dir = np.count_nonzero(plan.spatial(ids=one, want_weights=True)["weights"], axis=1)
    dirs = np.flatnonzero(per_dir > cap).astype(np.int32)
    rec = plan.read_records()
    assert np.array_equal(np.flatnonzero(rec >> 31), dirs), "the record's overflow bit marks the same directions"
    assert dirs.size > n_ovf >= 1
    return dirs, rec[dirs] & 0xFFFF


def both(engine, plan, **kw):
    """the same call through the compact record and through the forced 8-byte record"""
    engine.test_rec8(False)
    assert plan.record_bytes() == 4
    a = plan.spatial(want_weights=True, **kw)
    engine.test_rec8(True)
    try:
        assert plan.record_bytes() == 8
        b = plan.spatial(want_weights=True, **kw)
    finally:
        engine.test_rec8(False)
    return a, b


def same_bytes(x, y):
    assert x["entropy"].tobytes() == y["entropy"].tobytes()
    assert x["assign"].tobytes() == y["assign"].tobytes()
    assert x["present"].tobytes() == y["present"].tobytes()
    assert x["weights"].tobytes() == y["weights"].tobytes()
    assert x["code"] == y["code"]


def walk_video(U, T, seed, p_absent=0.1):
    rng = np.random.default_rng(seed)
    mu = np.mod(0.5 + np.cumsum(rng.normal(0, 0.02, (T, U)), axis=0) + rng.random((1, U)), 1.0)
    mv = np.clip(0.5 + np.cumsum(rng.normal(0, 0.01, (T, U)), axis=0) + rng.normal(0, 0.2, (1, U)), 0.0, 1.0)
    gone = rng.random((T, U)) < p_absent
    gone[np.arange(T), rng.integers(0, U, T)] = False
    mu[gone] = np.nan
    mv[gone] = np.nan
    return mu, mv


@pytest.mark.parametrize("U", USERS)
def test_random_walk_with_absent_samples(engine, plan, U):
    for T in FRAMES:
        mu, mv = walk_video(U, T, seed=U + T)
        a, b = both(engine, plan, mu=mu, mv=mv)
        same_bytes(a, b)
        assert np.isfinite(a["entropy"]).all()
        assert np.array_equal(a["present"], np.count_nonzero(~np.isnan(mu), axis=1))
        assert np.array_equal(a["assign"] < 0, np.isnan(mu))
        # direction ids with the same absent samples: the kernel's other sample path
        ids = np.where(np.isnan(mu), -1, np.rint(mv * H) * (W + 1) + np.rint(mu * W)).astype(np.int32)
        c, d = both(engine, plan, ids=ids)
        same_bytes(c, d)
        assert np.array_equal(c["present"], a["present"])


@pytest.mark.parametrize("U", USERS)
def test_every_user_in_one_direction(engine, plan, overflow, U):
    """one row of multiplicity U: at 2 048 users the largest count the walk word holds"""
    ids = np.empty((7, U), dtype=np.int32)
    ids[0], ids[1], ids[2], ids[3] = 0, N_DIRS - 1, overflow[0][0], N_DIRS // 2
    ids[4], ids[5], ids[6] = overflow[0][-1], 12345, 777
    for T in FRAMES:
        a, b = both(engine, plan, ids=ids[:T])
        same_bytes(a, b)
        assert (a["present"] == U).all() and np.isfinite(a["entropy"]).all()
    # a frame of one direction is U times the one-user frame: the same entropy up to the rounding of the epilogue's logarithms
    # (sum v log2 v over 501 tiles in FP64: 1e-12 relative is 4 500 ulp), and exactly U times its histogram
    one = plan.spatial(ids=ids[:, :1], want_weights=True)
    np.testing.assert_allclose(a["entropy"], one["entropy"], rtol=1e-12)
    assert np.array_equal(a["weights"], one["weights"] * U)


@pytest.mark.parametrize("U", USERS)
def test_users_on_overflow_rows_only(engine, plan, overflow, U):
    dirs, _ = overflow
    rng = np.random.default_rng(U)
    for T in FRAMES:
        ids = dirs[rng.integers(0, dirs.size, (T, U))]
        ids[rng.random((T, U)) < 0.1] = -1
        ids[:, 0] = ids[:, 1] = dirs[0]                       # a multiplicity above 1 in every frame
        a, b = both(engine, plan, ids=ids)
        same_bytes(a, b)
        assert np.isfinite(a["entropy"]).all()


def test_more_overflow_rows_than_the_lists_spare_slots(engine, plan, overflow):
    """every overflow direction in one frame: the overflow list holds max(2 * overflow rows, 128) entries, at most the chunk;
    the frame has more distinct (row, mirrored) keys on it than the list has slots beyond its minimum of 128"""
    dirs, keys = overflow
    n_ovf = plan.table_cap(0)[1]
    for U in (1024, 2048, 4096):
        take = dirs[:U]
        distinct = np.unique(keys[:U]).size
        slots = min(min(U, 2048), max(2 * n_ovf, SET_MIN_USERS))
        print(f"{U} users: {take.size} overflow directions, {distinct} distinct keys, {n_ovf} overflow rows, list of {slots} slots")
        assert distinct > slots - SET_MIN_USERS
        ids = np.empty((3, U), dtype=np.int32)
        ids[:, :take.size] = take
        ids[:, take.size:] = dirs[np.random.default_rng(U).integers(0, dirs.size, (3, U - take.size))]
        ids[1] = ids[0, ::-1]                                   # the same users in another order: the same sums
        ids[2, ::5] = -1
        a, b = both(engine, plan, ids=ids)
        same_bytes(a, b)
        assert a["entropy"][0] == a["entropy"][1] and np.isfinite(a["entropy"]).all()


@pytest.mark.parametrize("U", USERS)
def test_an_all_absent_frame_between_two_normal_ones(engine, plan, native, U):
    mu, mv = walk_video(U, 3, seed=3 * U)
    mu[1], mv[1] = np.nan, np.nan
    a, b = both(engine, plan, mu=mu, mv=mv, check=False)
    assert a["code"] == native.VET_ERR_EMPTY                 # status[1]
    same_bytes(a, b)
    assert np.isnan(a["entropy"][1]) and a["present"][1] == 0 and (a["assign"][1] == -1).all()
    assert not a["weights"][1].any()
    assert np.isfinite(a["entropy"][[0, 2]]).all() and (a["present"][[0, 2]] > 0).all()
    # the frames beside it are what they are without it
    c = plan.spatial(mu=mu[[0, 2]], mv=mv[[0, 2]], want_weights=True)
    assert c["entropy"].tobytes() == a["entropy"][[0, 2]].tobytes() and c["weights"].tobytes() == a["weights"][[0, 2]].tobytes()


@pytest.mark.parametrize("U", USERS)
def test_one_out_of_range_sample(engine, plan, native, U):
    ids = np.random.default_rng(U).integers(0, N_DIRS, (3, U)).astype(np.int32)
    ids[1, U - 1] = N_DIRS                                    # the frame's last sample: the last round's only one at 1 025 / 2 049
    a, b = both(engine, plan, ids=ids, check=False)
    assert a["code"] == native.VET_ERR_RANGE                 # status[0]
    same_bytes(a, b)
    assert a["assign"][1, U - 1] == -1 and np.array_equal(a["present"], [U, U - 1, U])
    mu, mv = walk_video(U, 3, seed=U, p_absent=0.0)
    mu[2, U // 2] = 1.5
    c, d = both(engine, plan, mu=mu, mv=mv, check=False)
    assert c["code"] == native.VET_ERR_RANGE
    same_bytes(c, d)


def test_against_the_numpy_oracle(engine, plan):
    """128 users x 3 frames: nearest tiles exact; entropy within 1e-6 relative, the contract of the table formulation that the
    suite holds every table path to (tests/test_rec32.py: check_against_oracle; tests/_tol.py has the tolerances of the weight
    values, which this plan, with the table's own histogram switched on, does not put out)"""
    engine.test_rec8(False)
    mu, mv = walk_video(128, 3, seed=77)
    res = plan.spatial(mu=mu, mv=mv)
    assert plan.record_bytes() == 4 and plan.last_formulation(0) == "table"
    ent, assign = vo.spatial_series(mu, mv, W, H, [500], fov_angle=120.0, power_factor=2.0)[:2]
    assert np.array_equal(res["assign"], assign)
    print("largest relative difference from the oracle:", np.max(np.abs(res["entropy"] - ent) / ent))
    np.testing.assert_allclose(res["entropy"], ent, rtol=1e-6)
