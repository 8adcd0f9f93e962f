"""Bucket-ordered row lists of the compact-record table kernel (k_spatial_lut<LB>).

One video, one frame per workgroup, the users in one chunk: the lists pass places a frame's walk words by row >> k into 256
buckets instead of leaving them in the order in which the users arrived, so that a direction and its mirror (one row) are
walked together and rows are asked for in ascending order.  The frame-group kernels this work also built and measured (FG = 2, 4
frames walked in step per workgroup, barriers per S buckets) lost to it and live in tools/experiments/ as a patch; the product
has no switch that selects among them, so the in-process reference here is the kernel of the forced 8-byte record
(vet_test_rec8), which keeps the arrival order.  Integer histogram adds commute: entropy, assignments, present counts and the
table's own histogram must be the same BYTES.

What this file can and cannot tell.  record_bytes() and last_formulation() assert that the compact record's table kernel served
a call; they are equally true of that kernel in arrival order, and since the two orders give the same bytes by design, NOTHING
here can tell the bucket-ordered kernel from the arrival-ordered one (tests/test_row_cap_blocks.py does, through
Plan.last_table_kernel(): it asserts which of the two each of its launches took).  By the launch rule (launch_lut:
compact record, one frame per workgroup, users in one chunk) every single-video call below of at most 2 048 users — each has
fewer than 4 * CUs frames, hence one frame per workgroup — runs the bucket-ordered kernel, and a wrong placement, count or scan
there breaks the byte comparison; a regression of the rule itself back to the arrival order would pass.  Two-chunk frames
(3 000 users) and batches keep the arrival order by the same rule and must give the same bytes all the same.

Frames 1, 3, 4, 5 and 9; users 128 (the set's threshold), 512 and 1 024; both input forms.  One case is held against the C
port of the reference, so the file does not rest on the sibling kernel alone."""
import numpy as np
import pytest

from oracle import vet_oracle as vo

pytestmark = pytest.mark.gpu

W, H = 100, 200
N_DIRS = (W + 1) * (H + 1)
USERS = (128, 512, 1024)
FRAMES = (1, 3, 4, 5, 9)


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
    p = native.Plan(engine, [vo.fibonacci_lattice(500)], 120.0, 2.0, True, W, H)
    p.set_table_policy(1)
    p.set_raw_weights(True)
    p.spatial(mu=np.full((1, 1), 0.5), mv=np.full((1, 1), 0.5))
    yield p
    p.close()


@pytest.fixture(scope="module")
def records(plan):
    """the compact direction records, read once: (set key = row | mirrored << 15 per direction, overflow directions)"""
    rec = plan.read_records()
    cap, n_ovf = plan.table_cap(0)
    one = np.arange(N_DIRS, dtype=np.int32).reshape(N_DIRS, 1)
    per_dir = np.count_nonzero(plan.spatial(ids=one, want_weights=True)["weights"], axis=1)
    ovf = np.flatnonzero(per_dir > cap).astype(np.int32)
    assert ovf.size > n_ovf >= 1
    return rec & 0xFFFF, ovf


def both(engine, plan, **kw):
    """the same call in bucket order (compact record) and in arrival order (forced 8-byte record)"""
    engine.test_rec8(False)
    assert plan.record_bytes() == 4
    a = plan.spatial(want_weights=True, **kw)
    assert plan.last_formulation(0) == "table"
    engine.test_rec8(True)
    try:
        assert plan.record_bytes() == 8
        b = plan.spatial(want_weights=True, **kw)
        assert plan.last_formulation(0) == "table"
    finally:
        engine.test_rec8(False)
    return a, b


def same_bits(x, y):
    assert np.array_equal(x["entropy"], y["entropy"], equal_nan=True)
    assert x["entropy"].tobytes() == y["entropy"].tobytes()
    assert np.array_equal(x["assign"], y["assign"])
    assert x["weights"].tobytes() == y["weights"].tobytes()
    assert np.array_equal(x["present"], y["present"])
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


def ids_of(mu, mv):
    return np.where(np.isnan(mu), -1, np.rint(mv * H) * (W + 1) + np.rint(mu * W)).astype(np.int32)


@pytest.mark.parametrize("U", USERS)
def test_random_walks_with_absent_samples(engine, plan, U):
    for T in FRAMES:
        mu, mv = walk_video(U, T, seed=100 * U + T)
        a, b = both(engine, plan, mu=mu, mv=mv)
        same_bits(a, b)
        assert np.isfinite(a["entropy"]).all()
        assert np.array_equal(a["present"], np.count_nonzero(~np.isnan(mu), axis=1))
        c, d = both(engine, plan, ids=ids_of(mu, mv))
        same_bits(c, d)
        assert np.array_equal(c["present"], a["present"])


@pytest.mark.parametrize("U", USERS)
def test_identical_and_disjoint_frames(engine, plan, U):
    """four frames with every row in common, then four whose directions are pairwise disjoint"""
    rng = np.random.default_rng(U)
    one = rng.integers(0, N_DIRS, (1, U)).astype(np.int32)
    a, b = both(engine, plan, ids=np.repeat(one, 4, axis=0))
    same_bits(a, b)
    assert (a["entropy"] == a["entropy"][0]).all() and (a["weights"] == a["weights"][0]).all()
    apart = rng.permutation(N_DIRS)[:4 * U].astype(np.int32).reshape(4, U)
    assert np.unique(apart).size == 4 * U
    c, d = both(engine, plan, ids=apart)
    same_bits(c, d)
    # a frame is what it is alone, whatever its neighbours hold
    alone = plan.spatial(ids=apart[2:3], want_weights=True)
    assert alone["entropy"].tobytes() == c["entropy"][2:3].tobytes() and alone["weights"].tobytes() == c["weights"][2:3].tobytes()


@pytest.mark.parametrize("U", USERS)
def test_directions_and_their_mirror_images(engine, plan, records, U):
    """frames made only of pairs (direction, mirrored direction): two list entries per row, which must meet in one bucket"""
    keys, _ = records
    row, mirrored = keys & 0x7FFF, keys >> 15
    plain = {int(r): d for d, r in enumerate(row) if not mirrored[d]}
    pairs = np.asarray([(plain[int(row[d])], d) for d in np.flatnonzero(mirrored) if int(row[d]) in plain], dtype=np.int32)
    assert len(pairs) > 1000, "the grid's mirror symmetry pairs most directions"
    rng = np.random.default_rng(7 * U)
    for T in (1, 4, 5):
        pick = pairs[rng.integers(0, len(pairs), (T, U // 2))]            # [T, U / 2, 2]
        ids = pick.reshape(T, U)
        a, b = both(engine, plan, ids=ids)
        same_bits(a, b)
        assert np.isfinite(a["entropy"]).all() and (a["present"] == U).all()


@pytest.mark.parametrize("U", USERS)
def test_overflow_directions(engine, plan, records, U):
    _, ovf = records
    rng = np.random.default_rng(11 * U)
    for T in FRAMES:
        ids = ovf[rng.integers(0, ovf.size, (T, U))]
        ids[rng.random((T, U)) < 0.1] = -1
        ids[:, 0] = ids[:, 1] = ovf[0]
        a, b = both(engine, plan, ids=ids)
        same_bits(a, b)
        assert np.isfinite(a["entropy"]).all()


@pytest.mark.parametrize("U", USERS)
def test_a_frame_with_no_user_present(engine, plan, native, U):
    for T in (1, 4, 5):
        mu, mv = walk_video(U, T, seed=3 * U + T)
        mu[T // 2], mv[T // 2] = np.nan, np.nan
        a, b = both(engine, plan, mu=mu, mv=mv, check=False)
        assert a["code"] == native.VET_ERR_EMPTY                 # status[1]
        same_bits(a, b)
        assert np.isnan(a["entropy"][T // 2]) and a["present"][T // 2] == 0 and not a["weights"][T // 2].any()
        rest = np.arange(T) != T // 2
        assert np.isfinite(a["entropy"][rest]).all()


@pytest.mark.parametrize("U", USERS)
def test_one_sample_outside_the_unit_square(engine, plan, native, U):
    mu, mv = walk_video(U, 5, seed=5 * U, p_absent=0.0)
    mu[3, U // 3] = 1.5
    a, b = both(engine, plan, mu=mu, mv=mv, check=False)
    assert a["code"] == native.VET_ERR_RANGE                     # status[0]
    same_bits(a, b)
    assert a["assign"][3, U // 3] == -1 and np.array_equal(a["present"], [U, U, U, U - 1, U])
    ids = ids_of(*walk_video(U, 4, seed=U, p_absent=0.0))
    ids[0, U - 1] = N_DIRS
    c, d = both(engine, plan, ids=ids, check=False)
    assert c["code"] == native.VET_ERR_RANGE
    same_bits(c, d)


def test_two_chunks_and_a_batch_keep_their_kernels(engine, plan):
    """3 000 users arrive in two chunks and a batch shares one grid: both keep the arrival order and give the same bytes"""
    mu, mv = walk_video(3000, 5, seed=31)
    a, b = both(engine, plan, mu=mu, mv=mv)
    same_bits(a, b)
    mu, mv = walk_video(1024, 9, seed=32)
    whole, _ = both(engine, plan, mu=mu, mv=mv)
    (x,) = plan.spatial_batch([(mu, mv)], want_assign=True, check=False)
    assert plan.last_formulation(0) == "table"
    assert x["entropy"].tobytes() == whole["entropy"].tobytes() and np.array_equal(x["assign"], whole["assign"])
    assert np.array_equal(x["present"], whole["present"])


def test_against_the_c_port_of_the_reference(engine, plan):
    """64 frames of the benchmark's default video: nearest tiles exact, entropy within 1e-6 (relative: the contract of the table
    formulation, tests/test_rec32.py)"""
    import bench
    from oracle import c_port
    mu, mv = bench.synth_video(1024, 64, 1234, 0)
    engine.test_rec8(False)
    res = plan.spatial(mu=mu, mv=mv)
    assert plan.record_bytes() == 4 and plan.last_formulation(0) == "table"
    ent, assign = c_port.spatial_series(mu, mv, W, H, [500], fov_angle=120.0, power_factor=2.0)[:2]
    assert np.array_equal(res["assign"], assign)
    print("largest relative difference from the C port:", np.max(np.abs(res["entropy"] - ent) / ent))
    np.testing.assert_allclose(res["entropy"], ent, rtol=1e-6)
