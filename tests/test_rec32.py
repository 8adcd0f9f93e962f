"""The compact direction record of the capped table kernels: one 4-byte gather per sample (row | mirrored | nearest tile |
-shift | overflow bit) instead of the 8-byte record, no meta list in LDS.  Rows, shifts and tiles are the same and integer
adds commute, so entropy, assignments and the table's own histogram must equal the 8-byte-record path bit for bit
(vet_test_rec8, a switch of the engine read at every launch: one plan runs both kernels in this process)."""
import numpy as np
import pytest

from oracle import vet_oracle as vo

pytestmark = pytest.mark.gpu

W, H = 100, 200
N_DIRS = (W + 1) * (H + 1)


@pytest.fixture(scope="module")
def native():
    from viewport_entropy_toolkit import _native
    return _native


@pytest.fixture(scope="module")
def engine(native):
    e = native.Engine(0)
    yield e
    e.close()


def make_plan(native, engine, tcs, fov=120.0, power=2.0, w=W, h=H):
    plan = native.Plan(engine, [vo.fibonacci_lattice(tc) for tc in tcs], fov, power, True, w, h)
    plan.set_table_policy(1)
    plan.set_raw_weights(True)            # the table's own histogram: compared bit for bit beside the entropy
    return plan


@pytest.fixture(scope="module")
def plan(native, engine):
    """the config-3 plan shape, its table built"""
    p = make_plan(native, engine, [500])
    p.spatial(mu=np.full((1, 1), 0.5), mv=np.full((1, 1), 0.5))
    yield p
    p.close()


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


def same_bits(x, y):
    assert np.array_equal(x["entropy"], y["entropy"], equal_nan=True)
    assert x["entropy"].tobytes() == y["entropy"].tobytes()
    assert np.array_equal(x["assign"], y["assign"])
    assert x["weights"].tobytes() == y["weights"].tobytes()
    assert np.array_equal(x["present"], y["present"])


def walk_video(U, T, seed, p_absent=0.0):
    rng = np.random.default_rng(seed)
    mu = np.mod(0.5 + np.cumsum(rng.normal(0, 0.02, (T, U)), axis=0) + rng.random((1, U)), 1.0)
    mv = np.clip(0.5 + np.cumsum(rng.normal(0, 0.01, (T, U)), axis=0) + rng.normal(0, 0.2, (1, U)), 0.0, 1.0)
    if p_absent:
        gone = rng.random((T, U)) < p_absent
        gone[np.arange(T), rng.integers(0, U, T)] = False
        mu[gone] = np.nan
        mv[gone] = np.nan
    return mu, mv


def uniform_video(U, T, seed):
    rng = np.random.default_rng(seed)
    return rng.random((T, U)), np.clip(np.arccos(1.0 - 2.0 * rng.random((T, U))) / np.pi, 0.0, 1.0)


def clustered_video(U, T, seed):
    rng = np.random.default_rng(seed)
    cu = np.mod(0.5 + np.cumsum(rng.normal(0.0, 0.004, (T, 1)), axis=0), 1.0)
    cv = np.clip(0.5 + np.cumsum(rng.normal(0.0, 0.002, (T, 1)), axis=0), 0.2, 0.8)
    return np.mod(cu + rng.normal(0.0, 0.02, (T, U)), 1.0), np.clip(cv + rng.normal(0.0, 0.02, (T, U)), 0.0, 1.0)


def test_the_record_is_the_eight_byte_one_repacked(plan):
    """row, mirror flag and nearest tile of the alias / nearest tables, -shift and overflow bit of the row's meta word"""
    cap, n_ovf = plan.table_cap(0)
    assert cap == 128 and n_ovf >= 1 and plan.record_bytes() == 4
    rec = plan.read_records()
    t = plan.read_table(0)
    rows = plan.table_rows()
    assert rows + 1 <= 1 << 15
    row, mirrored = rec & 0x7FFF, (rec >> 15) & 1
    assert row.max() == rows - 1 and set(np.unique(row)) == set(range(rows))
    assert np.array_equal((rec >> 16) & 0x3FF, plan.read_nearest(0).astype(np.uint32))
    meta = t["meta"][row]
    assert np.array_equal(16 - ((rec >> 26) & 31), meta >> 16), "the field holds -shift; the meta word 16 + shift"
    assert ((meta >> 16) <= 16).all()
    assert np.array_equal(rec >> 31, (meta >> 15) & 1)
    assert np.array_equal((rec >> 31).astype(bool), t["ovf_of_row"][row] != 0xFFFFFFFF)
    assert 0 < mirrored.sum() < N_DIRS, "mirror images share rows on this plan"


@pytest.mark.parametrize("kind", ["random_walk", "uniform", "clustered"])
def test_videos_have_the_same_bits(engine, plan, kind):
    U, T = 1024, 96
    mu, mv = {"random_walk": walk_video, "uniform": uniform_video, "clustered": clustered_video}[kind](U, T, seed=21)
    a, b = both(engine, plan, mu=mu, mv=mv)
    same_bits(a, b)
    assert np.isfinite(a["entropy"]).all() and (a["present"] == U).all()


def test_frames_with_absent_users_have_the_same_bits(engine, plan, native):
    mu, mv = walk_video(1024, 64, seed=4, p_absent=0.3)
    mu[5], mv[5] = np.nan, np.nan                          # a frame without users: NaN entropy on both paths
    a, b = both(engine, plan, mu=mu, mv=mv, check=False)
    assert a["code"] == b["code"] == native.VET_ERR_EMPTY
    same_bits(a, b)
    assert np.isnan(a["entropy"][5]) and a["present"][5] == 0 and (a["assign"][5] == -1).all()
    assert np.isfinite(np.delete(a["entropy"], 5)).all()


def test_one_direction_for_all_users(engine, plan):
    """the largest multiplicities a chunk can hold: 1024, 2048 (one full chunk) and 3000 users (two chunks) in one direction"""
    rec = plan.read_records()
    ovf_dir = int(np.flatnonzero(rec >> 31)[0])
    for U in (1024, 2048, 3000):
        ids = np.empty((6, U), dtype=np.int32)
        ids[0], ids[1], ids[2] = 0, N_DIRS - 1, ovf_dir
        ids[3] = N_DIRS // 2
        ids[4] = ovf_dir
        ids[4, 1::7] = -1
        ids[5] = 12345
        a, b = both(engine, plan, ids=ids)
        same_bits(a, b)
        assert np.isfinite(a["entropy"]).all() and np.array_equal(a["present"], [U, U, U, U, U - len(range(1, U, 7)), U])


def test_frames_below_the_set_threshold(engine, plan):
    """videos of fewer than 128 users run without the set (and read the 8-byte record on their own); in a batch beside a
    large video they run the compact-record kernel with one list entry per user"""
    rec = plan.read_records()
    ovf_dirs = np.flatnonzero(rec >> 31)
    for U in (1, 17, 127):
        mu, mv = walk_video(U, 40, seed=U, p_absent=0.2 if U > 1 else 0.0)
        a, b = both(engine, plan, mu=mu, mv=mv)
        same_bits(a, b)
    big, small, tiny = walk_video(512, 12, seed=8), walk_video(60, 30, seed=9, p_absent=0.1), walk_video(3, 50, seed=10)
    # a small video of overflow directions: pixel centres of those directions
    d = ovf_dirs[np.random.default_rng(2).integers(0, ovf_dirs.size, (20, 40))]
    over = (np.minimum((d % (W + 1) + 0.25) / W, 1.0), np.minimum((d // (W + 1) + 0.25) / H, 1.0))
    vids = [big, small, tiny, over]
    engine.test_rec8(False)
    xs = plan.spatial_batch(vids, want_assign=True, check=False)
    engine.test_rec8(True)
    try:
        ys = plan.spatial_batch(vids, want_assign=True, check=False)
    finally:
        engine.test_rec8(False)
    for x, y, (mu, mv) in zip(xs, ys, vids):
        assert x["entropy"].tobytes() == y["entropy"].tobytes()
        assert np.array_equal(x["assign"], y["assign"]) and np.array_equal(x["present"], y["present"])
        z = plan.spatial(mu=mu, mv=mv)                     # and the batch gives the single call's bits
        assert x["entropy"].tobytes() == z["entropy"].tobytes() and np.array_equal(x["assign"].reshape(z["assign"].shape), z["assign"])


def test_frames_of_overflow_rows_have_the_same_bits(engine, plan):
    """directions whose meta word has the overflow bit (vet_plan_read_table), alone and among others"""
    t = plan.read_table(0)
    rows = plan.table_rows()
    rec = plan.read_records()
    ovf_rows = np.flatnonzero((t["meta"][:rows] >> 15) & 1)
    ovf_dirs = np.flatnonzero(np.isin(rec & 0x7FFF, ovf_rows)).astype(np.int32)
    assert ovf_rows.size == plan.table_cap(0)[1] and ovf_dirs.size > ovf_rows.size
    rng = np.random.default_rng(5)
    for U, T in ((128, 40), (1024, 16), (3000, 3)):
        ids = ovf_dirs[rng.integers(0, ovf_dirs.size, (T, U))]
        ids[rng.random((T, U)) < 0.05] = -1
        ids[:, 0] = ids[:, 1] = ovf_dirs[0]
        a, b = both(engine, plan, ids=ids)
        same_bits(a, b)
        assert np.isfinite(a["entropy"]).all()
    ids = rng.integers(0, N_DIRS, (32, 512)).astype(np.int32)
    ids[:, ::2] = ovf_dirs[rng.integers(0, ovf_dirs.size, (32, 256))]
    a, b = both(engine, plan, ids=ids)
    same_bits(a, b)


def test_every_direction_as_a_one_user_frame(engine, plan):
    """all 20 301 directions, each the only present user of a 128-user frame (the kernels with the set) and as a frame of one
    user: nearest tile, entropy and histogram equal the 8-byte path"""
    ids = np.full((N_DIRS, 128), -1, dtype=np.int32)
    ids[np.arange(N_DIRS), np.arange(N_DIRS) % 128] = np.arange(N_DIRS)
    a, b = both(engine, plan, ids=ids)
    same_bits(a, b)
    assert (a["present"] == 1).all()
    one = np.arange(N_DIRS, dtype=np.int32).reshape(N_DIRS, 1)
    c, d = both(engine, plan, ids=one)
    same_bits(c, d)
    assert c["entropy"].tobytes() == a["entropy"].tobytes() and c["weights"].tobytes() == a["weights"].tobytes()
    assert np.array_equal(c["assign"][:, 0], a["assign"][np.arange(N_DIRS), np.arange(N_DIRS) % 128])
    assert np.array_equal(c["assign"][:, 0], plan.read_nearest(0))


def test_out_of_range_ids_are_reported_alike(engine, plan, native):
    ids = np.random.default_rng(3).integers(0, N_DIRS, (8, 256)).astype(np.int32)
    ids[2, 5] = N_DIRS
    ids[3, 9] = -7                                          # negative: absent
    a, b = both(engine, plan, ids=ids, check=False)
    assert a["code"] == b["code"] == native.VET_ERR_RANGE
    same_bits(a, b)


def check_against_oracle(plan, tcs, w, h, fov=120.0, power=2.0):
    mu, mv = walk_video(160, 6, seed=77, p_absent=0.1)
    res = plan.spatial(mu=mu, mv=mv)
    ent, assign = vo.spatial_series(mu, mv, w, h, tcs, fov_angle=fov, power_factor=power)[:2]
    assert np.array_equal(res["assign"], assign)
    np.testing.assert_allclose(res["entropy"], ent, rtol=1e-6)         # the formulations' contract


def test_plans_that_do_not_qualify_keep_the_eight_byte_record(native, engine):
    engine.test_rec8(False)
    # several lattices: the fused table, its own 8-byte records
    p = make_plan(native, engine, [50, 100, 200])
    check_against_oracle(p, [50, 100, 200], W, H)
    assert p.last_formulation(0) == "table" and p.record_bytes() == 8
    with pytest.raises(native.NativeError) as err:
        p.read_records()
    assert err.value.code == native.VET_ERR_INVALID
    p.close()
    # an FP table (never capped)
    p = make_plan(native, engine, [500], fov=10.0)
    p.spatial(mu=np.full((2, 200), 0.4), mv=np.full((2, 200), 0.6))
    assert p.last_formulation(0) == "ftable" and p.record_bytes() == 8
    p.close()
    # 200 x 400 pixels: capped, but more than 2^15 rows
    p = make_plan(native, engine, [500], w=200, h=400)
    check_against_oracle(p, [500], 200, 400)
    cap, n_ovf = p.table_cap(0)
    print(f"200x400: {p.table_rows()} rows, cap {cap}, {n_ovf} overflow rows, record {p.record_bytes()} B")
    assert p.table_rows() + 1 > 1 << 15 and n_ovf > 0 and p.record_bytes() == 8
    p.close()
    # short rows: no cap, nothing to drop from the record
    p = make_plan(native, engine, [50])
    check_against_oracle(p, [50], W, H)
    assert p.table_cap(0) == (64, 0) and p.record_bytes() == 8
    p.close()
    # the uncapped layout of the config-3 plan (vet_test_no_row_cap) keeps the old path
    whole = native.Engine(0)
    whole.test_no_row_cap(True)
    p = make_plan(native, whole, [500])
    check_against_oracle(p, [500], W, H)
    assert p.table_cap(0) == (192, 0) and p.record_bytes() == 8
    p.close()
    whole.close()


def test_the_tile_field_decides_at_1024_tiles(native, engine):
    """A nearest tile has 10 bits: lattices of 1 001 and 1 023 tiles fit, 1 025 and 1 101 do not (a Fibonacci lattice has
    2 * (n // 2) + 1 tiles: none has 1 024, and a tile count of 1 024 gives 1 025).  At fov 120 such lattices have rows
    beyond three blocks and are not capped at all.  A row holds the tiles inside a cone of half the field of view, about
    tiles * (1 - cos(fov / 2)) / 2 of them, so each lattice is tried at the field of view that puts its rows just under two
    blocks with a few past them (counted per direction with the oracle's geometry: 0.2-0.3 % of the rows are longer than 128
    entries, none longer than 130, none shorter than 116): there its rows cap at two blocks."""
    engine.test_rec8(False)
    for n, fov in ((1001, 82.5), (1023, 81.5), (1024, 81.5), (1100, 78.5)):
        tiles = len(vo.fibonacci_lattice(n))
        p = make_plan(native, engine, [n], fov=fov)
        p.spatial(mu=np.full((2, 200), 0.4), mv=np.full((2, 200), 0.6))
        cap, n_ovf = p.table_cap(0)
        print(f"{n} -> {tiles} tiles, fov {fov}: {p.last_formulation(0)}, cap {cap}, {n_ovf} overflow rows, "
              f"{p.table_rows()} rows, record {p.record_bytes()} B")
        assert p.last_formulation(0) == "table" and cap == 128 and n_ovf > 0, (n, fov)
        assert p.table_rows() + 1 <= 1 << 15
        assert p.record_bytes() == (4 if tiles <= 1024 else 8), (n, tiles, fov)
        mu, mv = walk_video(300, 20, seed=n, p_absent=0.1)
        x = p.spatial(mu=mu, mv=mv, want_weights=True)
        if tiles <= 1024:
            assert np.array_equal((p.read_records() >> 16) & 0x3FF, p.read_nearest(0).astype(np.uint32))
            engine.test_rec8(True)
            try:
                assert p.record_bytes() == 8
                y = p.spatial(mu=mu, mv=mv, want_weights=True)
            finally:
                engine.test_rec8(False)
            same_bits(x, y)
        else:
            with pytest.raises(native.NativeError) as err:
                p.read_records()
            assert err.value.code == native.VET_ERR_INVALID
        assert np.array_equal(x["assign"], vo.spatial_series(mu, mv, W, H, [n], fov_angle=fov, power_factor=2.0)[1])
        p.close()
