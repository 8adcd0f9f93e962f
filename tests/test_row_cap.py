"""Capped rows of the one-lattice weight table: main rows of `cap` entries walked with a fixed trip count, the tails of the
few longer rows in an overflow table walked in a second pass.  Integer adds commute, so the capped layout must give the bits
of the uncapped one (vet_test_no_row_cap, a switch of the engine: both layouts run in this process)."""
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
def engines(native):
    """(capped, uncapped): the switch belongs to the engine and is read when a plan builds its table"""
    capped, whole = native.Engine(0), native.Engine(0)
    whole.test_no_row_cap(True)
    yield capped, whole
    whole.close()
    capped.close()


def make_plan(native, engine, tcs):
    plan = native.Plan(engine, [vo.fibonacci_lattice(tc) for tc in tcs], 120.0, 2.0, True, W, H)
    plan.set_table_policy(1)
    plan.set_raw_weights(True)            # the table's own histogram: what the two layouts are compared on
    return plan


@pytest.fixture(scope="module")
def plans(native, engines):
    a, b = make_plan(native, engines[0], [500]), make_plan(native, engines[1], [500])
    one = np.arange(N_DIRS, dtype=np.int32).reshape(N_DIRS, 1)
    ra = a.spatial(ids=one, want_weights=True)
    rb = b.spatial(ids=one, want_weights=True)
    yield a, b, ra, rb
    a.close()
    b.close()


def same_bits(x, y):
    assert np.array_equal(x["entropy"], y["entropy"], equal_nan=True)
    assert x["entropy"].tobytes() == y["entropy"].tobytes()
    assert np.array_equal(x["assign"], y["assign"])
    assert x["weights"].tobytes() == y["weights"].tobytes()
    assert np.array_equal(x["present"], y["present"])


def walk_video(U, T, seed, p_absent=0.1):
    rng = np.random.default_rng(seed)
    mu = np.mod(0.5 + np.cumsum(rng.normal(0, 0.02, (T, U)), axis=0) + rng.random((1, U)), 1.0)
    mv = np.clip(0.5 + np.cumsum(rng.normal(0, 0.01, (T, U)), axis=0) + rng.normal(0, 0.2, (1, U)), 0.0, 1.0)
    gone = rng.random((T, U)) < p_absent
    gone[np.arange(T), rng.integers(0, U, T)] = False
    mu[gone] = np.nan
    mv[gone] = np.nan
    return mu, mv


def test_cap_is_two_blocks_with_few_overflow_rows(plans):
    a, b, _, _ = plans
    assert a.last_formulation(0) == b.last_formulation(0) == "table"
    cap, n_ovf = a.table_cap(0)
    rows = a.table_rows()
    print(f"capped: cap {cap}, {n_ovf} overflow rows of {rows}; uncapped stride {b.table_stride(0)}")
    assert cap == 128 and a.table_stride(0) == 128
    assert 1 <= n_ovf <= rows // 32
    assert b.table_cap(0) == (192, 0) and b.table_stride(0) == 192


def test_every_one_user_frame_has_the_same_bits(plans):
    _, _, ra, rb = plans
    same_bits(ra, rb)


def test_frames_of_overflow_directions_have_the_same_bits(plans):
    a, b, _, rb = plans
    cap, n_ovf = a.table_cap(0)
    # a direction's row = the non-zero slots of its one-user frame (every in-FoV tile has a mantissa >= 1)
    per_dir = np.count_nonzero(rb["weights"], axis=1)
    ovf_dirs = np.flatnonzero(per_dir > cap).astype(np.int32)
    print(f"{ovf_dirs.size} of {N_DIRS} directions have more than {cap} entries (most: {per_dir.max()})")
    assert n_ovf <= ovf_dirs.size <= N_DIRS // 32 + 1 and per_dir.max() <= cap + 64
    assert ovf_dirs.size > n_ovf, "mirrored partners share a row: both must be among the overflow directions"
    rng = np.random.default_rng(5)
    for U, T in ((1, ovf_dirs.size), (64, 40), (256, 64), (1024, 16), (3000, 3)):
        ids = ovf_dirs[rng.integers(0, ovf_dirs.size, (T, U))] if U > 1 else ovf_dirs.reshape(T, 1)
        if U > 1:
            ids[rng.random((T, U)) < 0.05] = -1                      # absent users
            ids[:, 0] = ovf_dirs[0]
            ids[:, 1] = ovf_dirs[0]                                    # a multiplicity above 1 in every frame
        x, y = a.spatial(ids=ids, want_weights=True), b.spatial(ids=ids, want_weights=True)
        same_bits(x, y)
        assert np.isfinite(x["entropy"]).all()
    # overflow directions among others: half and half
    ids = rng.integers(0, N_DIRS, (32, 512)).astype(np.int32)
    ids[:, ::2] = ovf_dirs[rng.integers(0, ovf_dirs.size, (32, 256))]
    same_bits(a.spatial(ids=ids, want_weights=True), b.spatial(ids=ids, want_weights=True))


def test_random_walk_frames_have_the_same_bits(plans):
    a, b, _, _ = plans
    mu, mv = walk_video(1024, 256, seed=11)
    same_bits(a.spatial(mu=mu, mv=mv, want_weights=True), b.spatial(mu=mu, mv=mv, want_weights=True))
    (x,), (y,) = a.spatial_batch([(mu[:40], mv[:40])], want_assign=True, check=False), \
        b.spatial_batch([(mu[:40], mv[:40])], want_assign=True, check=False)
    assert x["entropy"].tobytes() == y["entropy"].tobytes() and np.array_equal(x["assign"], y["assign"])


def test_main_and_overflow_entries_are_the_uncapped_row(plans):
    a, b, _, _ = plans
    cap, n_ovf = a.table_cap(0)
    ta, tb = a.read_table(0), b.read_table(0)
    rows = a.table_rows()
    assert ta["ovf_w"].shape == (n_ovf + 1, 64) and not ta["ovf_w"][n_ovf].any()
    assert not ta["w"][rows].any() and not tb["w"][rows].any()
    ovf_of_row = ta["ovf_of_row"]
    has = ovf_of_row != 0xFFFFFFFF
    assert np.array_equal(ovf_of_row[has], np.arange(n_ovf, dtype=np.uint32)), "numbered densely, in row order"
    assert np.array_equal((ta["meta"][:rows] >> 15) & 1, has.astype(np.uint32))
    assert np.array_equal(ta["meta"][:rows] >> 16, tb["meta"][:rows] >> 16), "the row shift is unchanged"

    def entries(w, t):
        keep = w != 0
        return sorted(zip(t[keep].tolist(), w[keep].tolist()))
    len_b = tb["meta"][:rows] & 0xFFF
    assert np.array_equal(has, len_b > cap)
    for r in range(rows):
        whole = entries(tb["w"][r], tb["tile"][r])
        assert len(whole) == len_b[r]
        if has[r]:
            o = ovf_of_row[r]
            main, tail = entries(ta["w"][r], ta["tile"][r]), entries(ta["ovf_w"][o], ta["ovf_tile"][o])
            assert len(main) == cap == (ta["meta"][r] & 0xFFF) and len(tail) == len_b[r] - cap
            assert sorted(main + tail) == whole, r
        elif r % 16 == 0:
            assert entries(ta["w"][r], ta["tile"][r]) == whole, r


def test_short_rows_keep_one_layout(native, engines):
    """rows that fit one block: no multiple of the block below the stride, so cap == stride and no side table"""
    a, b = make_plan(native, engines[0], [50]), make_plan(native, engines[1], [50])
    mu, mv = walk_video(200, 30, seed=3)
    x, y = a.spatial(mu=mu, mv=mv, want_weights=True), b.spatial(mu=mu, mv=mv, want_weights=True)
    assert a.last_formulation(0) == "table"
    assert a.table_cap(0) == b.table_cap(0) == (a.table_stride(0), 0) and a.table_stride(0) == 64
    assert "ovf_w" not in a.read_table(0)
    same_bits(x, y)
    a.close()
    b.close()
