"""The phase walk of the bucket-ordered table kernel (k_spatial_lut<LB>): same bytes wherever a frame's walk begins.

A workgroup of that kernel begins its bucket-ordered row list at the bucket a device-wide sweep is in when the workgroup gets
there — read off the wall clock, one pass over the 256 buckets per 82 us — and wraps around, so that the frames resident on an
XCD move through the table together.  Integer histogram adds commute, so entropy, nearest tiles, present counts and the table's
own histogram (vet_plan_set_raw_weights) must be the BYTES of the kernel of the forced 8-byte record (vet_test_rec8), which
keeps the arrival order and never looks at the clock.

Every case runs three times on one context and once on a fresh one.  The start bucket is a function of the time alone: it
differs from run to run and, within a launch, from workgroup to workgroup (a launch of more workgroups than the device holds at
once, or one that lasts longer than a bucket's 0.32 us, sees several).  All runs must give the same bytes.

What this file cannot tell.  THE TEST CANNOT SEE WHICH START BUCKET A LAUNCH TOOK: the library has no read-back of it (its
exported symbols and environment variables are pinned, tests/test_cabi_symbols.py), and since the output does not depend on
the start by design, a kernel that always began at bucket 0 would pass.  What breaks the byte comparison is a wrong rotation —
an entry placed twice, dropped, or placed beyond the list —, which tests/test_lut_phase_rotation.py also checks on the CPU.

Shapes (frames x users).  4 096 x 128, 512 x 1 024 and 64 x 2 048 are the ones the work was specified with.  By the launch rule
(launch_lut: bucket order only with one frame per workgroup) 4 096 x 128 runs TWO frames per workgroup on a 256-CU device and
so keeps the arrival-order kernel; it stays as a case that must not change, and 2 560 x 576 is added: one frame per workgroup
at any frame count (more than 512 users), more workgroups than the 2 048 resident slots, a user count that is no power of two.
"""
import numpy as np
import pytest

from oracle import vet_oracle as vo

pytestmark = pytest.mark.gpu

W, H = 100, 200
N_DIRS = (W + 1) * (H + 1)
SHAPES = ((4096, 128), (512, 1024), (64, 2048), (2560, 576))
KINDS = ("random_walk", "one_direction", "pole", "one_bucket", "side_table", "absent")
LB = 8          # buckets (log2) of the bucket-ordered kernel


@pytest.fixture(scope="module")
def native():
    from viewport_entropy_toolkit import _native
    return _native


def make_plan(native, engine):
    p = native.Plan(engine, [vo.fibonacci_lattice(500)], 120.0, 2.0, True, W, H)
    p.set_table_policy(1)
    p.set_raw_weights(True)
    p.spatial(mu=np.full((1, 1), 0.5), mv=np.full((1, 1), 0.5))
    return p


@pytest.fixture(scope="module")
def engine(native):
    e = native.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def plan(native, engine):
    p = make_plan(native, engine)
    yield p
    p.close()


@pytest.fixture(scope="module")
def records(plan):
    """the compact direction records, read once: (row per direction, directions whose row continues in the side table)"""
    rec = plan.read_records()
    ovf = np.flatnonzero(rec >> 31).astype(np.int32)
    assert ovf.size >= 1 and plan.table_cap(0)[1] >= 1
    return (rec & 0x7FFF).astype(np.int64), ovf


def walk_video(U, T, seed):
    rng = np.random.default_rng(seed)
    mu = np.mod(0.5 + np.cumsum(rng.normal(0, 0.02, (T, U)), axis=0) + rng.random((1, U)), 1.0)
    mv = np.clip(0.5 + np.cumsum(rng.normal(0, 0.01, (T, U)), axis=0) + rng.normal(0, 0.2, (1, U)), 0.0, 1.0)
    return mu, mv


def samples(kind, T, U, records):
    """keyword arguments of Plan.spatial for one input kind"""
    row, ovf = records
    rng = np.random.default_rng(1000 * T + U + len(kind))
    if kind == "random_walk":
        mu, mv = walk_video(U, T, seed=T + U)
        return dict(mu=mu, mv=mv)
    if kind == "one_direction":         # the row list has one entry
        return dict(ids=np.full((T, U), 77 * (W + 1) + 31, dtype=np.int32))
    if kind == "pole":                  # every direction of the top pixel row is the pole: one row, whatever the longitude
        return dict(mu=rng.random((T, U)), mv=np.zeros((T, U)))
    if kind == "one_bucket":            # directions whose rows fall into one bucket (row >> kshift) of the 2^LB
        kshift = max(int(row.max() + 1).bit_length() - LB, 0)
        bucket = row >> kshift
        inside = np.flatnonzero(bucket == np.bincount(bucket).argmax()).astype(np.int32)
        assert np.unique(row[inside]).size > 1
        return dict(ids=inside[rng.integers(0, inside.size, (T, U))])
    if kind == "side_table":
        return dict(ids=ovf[rng.integers(0, ovf.size, (T, U))])
    if kind == "absent":                # absent (NaN) users in every frame and one frame with nobody
        mu, mv = walk_video(U, T, seed=3 * T + U)
        gone = rng.random((T, U)) < 0.1
        gone[T // 2] = True
        mu[gone] = np.nan
        mv[gone] = np.nan
        return dict(mu=mu, mv=mv)
    raise AssertionError(kind)


def same_bits(x, y):
    assert x["entropy"].tobytes() == y["entropy"].tobytes()
    assert np.array_equal(x["assign"], y["assign"])
    assert x["weights"].tobytes() == y["weights"].tobytes()
    assert np.array_equal(x["present"], y["present"])
    assert x["code"] == y["code"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T,U", SHAPES)
def test_same_bytes_wherever_the_walk_begins(native, engine, plan, records, T, U, kind):
    kw = samples(kind, T, U, records)
    engine.test_rec8(True)
    try:
        assert plan.record_bytes() == 8
        ref = plan.spatial(want_weights=True, check=False, **kw)
        assert plan.last_formulation(0) == "table"
    finally:
        engine.test_rec8(False)
    assert plan.record_bytes() == 4
    for _ in range(3):
        got = plan.spatial(want_weights=True, check=False, **kw)
        assert plan.last_formulation(0) == "table"
        same_bits(got, ref)
    fresh_engine = native.Engine(0)
    try:
        fresh_plan = make_plan(native, fresh_engine)
        try:
            assert fresh_plan.record_bytes() == 4
            got = fresh_plan.spatial(want_weights=True, check=False, **kw)
            assert fresh_plan.last_formulation(0) == "table"
            same_bits(got, ref)
        finally:
            fresh_plan.close()
    finally:
        fresh_engine.close()
    if kind == "absent":
        assert ref["code"] == native.VET_ERR_EMPTY
        assert np.isnan(ref["entropy"][T // 2]) and ref["present"][T // 2] == 0 and not ref["weights"][T // 2].any()
        assert np.isfinite(np.delete(ref["entropy"], T // 2)).all()
    else:
        assert ref["code"] == 0 and np.isfinite(ref["entropy"]).all() and (ref["present"] == U).all()


def test_against_the_c_port_of_the_reference(plan):
    """the first frames of the benchmark's default video: nearest tiles exact, entropy within 1e-6 (relative: the contract of
    the table formulation, tests/test_rec32.py)"""
    import bench
    from oracle import c_port
    mu, mv = bench.synth_video(1024, 16, 1234, 0)
    res = plan.spatial(mu=mu, mv=mv)
    assert plan.record_bytes() == 4 and plan.last_formulation(0) == "table"
    ent, assign = c_port.spatial_series(mu, mv, W, H, [500], fov_angle=120.0, power_factor=2.0)[:2]
    assert np.array_equal(res["assign"], assign)
    print("largest relative difference from the C port:", np.max(np.abs(res["entropy"] - ent) / ent))
    np.testing.assert_allclose(res["entropy"], ent, rtol=1e-6)
