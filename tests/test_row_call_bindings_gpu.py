"""GPU: the layers above the seven row calls' C entries — windowed / per-viewer spatial entropy, viewer / crowd / window
divergence, windowed / per-viewer transition entropy.  The Plan host wrappers against the ``_host`` symbols called directly, with
arrays this file allocates from its own shape table (CALLS below, written out here and not imported from the binding); the Plan
device wrappers against the host results; the analyzers' row-call runner on the three paths it has (cached plan, temporary
``dir_table`` plan, the naive analyzer's lat/lon plan) and its error translation.  The row kernels are bit-reproducible
(tools/ab_bits.py relies on it), so arrays are compared as bytes; only the hand-assigned-vectors path, which runs other kernels on
another plan, is compared to the grid path by tests/test_user_entropy_gpu.py's RTOL.

The naive analyzer bins its own ingest only: it has no hand-assigned-vectors path, so that case runs on the other two."""
import numpy as np
import pytest

from tests.test_user_entropy_gpu import RTOL

pytestmark = pytest.mark.gpu

W, H = 100, 200
U, T = 3, 12
TILE_COUNT = 50                                  # the lattice of tile count 50 has 51 tiles: n0 is read from the plan
F64, I32 = np.float64, np.int32
FRAME_ROWS = ((5, 2, 4), (12, 1, 1))             # (window, stride, R) over the 12 frames
PAIR_ROWS = ((5, 2, 4), (11, 1, 1))              # over the 11 frame pairs

# Plan method, C symbol stem, rows over frame pairs, window=None allowed, the keyword of the optional output, takes max_lag,
# outputs in the entry's order: (result key, shape from (U, R, n0, L), dtype, optional)
CALLS = {
    "spatial_windowed": ("vet_spatial_entropy_windowed", False, False, "want_weights", False, (
        ("entropy", lambda u, r, n, l: (r,), F64, False), ("weights", lambda u, r, n, l: (r, n), F64, True),
        ("samples", lambda u, r, n, l: (r,), I32, False))),
    "spatial_per_user": ("vet_user_entropy", False, True, "want_weights", False, (
        ("entropy", lambda u, r, n, l: (u, r), F64, False), ("weights", lambda u, r, n, l: (u, r, n), F64, True),
        ("samples", lambda u, r, n, l: (u, r), I32, False))),
    "spatial_user_divergence": ("vet_user_divergence", False, True, None, False, (
        ("divergence", lambda u, r, n, l: (r, u, u), F64, False), ("samples", lambda u, r, n, l: (u, r), I32, False))),
    "spatial_crowd_divergence": ("vet_crowd_divergence", False, True, None, False, (
        ("divergence", lambda u, r, n, l: (u, r), F64, False), ("rows", lambda u, r, n, l: (3, r), F64, False),
        ("samples", lambda u, r, n, l: (u, r), I32, False))),
    "spatial_window_divergence": ("vet_window_divergence", False, False, None, True, (
        ("divergence", lambda u, r, n, l: (r, l), F64, False), ("samples", lambda u, r, n, l: (r,), I32, False))),
    "transition_windowed": ("vet_transition_entropy_windowed", True, False, "want_srccount", False, (
        ("entropy", lambda u, r, n, l: (r,), F64, False), ("srccount", lambda u, r, n, l: (r, n), I32, True),
        ("samples", lambda u, r, n, l: (r,), I32, False))),
    "transition_per_user": ("vet_user_transition_entropy", True, True, "want_srccount", False, (
        ("entropy", lambda u, r, n, l: (u, r), F64, False), ("srccount", lambda u, r, n, l: (u, r, n), I32, True),
        ("samples", lambda u, r, n, l: (u, r), I32, False))),
}
WITH_D_IDS = ("spatial_crowd_divergence", "spatial_window_divergence")


@pytest.fixture(scope="module")
def native():
    from viewport_entropy_toolkit import _native
    return _native


@pytest.fixture(scope="module")
def engine(native):
    return native.Engine.default()


@pytest.fixture(scope="module")
def plan(native, engine):
    from viewport_entropy_toolkit import _quantiser
    p = native.Plan(engine, [_quantiser.lattice_xyz(TILE_COUNT)], 120.0, 2.0, True, W, H)
    yield p
    p.close()


def video_arrays():
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(U, T, base_seed=7, p_absent=0.1)
    mu[4:9, 1] = np.nan
    mv[4:9, 1] = np.nan
    return mu, mv


@pytest.fixture(scope="module")
def video():
    """(mu, mv, ids): the 12 x 3 video with user 1 absent over frames 4..8, and its direction ids as tools/ab_bits.py takes them."""
    mu, mv = video_arrays()
    absent = np.isnan(mu) | np.isnan(mv)
    px, py = (np.nan_to_num(mu) * W).astype(np.int64), (np.nan_to_num(mv) * H).astype(np.int64)
    ids = np.where(absent, -1, py * (W + 1) + px).astype(np.int32)
    for a in (mu, mv, ids):
        a.setflags(write=False)
    return mu, mv, ids


def same_array(got, want, msg):
    assert got.dtype == want.dtype and got.shape == want.shape and got.flags.c_contiguous, msg
    assert got.tobytes() == want.tobytes(), msg


def row_cases(pairs, whole, has_lag):
    """(window, stride, R, the max_lag arguments) of one call: the two written-out shapes, window=None where allowed."""
    n = T - 1 if pairs else T
    cases = list(PAIR_ROWS if pairs else FRAME_ROWS) + ([(None, 1, 1)] if whole else [])
    return [(w, s, r, sorted({1, r - 1}) if has_lag else [None]) for w, s, r in cases], n


# ------------------------------------------------------------------------------------------------------- the host wrappers
@pytest.mark.parametrize("method", list(CALLS))
def test_host_wrapper_is_the_direct_call(native, plan, video, method):
    stem, pairs, whole, want_kw, has_lag, outputs = CALLS[method]
    lib = native.load_library()
    entry = getattr(lib, stem + "_host")
    mu, mv, ids = video
    cases, n = row_cases(pairs, whole, has_lag)
    wrapper = getattr(plan, method)
    if not whole:
        with pytest.raises(ValueError, match=r"^window \(a number of frame%s\) is required$" % (" pairs" if pairs else "s")):
            wrapper(mu=mu, mv=mv)
    for samples, raw in ((dict(mu=mu, mv=mv), (mu, mv, None)), (dict(ids=ids), (None, None, ids))):
        for window, stride, R, lags in cases:
            for lag in lags:
                for want in ((False, True) if want_kw else (False,)):
                    msg = f"{method} {'ids' if raw[2] is not None else 'mu_mv'} window={window} stride={stride} lag={lag} want={want}"
                    kw = dict(window=window, stride=stride)
                    if want_kw:
                        kw[want_kw] = want
                    if has_lag:
                        kw["max_lag"] = lag
                        if lag < 1 or R == 1:                  # one row has no lag to offer
                            with pytest.raises(ValueError, match=r"^need 1 <= max_lag <= rows - 1 = 0 \(got max_lag=%d; " % lag):
                                wrapper(**samples, **kw)
                            continue
                    res = wrapper(**samples, **kw)
                    bufs = [None if optional and not want else np.full(shape(U, R, plan.n_tiles[0], lag), -7, dtype=dtype)
                            for _, shape, dtype, optional in outputs]
                    rc = entry(plan.handle, *(native._ptr(a) for a in raw), U, T, n if window is None else window, stride,
                               *([lag] if has_lag else []), *(native._ptr(b) for b in bufs))
                    assert list(res) == [key for key, *_ in outputs] + ["code"], msg
                    assert res["code"] == rc == native.VET_OK, msg
                    for (key, *_), want_arr in zip(outputs, bufs):
                        if want_arr is None:
                            assert res[key] is None, (msg, key)
                        else:
                            same_array(res[key], want_arr, (msg, key))


# ----------------------------------------------------------------------------------------------------- the device wrappers
@pytest.mark.parametrize("method", list(CALLS))
def test_device_wrapper_is_the_host_result(native, engine, plan, video, method):
    import torch
    stem, pairs, whole, want_kw, has_lag, outputs = CALLS[method]
    mu, mv, ids = video
    window, stride, R = (PAIR_ROWS if pairs else FRAME_ROWS)[0]
    lag = R - 1 if has_lag else None
    kw = dict(window=window, stride=stride, **({want_kw: True} if want_kw else {}), **({"max_lag": lag} if has_lag else {}))
    host = getattr(plan, method)(mu=mu, mv=mv, **kw)
    dev = torch.device("cuda", 0)
    d_mu, d_mv, d_ids = (torch.from_numpy(np.array(a)).to(dev) for a in (mu, mv, ids))
    tdt = {F64: torch.float64, I32: torch.int32}
    for src in ("mu_mv", "ids") if method in WITH_D_IDS else ("mu_mv",):
        bufs = [torch.full(shape(U, R, plan.n_tiles[0], lag), -7, dtype=tdt[dtype], device=dev) for _, shape, dtype, _ in outputs]
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        getattr(plan, method + "_device")(d_mu.data_ptr(), d_mv.data_ptr(), U, T, window, stride, *([lag] if has_lag else []),
                                          *(b.data_ptr() for b in bufs), d_status=status.data_ptr(),
                                          **(dict(d_ids=d_ids.data_ptr()) if src == "ids" else {}))
        engine.synchronize()
        for (key, *_), b in zip(outputs, bufs):
            same_array(b.cpu().numpy(), host[key], (method, src, key))
        assert status.cpu().numpy()[0] == 0, (method, src)          # no sample out of range


# ------------------------------------------------------------------------------------------------------------ the analyzers
def make_analyzer(kind):
    import viewport_entropy_toolkit as vt
    from viewport_entropy_toolkit.config import AnalyzerConfig, EntropyConfig, NaiveAnalyzerConfig
    ec = EntropyConfig(use_weight_distribution=True)
    if kind == "naive":
        return vt.NaiveSpatialEntropyAnalyzer(NaiveAnalyzerConfig(tile_height=10, tile_width=20, video_width=W, video_height=H,
                                                                  entropy_config=ec))
    cls = vt.SpatialEntropyAnalyzer if kind == "spatial" else vt.TransitionEntropyAnalyzer
    return cls(AnalyzerConfig(tile_counts=[TILE_COUNT], video_width=W, video_height=H, entropy_config=ec))


def loaded(kind, mu, mv):
    an = make_analyzer(kind)
    an.load_arrays(np.arange(T) * 0.1, np.array(mu), np.array(mv))
    return an


def row_methods(an):
    """(method, arguments) of the analyzer's row calls at window 5, stride 2; the windowed ones first."""
    out = [("compute_windowed_entropy", dict(window=5, stride=2)), ("compute_user_entropy", dict(window=5, stride=2))]
    if hasattr(an, "compute_user_divergence"):
        out += [("compute_user_divergence", dict(window=5, stride=2)), ("compute_window_divergence", dict(window=5, stride=2, max_lag=2)),
                ("compute_crowd_divergence", dict(window=5, stride=2))]
    return out


@pytest.mark.parametrize("kind", ["spatial", "transition"])
def test_analyzer_hand_assigned_vectors_run_on_a_temporary_plan(video, kind):
    import pandas as pd
    from viewport_entropy_toolkit.analyzers._base import _DataCache
    from viewport_entropy_toolkit.data_types import Vector
    mu, mv, ids = video
    an = loaded(kind, mu, mv)
    grid = an.compute_user_entropy(5, 2)
    cached = an._plan
    dirs = cached.read_dirs()
    names = an._dense[3]
    frame = {"time": np.arange(T) * 0.1}
    for u, name in enumerate(names):
        frame[name] = [None if i < 0 else Vector(*map(float, dirs[i])) for i in ids[:, u]]
    cache = _DataCache([], W, H)
    cache["vectors"] = pd.DataFrame(frame)                   # a caller's own frame table: the ids path
    an._data_cache = cache
    assert an._samples()[0] == "ids"
    made, get_plan = [], an._get_plan

    def spy(dir_table=None):
        p = get_plan(dir_table=dir_table)
        made.append((dir_table is not None, p))
        return p

    an._get_plan = spy
    vec = an.compute_user_entropy(5, 2)
    assert [temporary for temporary, _ in made] == [True] and made[0][1] is not cached
    assert made[0][1].handle is None and cached.handle is not None          # the temporary plan is closed, the cached one lives
    assert list(vec.columns) == list(grid.columns) and vec["user"].tolist() == grid["user"].tolist()
    assert np.array_equal(vec["samples"], grid["samples"])
    got, want = vec["entropy"].to_numpy(), grid["entropy"].to_numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).any()
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0, equal_nan=True)


@pytest.mark.parametrize("kind", ["spatial", "naive", "transition"])
def test_analyzer_sample_out_of_range_is_the_engines_refusal(video, kind):
    from viewport_entropy_toolkit import ValidationError
    mu, mv, _ = video
    an = loaded(kind, mu, mv)
    an._dense[1][2, 0], an._dense[2][2, 0] = 1.5, 0.5            # after load_arrays' own check: the engine has to refuse it
    for method, kw in row_methods(an):
        with pytest.raises(ValidationError, match="^Normalized coordinates must be between 0 and 1$"):
            getattr(an, method)(**kw)


@pytest.mark.parametrize("kind", ["spatial", "naive", "transition"])
def test_analyzer_window_without_a_sample(video, kind):
    """Frames 0..4 hold no sample: row 0 of every call.  The windowed methods raise what they raised before the runner existed;
    for the other methods the row is data."""
    from viewport_entropy_toolkit import ValidationError
    mu, mv = (np.array(a) for a in video[:2])
    mu[0:5] = np.nan
    mv[0:5] = np.nan
    an = loaded(kind, mu, mv)
    (windowed, kw), *others = row_methods(an)
    if kind == "transition":
        want = an._empty_window_error("grid", mu, mv, 5, 2)
        assert type(want) is ValidationError and str(want) == "Empty vector dictionary"
    else:
        want = ValidationError("Empty vector dictionary" if kind == "spatial" else "Empty radial points dictionary")
    with pytest.raises(type(want)) as e:
        getattr(an, windowed)(**kw)
    assert type(e.value) is type(want) and str(e.value) == str(want)
    assert len(others) == (1 if kind == "transition" else 4)
    for method, kw in others:
        df = getattr(an, method)(**kw)
        if method == "compute_user_entropy":
            first = df[df["time"] == 0.1 if kind == "transition" else df["time"] == 0.0]
            assert len(first) == U and np.isnan(first["entropy"]).all() and (first["samples"] == 0).all(), method
            assert np.isfinite(df["entropy"]).any()
        elif method == "compute_user_divergence":
            assert np.isnan(df["divergence"][0]).all() and (df["samples"][0] == 0).all() and np.isfinite(df["divergence"][3]).all()
        elif method == "compute_window_divergence":
            assert df["samples"][0] == 0 and np.isnan(df["shift"][0]) and np.isnan(df["divergence"][0]).all()
            assert np.isfinite(df["shift"][1])
        else:
            first = df[df["time"] == 0.0]
            assert len(first) == U and np.isnan(first["divergence"]).all() and (first["samples"] == 0).all()
            assert df.attrs["rows"]["samples"][0] == 0 and np.isfinite(df["divergence"]).any()
