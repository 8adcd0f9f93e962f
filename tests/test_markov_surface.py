"""Windowed Markov transition statistics (entropy rate, stationary / destination entropy, mutual information at a lag, stay share,
the transition matrix), CPU side: the C-ABI surface, the analyzer's argument handling, and the claim the GPU tests rest on — the
numpy oracles of tests/_markov_oracle.py reproduce golden G24, the textbook forms applied in plain Python to the REAL reference's
own (source tile, destination tile) pairs (tools/gen_golden_markov.py).  No GPU."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from tests import _markov_oracle as mo

W, H = 100, 200
T = 60
SYMBOLS = ("vet_transition_markov", "vet_transition_markov_ids", "vet_transition_markov_host", "vet_test_markov_chunk_rows")
TILE_COUNTS = ([50], [50, 100, 200])
ATOL = 1e-12


@pytest.fixture(scope="module")
def g15(golden_dir):
    return np.load(golden_dir / "g15_windowed_transition.npz")


@pytest.fixture(scope="module")
def g24(golden_dir):
    return np.load(golden_dir / "g24_markov.npz")


def case_tags():
    """(tag, tile counts, window, stride, lag) of every golden case; the whole video is window = T - lag"""
    return [(f"tc{'_'.join(map(str, tcs))}_w{w}_s{s}_l{lag}", tcs, w, s, lag)
            for tcs in TILE_COUNTS for lag in (1, 3) for w in (1, 2, 20, T - lag) for s in (1, 7)]


def same(got, want, msg):
    print(msg, "max abs err", float(np.nanmax(np.abs(got - want), initial=0.0)))
    assert np.array_equal(np.isnan(got), np.isnan(want)), msg
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL, equal_nan=True, err_msg=msg)


def test_library_exports_the_markov_entry_points():
    from viewport_entropy_toolkit import _native
    lib = ctypes.CDLL(str(_native.LIB_PATH))
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _native.SIGNATURES
    # vet_transition_entropy_windowed's signatures with `int lag` behind stride
    for tail, at in (("", 7), ("_ids", 6), ("_host", 8)):
        res, args = _native.SIGNATURES["vet_transition_entropy_windowed" + tail]
        assert _native.SIGNATURES["vet_transition_markov" + tail] == (res, args[:at] + [ctypes.c_int] + args[at:]), tail
    assert _native.SIGNATURES["vet_test_markov_chunk_rows"] == _native.SIGNATURES["vet_test_coverage_chunk_rows"]
    for name in ("transition_markov", "transition_markov_device"):
        assert hasattr(_native.Plan, name)
    assert hasattr(_native.Engine, "test_markov_chunk_rows")
    assert "transition_markov" in _native._ROW_CALLS and len(_native._ROW_CALLS) == 11
    stem, pairs, whole, empty_ok, outputs = _native._ROW_CALLS["transition_markov"]
    assert (stem, pairs, whole, empty_ok) == ("vet_transition_markov", True, True, False)
    assert [(key, dims, optional) for key, dims, _, optional in outputs] == \
        [("stats", "5R", False), ("matrix", "Rnn", True), ("samples", "R", False)]
    assert _native.load_library().vet_version() == 141


def test_header_and_ctypes_table_agree():
    from viewport_entropy_toolkit import _native
    header = (Path(__file__).resolve().parent.parent / "include" / "vet.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(vet_[a-z0-9_]+)\s*\(", text))
    assert set(SYMBOLS) <= declared and declared == set(_native.SIGNATURES)
    for name in SYMBOLS:                # argument counts of the declarations
        args = re.search(rf"\b{name}\s*\(([^)]*)\)", text).group(1)
        assert len(args.split(",")) == len(_native.SIGNATURES[name][1]), name
    assert "#define VET_VERSION 141" in header


def test_window_rows_arithmetic_for_lagged_pairs():
    from viewport_entropy_toolkit import _native
    rows = _native.load_library().vet_window_rows
    for frames in (2, 8, 60, 10000):
        for lag in (1, 3, frames - 1):
            P = frames - lag
            if P < 1:
                continue
            for w in (1, 2, 20, P):
                if w > P:
                    continue
                for s in (1, 7, w):
                    assert rows(P, w, s) == mo.n_rows(frames, w, s, lag) == len(range(0, P - w + 1, s))
    assert rows(57, 20, 7) == 6 and rows(57, 57, 1) == 1 and rows(57, 58, 1) < 0


def test_analyzer_method_exists_and_validates_arguments_before_the_engine():
    """No GPU here: every refusal below comes before a plan is built."""
    from viewport_entropy_toolkit import TransitionEntropyAnalyzer, ValidationError
    from viewport_entropy_toolkit.config import AnalyzerConfig
    mu = np.full((30, 4), 0.5)
    an = TransitionEntropyAnalyzer(AnalyzerConfig(tile_counts=[20]))
    with pytest.raises(ValidationError, match="No data available"):
        an.compute_markov_entropy(5)
    an.load_arrays(np.arange(30) * 0.1, mu, mu)

    def no_engine(*a, **k):
        raise AssertionError("the engine was touched before the arguments were checked")

    an._get_plan = no_engine
    # 30 frames at lag 3 are 27 pairs: a window of 28 is too long; lag 30 leaves no pair
    for kw in (dict(window=0), dict(window=-2), dict(window=5, stride=0), dict(window=5, stride=-1), dict(window=30),
               dict(window=28, lag=3), dict(window=2.5), dict(window=5, stride=1.5), dict(window=True), dict(window="5"),
               dict(window=5, lag=0), dict(window=5, lag=-1), dict(window=1, lag=30), dict(lag=30), dict(window=5, lag=1.0),
               dict(window=5, lag=True), dict(window=5, lag="1")):
        with pytest.raises(ValueError):
            an.compute_markov_entropy(**kw)
    for name in ("compute_user_divergence", "compute_window_divergence", "compute_crowd_divergence"):
        assert not hasattr(an, name)                 # tests/test_row_call_bindings_gpu.py tells the analyzers apart by them
    doc = TransitionEntropyAnalyzer.compute_markov_entropy.__doc__
    assert "lag" in doc and "mutual" in doc and "keep_matrix" in doc


def test_plan_wrapper_refuses_a_bad_lag_before_the_library_is_called():
    from viewport_entropy_toolkit import _native
    for lag in (0, -1, 1.5, True, "1"):
        with pytest.raises(ValueError, match="lag"):
            _native.Plan._pair_lag(lag, 30)
    with pytest.raises(ValueError, match=r"need 1 <= lag <= n_frames - 1 \(got lag=30, 30 frames\)"):
        _native.Plan._pair_lag(30, 30)
    assert _native.Plan._pair_lag(np.int64(29), 30) == 29


# ------------------------------------------------------------------------------------------- golden G24
def test_golden_holds_the_cases_the_feature_is_pinned_on(g15, g24):
    tags = case_tags()
    assert sorted({k.rsplit("__", 1)[0] for k in g24.files}) == sorted(tag for tag, *_ in tags)
    assert len(tags) == 32
    total = 0
    for tag, tcs, w, s, lag in tags:
        rows = g24[f"{tag}__rows"]
        R = mo.n_rows(T, w, s, lag)
        total += len(rows)
        assert np.array_equal(rows, np.unique([0, R // 2, max(R - 2, 0), R - 1])), tag
        assert g24[f"{tag}__stats"].shape == (5, len(rows)) and g24[f"{tag}__samples"].shape == (len(rows),), tag
        assert g24[f"{tag}__matrix"].shape == (len(rows), 51, 51) and g24[f"{tag}__matrix"].dtype == np.int32, tag
    assert total >= 100
    # only lattice 0's matrix is stored: the two plans share it
    for tag, tcs, w, s, lag in tags:
        if len(tcs) == 1:
            other = tag.replace("tc50_", "tc50_100_200_", 1)
            assert g24[f"{tag}__matrix"].tobytes() == g24[f"{other}__matrix"].tobytes(), tag
            assert g24[f"{tag}__samples"].tobytes() == g24[f"{other}__samples"].tobytes(), tag


def test_golden_identities(g15, g24):
    seen_single = False
    for tag, tcs, w, s, lag in case_tags():
        stats, samples, matrix = g24[f"{tag}__stats"], g24[f"{tag}__samples"], g24[f"{tag}__matrix"]
        assert (samples > 0).all(), tag                                        # G15's video has no empty window
        assert np.array_equal(matrix.sum(axis=(1, 2)), samples), tag
        assert (matrix >= 0).all(), tag
        rate, stationary, dest, mutual, stay = stats
        assert (rate >= 0).all() and (rate <= stationary + dest).all(), tag
        assert (mutual <= np.minimum(stationary, dest) + 1e-12).all(), tag
        np.testing.assert_allclose(mutual, dest - rate, rtol=0, atol=0 if len(tcs) == 1 else ATOL, err_msg=tag)   # a mean of differences
        assert ((stay >= 0) & (stay <= 1)).all(), tag
        if len(tcs) == 1:
            assert np.array_equal(stay, np.trace(matrix, axis1=1, axis2=2) / samples), tag
            single = ((matrix > 0).sum(axis=2) <= 1).all(axis=1)               # every source has one destination
            assert (rate[single] == 0.0).all(), tag
            seen_single |= bool(single.any())
        if lag == 1 and w != T - 1:                                            # the cases G15 shares: same rows, same pooled samples
            g15_tag = tag.rsplit("_l", 1)[0]
            assert np.array_equal(g15[f"{g15_tag}__rows"], g24[f"{tag}__rows"]), tag
            assert np.array_equal(matrix.sum(axis=2), g15[f"{g15_tag}__srccount"]), tag
            assert np.array_equal(samples, g15[f"{g15_tag}__samples"]), tag
    assert seen_single


@pytest.mark.parametrize("which", ["literal", "fast"])
def test_oracles_reproduce_the_golden(g15, g24, which):
    """samples and matrix exactly, stats to 1e-12 absolute with NaN in the same places."""
    mu, mv = g15["mu"], g15["mv"]
    tiles = {tuple(tcs): mo.tiles_of(mu, mv, W, H, tcs) for tcs in TILE_COUNTS}
    for tag, tcs, w, s, lag in case_tags():
        stats, samples, matrix = getattr(mo, which)(mu, mv, W, H, tcs, w, s, lag, rows=g24[f"{tag}__rows"], tiles=tiles[tuple(tcs)])
        assert np.array_equal(samples, g24[f"{tag}__samples"]), tag
        assert np.array_equal(matrix, g24[f"{tag}__matrix"]), tag
        same(stats, g24[f"{tag}__stats"], f"{which} {tag}")


def test_fast_oracle_equals_the_literal_walk_on_every_row():
    """The form the kernels evaluate against the textbook walk, 1e-12, on every row (none left out) — with absent samples, a span
    of frames nobody is in (empty rows: NaN in both), one-sample rows (all zero but stay) and the whole video (window=None)."""
    from viewport_entropy_toolkit import _synthetic
    mu, mv = _synthetic.random_walk_video(7, 60, base_seed=41, p_absent=0.3)
    mu[20:27] = np.nan
    mv[20:27] = np.nan
    seen_empty = seen_one = False
    for tcs in ([20], [20, 50]):
        tiles = mo.tiles_of(mu, mv, W, H, tcs)
        for window, stride, lag in ((1, 1, 1), (2, 1, 3), (5, 2, 1), (20, 7, 3), (None, 1, 1), (None, 1, 3)):
            a = mo.literal(mu, mv, W, H, tcs, window, stride, lag, tiles=tiles)
            b = mo.fast(mu, mv, W, H, tcs, window, stride, lag, tiles=tiles)
            assert a[0].shape == (5, mo.n_rows(60, 60 - lag if window is None else window, stride, lag))
            same(b[0], a[0], f"{tcs} {window} {stride} {lag}")
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[2].sum(axis=(1, 2)), a[1])
            assert np.isnan(a[0][:, a[1] == 0]).all() and not np.isnan(a[0][:, a[1] > 0]).any()
            one = a[1] == 1
            assert (a[0][:4, one] == 0).all() and np.isin(a[0][4, one] * len(tcs), np.arange(len(tcs) + 1)).all()   # stay: 0 or 1 per lattice
            assert (b[0][:4, one] == 0).all()
            seen_empty |= bool((a[1] == 0).any())
            seen_one |= bool(one.any())
    assert seen_empty and seen_one
