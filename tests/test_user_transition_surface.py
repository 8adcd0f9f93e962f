"""Per-viewer transition entropy, CPU side: the C-ABI surface, the analyzer's argument handling, and the claim the GPU tests rest
on — the numpy oracle's dict walk on one viewer's (source, destination) sequence of a row reproduces golden G17, the REAL
reference's compute_transition_entropy on that viewer's pooled dicts (tools/gen_golden_user_transition.py), and the closed form
the kernels evaluate equals the dict walk.  No GPU."""
import ctypes

import numpy as np
import pytest

from tests import _user_transition_oracle as ut

W, H = 100, 200
SYMBOLS = ("vet_user_transition_entropy", "vet_user_transition_entropy_ids", "vet_user_transition_entropy_host",
           "vet_test_user_transition_hash")
SHAPES = ((299, 1), (20, 20), (20, 7), (64, 5), (65, 5), (2, 1))
TILE_COUNTS = ((50,), (50, 100, 200), (20,))


def cases():
    for tcs in TILE_COUNTS:
        for w, s in SHAPES:
            yield f"tc{'_'.join(map(str, tcs))}_w{w}_s{s}", list(tcs), w, s


@pytest.fixture(scope="module")
def data(golden_dir):
    g16 = np.load(golden_dir / "g16_user_entropy.npz")
    return g16["mu"], g16["mv"], np.load(golden_dir / "g17_user_transition.npz")


@pytest.fixture(scope="module")
def literal_rows(data):
    """the dict-walk oracle on every stored row of every case, computed once"""
    mu, mv, g = data
    out = {}
    for tag, tcs, w, s in cases():
        out[tag] = ut.literal(mu, mv, W, H, tcs, w, s, rows=g[f"{tag}__rows"])
    return out


def test_library_exports_the_per_user_transition_entry_points():
    from viewport_entropy_toolkit import _native
    lib = ctypes.CDLL(str(_native.LIB_PATH))
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _native.SIGNATURES
    assert hasattr(_native.Plan, "transition_per_user") and hasattr(_native.Plan, "transition_per_user_device")
    assert hasattr(_native.Engine, "test_user_transition_hash")


def test_analyzer_method_exists_and_validates_arguments():
    from viewport_entropy_toolkit import TransitionEntropyAnalyzer, ValidationError
    from viewport_entropy_toolkit.config import AnalyzerConfig
    mu = np.full((30, 4), 0.5)
    an = TransitionEntropyAnalyzer(AnalyzerConfig(tile_counts=[20]))
    with pytest.raises(ValidationError, match="No data available"):
        an.compute_user_entropy(5)
    an.load_arrays(np.arange(30) * 0.1, mu, mu)
    # 30 frames are 29 pairs: a window of 30 is too long; the wording is compute_windowed_entropy's
    for window, stride in ((0, 1), (-2, 1), (5, 0), (5, -1), (30, 1), (2.5, 1), (5, 1.5), (True, 1), ("5", 1)):
        with pytest.raises(ValueError) as a:
            an.compute_user_entropy(window, stride)
        with pytest.raises(ValueError) as b:
            an.compute_windowed_entropy(window, stride)
        assert str(a.value) == str(b.value)
    assert "frame pairs" in TransitionEntropyAnalyzer.compute_user_entropy.__doc__


def test_golden_holds_the_cases_the_feature_is_pinned_on(data):
    mu, mv, g = data
    assert mu.shape == (300, 8) and np.isnan(mu[100:200, 3]).all()
    assert sorted({k.rsplit("__", 1)[0] for k in g.files}) == sorted(tag for tag, *_ in cases())
    for tag, tcs, w, s in cases():
        rows, ent, n, src = (g[f"{tag}__{k}"] for k in ("rows", "entropy", "samples", "srccount"))
        R = ut.n_rows(300, w, s)
        assert rows[0] == 0 and rows[-1] == R - 1 and (len(rows) == R or (w, s) == (2, 1))
        assert ent.shape == n.shape == (8, len(rows)) and src.shape == (8, len(rows), len(ut.vo.fibonacci_lattice(tcs[0])))
        assert np.array_equal(src.sum(axis=2), n) and np.array_equal(np.isnan(ent), n <= 1)      # empty rows and 0 / 0
        if w in (20, 64, 65):
            assert 5 <= (n == 0).sum() <= 11, tag                      # user 3's stretch away
        if (w, s) in ((20, 7), (2, 1)):
            assert (n == 1).any(), tag
        if w == 299:
            assert (n > src.shape[-1]).all(), tag                      # N > n_0: the log2(n) normaliser
        else:
            assert ((n > 1) & (n <= tcs[0])).any(), tag                # 1 < N <= n: the log2(N) normaliser
        if w in (64, 65):
            assert (n > len(ut.vo.fibonacci_lattice(tcs[0]))).sum() >= 183, tag      # N > n next to N <= n in one case
        if w in (20, 64, 65):                                          # many distinct values (the smallest case: 21 tiles, 14 rows)
            assert len(np.unique(ent[np.isfinite(ent)])) >= (59 if tag == "tc20_w20_s20" else 80), tag
        if (w, s) == (2, 1):                                           # the rows where user 3 leaves and returns
            assert set(range(95, 104)) | set(range(195, 204)) <= set(rows.tolist())


def test_oracle_dict_walk_reproduces_the_reference(data, literal_rows):
    """Entropy to 1e-12 relative (NaN = NaN); samples and lattice 0's source counts exact."""
    _, _, g = data
    for tag, *_ in cases():
        ent, samples, src = literal_rows[tag]
        np.testing.assert_allclose(ent, g[f"{tag}__entropy"], rtol=1e-12, atol=0, equal_nan=True, err_msg=tag)
        assert np.array_equal(samples, g[f"{tag}__samples"]), tag
        assert np.array_equal(src, g[f"{tag}__srccount"]), tag


def test_closed_form_equals_the_dict_walk_on_every_stored_row(data, literal_rows):
    mu, mv, g = data
    for tag, tcs, w, s in cases():
        a = literal_rows[tag]
        b = ut.fast(mu, mv, W, H, tcs, w, s, rows=g[f"{tag}__rows"])
        np.testing.assert_allclose(b[0], a[0], rtol=1e-12, atol=0, equal_nan=True, err_msg=tag)
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), tag
