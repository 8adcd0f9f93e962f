"""Lat/lon cell heatmaps of the naive analyzer, the parts that run without a GPU: the C-ABI surface, the argument checks
that come before any device call, the analyzer's checks before compute_entropy, and the oracle's own invariants."""
import ctypes

import numpy as np
import pytest

from tests import _naive_heatmap_oracle as nho
from tests.test_cabi_symbols import header_functions

ENTRIES = ["vet_heatmap_create_latlon", "vet_heatmap_render_binned", "vet_heatmap_render_binned_host"]
GRIDS = [(10, 10), (45, 30), (20, 20), (180, 90), (360, 180), (1, 1), (20, 10), (72, 60)]   # (tile_width, tile_height)


# --------------------------------------------------------------------------- C-ABI
def test_header_library_and_signatures():
    from viewport_entropy_toolkit import _native
    fns = header_functions()
    assert set(ENTRIES) <= set(fns)
    lib = ctypes.CDLL(str(_native.LIB_PATH))
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert set(ENTRIES) <= set(_native.SIGNATURES)
    assert sorted(_native.SIGNATURES) == fns
    assert _native.load_library().vet_version() == 141


def test_null_and_invalid_arguments_without_a_device():
    """Argument checks come before any device call."""
    from viewport_entropy_toolkit import _native
    lib = _native.load_library()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    out = ctypes.c_void_p()
    INVALID = _native.VET_ERR_INVALID
    assert lib.vet_heatmap_create_latlon(None, 10, 10, 64, 32, 200, 100, 2, ctypes.byref(out)) == INVALID
    assert b"NULL" in lib.vet_last_error()
    assert lib.vet_heatmap_create_latlon(p, 10, 10, 64, 32, 200, 100, 2, None) == INVALID
    assert lib.vet_heatmap_render_binned(None, None, None, None, 0, 0, 1, None, None) == INVALID
    assert lib.vet_heatmap_render_binned(None, p, p, p, 4, 1, 1, p, None) == INVALID
    assert lib.vet_heatmap_render_binned(p, None, p, p, 4, 1, 1, p, None) == INVALID
    assert lib.vet_heatmap_render_binned(p, p, None, p, 4, 1, 1, p, None) == INVALID
    assert lib.vet_heatmap_render_binned(p, p, p, None, 4, 1, 1, p, None) == INVALID
    assert lib.vet_heatmap_render_binned(p, p, p, p, 4, 1, 1, None, None) == INVALID
    assert lib.vet_heatmap_render_binned_host(None, None, None, None, 0, 0, 1, None) == INVALID
    assert lib.vet_heatmap_render_binned_host(None, p, p, p, 4, 1, 1, p) == INVALID
    assert lib.vet_heatmap_render_binned_host(p, None, p, p, 4, 1, 1, p) == INVALID
    assert lib.vet_heatmap_render_binned_host(p, p, p, None, 4, 1, 1, p) == INVALID
    assert lib.vet_heatmap_render_binned_host(p, p, p, p, 4, 1, 1, None) == INVALID
    assert b"NULL" in lib.vet_last_error()


# --------------------------------------------------------------------------- the analyzer
def _analyzer(tmp_path):
    import viewport_entropy_toolkit as vt
    from viewport_entropy_toolkit.config import NaiveAnalyzerConfig
    return vt.NaiveSpatialEntropyAnalyzer(NaiveAnalyzerConfig(output_dir=tmp_path / "out", tile_width=20, tile_height=10))


def test_heatmaps_before_compute_entropy(tmp_path):
    from viewport_entropy_toolkit.data_types import ValidationError
    an = _analyzer(tmp_path)
    with pytest.raises(ValidationError, match="No entropy results. Call compute_entropy first."):
        an.render_heatmaps()
    for name in ("h.npy", "h.mp4"):
        with pytest.raises(ValidationError, match="No entropy results. Call compute_entropy first."):
            an.save_heatmaps(tmp_path / name)
        assert not (tmp_path / name).exists()
    (tmp_path / "png").mkdir()
    with pytest.raises(ValidationError, match="No entropy results. Call compute_entropy first."):
        an.save_heatmaps(tmp_path / "png")
    assert list((tmp_path / "png").iterdir()) == []


def test_naive_analyzer_uses_the_shared_writers():
    """The writers are the mixin's; only the device part is the naive class's own, and the other two analyzers still
    resolve every heatmap method to the mixin."""
    import viewport_entropy_toolkit as vt
    from viewport_entropy_toolkit.analyzers._heatmaps import _HeatmapMixin
    for name in ("render_heatmaps", "save_heatmaps", "_frame_range", "_heatmap_job"):
        assert getattr(vt.NaiveSpatialEntropyAnalyzer, name) is getattr(_HeatmapMixin, name)
    for name in ("_heatmap", "_render_block"):
        assert getattr(vt.NaiveSpatialEntropyAnalyzer, name) is not getattr(_HeatmapMixin, name)
        assert getattr(vt.SpatialEntropyAnalyzer, name) is getattr(_HeatmapMixin, name)
        assert getattr(vt.TransitionEntropyAnalyzer, name) is getattr(_HeatmapMixin, name)


# --------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("tw,th", GRIDS)
@pytest.mark.parametrize("W,H", [(200, 100), (640, 480), (1200, 600), (7, 5)])
def test_oracle_cells_are_inside_the_plan_grid(tw, th, W, H):
    m = nho.cell_map(tw, th, W, H)
    n = nho.n_cells(tw, th)
    assert n <= 65535 and m.min() >= 0 and m.max() < n
    # no pixel centre reaches the lon-180 column or the lat-90 row
    li, lj = m // nho.n_lat(th), m % nho.n_lat(th)
    assert li.max() < 360 // tw and lj.max() < 180 // th
    # row 0 is the top: latitudes fall down the rows
    assert (np.diff(lj, axis=0) <= 0).all()


@pytest.mark.parametrize("tw,th", GRIDS)
def test_oracle_plan_cells_match_the_naive_plan_numbering(tw, th):
    """The oracle's direction cells are the bins the naive plan builds: same count, same LUT."""
    from viewport_entropy_toolkit import _quantiser
    VW, VH = 200, 100
    d = nho.direction_cells(tw, th, VW, VH)
    lon, lat = _quantiser.axis_angles(VW, VH)
    li = ((lon + 180) / tw).astype(np.int64)
    lj = ((lat + 90) / th).astype(np.int64)
    assert (int(li.max()) + 1) * (int(lj.max()) + 1) == nho.n_cells(tw, th)
    assert d.min() >= 0 and d.max() < nho.n_cells(tw, th)
    assert d[0, 0] == (180 // tw) * nho.n_lat(th) + 180 // th       # px = 0 is lon 0, py = 0 is lat 90
    assert d[VH // 2, VW] // nho.n_lat(th) == 360 // tw            # px = W is lon 180: the extra column


@pytest.mark.parametrize("tw,th", [(10, 10), (1, 1), (360, 180)])
def test_oracle_counts_sum_to_present(tw, th):
    rng = np.random.default_rng(5)
    T, U = 12, 40
    mu, mv = rng.random((T, U)), rng.random((T, U))
    mu[rng.random((T, U)) < 0.2] = np.nan
    mu[3] = np.nan                                    # a frame with nobody
    mu[4, :3] = [0.0, 1.0, 1.5]                       # px = 0, px = W, out of range
    mv[5, :2] = [0.0, -0.1]                           # py = 0, out of range
    cnt, present = nho.counts(mu, mv, tw, th, 200, 100)
    assert (cnt.sum(axis=1) == present).all()
    assert present[3] == 0 and present[4] == (~np.isnan(mu[4])).sum() - 1
    frames = nho.render(mu, mv, tw, th, 40, 20, 200, 100, markers=False)
    assert (frames[3] == 204).all()                   # nobody: grey everywhere
