"""Per-frame tile-attention heatmaps, the parts that run without a GPU: the C-ABI surface, the oracle's frame definition
(colours, marker positions), the reference's visualisation names and the reference's own test module."""
import ctypes
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import _heatmap_oracle as ho
from tests.test_cabi_symbols import header_functions

ROOT = Path(__file__).resolve().parent.parent
HEATMAP_ENTRIES = ["vet_heatmap_create", "vet_heatmap_destroy", "vet_heatmap_read_map", "vet_heatmap_render",
                   "vet_heatmap_render_result"]
REFERENCE_NAMES = ["PlotManager", "create_animation", "save_video", "save_fb_tiling_visualization_image",
                   "save_fb_tiling_visualization_video", "save_tiling_visualization_image", "save_tiling_visualization_video"]


# --------------------------------------------------------------------------- C-ABI
def test_header_library_and_signatures():
    from viewport_entropy_toolkit import _native
    fns = header_functions()
    assert set(HEATMAP_ENTRIES) <= set(fns)
    lib = ctypes.CDLL(str(_native.LIB_PATH))
    for name in HEATMAP_ENTRIES:
        assert hasattr(lib, name), name
    assert set(HEATMAP_ENTRIES) <= set(_native.SIGNATURES)
    assert sorted(_native.SIGNATURES) == fns
    assert _native.load_library().vet_version() == 141


def test_null_arguments_are_invalid_without_a_device():
    """Argument checks come before any device call."""
    from viewport_entropy_toolkit import _native
    lib = _native.load_library()
    out = ctypes.c_void_p()
    assert lib.vet_heatmap_create(None, None, 0, 0, 0, 0, 0, 0, ctypes.byref(out)) == _native.VET_ERR_INVALID
    assert lib.vet_heatmap_read_map(None, None) == _native.VET_ERR_INVALID
    assert lib.vet_heatmap_render(None, None, None, None, None, 0, 0, None, None) == _native.VET_ERR_INVALID
    assert lib.vet_heatmap_render_result(None, None, None, None, None, 0, 0, 0, None) == _native.VET_ERR_INVALID
    assert lib.vet_heatmap_destroy(None) == _native.VET_OK


# --------------------------------------------------------------------------- colours
def test_colour_examples():
    assert ho.colour(0.0, 1).tolist() == [204, 204, 204]
    assert ho.colour(0.5, 1).tolist() == [230, 102, 102]
    assert ho.colour(1.0, 1).tolist() == [255, 0, 0]
    assert ho.colour(1.5, 3).tolist() == [230, 102, 102]
    assert (1 - 0.8) == 0.19999999999999996


def test_colour_clip_zero_users_and_signed_zero():
    assert ho.colour(2.0, 1).tolist() == [255, 0, 0]           # clipped to 1
    assert ho.colour(-1.0, 1).tolist() == [204, 204, 204]      # clipped to 0
    assert ho.colour(5.0, 0).tolist() == [204, 204, 204]       # no user present: intensity 0
    assert ho.colour(-0.0, 4).tolist() == [204, 204, 204]      # a zero-valued key
    w = np.array([[0.0, 0.25, 3.0], [1.0, 1.0, 1.0]])
    got = ho.colour(w, np.array([[4], [0]]))
    assert got.shape == (2, 3, 3) and got.dtype == np.uint8
    assert got[1].tolist() == [[204, 204, 204]] * 3


def test_colour_matches_the_reference_formula():
    """Every byte is floor(v * 255 + 0.5) of the reference's RGBA floats."""
    def reference_rgb(intensity):                             # PlotManager._get_color_from_intensity
        intensity = np.clip(intensity, 0, 1)
        grey_intensity = 0.8
        red = (intensity * (1 - grey_intensity)) + grey_intensity
        green = blue = grey_intensity - (intensity * grey_intensity)
        return (red, green, blue, 1.0)
    rng = np.random.default_rng(5)
    for w, n in zip(rng.uniform(0, 40, 500), rng.integers(1, 40, 500)):
        r, g, b, _ = reference_rgb(w / n)
        assert ho.colour(w, n).tolist() == [int(np.floor(v * 255 + 0.5)) for v in (r, g, b)]


# --------------------------------------------------------------------------- markers
def test_marker_centre_edges():
    VW, VH, W, H = 1200, 600, 97, 61
    row, col = ho.marker_centres(np.array([0.0, 1.0, 0.5, np.nan, 1.5, 0.999999]),
                                 np.array([0.0, 1.0, 0.5, 0.5, 0.5, 0.999999]), VW, VH, W, H)
    assert col.tolist() == [0, W - 1, 600 * W // VW, -1, -1, 1199 * W // VW]
    assert row.tolist() == [0, H - 1, 300 * H // VH, -1, -1, 599 * H // VH]


def _blank(T=1, H=9, W=11):
    return np.full((T, H, W, 3), 200, dtype=np.uint8)


def test_marker_wraps_longitude_and_clamps_latitude():
    VW, VH = 110, 90
    f = ho.paint_markers(_blank(), np.array([[0.0]]), np.array([[0.0]]), VW, VH, 2)[0]
    black = np.argwhere((f == 0).all(-1))
    assert sorted({int(r) for r, _ in black}) == [0, 1, 2]                   # rows -2, -1 clamped away
    assert sorted({int(c) for _, c in black}) == [0, 1, 2, 9, 10]             # columns -2, -1 wrap to W-2, W-1
    f = ho.paint_markers(_blank(), np.array([[1.0]]), np.array([[1.0]]), VW, VH, 2)[0]
    black = np.argwhere((f == 0).all(-1))
    assert sorted({int(r) for r, _ in black}) == [6, 7, 8]
    assert sorted({int(c) for _, c in black}) == [0, 1, 8, 9, 10]


@pytest.mark.parametrize("radius,count", [(0, 1), (3, 49)])
def test_marker_radius(radius, count):
    f = ho.paint_markers(_blank(H=21, W=21), np.array([[0.5]]), np.array([[0.5]]), 210, 210, radius)[0]
    assert int((f == 0).all(-1).sum()) == count
    assert (f[10, 10] == 0).all()


def test_render_composes_palette_and_markers():
    tile_map = np.array([[0, 1], [1, 0]])
    frames = ho.render(tile_map, np.array([[1.0, 0.0]]), np.array([1]), np.array([[0.0]]), np.array([[0.0]]), 4, 4, 0)
    assert frames.shape == (1, 2, 2, 3)
    assert frames[0, 0, 0].tolist() == [0, 0, 0]
    assert frames[0, 0, 1].tolist() == [204, 204, 204] and frames[0, 1, 1].tolist() == [255, 0, 0]


# --------------------------------------------------------------------------- the reference's names
@pytest.mark.parametrize("name", REFERENCE_NAMES)
def test_reference_visualisation_names(name):
    import viewport_entropy_toolkit.utilities as u
    from viewport_entropy_toolkit.utilities import visualization_utils as vz
    assert name in u.__all__
    assert getattr(u, name) is getattr(vz, name)
    with pytest.raises(RuntimeError) as e:
        getattr(u, name)()
    msg = str(e.value)
    assert ("pyvista" in msg) if "tiling" in name else ("save_heatmaps" in msg)


def test_reference_test_module_passes_against_the_drop_in(tmp_path):
    ref = Path("/root/reference/tests/test_core.py")
    if not ref.exists():
        pytest.skip("the reference's tests are not on this machine")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(ROOT / "viewport-entropy-toolkit_amd"), str(ROOT)]))
    r = subprocess.run([sys.executable, "-m", "pytest", str(ref), "-q", "-p", "no:cacheprovider", "--rootdir", str(tmp_path)],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert "5 passed" in r.stdout, r.stdout + r.stderr


def test_heatmaps_before_compute_entropy(tmp_path):
    import viewport_entropy_toolkit as vt
    from viewport_entropy_toolkit.config import AnalyzerConfig
    from viewport_entropy_toolkit.data_types import ValidationError
    an = vt.SpatialEntropyAnalyzer(AnalyzerConfig(output_dir=tmp_path / "out"))
    with pytest.raises(ValidationError, match="No entropy results. Call compute_entropy first."):
        an.render_heatmaps()
    with pytest.raises(ValidationError, match="No entropy results. Call compute_entropy first."):
        an.save_heatmaps(tmp_path / "h.npy")
    assert not (tmp_path / "h.npy").exists()
