"""Tilings drawn on the unit sphere, the parts that run without a GPU: the C-ABI surface and its argument checks, the
oracle's frame definition on hand-computed scenes, the orbit cameras and the writers' names and checks."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import _tiling_oracle as to
from tests.test_cabi_symbols import header_functions

TILING_ENTRIES = ["vet_tiling_create", "vet_tiling_destroy", "vet_tiling_render", "vet_tiling_render_host"]
CAM = ((0, 0, 5), (0, 1, 0), (0, 0, 0))


# --------------------------------------------------------------------------- C-ABI
def test_header_library_and_signatures():
    from viewport_entropy_toolkit import _native
    fns = header_functions()
    assert set(TILING_ENTRIES) <= set(fns)
    lib = ctypes.CDLL(str(_native.LIB_PATH))
    for name in TILING_ENTRIES:
        assert hasattr(lib, name), name
    assert set(TILING_ENTRIES) <= set(_native.SIGNATURES)
    assert sorted(_native.SIGNATURES) == fns
    assert _native.load_library().vet_version() == 141


def test_null_and_size_errors_without_a_device():
    """Argument checks come before any device call."""
    from viewport_entropy_toolkit import _native
    lib = _native.load_library()
    INVALID = _native.VET_ERR_INVALID
    out = ctypes.c_void_p()
    arcs = np.zeros((1, 2, 3))
    p = arcs.ctypes.data_as(ctypes.c_void_p)
    fake_ctx = ctypes.c_void_p(8)                  # never dereferenced: every case below fails its checks first
    assert lib.vet_tiling_create(None, None, 0, None, 0, 0, 0, ctypes.byref(out)) == INVALID
    assert lib.vet_tiling_create(fake_ctx, p, 0, None, 0, 64, 48, ctypes.byref(out)) == INVALID
    assert lib.vet_tiling_create(fake_ctx, p, -1, None, 0, 64, 48, ctypes.byref(out)) == INVALID
    assert lib.vet_tiling_create(fake_ctx, p, 1, None, 0, 0, 48, ctypes.byref(out)) == INVALID
    assert lib.vet_tiling_create(fake_ctx, p, 1, None, 0, 64, -2, ctypes.byref(out)) == INVALID
    assert lib.vet_tiling_create(fake_ctx, p, 1, None, 0, 16385, 48, ctypes.byref(out)) == INVALID
    assert lib.vet_tiling_create(fake_ctx, p, 1, None, 0, 64, 16385, ctypes.byref(out)) == INVALID
    assert lib.vet_tiling_create(fake_ctx, p, 1, None, 3, 64, 48, ctypes.byref(out)) == INVALID     # centres NULL
    assert lib.vet_tiling_create(fake_ctx, p, 1, None, -1, 64, 48, ctypes.byref(out)) == INVALID
    assert lib.vet_tiling_create(fake_ctx, p, (1 << 22) + 1, None, 0, 64, 48, ctypes.byref(out)) == INVALID
    assert lib.vet_tiling_create(fake_ctx, p, 1, None, 0, 64, 48, None) == INVALID
    assert out.value is None
    assert lib.vet_tiling_render(None, None, 0, None, None, None) == INVALID
    assert lib.vet_tiling_render_host(None, None, 0, None, None) == INVALID
    assert lib.vet_tiling_destroy(None) == _native.VET_OK


# --------------------------------------------------------------------------- the oracle's frame
def test_linspace_and_sin15():
    t = np.linspace(0, 1, 50)
    assert t[-1] == 1.0 and all(t[i] == i * (1.0 / 49) for i in range(49))
    assert to.SIN15 == np.sin(np.radians(15))


def test_pixel_size_and_origin():
    c = to.camera(CAM, 1024, 768)
    assert c["s"] == 2.0 * 5.0 * to.SIN15 / 768
    assert (c["X0"], c["Y0"]) == (512.0, 384.0)
    assert c["r"] == (1.0, 0.0, 0.0) and c["u"] == (0.0, 1.0, 0.0) and c["nd"] == (-0.0, -0.0, 1.0)
    with pytest.raises(ValueError):
        to.camera(((1, 2, 3), (0, 1, 0), (1, 2, 3)), 64, 48)
    with pytest.raises(ValueError):
        to.camera(((0, 0, 5), (0, 0, 2), (0, 0, 0)), 64, 48)


def test_arc_is_a_horizontal_band():
    """(1,0,0) -> (0,0,1) seen from (0,0,5): black on rows H/2-1 and H/2 from the centre to x = 1, and nowhere else."""
    W, H = 1024, 768
    img, amb, f = to.render_frame(to.chord_points([[[1, 0, 0], [0, 0, 1]]]), None, CAM, W, H)
    black = (img == 0).all(-1)
    rows = np.nonzero(black.any(1))[0]
    assert rows.tolist() == [H // 2 - 1, H // 2]
    end = W / 2 + 1 / to.camera(CAM, W, H)["s"]               # x = 1 projects here
    cols = np.nonzero(black[H // 2])[0]
    assert cols.min() == W // 2 - 1 and abs(cols.max() - end) <= 1.5
    inner = slice(W // 2 + 5, int(end) - 5)                   # away from the ends: front, a solid two-row band
    assert black[H // 2 - 1, inner].all() and black[H // 2, inner].all()
    assert f["front_line"][H // 2, inner].all()
    assert not black[H // 2 - 2].any() and not black[H // 2 + 1].any()
    assert not amb[H // 2 - 1:H // 2 + 1, inner].any()


def test_back_centre_is_red_through_the_blend():
    W, H = 200, 150
    img, _, f = to.render_frame(to.chord_points([[[1, 0, 0], [0, 1, 0]]]), np.array([[0.0, 0.0, -1.0]]), CAM, W, H)
    blended_red = [int(math.floor(0.3 * 128.0 + 0.7 * v + 0.5)) for v in (255, 0, 0)]
    assert blended_red == [217, 38, 38]
    assert f["back_point"][H // 2, W // 2] and not f["front_point"].any()
    assert img[H // 2, W // 2].tolist() == blended_red
    # the square: |X(c) - X_q| < 5 with X(c) = W / 2: columns W/2 - 5 .. W/2 + 4 (10 pixels)
    cols = np.nonzero(f["back_point"][H // 2])[0]
    assert cols.tolist() == list(range(W // 2 - 5, W // 2 + 5))
    front = to.render_frame(to.chord_points([[[1, 0, 0], [0, 1, 0]]]), np.array([[0.0, 0.0, 1.0]]), CAM, W, H)[0]
    assert front[H // 2, W // 2].tolist() == [255, 0, 0]     # a front centre is red, unblended


def test_disc_edge_and_background():
    W, H = 1024, 768
    bg = (10, 200, 30)
    img, _, f = to.render_frame(to.chord_points([[[1, 0, 0], [1, 0, 0]]]), None, CAM, W, H, bg)   # coincident: nothing
    assert not f["front_line"].any() and not f["back_line"].any()
    radius = 1 / to.camera(CAM, W, H)["s"]                    # 296.73 pixels
    row = img[H // 2]
    inside = [int(math.floor(0.3 * 128.0 + 0.7 * v + 0.5)) for v in bg]
    edge = W // 2 + int(math.floor(radius - 0.5))              # last column whose centre is inside
    assert row[edge].tolist() == inside and row[edge + 1].tolist() == list(bg)
    assert img[0, 0].tolist() == list(bg)
    assert f["disc"].sum() == pytest.approx(math.pi * radius ** 2, rel=1e-2)


def test_antipodal_and_non_finite_arcs_draw_nothing():
    pts = to.chord_points([[[1, 0, 0], [-1, 0, 0]], [[0, 0, 2], [0, 0, 2]], [[np.nan, 0, 1], [0, 1, 0]]])
    assert np.isnan(pts).all()
    img, _, f = to.render_frame(pts, None, CAM, 64, 48)
    assert not (f["front_line"] | f["back_line"]).any()


# --------------------------------------------------------------------------- orbit cameras
def _basis(cam):
    P, U, F = cam
    d = (F - P) / np.linalg.norm(F - P)
    r = np.cross(d, U)
    r /= np.linalg.norm(r)
    return r, np.cross(r, d), d


def test_orbit_horizontal_ends_behind_the_sphere():
    from viewport_entropy_toolkit.utilities import tiling_orbit_cameras
    cams = tiling_orbit_cameras(True, False)
    assert cams.shape == (180, 3, 3)
    np.testing.assert_allclose(cams[-1, 0], [0, 0, -5], atol=1e-12)
    np.testing.assert_allclose(cams[-1, 1], [0, 1, 0], atol=1e-12)
    np.testing.assert_allclose(cams[89, 0], [5, 0, 0], atol=1e-12)       # right-handed about +y: via +x
    assert not np.allclose(cams[0, 0], [0, 0, 5])                          # the first frame has already moved


def test_orbit_vertical_passes_over_the_pole():
    from viewport_entropy_toolkit.utilities import tiling_orbit_cameras
    cams = tiling_orbit_cameras(False, True)
    np.testing.assert_allclose(cams[-1, 0], [0, 0, -5], atol=1e-12)
    np.testing.assert_allclose(cams[-1, 1], [0, -1, 0], atol=1e-12)
    np.testing.assert_allclose(cams[89, 0], [0, -5, 0], atol=1e-12)


@pytest.mark.parametrize("pans", [(True, True), (True, False), (False, True)])
def test_orbit_keeps_distance_and_an_orthonormal_basis(pans):
    from viewport_entropy_toolkit.utilities import tiling_orbit_cameras
    cams = tiling_orbit_cameras(*pans, camera_position=(1, 2, 6), camera_up=(0.2, 1, 0), camera_focal_point=(1, 2, 1))
    for cam in cams:
        assert np.linalg.norm(cam[0] - cam[2]) == pytest.approx(5, abs=1e-12)
        np.testing.assert_array_equal(cam[2], [1, 2, 1])
        B = np.stack(_basis(cam))
        np.testing.assert_allclose(B @ B.T, np.eye(3), atol=1e-12)
        to.camera(cam, 64, 48)                                             # a valid camera


def test_no_pan_is_a_validation_error(tmp_path):
    from viewport_entropy_toolkit.data_types import ValidationError
    from viewport_entropy_toolkit.utilities import (tiling_orbit_cameras, write_fb_tiling_video,
                                                    write_tiling_video)
    msg = "Video must pan horizontally or vertically or both!"
    with pytest.raises(ValidationError, match=msg):
        tiling_orbit_cameras(False, False)
    with pytest.raises(ValidationError, match=msg):
        write_tiling_video({"a": [[(1, 0, 0), (0, 1, 0)]]}, tmp_path, "", False, False)
    with pytest.raises(ValidationError, match=msg):
        write_fb_tiling_video(20, tmp_path, False, False)
    assert not os.listdir(tmp_path)


# --------------------------------------------------------------------------- writers
def test_file_names_follow_the_reference(monkeypatch, tmp_path):
    from viewport_entropy_toolkit.utilities import visualization_utils as vz
    written = []
    monkeypatch.setattr(vz, "_write_image", lambda path, *a: written.append(path.name) or path)
    monkeypatch.setattr(vz, "_fb_scene", lambda n: (np.zeros((1, 2, 3)), None))
    arcs = np.array([[[1, 0, 0], [0, 1, 0]]], dtype=float)
    p = vz.write_tiling_image(arcs, tmp_path)
    assert p == tmp_path / "tiling_visualization-camera_position_0_0_5-camera_up_0_1_0.png"
    vz.write_tiling_image(arcs, tmp_path, "run1_", (1.5, -2.0, 3), (0, 0, 1.0))
    vz.write_fb_tiling_image(500, tmp_path)
    vz.write_fb_tiling_image(20, tmp_path, (0.5, 0, 5), (0, 1, 0))
    assert written[1:] == ["run1_tiling_visualization-camera_position_1.5_-2.0_3-camera_up_0_0_1.0.png",
                           "fibonacci_lattice-500_tiles-camera_position_0_0_5-camera_up_0_1_0.png",
                           "fibonacci_lattice-20_tiles-camera_position_0.5_0_5-camera_up_0_1_0.png"]


def test_video_needs_ffmpeg_and_even_dimensions(monkeypatch, tmp_path):
    from viewport_entropy_toolkit.data_types import ValidationError
    from viewport_entropy_toolkit.utilities import visualization_utils as vz
    monkeypatch.setattr(vz.shutil, "which", lambda name: None)
    monkeypatch.setattr(vz, "_fb_scene", lambda n: pytest.fail("the scene is built before the checks"))
    with pytest.raises(RuntimeError, match="ffmpeg"):
        vz.write_fb_tiling_video(20, tmp_path)
    with pytest.raises(RuntimeError, match="ffmpeg"):
        vz.write_tiling_video({"a": [[(1, 0, 0), (0, 1, 0)]]}, tmp_path, "x_", True, False)
    with pytest.raises(ValidationError, match="even"):
        vz.write_fb_tiling_video(20, tmp_path, width=641)
    assert not os.listdir(tmp_path)


def test_tile_count_must_be_positive(tmp_path):
    from viewport_entropy_toolkit.data_types import ValidationError
    from viewport_entropy_toolkit.utilities import write_fb_tiling_image, write_fb_tiling_video
    msg = "Tile counts cannot be less than 1 for to visualize tiling!"
    for n in (0, -3):
        with pytest.raises(ValidationError, match=msg):
            write_fb_tiling_image(n, tmp_path)
        with pytest.raises(ValidationError, match=msg):
            write_fb_tiling_video(n, tmp_path)
    assert not os.listdir(tmp_path)


def test_render_tiling_checks_its_inputs():
    from viewport_entropy_toolkit.data_types import ValidationError
    from viewport_entropy_toolkit.utilities import render_tiling
    arcs = np.array([[[1, 0, 0], [0, 1, 0]]], dtype=float)
    with pytest.raises(ValidationError):
        render_tiling({})
    with pytest.raises(ValidationError):
        render_tiling(np.zeros((3, 3)))
    with pytest.raises(ValidationError):
        render_tiling(arcs, width=0)
    with pytest.raises(ValidationError):
        render_tiling(arcs, height=20000)
    with pytest.raises(ValidationError):
        render_tiling(arcs, background=(0, 0, 256))
    with pytest.raises(ValidationError):
        render_tiling(arcs, cameras=np.zeros((2, 3)))


def test_public_names():
    import viewport_entropy_toolkit.utilities as u
    for name in ("render_tiling", "tiling_orbit_cameras", "write_tiling_image", "write_tiling_video",
                 "write_fb_tiling_image", "write_fb_tiling_video"):
        assert name in u.__all__ and callable(getattr(u, name))
    with pytest.raises(RuntimeError, match="pyvista") as e:
        u.save_fb_tiling_visualization_image()
    assert "write_fb_tiling_image" in str(e.value)
