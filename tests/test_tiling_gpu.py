"""Tilings drawn on the unit sphere on the MI355X: device frames against the numpy oracle (tests/_tiling_oracle.py) bit for
bit outside its ambiguous mask, orbits, determinism, frame blocks, the device-pointer entry and the writers."""
import shutil

import numpy as np
import pytest

from tests import _tiling_oracle as to

pytestmark = pytest.mark.gpu

CAM = ((0, 0, 5), (0, 1, 0), (0, 0, 0))


def _fb(n):
    from viewport_entropy_toolkit.utilities.visualization_utils import _fb_scene
    return _fb_scene(n)


def _latlon(h, v):
    from viewport_entropy_toolkit.utilities import get_lat_lon_tiles
    from viewport_entropy_toolkit.utilities.visualization_utils import _arcs_of
    return _arcs_of(get_lat_lon_tiles(h, v))


def _check(dev, arcs, centres, cameras, W, H, background=(255, 255, 255)):
    ref, amb = to.render(arcs, centres, cameras, W, H, background)
    assert dev.shape == ref.shape and dev.dtype == np.uint8
    assert amb.mean() < 1e-3, f"ambiguous share {amb.mean():.2e}"
    bad = (dev != ref).any(-1) & ~amb
    assert not bad.any(), f"{int(bad.sum())} pixels differ, first at {np.argwhere(bad)[0].tolist()}"
    return ref


def _render(arcs, centres, cameras, W, H, background=(255, 255, 255)):
    from viewport_entropy_toolkit.utilities import render_tiling
    return render_tiling(arcs, centres, cameras, W, H, background)


@pytest.mark.parametrize("n,W,H", [(20, 320, 240), (50, 320, 240), (250, 640, 480), (1001, 1024, 768)])
def test_fb_tilings_match_the_oracle(n, W, H):
    arcs, centres = _fb(n)
    cams = np.array([CAM, ((3, 2, 4), (0, 0, 1), (0, 0, 0))], dtype=float)
    ref = _check(_render(arcs, centres, cams, W, H), arcs, centres, cams, W, H)
    assert (ref == [255, 0, 0]).all(-1).any() and (ref == 0).all(-1).any()      # centres and lines are drawn


# Seen from (0, 0, 5) a lat/lon tiling's equator is the sphere's silhouette: every point of it has depth ~6e-17, within the
# oracle's depth band.  The lat/lon scenes use cameras off the axes, so that no edge lies on the silhouette.
OBLIQUE = np.array([((3, 2, 4), (0, 0, 1), (0, 0, 0)), ((-2, 1, 3), (0, 0, 1), (0, 0, 0))], dtype=float)


def test_lat_lon_tilings_match_the_oracle():
    W, H = 256, 192
    arcs = _latlon(8, 4)
    _check(_render(arcs, None, OBLIQUE, W, H), arcs, None, OBLIQUE, W, H)


def test_lat_lon_2x2_antipodal_edges_draw_nothing():
    W, H = 256, 192
    arcs = _latlon(2, 2)
    a, b = arcs[:, 0], arcs[:, 1]
    antipodal = (a * b).sum(1) / np.linalg.norm(a, axis=1) / np.linalg.norm(b, axis=1) == -1.0
    assert antipodal.sum() == 4
    dev = _render(arcs, None, OBLIQUE, W, H)
    _check(dev, arcs, None, OBLIQUE, W, H)
    np.testing.assert_array_equal(dev, _render(arcs[~antipodal], None, OBLIQUE, W, H))


def test_off_origin_focal_point_and_oblique_view_up():
    W, H = 320, 240
    arcs, centres = _fb(50)
    cams = np.array([((2, 1, 4), (0, 1, 0), (0.3, -0.2, 0.1)),       # off-origin focal point
                     ((0, 0, 5), (0.3, 1, 0.5), (0, 0, 0)),          # view-up not orthogonal to the view
                     ((0, 0, 1.5), (0, 1, 0), (0, 0, 0))], dtype=float)   # close: long chords, sphere beyond the frame
    _check(_render(arcs, centres, cams, W, H, (20, 40, 60)), arcs, centres, cams, W, H, (20, 40, 60))


def test_odd_frame_sizes_and_a_ragged_tail():
    W, H = 321, 241                                # W * H * n % 4 == 3: the byte-wise tail, and HW % 4 != 0
    arcs, centres = _fb(50)
    from viewport_entropy_toolkit.utilities import tiling_orbit_cameras
    cams = tiling_orbit_cameras(True, True, n_frames=30)[[4, 17, 29]]
    assert (W * H * len(cams)) % 4 == 3
    _check(_render(arcs, centres, cams, W, H), arcs, centres, cams, W, H)


@pytest.mark.parametrize("pans", [(True, True), (True, False), (False, True)])
def test_orbit_frames_match_the_oracle(pans):
    from viewport_entropy_toolkit.utilities import tiling_orbit_cameras
    W, H = 256, 192
    arcs, centres = _fb(50)
    cams = tiling_orbit_cameras(*pans)[[0, 44, 89, 134, 179]]
    _check(_render(arcs, centres, cams, W, H), arcs, centres, cams, W, H)


def test_renders_are_byte_identical():
    arcs, centres = _fb(250)
    from viewport_entropy_toolkit.utilities import tiling_orbit_cameras
    cams = tiling_orbit_cameras()[:8]
    a = _render(arcs, centres, cams, 640, 480)
    b = _render(arcs, centres, cams, 640, 480)
    assert np.array_equal(a, b)


def test_one_call_equals_blocks_and_the_device_entry():
    """150 frames at 48 x 36 cross the internal block of 64 frames; calls over other splits and the asynchronous
    device-pointer entry give the same bytes."""
    import torch
    from viewport_entropy_toolkit import _native
    from viewport_entropy_toolkit.utilities import tiling_orbit_cameras
    W, H = 48, 36
    arcs, centres = _fb(20)
    cams = tiling_orbit_cameras(n_frames=150)
    tl = _native.Tiling(_native.Engine.default(), arcs, centres, W, H)
    try:
        whole = tl.render(cams, (1, 2, 3))
        parts = np.concatenate([tl.render(cams[a:b], (1, 2, 3)) for a, b in ((0, 60), (60, 129), (129, 150))])
        np.testing.assert_array_equal(whole, parts)
        d = torch.empty((150, H, W, 3), dtype=torch.uint8, device="cuda")
        stream = torch.cuda.Stream()
        tl.render_device(cams, d.data_ptr(), (1, 2, 3), stream=stream.cuda_stream)
        stream.synchronize()
        np.testing.assert_array_equal(d.cpu().numpy(), whole)
    finally:
        tl.close()
    _check(whole[[0, 63, 64, 127, 128, 149]], arcs, centres, cams[[0, 63, 64, 127, 128, 149]], W, H, (1, 2, 3))


def test_invalid_camera_is_a_validation_error():
    from viewport_entropy_toolkit.data_types import ValidationError
    arcs, _ = _fb(20)
    with pytest.raises(ValidationError):
        _render(arcs, None, ((1, 1, 1), (0, 1, 0), (1, 1, 1)), 64, 48)
    with pytest.raises(ValidationError):
        _render(arcs, None, ((0, 0, 5), (0, 0, 1), (0, 0, 0)), 64, 48)


def test_vector_dict_equals_edge_array():
    from viewport_entropy_toolkit.utilities import generate_fibonacci_lattice, get_fb_tile_boundaries
    arcs, centres = _fb(50)
    np.testing.assert_array_equal(_render(get_fb_tile_boundaries(50), centres, CAM, 320, 240),
                                  _render(arcs, centres, CAM, 320, 240))
    vectors = generate_fibonacci_lattice(50)
    np.testing.assert_array_equal(_render(arcs, vectors, CAM, 320, 240),
                                  _render(arcs, np.array([[v.x, v.y, v.z] for v in vectors]), CAM, 320, 240))


def test_image_writers_read_back(tmp_path):
    from PIL import Image
    from viewport_entropy_toolkit.utilities import (get_lat_lon_tiles, render_tiling, write_fb_tiling_image,
                                                    write_tiling_image)
    p = write_fb_tiling_image(500, tmp_path)
    assert p.name == "fibonacci_lattice-500_tiles-camera_position_0_0_5-camera_up_0_1_0.png" and p.exists()
    arcs, centres = _fb(500)
    np.testing.assert_array_equal(np.asarray(Image.open(p).convert("RGB")), render_tiling(arcs, centres)[0])
    tiles = get_lat_lon_tiles(12, 6)
    q = write_tiling_image(tiles, tmp_path, "ll_", (3, 3, 3), (0, 0, 1), width=300, height=200, background=(0, 0, 64))
    assert q.name == "ll_tiling_visualization-camera_position_3_3_3-camera_up_0_0_1.png"
    np.testing.assert_array_equal(np.asarray(Image.open(q).convert("RGB")),
                                  render_tiling(tiles, None, ((3, 3, 3), (0, 0, 1), (0, 0, 0)), 300, 200, (0, 0, 64))[0])


def test_video_writers(tmp_path):
    from viewport_entropy_toolkit.utilities import get_lat_lon_tiles, write_fb_tiling_video, write_tiling_video
    if shutil.which("ffmpeg") is None:
        with pytest.raises(RuntimeError, match="ffmpeg"):
            write_fb_tiling_video(50, tmp_path, width=128, height=96)
        with pytest.raises(RuntimeError, match="ffmpeg"):
            write_tiling_video(get_lat_lon_tiles(8, 4), tmp_path)
        assert not list(tmp_path.iterdir())
        return
    p = write_fb_tiling_video(50, tmp_path, True, False, width=128, height=96)
    assert p.name == "fibonacci_lattice-50_tiles-horizontal.mp4" and p.stat().st_size > 0
    q = write_tiling_video(get_lat_lon_tiles(8, 4), tmp_path, "ll_", width=128, height=96)
    assert q.name == "ll_tiling_visualization-vertical_horizontal.mp4" and q.stat().st_size > 0
