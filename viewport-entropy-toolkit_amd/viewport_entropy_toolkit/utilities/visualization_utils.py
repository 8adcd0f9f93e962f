"""Visualisation configuration and the entropy-over-time graph.

The configuration dataclass that ``AnalyzerConfig`` embeds (reference visualization_utils.py:32-60)
and the plain matplotlib line graph are provided here.  The per-frame tile-attention animation is
rendered on the GPU by ``SpatialEntropyAnalyzer.render_heatmaps`` / ``save_heatmaps``; the
reference's matplotlib names for it (``PlotManager``, ``create_animation``, ``save_video``) and its
pyvista sphere renderers exist so that code importing them loads, and raise ``RuntimeError`` when
called.  The scenes of those sphere renderers (a tiling's boundary arcs and centres on a translucent
unit sphere, one camera or a 180-frame orbit) are drawn on the GPU under new names:
``render_tiling``, ``tiling_orbit_cameras`` and ``write_tiling_image`` / ``write_tiling_video`` /
``write_fb_tiling_image`` / ``write_fb_tiling_video`` (frame definition: include/vet.h).
"""

from __future__ import annotations

import os
import shutil
import subprocess
from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Sequence, Tuple

import numpy as np

from .. import _native, _quantiser
from ..data_types import ValidationError


@dataclass
class VisualizationConfig:
    """Plot / video parameters (all must be positive)."""

    figure_size: Tuple[int, int] = (12, 6)
    fov_point_size: int = 10
    tile_point_size: int = 40
    fps: int = 10
    dpi: int = 100

    def __post_init__(self) -> None:
        if any(x <= 0 for x in self.figure_size):
            raise ValidationError("Figure dimensions must be positive")
        for value, label in ((self.fov_point_size, "FOV point size"), (self.tile_point_size, "Tile point size"),
                             (self.fps, "FPS"), (self.dpi, "DPI")):
            if value <= 0:
                raise ValidationError(f"{label} must be positive")


def save_graph(entropy_values: Sequence[float], time_values: Sequence[float], output_path: Path,
               config: Optional[VisualizationConfig] = None) -> None:
    """Entropy-over-time line graph as a png (host matplotlib, Agg backend)."""
    if len(entropy_values) != len(time_values):
        raise ValueError("Entropy values length must match time values length!")
    import matplotlib
    matplotlib.use("Agg", force=False)
    import matplotlib.pyplot as plt

    fig = plt.figure(figsize=(10, 6))
    plt.plot(list(time_values), list(entropy_values), marker="o", linestyle="-")
    plt.xlabel("Time")
    plt.ylabel("Entropy")
    plt.title("Entropy over Time")
    plt.grid(True)
    plt.savefig(output_path)
    plt.close(fig)


_USE_HEATMAPS = ("{name}: the matplotlib scatter animation is not part of this engine; render the per-frame tile-attention "
                 "frames on the GPU with SpatialEntropyAnalyzer.render_heatmaps / save_heatmaps (.npy, a PNG directory or .mp4)")
_NO_PYVISTA = ("{name}: 3-D tiling renders need pyvista and are not part of this engine. render_tiling and "
               "write_tiling_image / write_tiling_video / write_fb_tiling_image / write_fb_tiling_video draw the same scenes "
               "on the GPU")


class PlotManager:
    """Reference name (matplotlib scatter animation, visualization_utils.py:63-204); raises ``RuntimeError``."""

    def __init__(self, *args, **kwargs):
        raise RuntimeError(_USE_HEATMAPS.format(name="PlotManager"))


def _unavailable(name: str, message: str):
    def stub(*args, **kwargs):
        raise RuntimeError(message.format(name=name))
    stub.__name__ = stub.__qualname__ = name
    stub.__doc__ = f"Reference name; raises ``RuntimeError``: {message.format(name=name)}."
    return stub


create_animation = _unavailable("create_animation", _USE_HEATMAPS)
save_video = _unavailable("save_video", _USE_HEATMAPS)
save_fb_tiling_visualization_image = _unavailable("save_fb_tiling_visualization_image", _NO_PYVISTA)
save_fb_tiling_visualization_video = _unavailable("save_fb_tiling_visualization_video", _NO_PYVISTA)
save_tiling_visualization_image = _unavailable("save_tiling_visualization_image", _NO_PYVISTA)
save_tiling_visualization_video = _unavailable("save_tiling_visualization_video", _NO_PYVISTA)


# ------------------------------------------------------------------ tilings on the sphere, on the GPU
_DEFAULT_CAMERA = ((0, 0, 5), (0, 1, 0), (0, 0, 0))
_VIDEO_FPS = 24                  # pyvista's open_movie default
_VIDEO_BLOCK = 32                # frames rendered per call while a video is encoded


def _xyz(v) -> np.ndarray:
    return np.array([v.x, v.y, v.z], dtype=np.float64) if hasattr(v, "x") else np.asarray(v, dtype=np.float64)


def _arcs_of(tile_boundaries) -> np.ndarray:
    """The reference's {key: [[V1, V2], ...]} dict (edges in dict order) or an [n_arcs, 2, 3] array -> [n_arcs, 2, 3]."""
    if isinstance(tile_boundaries, dict):
        arcs = np.array([[_xyz(a), _xyz(b)] for edges in tile_boundaries.values() for a, b in edges],
                        dtype=np.float64).reshape(-1, 2, 3)
    else:
        arcs = np.asarray(tile_boundaries, dtype=np.float64)
    if arcs.ndim != 3 or arcs.shape[1:] != (2, 3):
        raise ValidationError(f"tile_boundaries must be a dict of [[V1, V2], ...] edges or an [n, 2, 3] array "
                              f"(got shape {arcs.shape})")
    if len(arcs) == 0:
        raise ValidationError("No tile boundaries to draw")
    return arcs


def _frame_args(width, height, background):
    width, height = int(width), int(height)
    if not (0 < width <= 16384 and 0 < height <= 16384):
        raise ValidationError(f"Frame dimensions must be in [1, 16384] (got {width} x {height})")
    bg = tuple(int(c) for c in background)
    if len(bg) != 3 or any(not 0 <= c <= 255 for c in bg):
        raise ValidationError(f"background must be three values in [0, 255] (got {background})")
    return width, height, bg


def _tiling(arcs: np.ndarray, centres: Optional[np.ndarray], width: int, height: int) -> "_native.Tiling":
    try:
        return _native.Tiling(_native.Engine.default(), arcs, centres, width, height)
    except _native.NativeError as e:
        if e.code == _native.VET_ERR_INVALID:
            raise ValidationError(str(e))
        raise


def _render(tiling: "_native.Tiling", cameras: np.ndarray, bg) -> np.ndarray:
    try:
        return tiling.render(cameras, bg)
    except _native.NativeError as e:
        if e.code == _native.VET_ERR_INVALID:
            raise ValidationError(str(e))
        raise


def render_tiling(tile_boundaries, tile_centers=None, cameras=_DEFAULT_CAMERA, width: int = 1024, height: int = 768,
                  background=(255, 255, 255)) -> np.ndarray:
    """A tiling drawn on the unit sphere, rendered on the GPU: uint8 ``[n, height, width, 3]`` RGB, row 0 at the top.

    ``tile_boundaries``: the reference's ``{key: [[V1, V2], ...]}`` dict (``get_fb_tile_boundaries``,
    ``get_lat_lon_tiles``) or an ``[n_arcs, 2, 3]`` array; every edge is a great-circle arc drawn as 49 black chords
    (line width 2).  ``tile_centers``: ``None``, Vectors or an ``[m, 3]`` array, drawn as red squares of side 10.
    ``cameras``: one (position, view-up, focal point) triple or an ``[n, 3, 3]`` array (``tiling_orbit_cameras``), seen
    through a parallel projection.  The sphere is grey 128 at opacity 0.3 over ``background``.  No lighting,
    anti-aliasing or axes: a frame is a pure function of its inputs (definition: include/vet.h)."""
    width, height, bg = _frame_args(width, height, background)
    arcs = _arcs_of(tile_boundaries)
    centres = None
    if tile_centers is not None:
        centres = np.array([_xyz(c) for c in tile_centers], dtype=np.float64).reshape(-1, 3)
    cameras = np.asarray(cameras, dtype=np.float64)
    if cameras.shape == (3, 3):
        cameras = cameras[None]
    if cameras.ndim != 3 or cameras.shape[1:] != (3, 3) or len(cameras) == 0:
        raise ValidationError(f"cameras must be one (position, up, focal point) triple or an [n, 3, 3] array "
                              f"(got shape {cameras.shape})")
    tiling = _tiling(arcs, centres, width, height)
    try:
        return _render(tiling, cameras, bg)
    finally:
        tiling.close()


def _rotate(v: np.ndarray, axis: np.ndarray, degrees: float) -> np.ndarray:
    """Right-handed rotation of ``v`` about the unit ``axis`` (Rodrigues)."""
    a = np.radians(degrees)
    c, s = np.cos(a), np.sin(a)
    return v * c + np.cross(axis, v) * s + axis * (np.dot(axis, v) * (1.0 - c))


def _pan_steps(horizontal_pan: bool, vertical_pan: bool) -> Tuple[float, float, str]:
    """(azimuth, elevation) degrees per frame and the file-name suffix, as the reference's video loop."""
    if horizontal_pan and vertical_pan:
        return 0.5, 0.5, "-vertical_horizontal"
    if horizontal_pan:
        return 1.0, 0.0, "-horizontal"
    if vertical_pan:
        return 0.0, 1.0, "-vertical"
    raise ValidationError("Video must pan horizontally or vertically or both!")


def tiling_orbit_cameras(horizontal_pan: bool = True, vertical_pan: bool = True, camera_position=(0, 0, 5),
                         camera_up=(0, 1, 0), camera_focal_point=(0, 0, 0), n_frames: int = 180) -> np.ndarray:
    """The cameras of the reference's tiling videos: ``[n_frames, 3, 3]`` (position, view-up, focal point).

    Frame i (1-based) is the camera after i steps; each step rotates the position about the axis through the focal
    point along the current view-up by the azimuth step, then the position and the view-up about the current right
    vector by the elevation step, both right-handed: (0.5, 0.5) degrees when panning both ways, (1, 0) horizontally
    only, (0, 1) vertically only.  The view-up turns with the camera (VTK's Elevation keeps it fixed), so a vertical
    pan passes over the pole.  Pure host code."""
    h, e, _ = _pan_steps(horizontal_pan, vertical_pan)
    n_frames = int(n_frames)
    if n_frames <= 0:
        raise ValidationError("n_frames must be positive")
    P = np.asarray(camera_position, dtype=np.float64).reshape(3).copy()
    u = np.asarray(camera_up, dtype=np.float64).reshape(3).copy()
    F = np.asarray(camera_focal_point, dtype=np.float64).reshape(3).copy()

    def basis(P, u):
        v = F - P
        dist = np.sqrt(np.dot(v, v))
        if not dist > 0:
            raise ValidationError("The camera position must differ from the focal point")
        d = v / dist
        x = np.cross(d, u)
        n = np.sqrt(np.dot(x, x))
        if not n > 0:
            raise ValidationError("The camera's view-up must not be parallel to its view direction")
        r = x / n
        return d, r, np.cross(r, d)

    out = np.empty((n_frames, 3, 3), dtype=np.float64)
    for i in range(n_frames):
        _, r, u = basis(P, u)
        if h:
            P = F + _rotate(P - F, u, h)
        if e:
            _, r, u = basis(P, u)
            P = F + _rotate(P - F, r, e)
            u = _rotate(u, r, e)
        out[i] = (P, u, F)
    return out


def _camera_suffix(camera_position, camera_up) -> str:
    return (f"-camera_position_{camera_position[0]}_{camera_position[1]}_{camera_position[2]}"
            f"-camera_up_{camera_up[0]}_{camera_up[1]}_{camera_up[2]}")


def _fb_scene(tile_count: int):
    """Boundary arcs (Engine.fb_tile_boundaries, tile by tile in edge order) and centres of the Fibonacci tiling."""
    if tile_count <= 0:
        raise ValidationError("Tile counts cannot be less than 1 for to visualize tiling!")
    tiles = _quantiser.lattice_xyz(tile_count)
    edges, count = _native.Engine.default().fb_tile_boundaries(tiles)
    return edges[np.arange(edges.shape[1])[None, :] < count[:, None]], tiles


def _write_image(path: Path, arcs, centres, camera, width, height, background) -> Path:
    from PIL import Image
    width, height, bg = _frame_args(width, height, background)
    tiling = _tiling(arcs, centres, width, height)
    try:
        frame = _render(tiling, np.asarray(camera, dtype=np.float64)[None], bg)[0]
    finally:
        tiling.close()
    Image.fromarray(frame).save(path)
    return path


def _write_video(path: Path, scene, horizontal_pan, vertical_pan, width, height, background) -> Path:
    """Orbit frames of ``scene()`` = (arcs, centres) piped to ffmpeg as raw rgb24.  Every check (pans, even width and
    height, ffmpeg on PATH) comes before the scene is built or anything is rendered."""
    _pan_steps(horizontal_pan, vertical_pan)
    width, height, bg = _frame_args(width, height, background)
    if width % 2 or height % 2:
        raise ValidationError(f"an .mp4 needs even frame dimensions (got {width} x {height})")
    ffmpeg = shutil.which("ffmpeg")
    if ffmpeg is None:
        raise RuntimeError("Error saving video: ffmpeg was not found on PATH")
    arcs, centres = scene()
    cameras = tiling_orbit_cameras(horizontal_pan, vertical_pan)
    tiling = _tiling(arcs, centres, width, height)
    cmd = [ffmpeg, "-y", "-loglevel", "error", "-f", "rawvideo", "-pix_fmt", "rgb24", "-s", f"{width}x{height}",
           "-r", str(_VIDEO_FPS), "-i", "-", "-pix_fmt", "yuv420p", str(path)]
    proc = subprocess.Popen(cmd, stdin=subprocess.PIPE, stderr=subprocess.PIPE)
    try:
        for b0 in range(0, len(cameras), _VIDEO_BLOCK):
            proc.stdin.write(_render(tiling, cameras[b0:b0 + _VIDEO_BLOCK], bg).tobytes())
    except BrokenPipeError:
        pass                                           # ffmpeg ended early: its exit status says why
    except BaseException:
        proc.kill()
        proc.communicate()
        path.unlink(missing_ok=True)
        raise
    finally:
        tiling.close()
    err = proc.communicate()[1]
    if proc.returncode != 0:
        raise RuntimeError(f"Error saving video: ffmpeg exited with {proc.returncode}: {err.decode(errors='replace')}")
    return path


def write_tiling_image(tile_boundaries, output_dir: Path, output_prefix: str = "", camera_position=(0, 0, 5),
                       camera_up=(0, 1, 0), camera_focal_point=(0, 0, 0), *, width: int = 1024, height: int = 768,
                       background=(255, 255, 255)) -> Path:
    """``save_tiling_visualization_image``'s scene (the arcs, no centres) rendered on the GPU to
    ``{output_prefix}tiling_visualization-camera_position_..-camera_up_...png`` in ``output_dir``; returns the path."""
    arcs = _arcs_of(tile_boundaries)
    path = Path(os.path.join(str(output_dir), f"{output_prefix}tiling_visualization"
                                              f"{_camera_suffix(camera_position, camera_up)}.png"))
    return _write_image(path, arcs, None, (camera_position, camera_up, camera_focal_point), width, height, background)


def write_tiling_video(tile_boundaries, output_dir: Path, output_prefix: str = "", horizontal_pan: bool = True,
                       vertical_pan: bool = True, *, width: int = 1024, height: int = 768,
                       background=(255, 255, 255)) -> Path:
    """``save_tiling_visualization_video``'s 180-frame orbit (``tiling_orbit_cameras`` from (0, 0, 5), view-up (0, 1, 0))
    rendered on the GPU and encoded by ffmpeg to ``{output_prefix}tiling_visualization{-vertical_horizontal |
    -horizontal | -vertical}.mp4`` in ``output_dir``; returns the path.  ``RuntimeError`` before any rendering when ffmpeg
    is not on PATH."""
    _, _, suffix = _pan_steps(horizontal_pan, vertical_pan)
    path = Path(os.path.join(str(output_dir), f"{output_prefix}tiling_visualization{suffix}.mp4"))
    return _write_video(path, lambda: (_arcs_of(tile_boundaries), None), horizontal_pan, vertical_pan, width, height,
                        background)


def write_fb_tiling_image(tile_count: int, output_dir: Path, camera_position=(0, 0, 5), camera_up=(0, 1, 0),
                          camera_focal_point=(0, 0, 0), *, width: int = 1024, height: int = 768,
                          background=(255, 255, 255)) -> Path:
    """``save_fb_tiling_visualization_image``'s scene (the Fibonacci tiling's boundary arcs and red tile centres)
    rendered on the GPU to ``fibonacci_lattice-{tile_count}_tiles-camera_position_..-camera_up_...png`` in
    ``output_dir``; returns the path."""
    arcs, centres = _fb_scene(tile_count)
    path = Path(os.path.join(str(output_dir), f"fibonacci_lattice-{tile_count}_tiles"
                                              f"{_camera_suffix(camera_position, camera_up)}.png"))
    return _write_image(path, arcs, centres, (camera_position, camera_up, camera_focal_point), width, height, background)


def write_fb_tiling_video(tile_count: int, output_dir: Path, horizontal_pan: bool = True, vertical_pan: bool = True, *,
                          width: int = 1024, height: int = 768, background=(255, 255, 255)) -> Path:
    """``save_fb_tiling_visualization_video``'s 180-frame orbit of the Fibonacci tiling rendered on the GPU and encoded by
    ffmpeg to ``fibonacci_lattice-{tile_count}_tiles{-vertical_horizontal | -horizontal | -vertical}.mp4`` in
    ``output_dir``; returns the path.  ``RuntimeError`` before any rendering when ffmpeg is not on PATH."""
    _, _, suffix = _pan_steps(horizontal_pan, vertical_pan)
    if tile_count <= 0:
        raise ValidationError("Tile counts cannot be less than 1 for to visualize tiling!")
    path = Path(os.path.join(str(output_dir), f"fibonacci_lattice-{tile_count}_tiles{suffix}.mp4"))
    return _write_video(path, lambda: _fb_scene(tile_count), horizontal_pan, vertical_pan, width, height, background)
