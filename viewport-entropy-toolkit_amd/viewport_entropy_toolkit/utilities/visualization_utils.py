"""Visualisation configuration and the entropy-over-time graph.

The configuration dataclass that ``AnalyzerConfig`` embeds (reference visualization_utils.py:32-60)
and the plain matplotlib line graph are provided here.  The per-frame tile-attention animation is
rendered on the GPU by ``SpatialEntropyAnalyzer.render_heatmaps`` / ``save_heatmaps``; the
reference's matplotlib names for it (``PlotManager``, ``create_animation``, ``save_video``) and its
pyvista sphere renderers exist so that code importing them loads, and raise ``RuntimeError`` when
called.
"""

from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Sequence, Tuple

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
_NO_PYVISTA = "{name}: 3-D tiling renders need pyvista and are not part of this engine"


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
