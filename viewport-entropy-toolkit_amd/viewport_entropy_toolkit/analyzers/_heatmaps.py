"""GPU-rendered per-frame tile-attention heatmaps (include/vet.h: vet_heatmap_*) of an analyzer's device-resident
result: the reference's tile-attention animation (create_animation / save_video, utilities/visualization_utils.py:99-247),
shared by SpatialEntropyAnalyzer and TransitionEntropyAnalyzer."""

from __future__ import annotations

import shutil
import subprocess
from pathlib import Path
from typing import Optional, Union

import numpy as np

from .. import _native
from ..data_types import ValidationError


class _HeatmapMixin:
    """``render_heatmaps`` / ``save_heatmaps`` over ``self._device_result``.  The analyzer supplies ``_frame_present()``
    (users present per result row, int32), ``_marker_samples`` ((mu, mv) [T, U] whose row r belongs to result row r, or
    None) and ``_heatmap_entry`` (the ``_native.Heatmap`` method that renders its result kind)."""

    _heatmap_entry = "render_result"

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._present = None          # users present per result row of the last compute_entropy
        self._marker_samples = None   # (mu, mv) [T, U] of that run, or None (samples given as Vectors: no markers)
        self._heatmaps = {}

    def _frame_present(self) -> np.ndarray:  # pragma: no cover - overridden
        raise NotImplementedError

    def _frame_range(self, frames, T: int):
        if frames is None:
            return 0, T
        if isinstance(frames, (range, slice)):
            start, stop, step = (frames.start, frames.stop, frames.step) if isinstance(frames, range) \
                else frames.indices(T)
            if step != 1 or not 0 <= start <= stop <= T:
                raise ValidationError(f"frames must be a contiguous range within [0, {T}) (got {frames})")
            return start, stop - start
        raise ValidationError("frames must be None, a range or a slice")

    def _heatmap(self, width: int, height: int, marker_radius: int) -> "_native.Heatmap":
        key = (self.config.tile_counts[0], width, height, self.config.video_width, self.config.video_height, marker_radius)
        if key not in self._heatmaps:
            tiles = np.array([[v.x, v.y, v.z] for v in self._fibonacci_vectors[self.config.tile_counts[0]]], dtype=np.float64)
            try:
                self._heatmaps[key] = _native.Heatmap(_native.Engine.default(), tiles, width, height, self.config.video_width,
                                                      self.config.video_height, marker_radius)
            except _native.NativeError as e:
                if e.code == _native.VET_ERR_INVALID:
                    raise ValidationError(str(e))
                raise
        return self._heatmaps[key]

    def _heatmap_job(self, frames, width, height, markers, marker_radius):
        if self._entropy_results is None:
            raise ValidationError("No entropy results. Call compute_entropy first.")
        vc = self.config.visualization_config
        width = int(vc.figure_size[0] * vc.dpi) if width is None else int(width)
        height = int(vc.figure_size[1] * vc.dpi) if height is None else int(height)
        if width <= 0 or height <= 0:
            raise ValidationError("Heatmap dimensions must be positive")
        row0, n = self._frame_range(frames, len(self._entropy_results))
        return row0, n, width, height, self._heatmap(width, height, int(marker_radius)), bool(markers)

    def _render_block(self, hm, row0: int, n: int, markers: bool, out=None) -> np.ndarray:
        mu = mv = None
        if markers and self._marker_samples is not None:
            mu, mv = (x[row0:row0 + n] for x in self._marker_samples)
        render = getattr(hm, self._heatmap_entry)
        return render(self._device_result, self._frame_present()[row0:row0 + n], mu, mv, row0, n, out=out)

    def render_heatmaps(self, frames: Union[None, range, slice] = None, width: Optional[int] = None,
                        height: Optional[int] = None, markers: bool = True, marker_radius: int = 2) -> np.ndarray:
        """Per-frame tile-attention heatmaps of the last ``compute_entropy``, rendered on the GPU: uint8
        ``[n, height, width, 3]`` RGB, equirectangular (column c covers longitude [-180 + 360c/W, -180 + 360(c+1)/W),
        row 0 is latitude +90), one per row of the result.  Every pixel takes the colour of its nearest tile of
        ``tile_counts[0]`` — the reference animation's ``tile_weights / users present`` (grey 204 -> red 255) — and each
        present user's viewport is a black square of side ``2 * marker_radius + 1`` (``markers=False``: none).  For a
        transition result, row r (frames r -> r+1) uses the users counted per source tile over the users present in
        frame r, and frame r's viewports.  The default size is ``visualization_config.figure_size x dpi``
        (1200 x 600).  ``frames``: a contiguous range or slice of result rows (default all).  Samples given as a
        hand-assigned ``_data_cache['vectors']`` render without markers (they carry no pixel position).  The tile
        weights never leave the device."""
        row0, n, width, height, hm, markers = self._heatmap_job(frames, width, height, markers, marker_radius)
        return self._render_block(hm, row0, n, markers)

    def save_heatmaps(self, path: Union[str, Path], frames: Union[None, range, slice] = None, width: Optional[int] = None,
                      height: Optional[int] = None, markers: bool = True, marker_radius: int = 2,
                      block_frames: int = 256) -> Path:
        """``render_heatmaps`` streamed to ``path`` in blocks of ``block_frames`` frames:
        ``*.npy`` -> one uint8 [n, H, W, 3] array (``np.lib.format.open_memmap``); an existing directory ->
        ``frame_{t:06d}.png`` per frame t (PIL); ``*.mp4`` -> raw rgb24 piped to ``ffmpeg`` at ``visualization_config.fps``
        (``RuntimeError`` before any rendering when ffmpeg is not on PATH; width and height must be even)."""
        row0, n, width, height, hm, markers = self._heatmap_job(frames, width, height, markers, marker_radius)
        path = Path(path)
        if block_frames <= 0:
            raise ValidationError("block_frames must be positive")
        if path.suffix.lower() == ".npy":
            kind = "npy"
        elif path.suffix.lower() == ".mp4":
            kind = "mp4"
            if width % 2 or height % 2:
                raise ValidationError(f"an .mp4 needs even frame dimensions (got {width} x {height})")
            ffmpeg = shutil.which("ffmpeg")
            if ffmpeg is None:
                raise RuntimeError("Error saving video: ffmpeg was not found on PATH")
        elif path.is_dir():
            kind = "png"
        else:
            raise ValidationError(f"{path}: expected a .npy or .mp4 file, or an existing directory for PNG frames")
        blocks = [(b0, min(block_frames, row0 + n - b0)) for b0 in range(row0, row0 + n, block_frames)]
        if kind == "npy":
            arr = np.lib.format.open_memmap(path, mode="w+", dtype=np.uint8, shape=(n, height, width, 3))
            for b0, bn in blocks:
                self._render_block(hm, b0, bn, markers, out=arr[b0 - row0:b0 - row0 + bn])
            arr.flush()
            del arr
        elif kind == "png":
            from PIL import Image
            for b0, bn in blocks:
                rgb = self._render_block(hm, b0, bn, markers)
                for j in range(bn):
                    Image.fromarray(rgb[j], mode="RGB").save(path / f"frame_{b0 + j:06d}.png")
        else:
            cmd = [ffmpeg, "-y", "-loglevel", "error", "-f", "rawvideo", "-pix_fmt", "rgb24", "-s", f"{width}x{height}",
                   "-r", str(self.config.visualization_config.fps), "-i", "-", "-pix_fmt", "yuv420p", str(path)]
            proc = subprocess.Popen(cmd, stdin=subprocess.PIPE, stderr=subprocess.PIPE)
            try:
                for b0, bn in blocks:
                    proc.stdin.write(self._render_block(hm, b0, bn, markers).tobytes())
            except BrokenPipeError:
                pass                                   # ffmpeg ended early: its exit status says why
            except BaseException:
                proc.kill()
                proc.communicate()
                raise
            err = proc.communicate()[1]
            if proc.returncode != 0:
                raise RuntimeError(f"Error saving video: ffmpeg exited with {proc.returncode}: {err.decode(errors='replace')}")
        return path
