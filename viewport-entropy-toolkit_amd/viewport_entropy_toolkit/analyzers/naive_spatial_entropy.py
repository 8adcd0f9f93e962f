"""NaiveSpatialEntropyAnalyzer: per-frame entropy of the users over a latitude-longitude grid of
``tile_height`` x ``tile_width`` degree cells (reference analyzers/naive_spatial_entropy.py:102-152,
utilities/entropy_utils.py:383-452), on the HIP engine's integer histogram kernels.

The cell of a sample depends only on its pixel direction, so the host turns the two axis tables
(lon per px, lat per py) into a direction -> cell table once and the device path is the same
16-B-in / 4-B-out stream as the unweighted Fibonacci mode.  As in the reference the result frame
carries ``None`` in ``tile_weights`` / ``tile_assignments``.  ``render_heatmaps`` / ``save_heatmaps`` count the
cells of each frame again on the GPU, from the samples of the last ``compute_entropy``."""

from __future__ import annotations

import logging
import time
from typing import Optional

import numpy as np
import pandas as pd

from .. import _native, _quantiser
from ..config import NaiveAnalyzerConfig
from ..data_types import ValidationError
from ..utilities.entropy_utils import naive_tile_count
from ._base import _EntropyAnalyzerBase
from ._heatmaps import _HeatmapMixin

logger = logging.getLogger(__name__)


class NaiveSpatialEntropyAnalyzer(_HeatmapMixin, _EntropyAnalyzerBase):
    """Drop-in analyzer for the lat/lon-cut tiling; ``config`` is a ``NaiveAnalyzerConfig``.  The heatmap methods are the
    mixin's, over lat/lon cells: ``_heatmap`` and ``_render_block`` render the samples of the last ``compute_entropy``
    through its plan (include/vet.h: vet_heatmap_render_binned_host); no result stays on the device."""

    _logger = logger

    def __init__(self, config: Optional[NaiveAnalyzerConfig] = None):
        self.config = config or NaiveAnalyzerConfig()
        self.plot_manager = None
        self._data_cache = {}
        self._entropy_results = None
        self._fibonacci_vectors = {}
        self._dense = None
        self._plan = None
        self._plan_key = None
        self.last_timing = {}
        self._heatmaps = {}
        self._heatmap_source = None   # (plan, mu, mv, tile_width, tile_height) of the last compute_entropy

    def _naive_plan(self) -> "_native.Plan":
        cfg = self.config
        th, tw = cfg.tile_height, cfg.tile_width
        if 180 % th != 0:
            raise ValidationError("Tile height must divide 180!")
        if 360 % tw != 0:
            raise ValidationError("Tile width must divide 360!")
        key = (cfg.video_width, cfg.video_height, th, tw, cfg.entropy_config.use_weight_distribution)
        if self._plan is None or self._plan_key != key:
            lon, lat = _quantiser.axis_angles(cfg.video_width, cfg.video_height)
            li = ((lon + 180) / tw).astype(np.int64)            # int() truncation, entropy_utils.py:378-379
            lj = ((lat + 90) / th).astype(np.int64)
            n_lat = int(lj.max()) + 1
            bins = (int(li.max()) + 1) * n_lat
            if li.min() < 0 or lj.min() < 0 or bins > 65535:
                raise ValidationError("tile dimensions give an unsupported number of grid cells")
            lut = (li[None, :] * n_lat + lj[:, None]).astype(np.uint16)      # [H+1][W+1]
            num_tiles = naive_tile_count(th, tw)
            ec = cfg.entropy_config
            self._plan = _native.Plan(_native.Engine.default(), [None], ec.fov_angle, ec.power_factor,
                                      ec.use_weight_distribution, cfg.video_width, cfg.video_height,
                                      bin_luts=[lut], bin_counts=[bins],
                                      bin_max_entropy=[_quantiser.max_entropy(num_tiles)], bin_norm_tiles=[num_tiles])
            self._plan_key = key
        return self._plan

    def _samples(self):
        """The engine's dense samples: this analyzer bins its own ingest only (no hand-assigned vectors)."""
        if not self._data_cache or self._dense is None:
            raise ValidationError("No data available. Call process_directory first.")
        times, mu, mv, names = self._dense
        return "grid", times, mu, mv, names

    def _grid_plan(self) -> "_native.Plan":
        return self._naive_plan()

    def compute_entropy(self) -> pd.DataFrame:
        _, times, mu, mv, _ = self._samples()
        t_start = time.perf_counter()
        try:
            plan = self._naive_plan()
            res = plan.spatial(mu=mu, mv=mv, want_assign=False, want_weights=False)
        except _native.NativeError as e:
            if e.code == _native.VET_ERR_RANGE:
                raise ValidationError(str(e))
            if e.code == _native.VET_ERR_EMPTY:
                raise ValidationError("Empty radial points dictionary")
            raise
        self._record_compute(time.perf_counter() - t_start, mu.size, len(times))
        self._entropy_results = pd.DataFrame({
            "time": times,
            "entropy": res["entropy"],
            "tile_weights": [None] * len(times),
            "tile_assignments": [None] * len(times),
        })
        self._heatmap_source = (plan, mu, mv, self.config.tile_width, self.config.tile_height)
        return self._entropy_results

    def compute_windowed_entropy(self, window: int, stride: int = 1) -> pd.DataFrame:
        """Entropy of the users pooled over sliding windows of frames: row r counts every present sample of frames
        [r * stride, r * stride + window) in ONE lat/lon cell histogram and takes ``compute_naive_spatial_entropy``'s
        normalised entropy of it (the normaliser compares the window's samples, not users, with the tile count).
        ``window`` and ``stride`` count frames, i.e. rows of ``vectors_df``.

        Uses the data ``process_directory`` cached.  Returns a new DataFrame with ``time`` / ``time_end`` (of the window's
        first / last frame), ``entropy`` and ``samples`` (present samples of the window).  Raises ``ValidationError`` before
        data is loaded, ``ValueError`` for an illegal ``window`` / ``stride``."""
        times, names, call = self._row_call("spatial_windowed", lambda *_: ValidationError("Empty radial points dictionary"))
        window, stride = self._window_args(window, stride, len(times))
        res = call(window=window, stride=stride)
        first = np.arange(len(res["entropy"]), dtype=np.int64) * stride
        return pd.DataFrame({
            "time": np.asarray(times)[first],
            "time_end": np.asarray(times)[first + window - 1],
            "entropy": res["entropy"],
            "samples": res["samples"],
        })

    def compute_user_entropy(self, window: Optional[int] = None, stride: int = 1) -> pd.DataFrame:
        """How many lat/lon cells each viewer visits: row (user, r) counts that user's present samples of frames
        [r * stride, r * stride + window) in ONE cell histogram and takes ``compute_naive_spatial_entropy``'s normalised
        entropy of it.  ``window=None`` is the whole video (one row per user); ``window`` and ``stride`` count frames.

        Uses the data ``process_directory`` cached.  Returns a new DataFrame, user-major, one row per (user, r): ``user``,
        ``time`` / ``time_end`` (of the row's first / last frame), ``entropy`` and ``samples``.  A row in which the user has no
        sample is NaN with ``samples`` 0 — returned, never raised.  Raises ``ValidationError`` before data is loaded and for
        samples outside [0, 1], ``ValueError`` for an illegal ``window`` / ``stride``."""
        times, names, call = self._row_call("spatial_per_user")
        window, stride = self._window_args(len(times) if window is None else window, stride, len(times))
        res = call(window=window, stride=stride)
        return self._user_frame(names, times, window, stride, res)

    def compute_user_divergence(self, window: Optional[int] = None, stride: int = 1) -> pd.DataFrame:
        """Do viewers look at the same lat/lon cells: for every row r — frames [r * stride, r * stride + window),
        ``window=None`` the whole video — the U x U matrix of Jensen-Shannon divergences, in bits, between the viewers' cell
        counts of the row, each viewer weighted by their samples (``SpatialEntropyAnalyzer.compute_user_divergence`` on
        ``compute_naive_spatial_entropy``'s histogram).

        Uses the data ``process_directory`` cached.  Returns a new DataFrame with one row per window: ``time`` / ``time_end``,
        ``divergence`` (a [U, U] view into the one result array) and ``samples`` ([U]); ``attrs["users"]`` holds the user names
        in matrix order.  A viewer without a sample in the window has NaN rows and columns and ``samples`` 0 — returned, never
        raised.  Raises ``ValidationError`` before data is loaded and for samples outside [0, 1], ``ValueError`` for an illegal
        ``window`` / ``stride``."""
        times, names, call = self._row_call("spatial_user_divergence")
        window, stride = self._window_args(len(times) if window is None else window, stride, len(times))
        res = call(window=window, stride=stride)
        return self._divergence_frame(names, times, window, stride, res)

    def compute_window_divergence(self, window: int, stride: int = 1, max_lag: int = 1) -> pd.DataFrame:
        """When does the audience's attention move between lat/lon cells: for every row r — frames
        [r * stride, r * stride + window) — and every lag l = 1 .. ``max_lag`` (in rows) the Jensen-Shannon divergence, in bits,
        between the pooled cell counts of rows r and r + l, each window weighted by its samples
        (``SpatialEntropyAnalyzer.compute_window_divergence`` on ``compute_naive_spatial_entropy``'s histogram).

        Uses the data ``process_directory`` cached.  Returns a new DataFrame with one row per window: ``time`` / ``time_end``,
        ``samples``, ``shift`` (the lag-1 value) and ``divergence`` (an [L] view into the one result array);
        ``attrs["lags"]`` = [1 .. L], ``attrs["lag_frames"]`` = [stride, 2 stride, ...].  Entries whose partner row does not
        exist are NaN, and so are the pairs of a window without a sample — returned, never raised.  Raises ``ValidationError``
        before data is loaded and for samples outside [0, 1], ``ValueError`` for an illegal ``window`` / ``stride`` /
        ``max_lag``."""
        times, names, call = self._row_call("spatial_window_divergence")
        window, stride = self._window_args(window, stride, len(times))
        max_lag = self._lag_args(max_lag, window, stride, len(times))
        res = call(window=window, stride=stride, max_lag=max_lag)
        return self._window_divergence_frame(times, window, stride, res)

    def compute_coverage(self, window: int = 1, stride: int = 1, fractions=(0.5, 0.8, 0.95), max_lag: int = 0,
                         keep_order: bool = False) -> pd.DataFrame:
        """Which lat/lon cells hold the audience's attention, and for how long: for every row r — frames
        [r * stride, r * stride + window) — the cells are ranked by the window's pooled sample counts and the top-ranked cells
        that hold 50 % / 80 % / 95 % (``fractions``) of the samples are counted; then the share of the NEXT windows' samples in
        those same cells is taken (``SpatialEntropyAnalyzer.compute_coverage`` on ``compute_naive_spatial_entropy``'s histogram;
        cells are numbered ``lon index * cells per column + lat index`` and differ in area).

        Uses the data ``process_directory`` cached.  Returns a new DataFrame with one row per window: ``time`` / ``time_end`` (of
        the row's first / last frame), ``samples``, ``tiles`` ([Q]: the smallest number of top-ranked cells whose running sum
        reaches each fraction of the window's mass), ``share`` (``tiles / n``: a share of the cells, not of the sphere's area),
        ``covered`` ([Q]: the share actually reached, lag 0), ``forecast`` (an [L, Q] view: the share of the mass of the windows
        1 .. ``max_lag`` rows later that the same cells hold) and, with ``keep_order``, ``order`` ([n]: the cells by weight
        descending, equal weights by index).  ``attrs`` hold ``fractions``, ``lags`` = [1 .. L], ``lag_frames`` = [stride,
        2 stride, ...] and ``n_tiles``.  A window without mass has ``tiles`` 0 and NaN shares, and so have the lags that reach
        past the last window — returned, never raised.  Raises ``ValidationError`` before data is loaded and for samples outside
        [0, 1], ``ValueError`` for an illegal ``window`` / ``stride`` / ``fractions`` (1 to 8 numbers in (0, 1], strictly
        increasing) / ``max_lag`` (0 .. rows - 1)."""
        return self._coverage(window, stride, fractions, max_lag, keep_order, lambda: self._naive_plan().n_tiles[0])

    def compute_crowd_divergence(self, window: Optional[int] = None, stride: int = 1) -> pd.DataFrame:
        """How typical each viewer is of the audience, on lat/lon cells: for every row r — frames
        [r * stride, r * stride + window), ``window=None`` the whole video — and viewer u the Kullback-Leibler divergence, in
        bits, of the viewer's cell counts from the window's pooled cell counts
        (``SpatialEntropyAnalyzer.compute_crowd_divergence`` on ``compute_naive_spatial_entropy``'s histogram).

        Uses the data ``process_directory`` cached.  Returns a new DataFrame, user-major, one row per (user, r): ``user``,
        ``time`` / ``time_end``, ``divergence`` and ``samples``; ``attrs["rows"]`` is the per-window DataFrame (``time``,
        ``time_end``, ``samples``, ``pooled``, ``within``, ``between``), ``attrs["users"]`` the user names.  A viewer without a
        sample in the window is NaN with ``samples`` 0 — returned, never raised.  Raises ``ValidationError`` before data is
        loaded and for samples outside [0, 1], ``ValueError`` for an illegal ``window`` / ``stride``."""
        times, names, call = self._row_call("spatial_crowd_divergence")
        window, stride = self._window_args(len(times) if window is None else window, stride, len(times))
        res = call(window=window, stride=stride)
        return self._crowd_frame(names, times, window, stride, res)

    def compute_entropy_bootstrap(self, window: int = 1, stride: int = 1, replicates: int = 200, confidence: float = 0.95,
                                  seed: int = 0, keep_replicates: bool = False) -> pd.DataFrame:
        """Bootstrap confidence bands for the per-frame / windowed lat/lon cell entropy
        (``SpatialEntropyAnalyzer.compute_entropy_bootstrap`` on ``compute_naive_spatial_entropy``'s histogram).

        Viewers are the independent unit, so the audience is resampled with replacement ``replicates`` times (the cluster
        bootstrap: the same resample for every window, a viewer's whole trajectory stays together; the draw is a counter-based
        generator on ``seed``, include/vet.h) and every window is recomputed for each resample on the GPU.  ``window=1,
        stride=1`` is the per-frame series.

        Uses the data ``process_directory`` cached.  Returns a new DataFrame with one row per window: ``time`` / ``time_end`` (of
        the window's first / last frame), ``entropy`` and ``samples`` (the point estimate: ``compute_windowed_entropy``'s values,
        NaN with ``samples`` 0 for a window without a sample), ``mean`` and ``sd`` (ddof = 1) of the finite replicates, ``lo`` /
        ``hi`` (their quantiles (1 - confidence) / 2 and 1 - (1 - confidence) / 2, linear interpolation) and ``valid`` (how many
        replicates are finite: a resample whose viewers have no sample in the window is NaN).  ``keep_replicates`` adds
        ``replicates``, a [B] view into the one result array per row.  ``attrs`` holds ``replicates``, ``seed`` and
        ``confidence``.  Raises ``ValidationError`` before data is loaded and for samples outside [0, 1], ``ValueError`` for an
        illegal ``window`` / ``stride`` / ``replicates`` (1 .. 4096) / ``confidence`` (inside (0, 1)) / ``seed``."""
        return self._entropy_bootstrap(window, stride, replicates, confidence, seed, keep_replicates)

    def compute_group_divergence(self, groups, window: Optional[int] = None, stride: int = 1, permutations: int = 999,
                                 confidence: float = 0.95, seed: int = 0, keep_null: bool = False) -> pd.DataFrame:
        """Do two audiences look at different places, in which segments, and by more than chance: a permutation test of the
        attention divergence between two groups of viewers on
        ``compute_naive_spatial_entropy``'s lat/lon cell histogram.

        ``groups`` is a sequence aligned with the analyzer's user order, or a mapping from user name to label.  There must be
        exactly two distinct labels; in sorted order the first is audience A.  ``None`` / NaN (or a user the mapping does not
        name) is excluded.  Every window (``window=None``: the whole video as one row) gets the mass-weighted Jensen-Shannon
        divergence, in bits, between the pooled histograms of the two audiences, and the same statistic for ``permutations``
        relabellings of the included viewers that keep the group sizes (the same relabelling for every window: a viewer's
        trajectory stays together; the draw is a counter-based generator on ``seed``, include/vet.h), all on the GPU.

        Uses the data ``process_directory`` cached.  Returns a new DataFrame with one row per window: ``time`` / ``time_end``,
        ``samples_a`` / ``samples_b`` (present samples of each audience), ``divergence`` (NaN where an audience has no sample),
        ``p_value`` ((1 + relabellings at least as divergent) / (1 + finite relabellings)), ``p_adjusted`` (the max-statistic
        family-wise correction over the windows of the call), ``null_mean``, ``null_crit`` (the ``confidence`` quantile of the
        null, linear interpolation) and ``valid`` (finite relabellings).  ``keep_null`` adds ``null``, a [P] view into the one
        result array per row.  ``attrs`` holds ``groups`` (the two labels), ``sizes``, ``users``, ``permutations``, ``seed`` and
        ``confidence``.  Raises ``ValidationError`` before data is loaded and for samples outside [0, 1], ``ValueError`` for
        illegal ``groups`` / ``window`` / ``stride`` / ``permutations`` (1 .. 4096) / ``confidence`` (inside (0, 1)) / ``seed``."""
        return self._group_divergence(groups, window, stride, permutations, confidence, seed, keep_null)

    # ------------------------------------------------------------------ heatmaps (_HeatmapMixin)
    def _heatmap(self, width: int, height: int, marker_radius: int) -> "_native.Heatmap":
        plan, _, _, tw, th = self._heatmap_source
        key = (tw, th, width, height, plan.width, plan.height, marker_radius)
        if key not in self._heatmaps:
            try:
                self._heatmaps[key] = _native.Heatmap.latlon(_native.Engine.default(), tw, th, width, height, plan.width,
                                                             plan.height, marker_radius)
            except _native.NativeError as e:
                if e.code == _native.VET_ERR_INVALID:
                    raise ValidationError(str(e))
                raise
        return self._heatmaps[key]

    def _render_block(self, hm, row0: int, n: int, markers: bool, out=None) -> np.ndarray:
        plan, mu, mv, _, _ = self._heatmap_source
        return hm.render_binned(plan, mu, mv, row0, n, markers, out=out)
