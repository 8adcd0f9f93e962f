"""SpatialEntropyAnalyzer: per-frame normalised Shannon entropy of the FoV-weighted tile
histogram, averaged over the configured lattice sizes (reference
analyzers/spatial_entropy.py:107-164), computed by the HIP engine in one call per video."""

from __future__ import annotations

import logging
import time
from typing import Optional

import numpy as np
import pandas as pd

from .. import _native
from ..config import AnalyzerConfig
from ..data_types import ValidationError
from .._results import DeviceRows, FrameDictArray, TileAssignments, TileWeights
from ._base import _EntropyAnalyzerBase
from ._heatmaps import _HeatmapMixin

logger = logging.getLogger(__name__)


class SpatialEntropyAnalyzer(_HeatmapMixin, _EntropyAnalyzerBase):
    """Drop-in analyzer: ``process_directory`` / ``compute_entropy`` / ``create_visualization`` /
    ``run_analysis`` with the reference's result schema
    (``time``, ``entropy``, ``tile_weights``, ``tile_assignments``)."""

    _logger = logger

    def __init__(self, config: Optional[AnalyzerConfig] = None, *, fp64: bool = False):
        """``fp64=True``: the entropy in FP64 arithmetic from start to end (``Plan.set_fp64``: exact FP64 weights summed in
        FP64, the reference's own arithmetic) instead of the engine's default formulations.  The tile weights are the same
        values either way."""
        super().__init__(config)
        self._fp64 = bool(fp64)

    def compute_entropy(self) -> pd.DataFrame:
        kind, times, a, b, names = self._samples()
        t_start = time.perf_counter()
        try:
            # only the entropy series crosses PCIe; tile weights / assignments stay in device memory and are
            # fetched by frame when a cell of the result is read
            if kind == "grid":
                res = self._get_plan().spatial_resident(mu=a, mv=b)
            else:
                plan = self._get_plan(dir_table=b)
                try:
                    res = plan.spatial_resident(ids=a)
                finally:
                    plan.close()
        except _native.NativeError as e:
            if e.code == _native.VET_ERR_RANGE:
                raise ValidationError(str(e))
            if e.code == _native.VET_ERR_EMPTY:
                raise ValidationError("Empty vector dictionary")
            raise
        self._record_compute(time.perf_counter() - t_start, a.size, len(res["entropy"]))
        tiles = self._fibonacci_vectors[self.config.tile_counts[0]]
        T = len(res["entropy"])
        self._device_result = res["result"]
        self._present = res["present"]
        self._marker_samples = (a, b) if kind == "grid" else None
        self._entropy_results = pd.DataFrame({
            "time": times,
            "entropy": res["entropy"],
            "tile_weights": FrameDictArray(DeviceRows(res["result"], 1, T), lambda row: TileWeights(tiles, row)),
            "tile_assignments": FrameDictArray(DeviceRows(res["result"], 0, T), lambda row: TileAssignments(names, row)),
        })
        return self._entropy_results

    def compute_windowed_entropy(self, window: int, stride: int = 1) -> pd.DataFrame:
        """Entropy of the attention pooled over sliding windows of frames: row r puts every present sample of frames
        [r * stride, r * stride + window) into ONE histogram per lattice and takes the reference's normalised entropy of it
        (``compute_spatial_entropy`` on a dict holding all those samples), averaged over the lattices — not the mean of the
        per-frame entropies.  ``window`` and ``stride`` count frames, i.e. rows of ``vectors_df`` (0.1 s each at the
        reference's sampling): ``window=20, stride=1`` is a 2-second window every frame.

        Uses the data ``process_directory`` cached.  Returns a new DataFrame (``compute_entropy``'s results are left alone)
        with ``time`` / ``time_end`` (of the window's first / last frame), ``entropy``, ``samples`` (present samples of the
        window) and ``tile_weights`` (lattice 0's pooled weights, the reference's dict-of-``Vector`` shape).
        Raises ``ValidationError`` before data is loaded, ``ValueError`` for an illegal ``window`` / ``stride``."""
        times, names, call = self._row_call("spatial_windowed", lambda *_: ValidationError("Empty vector dictionary"))
        window, stride = self._window_args(window, stride, len(times))
        res = call(window=window, stride=stride, want_weights=True)
        tiles = self._fibonacci_vectors[self.config.tile_counts[0]]
        first = np.arange(len(res["entropy"]), dtype=np.int64) * stride
        return pd.DataFrame({
            "time": np.asarray(times)[first],
            "time_end": np.asarray(times)[first + window - 1],
            "entropy": res["entropy"],
            "samples": res["samples"],
            "tile_weights": FrameDictArray(res["weights"], lambda row: TileWeights(tiles, row)),
        })

    def compute_user_entropy(self, window: Optional[int] = None, stride: int = 1) -> pd.DataFrame:
        """How much of the sphere each viewer visits: row (user, r) puts that user's present samples of frames
        [r * stride, r * stride + window) into ONE histogram per lattice and takes the reference's normalised entropy of it
        (``compute_spatial_entropy`` on a dict holding those samples in frame order), averaged over the lattices.
        ``window=None`` is the whole video (one row per user); ``window`` and ``stride`` count frames, i.e. rows of
        ``vectors_df``.

        Uses the data ``process_directory`` cached.  Returns a new DataFrame (``compute_entropy``'s results are left alone),
        user-major, one row per (user, r): ``user`` (the column name from ingest), ``time`` / ``time_end`` (of the row's first /
        last frame), ``entropy``, ``samples`` (the user's present samples of the row) and ``tile_weights`` (lattice 0's
        histogram, the reference's dict-of-``Vector`` shape).  A row in which the user has no sample is NaN with ``samples`` 0
        — returned, never raised.  Raises ``ValidationError`` before data is loaded and for samples outside [0, 1],
        ``ValueError`` for an illegal ``window`` / ``stride``."""
        times, names, call = self._row_call("spatial_per_user")
        window, stride = self._window_args(len(times) if window is None else window, stride, len(times))
        res = call(window=window, stride=stride, want_weights=True)
        tiles = self._fibonacci_vectors[self.config.tile_counts[0]]
        weights = res["weights"].reshape(-1, res["weights"].shape[-1])
        return self._user_frame(names, times, window, stride, res,
                                FrameDictArray(weights, lambda row: TileWeights(tiles, row)))

    def compute_user_divergence(self, window: Optional[int] = None, stride: int = 1) -> pd.DataFrame:
        """Do viewers look at the same places: for every row r — frames [r * stride, r * stride + window), ``window=None`` the
        whole video — the U x U matrix of Jensen-Shannon divergences, in bits, between the viewers' tile histograms of the row
        (``compute_user_entropy``'s ``tile_weights``), each viewer weighted by their mass, averaged over the lattices:
        ``D(u, v) = S(h_u + h_v) - (W_u S(h_u) + W_v S(h_v)) / (W_u + W_v)`` with ``S`` the reference's entropy of one dict
        before the normaliser.  0 = the same places in the same proportions, 1 = equal masses on disjoint tiles.

        Uses the data ``process_directory`` cached.  Returns a new DataFrame with one row per window: ``time`` / ``time_end`` (of
        the row's first / last frame), ``divergence`` (a [U, U] view into the one result array: symmetric, +0.0 diagonal) and
        ``samples`` ([U]: each viewer's present samples of the row); ``attrs["users"]`` holds the user names in matrix order.
        The rows and columns of a viewer without a sample in the window are NaN with ``samples`` 0 — returned, never raised.
        Raises ``ValidationError`` before data is loaded and for samples outside [0, 1], ``ValueError`` for an illegal
        ``window`` / ``stride``."""
        times, names, call = self._row_call("spatial_user_divergence")
        window, stride = self._window_args(len(times) if window is None else window, stride, len(times))
        res = call(window=window, stride=stride)
        return self._divergence_frame(names, times, window, stride, res)

    def compute_window_divergence(self, window: int, stride: int = 1, max_lag: int = 1) -> pd.DataFrame:
        """When does the audience's attention move: for every row r — frames [r * stride, r * stride + window) — and every lag
        l = 1 .. ``max_lag`` (in rows) the Jensen-Shannon divergence, in bits, between the pooled tile histograms of rows r and
        r + l (``compute_windowed_entropy``'s ``tile_weights``), each window weighted by its mass, averaged over the lattices:
        ``D(r, l) = S(P_r + P_{r+l}) - (W_r S(P_r) + W_{r+l} S(P_{r+l})) / (W_r + W_{r+l})`` with ``S`` the reference's entropy of
        one dict before the normaliser.  0 = the same tiles in the same proportions, 1 = equal masses on disjoint tiles: a crowd
        that jumps across the sphere keeps its entropy but shows here.

        Uses the data ``process_directory`` cached.  Returns a new DataFrame with one row per window: ``time`` / ``time_end`` (of
        the row's first / last frame), ``samples``, ``shift`` (the lag-1 value: the attention-shift series) and ``divergence``
        (an [L] view into the one result array; entry l - 1 is lag l); ``attrs["lags"]`` = [1 .. L] and
        ``attrs["lag_frames"]`` = [stride, 2 stride, ...].  Entries whose partner row does not exist are NaN, and so are the
        pairs of a window without a sample (``samples`` 0) — returned, never raised.  Raises ``ValidationError`` before data is
        loaded and for samples outside [0, 1], ``ValueError`` for an illegal ``window`` / ``stride`` / ``max_lag``."""
        times, names, call = self._row_call("spatial_window_divergence")
        window, stride = self._window_args(window, stride, len(times))
        max_lag = self._lag_args(max_lag, window, stride, len(times))
        res = call(window=window, stride=stride, max_lag=max_lag)
        return self._window_divergence_frame(times, window, stride, res)

    def compute_coverage(self, window: int = 1, stride: int = 1, fractions=(0.5, 0.8, 0.95), max_lag: int = 0,
                         keep_order: bool = False) -> pd.DataFrame:
        """Which tiles hold the audience's attention, and for how long: for every row r — frames
        [r * stride, r * stride + window) — the tiles of the first lattice are ranked by the window's pooled weight
        (``compute_windowed_entropy``'s ``tile_weights``) and the top-ranked tiles that hold 50 % / 80 % / 95 % (``fractions``) of
        the mass are counted; then the share of the NEXT windows' mass on those same tiles is taken — what a tile-based delivery
        that picks its high-quality tiles from this segment would still cover.  Only the first tile count takes part.

        Uses the data ``process_directory`` cached.  Returns a new DataFrame with one row per window: ``time`` / ``time_end`` (of
        the row's first / last frame), ``samples``, ``tiles`` ([Q]: the smallest number of top-ranked tiles whose running sum
        reaches each fraction of the window's mass), ``share`` (``tiles / n``: a share of the tiles, not of the sphere's area),
        ``covered`` ([Q]: the share actually reached, lag 0), ``forecast`` (an [L, Q] view: the share of the mass of the windows
        1 .. ``max_lag`` rows later that the same tiles hold) and, with ``keep_order``, ``order`` ([n]: the tiles by weight
        descending, equal weights by index).  ``attrs`` hold ``fractions``, ``lags`` = [1 .. L], ``lag_frames`` = [stride,
        2 stride, ...] and ``n_tiles``.  A window without mass has ``tiles`` 0 and NaN shares, and so have the lags that reach
        past the last window — returned, never raised.  Raises ``ValidationError`` before data is loaded and for samples outside
        [0, 1], ``ValueError`` for an illegal ``window`` / ``stride`` / ``fractions`` (1 to 8 numbers in (0, 1], strictly
        increasing) / ``max_lag`` (0 .. rows - 1)."""
        return self._coverage(window, stride, fractions, max_lag, keep_order,
                              lambda: len(self._fibonacci_vectors[self.config.tile_counts[0]]))

    def compute_crowd_divergence(self, window: Optional[int] = None, stride: int = 1) -> pd.DataFrame:
        """How typical each viewer is of the audience: for every row r — frames [r * stride, r * stride + window),
        ``window=None`` the whole video — and viewer u the Kullback-Leibler divergence, in bits, of the viewer's tile histogram
        (``compute_user_entropy``'s ``tile_weights``, total ``W_u``) from the window's pooled histogram
        (``compute_windowed_entropy``'s ``tile_weights``, total ``W_r``), averaged over the lattices:
        ``D(u, r) = sum_t q_t log2(q_t / p_t)``.  0 = the viewer looks where the crowd looks, in the crowd's proportions,
        ``log2(W_r / W_u)`` = the viewer shares no tile with anybody.

        Uses the data ``process_directory`` cached.  Returns a new DataFrame, user-major, one row per (user, r): ``user``,
        ``time`` / ``time_end`` (of the row's first / last frame), ``divergence`` and ``samples``.  ``attrs["rows"]`` is a
        DataFrame with one row per window: ``time``, ``time_end``, ``samples``, ``pooled`` (the entropy of the pooled histogram
        before the normaliser, bits), ``within`` (the mass-weighted mean of the viewers' own entropies) and ``between`` (the
        mass-weighted mean of ``divergence``: the generalised Jensen-Shannon divergence of the audience);
        ``pooled = within + between``.  ``attrs["users"]`` holds the user names.  A viewer without a sample in the window is NaN
        with ``samples`` 0 — returned, never raised.  Raises ``ValidationError`` before data is loaded and for samples outside
        [0, 1], ``ValueError`` for an illegal ``window`` / ``stride``."""
        times, names, call = self._row_call("spatial_crowd_divergence")
        window, stride = self._window_args(len(times) if window is None else window, stride, len(times))
        res = call(window=window, stride=stride)
        return self._crowd_frame(names, times, window, stride, res)

    def compute_entropy_bootstrap(self, window: int = 1, stride: int = 1, replicates: int = 200, confidence: float = 0.95,
                                  seed: int = 0, keep_replicates: bool = False) -> pd.DataFrame:
        """Is a dip attention converging, or too few viewers: bootstrap confidence bands for the per-frame / windowed entropy.

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
        attention divergence between two groups of viewers.

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

    def _frame_present(self):
        return self._present
