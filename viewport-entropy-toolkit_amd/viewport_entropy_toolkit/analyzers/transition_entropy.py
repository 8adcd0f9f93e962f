"""TransitionEntropyAnalyzer: per-frame entropy of the (t-1 -> t) nearest-tile transitions of
the users present in both frames (reference analyzers/transition_entropy.py:107-175 and
utilities/entropy_utils.py:213-332), computed by the HIP engine in one call per video.
Row 0 of the frame table only seeds the prior, so the result has T-1 rows."""

from __future__ import annotations

import logging
import time
from typing import Optional

import numpy as np
import pandas as pd

from .. import _native
from ..data_types import ValidationError
from .._results import DeviceRows, FrameDictArray, TilePairs, TileWeights
from ._base import _EntropyAnalyzerBase
from ._heatmaps import _HeatmapMixin

logger = logging.getLogger(__name__)


class TransitionEntropyAnalyzer(_HeatmapMixin, _EntropyAnalyzerBase):
    """Drop-in analyzer with the reference's result schema; ``tile_weights`` holds the user
    count per source tile and ``tile_assignments`` the (prior, current) tile index pairs."""

    _logger = logger
    _heatmap_entry = "render_transition_result"

    @staticmethod
    def _presence(kind, a, b) -> np.ndarray:
        """bool [T, U]: user u has a sample in frame t (grid: (mu, mv) not NaN; ids: a direction id)."""
        return (a >= 0) if kind != "grid" else ~(np.isnan(a) | np.isnan(b))

    @classmethod
    def _prior_frame_present(cls, kind, a, b) -> np.ndarray:
        """int32 [T-1]: the users present in frame r for every result row r (the pair r -> r+1) — the denominator of the
        reference's animation colours, len(points_list) of points_data.iloc[r] (utilities/visualization_utils.py:124-
        152), which counts a user who leaves at r+1 and is not the common-user count."""
        return cls._presence(kind, a, b)[:-1].sum(axis=1, dtype=np.int32)

    @classmethod
    def _empty_row_error(cls, kind, a, b) -> Exception:
        """The exception the reference raises at the FIRST frame pair without a common user: a frame whose dict is
        empty -> ValidationError("Empty vector dictionary") (utilities/entropy_utils.py:239-240); both frames have users
        but nobody is in both -> the division by the zero total weight (:322-327)."""
        present = cls._presence(kind, a, b)
        common = (present[:-1] & present[1:]).any(axis=1)
        r = int(np.argmin(common))                 # first row without a common user
        if not present[r].any() or not present[r + 1].any():
            return ValidationError("Empty vector dictionary")
        return ZeroDivisionError("division by zero")          # `1 / total_weight` with the int 0 (:326)

    def compute_entropy(self) -> pd.DataFrame:
        kind, times, a, b, names = self._samples()
        t_start = time.perf_counter()
        try:
            if kind == "grid":
                res = self._get_plan().transition_resident(mu=a, mv=b)
            else:
                plan = self._get_plan(dir_table=b)
                try:
                    res = plan.transition_resident(ids=a)
                finally:
                    plan.close()
        except _native.NativeError as e:
            if e.code == _native.VET_ERR_RANGE:
                raise ValidationError(str(e))
            if e.code == _native.VET_ERR_EMPTY:
                raise self._empty_row_error(kind, a, b)
            raise
        self._record_compute(time.perf_counter() - t_start, a.size, len(res["entropy"]))
        tiles = self._fibonacci_vectors[self.config.tile_counts[0]]
        R = len(res["entropy"])
        self._device_result = res["result"]
        # heatmaps: the presence of each row's prior frame is counted on the first render, from these references
        self._present = None
        self._present_samples = (kind, a, b if kind == "grid" else None)
        self._marker_samples = (a, b) if kind == "grid" else None
        self._entropy_results = pd.DataFrame({
            "time": times[1:],
            "entropy": res["entropy"],
            "tile_weights": FrameDictArray(DeviceRows(res["result"], 1, R), lambda row: TileWeights(tiles, row, as_int=True)),
            "tile_assignments": FrameDictArray(DeviceRows(res["result"], 0, R), lambda row: TilePairs(names, row)),
        })
        return self._entropy_results

    @classmethod
    def _empty_window_error(cls, kind, a, b, window: int, stride: int) -> Exception:
        """The exception the reference raises on the pooled dicts of the FIRST window without a common sample: no sample at
        all in the window's prior frames or in its current frames -> ValidationError("Empty vector dictionary")
        (utilities/entropy_utils.py:239-240); otherwise the division by the zero total weight (:322-327)."""
        present = cls._presence(kind, a, b)
        common = (present[:-1] & present[1:]).any(axis=1)
        for f0 in range(0, len(common) - window + 1, stride):
            if not common[f0:f0 + window].any():
                if not present[f0:f0 + window].any() or not present[f0 + 1:f0 + window + 1].any():
                    return ValidationError("Empty vector dictionary")
                break
        return ZeroDivisionError("division by zero")

    def compute_windowed_entropy(self, window: int, stride: int = 1) -> pd.DataFrame:
        """Transition entropy of the transitions pooled over sliding windows of frame pairs: row r puts the (t -> t+1)
        nearest-tile transition of every user present in both frames, for every pair of [r * stride, r * stride + window),
        into ONE call of the reference's ``compute_transition_entropy`` (both dicts keyed per (pair, user), pair-major then
        user order), averaged over the lattices — not the mean of the per-pair entropies.  ``window`` and ``stride`` count
        frame pairs, i.e. rows of ``compute_entropy``'s result (0.1 s each at the reference's sampling): ``window=20,
        stride=1`` is a 2-second window every frame.

        Uses the data ``process_directory`` cached.  Returns a new DataFrame (``compute_entropy``'s results are left alone)
        with ``time`` / ``time_end`` (the ``time`` ``compute_entropy`` gives the window's first / last pair), ``entropy``,
        ``samples`` (pooled (pair, user) samples of the window) and ``tile_weights`` (lattice 0's pooled count per source
        tile, in the shape of ``compute_entropy``'s column).  Raises ``ValidationError`` before data is loaded, ``ValueError``
        for an illegal ``window`` / ``stride``, and for a window without a common sample what the reference raises on its
        pooled dicts (``ValidationError("Empty vector dictionary")`` or ``ZeroDivisionError``)."""
        times, names, call = self._row_call(
            "transition_windowed", lambda kind, a, b, kw: self._empty_window_error(kind, a, b, kw["window"], kw["stride"]))
        window, stride = self._window_args(window, stride, len(times) - 1)
        res = call(window=window, stride=stride, want_srccount=True)
        tiles = self._fibonacci_vectors[self.config.tile_counts[0]]
        first = np.arange(len(res["entropy"]), dtype=np.int64) * stride
        pair_time = np.asarray(times)[1:]
        return pd.DataFrame({
            "time": pair_time[first],
            "time_end": pair_time[first + window - 1],
            "entropy": res["entropy"],
            "samples": res["samples"],
            "tile_weights": FrameDictArray(res["srccount"], lambda row: TileWeights(tiles, row, as_int=True)),
        })

    def compute_user_entropy(self, window: Optional[int] = None, stride: int = 1) -> pd.DataFrame:
        """How predictably each viewer moves between tiles: row (user, r) puts that user's own (t -> t+1) nearest-tile
        transitions of the pairs [r * stride, r * stride + window) in which the user is present in both frames into ONE call of
        the reference's ``compute_transition_entropy`` (both dicts keyed per pair, in ascending pair order), averaged over the
        lattices.  ``window=None`` is the whole video (one row per user); ``window`` and ``stride`` count frame pairs, i.e.
        rows of ``compute_entropy``'s result.

        Uses the data ``process_directory`` cached.  Returns a new DataFrame (``compute_entropy``'s results are left alone),
        user-major, one row per (user, r): ``user`` (the column name from ingest), then ``compute_windowed_entropy``'s columns:
        ``time`` / ``time_end`` (the ``time`` ``compute_entropy`` gives the row's first / last pair), ``entropy``, ``samples``
        (the user's pairs of the row present in both frames) and ``tile_weights`` (lattice 0's count per source tile).  A row
        without such a pair is NaN with ``samples`` 0 — returned, never raised; a row of one pair is the reference's NaN
        (0 / 0).  Raises ``ValidationError`` before data is loaded and for samples outside [0, 1], ``ValueError`` for an illegal
        ``window`` / ``stride``."""
        times, names, call = self._row_call("transition_per_user")
        window, stride = self._window_args(len(times) - 1 if window is None else window, stride, len(times) - 1)
        res = call(window=window, stride=stride, want_srccount=True)
        tiles = self._fibonacci_vectors[self.config.tile_counts[0]]
        src = res["srccount"].reshape(-1, res["srccount"].shape[-1])
        return self._user_frame(names, np.asarray(times)[1:], window, stride, res,
                                FrameDictArray(src, lambda row: TileWeights(tiles, row, as_int=True)))

    def compute_markov_entropy(self, window: Optional[int] = None, stride: int = 1, lag: int = 1,
                               keep_matrix: bool = False) -> pd.DataFrame:
        """The textbook statistics of the tile-to-tile moves, from integer transition counts: pair f is (frame f, frame f + lag),
        row r pools every (pair, user) of the pairs [r * stride, r * stride + window) with a sample in both frames (the frames in
        between do not matter) into the counts n_pc per (source tile, destination tile).  ``window`` and ``stride`` count pairs;
        ``window=None`` is the whole video (one row).  Not ``compute_entropy``'s statistic: that one is the reference's
        ``compute_transition_entropy``, which depends on the order in which users and destinations first appear.

        Uses the data ``process_directory`` cached.  Returns a new DataFrame (``compute_entropy``'s results are left alone), one row
        per window: ``time`` / ``time_end`` (the time of the later frame of the row's first / last pair), ``samples`` (pooled
        samples N), ``rate`` (the entropy rate H(next | current)), ``stationary`` (H(current)), ``dest`` (H(next)), ``mutual``
        (dest - rate: the bits about the tile ``lag`` frames ahead that the current tile gives) and ``stay`` (the share of samples
        that stay on their tile) — bits, averaged over the lattices — and with ``keep_matrix`` the column ``matrix``: lattice 0's
        [n, n] count matrix, source-major, a view into one result array.  ``attrs`` hold ``lag``, ``lag_frames``, ``n_tiles``
        and ``users``.  A window without a pooled sample is NaN with ``samples`` 0 — returned, never raised.  Raises
        ``ValidationError`` before data is loaded and for samples outside [0, 1], ``ValueError`` for an illegal ``window`` /
        ``stride`` / ``lag``."""
        times, names, call = self._row_call("transition_markov")
        lag = _native.Plan._pair_lag(lag, len(times))
        n_pairs = len(times) - lag
        window, stride = self._window_args(n_pairs if window is None else window, stride, n_pairs)
        res = call(window=window, stride=stride, lag=lag, want_matrix=bool(keep_matrix), check=False)
        if res["code"] == _native.VET_ERR_RANGE:
            raise ValidationError("Normalized coordinates must be between 0 and 1")
        rate, stationary, dest, mutual, stay = res["stats"]
        first = np.arange(len(rate), dtype=np.int64) * stride
        pair_time = np.asarray(times)[lag:]
        cols = {"time": pair_time[first], "time_end": pair_time[first + window - 1], "samples": res["samples"], "rate": rate,
                "stationary": stationary, "dest": dest, "mutual": mutual, "stay": stay}
        if keep_matrix:
            m_col = np.empty(len(rate), dtype=object)
            for r in range(len(rate)):
                m_col[r] = res["matrix"][r]
            cols["matrix"] = m_col
        df = pd.DataFrame(cols)
        df.attrs.update(lag=lag, lag_frames=lag, n_tiles=len(self._fibonacci_vectors[self.config.tile_counts[0]]), users=list(names))
        return df

    def _frame_present(self) -> np.ndarray:
        if self._present is None:
            self._present = self._prior_frame_present(*self._present_samples)
        return self._present
