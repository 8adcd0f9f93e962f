"""Shared analyzer shell: ingest, plan cache, visualisation outputs, run_analysis.

Mirrors the reference's analyzer classes (analyzers/spatial_entropy.py:40-253,
analyzers/transition_entropy.py) — same constructor, methods, cached attributes, output file
names and error conventions — with ``compute_entropy`` replaced by one call into the HIP
engine per video.
"""

from __future__ import annotations

import logging
import os
import time
from datetime import datetime
from pathlib import Path
from collections.abc import Mapping
from typing import Dict, List, Optional

import numpy as np
import pandas as pd

from .. import _ingest, _native, _quantiser
from ..config import AnalyzerConfig, DEFAULT_OUTPUT_FORMATS
from ..data_types import Vector, ValidationError
from ..utilities.data_utils import format_trajectory_data, generate_fibonacci_lattice
from ..utilities.visualization_utils import save_graph


class _DataCache(dict):
    """``{'trajectory_data', 'points', 'vectors'}`` of the reference, every entry built on first
    access from the cleaned samples (the engine itself only needs the dense arrays)."""

    def __init__(self, samples, width, height):
        super().__init__()
        self._samples, self._dims = samples, (width, height)
        self._lazy = {"trajectory_data", "points", "vectors"}
        self.user_vectors = False

    def _fill(self, key):
        if "trajectory_data" in self._lazy:
            self._lazy.discard("trajectory_data")
            dict.__setitem__(self, "trajectory_data",
                             [(name, _ingest.frame_of_samples(labels, t, a, b, *self._dims))
                              for labels, t, a, b, name in self._samples])
        if key != "trajectory_data" and key in self._lazy:
            self._lazy -= {"points", "vectors"}
            copies = [(name, df.copy()) for name, df in dict.__getitem__(self, "trajectory_data")]
            points, vectors = format_trajectory_data(copies)
            dict.__setitem__(self, "points", points)
            dict.__setitem__(self, "vectors", vectors)

    def __getitem__(self, key):
        if key in self._lazy:
            self._fill(key)
        return dict.__getitem__(self, key)

    def __setitem__(self, key, value):
        self._lazy.discard(key)
        if key == "vectors":
            self.user_vectors = True      # caller replaced the frame table: honour it
        dict.__setitem__(self, key, value)

    def get(self, key, default=None):
        try:
            return self[key]
        except KeyError:
            return default

    def __contains__(self, key):
        return key in self._lazy or dict.__contains__(self, key)

    def __bool__(self):
        return True

    def keys(self):
        return list(dict.keys(self)) + sorted(self._lazy)


class _EntropyAnalyzerBase:
    _logger = logging.getLogger(__name__)

    def __init__(self, config: Optional[AnalyzerConfig] = None):
        self.config = config or AnalyzerConfig()
        self.plot_manager = None          # matplotlib scatter animation is outside this engine
        self._data_cache: dict = {}
        self._entropy_results: Optional[pd.DataFrame] = None
        self._fibonacci_vectors: Dict[int, List[Vector]] = {
            count: generate_fibonacci_lattice(count) for count in self.config.tile_counts
        }
        self._dense = None                # (frame_times[T], mu[T,U], mv[T,U], user names)
        self._plan: Optional[_native.Plan] = None
        self._plan_key = None
        self.last_timing: Dict[str, float] = {}   # seconds / rates of the last ingest and compute

    # ------------------------------------------------------------------ ingest
    def process_directory(self, directory: Path) -> None:
        """Reads every ``*.csv`` of ``directory`` (one user each, in glob order)."""
        directory = Path(directory)
        if not directory.exists():
            raise FileNotFoundError(f"Directory not found: {directory}")
        t_start = time.perf_counter()
        try:
            files = list(directory.glob("*.csv"))          # glob order = user (column) order, as in the reference
            samples = _ingest.read_directory(files, self.config.video_width, self.config.video_height)
            times, mu, mv = _ingest.build_dense([(t, a, b) for _, t, a, b, _ in samples])
            self._dense = (times, mu, mv, [name for *_, name in samples])
            self._data_cache = _DataCache(samples, self.config.video_width, self.config.video_height)
            self._entropy_results = None
            self.last_timing = {"ingest_s": time.perf_counter() - t_start}
        except Exception as e:  # noqa: BLE001
            self._logger.error(f"Error processing directory {directory}: {str(e)}")
            raise ValidationError(f"Failed to process directory: {str(e)}")

    def load_arrays(self, frame_times: np.ndarray, mu: np.ndarray, mv: np.ndarray,
                    user_names: Optional[List[str]] = None) -> None:
        """Engine-native ingest: dense frame-major arrays (NaN = absent) instead of CSV files.

        This IS the ingest step, so the ingest's checks are made here and in the reference's order
        (process_viewport_data, data_utils.py:322-331: 2dmu range, 2dmv range, video dimensions): a sample outside
        [0, 1] raises ``ValidationError`` now, as ``process_directory`` would, and never competes with a compute-time
        error (an empty frame) of ``compute_entropy`` — whichever row either sits in."""
        mu = np.ascontiguousarray(mu, dtype=np.float64)
        mv = np.ascontiguousarray(mv, dtype=np.float64)
        if mu.ndim != 2 or mu.shape != mv.shape or len(frame_times) != mu.shape[0]:
            raise ValidationError("frame_times[T], mu[T,U], mv[T,U] expected")
        _ingest.check_normalized(mu, self.config.video_width)       # NaN = absent passes
        _ingest.check_normalized(mv, self.config.video_height)
        _ingest.check_video_dimensions(self.config.video_width, self.config.video_height)
        names = list(user_names) if user_names is not None else [f"user{u:03d}" for u in range(mu.shape[1])]
        self._dense = (np.asarray(frame_times, dtype=np.float64), mu, mv, names)
        self._data_cache = {"dense": True}
        self._entropy_results = None

    # ------------------------------------------------------------------ engine
    def _get_plan(self, dir_table: Optional[np.ndarray] = None) -> "_native.Plan":
        ec = self.config.entropy_config
        fp64 = getattr(self, "_fp64", False)        # SpatialEntropyAnalyzer(..., fp64=True)
        key = (tuple(self.config.tile_counts), self.config.video_width, self.config.video_height,
               ec.fov_angle, ec.power_factor, ec.use_weight_distribution, dir_table is None, fp64)
        if dir_table is not None or self._plan is None or self._plan_key != key:
            tiles = [np.array([[v.x, v.y, v.z] for v in self._fibonacci_vectors[c]], dtype=np.float64)
                     for c in self.config.tile_counts]
            plan = _native.Plan(_native.Engine.default(), tiles, ec.fov_angle, ec.power_factor,
                                ec.use_weight_distribution, self.config.video_width, self.config.video_height,
                                dir_table=dir_table)
            if fp64:
                plan.set_fp64(True)
            if dir_table is not None:
                return plan
            self._plan, self._plan_key = plan, key
        return self._plan

    def _samples(self):
        """Dense samples for the engine: ('grid', times, mu, mv, names) from this analyzer's own
        ingest, or ('ids', times, ids, table, names) for a hand-assigned ``_data_cache['vectors']``."""
        if not self._data_cache:
            raise ValidationError("No data available. Call process_directory first.")
        if self._dense is not None and not getattr(self._data_cache, "user_vectors", False):
            times, mu, mv, names = self._dense
            return "grid", times, mu, mv, names
        vectors_df = self._data_cache["vectors"]
        names = [c for c in vectors_df.columns if c != "time"]
        table: Dict[Vector, int] = {}
        ids = np.full((len(vectors_df), len(names)), -1, dtype=np.int32)
        for j, name in enumerate(names):
            for i, v in enumerate(vectors_df[name]):
                if v is not None:
                    ids[i, j] = table.setdefault(v, len(table))
        xyz = np.array([[v.x, v.y, v.z] for v in table], dtype=np.float64).reshape(-1, 3)
        return "ids", vectors_df["time"].to_numpy(dtype=np.float64), ids, xyz, names

    def _grid_plan(self) -> "_native.Plan":
        """The cached plan of this analyzer's own (mu, mv) samples."""
        return self._get_plan()

    def _row_call(self, method: str, on_empty=None):
        """One row call of the engine on the cached data.  Returns ``(times, names, call)``: ``call(**kwargs)`` runs
        ``Plan.<method>`` on the samples — through the cached plan, or for hand-assigned vectors a temporary ``dir_table`` plan
        — and returns its result dict.  Samples outside [0, 1] raise ``ValidationError``; rows without a sample (windowed calls
        only) raise ``on_empty(kind, a, b, kwargs)``, the samples as ``_samples`` names them and the arguments of the call."""
        kind, times, a, b, names = self._samples()

        def call(**kwargs):
            try:
                if kind == "grid":
                    return getattr(self._grid_plan(), method)(mu=a, mv=b, **kwargs)
                plan = self._get_plan(dir_table=b)
                try:
                    return getattr(plan, method)(ids=a, **kwargs)
                finally:
                    plan.close()
            except _native.NativeError as e:
                if e.code == _native.VET_ERR_RANGE:
                    raise ValidationError(str(e))
                if e.code == _native.VET_ERR_EMPTY and on_empty is not None:
                    raise on_empty(kind, a, b, kwargs)
                raise

        return times, names, call

    # ------------------------------------------------------------------ outputs
    def create_visualization(self, base_name: str) -> None:
        """Writes ``{base_name}_graph.png`` and ``{base_name}.csv`` (columns time, entropy).

        The reference's per-frame scatter animation / mp4 is not produced here; its GPU-rendered
        counterpart is opt-in: ``render_heatmaps`` / ``save_heatmaps`` of ``SpatialEntropyAnalyzer`` and
        ``TransitionEntropyAnalyzer``."""
        if self._entropy_results is None:
            raise ValidationError("No entropy results. Call compute_entropy first.")
        try:
            save_graph(entropy_values=self._entropy_results["entropy"], time_values=self._entropy_results["time"],
                       output_path=self.config.get_output_path(f"{base_name}_graph", DEFAULT_OUTPUT_FORMATS["plot"]),
                       config=self.config.visualization_config)
            self._entropy_results[["time", "entropy"]].to_csv(
                self.config.get_output_path(base_name, DEFAULT_OUTPUT_FORMATS["data"]), index=False)
        except Exception as e:  # noqa: BLE001
            self._logger.error(f"Error creating visualization: {str(e)}")
            raise RuntimeError(f"Failed to create visualization: {str(e)}")

    def run_analysis(self, directory: Path, output_prefix: str = "") -> None:
        """process_directory -> compute_entropy -> create_visualization; logs and re-raises."""
        try:
            directory = Path(directory)
            self.process_directory(directory)
            self.compute_entropy()
            timestamp = datetime.now().strftime("%Y%m%d_%H%M%S")
            base_name = f"{directory.stem}_{output_prefix}_{timestamp}"
            self.create_visualization(base_name)
            self._logger.info(f"Analysis completed successfully: {base_name}")
        except Exception as e:  # noqa: BLE001
            self._logger.error(f"Analysis failed: {str(e)}")
            raise

    def _record_compute(self, seconds: float, n_samples: int, n_rows: int) -> None:
        """Throughput counters of the last engine call (samples/s, frames/s)."""
        self.last_timing.update(compute_s=seconds, samples=float(n_samples), frames=float(n_rows),
                                samples_per_s=n_samples / max(seconds, 1e-12),
                                frames_per_s=n_rows / max(seconds, 1e-12))
        self._logger.info("entropy of %d frames x %d samples in %.3f ms (%.3g samples/s)", n_rows, n_samples,
                          seconds * 1e3, n_samples / max(seconds, 1e-12))

    @staticmethod
    def _window_args(window, stride, n_frames: int):
        """(window, stride) as ints; ``ValueError`` unless 1 <= window <= n_frames and stride >= 1."""
        for name, v in (("window", window), ("stride", stride)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"{name} must be an integer number of frames (got {v!r})")
        window, stride = int(window), int(stride)
        if window < 1 or stride < 1:
            raise ValueError(f"window and stride must be at least 1 frame (got window={window}, stride={stride})")
        if window > n_frames:
            raise ValueError(f"window of {window} frames is longer than the data's {n_frames} frames")
        return window, stride

    @staticmethod
    def _user_frame(names, times, window: int, stride: int, res: dict, tile_weights=None) -> pd.DataFrame:
        """The per-viewer result as a DataFrame, user-major: one row per (user, r) in the order of ``res``'s [U][R] arrays."""
        U, R = res["entropy"].shape
        first = np.tile(np.arange(R, dtype=np.int64) * stride, U)
        times = np.asarray(times)
        cols = {
            "user": np.repeat(np.asarray(list(names), dtype=object), R),
            "time": times[first],
            "time_end": times[first + window - 1],
            "entropy": res["entropy"].reshape(-1),
            "samples": res["samples"].reshape(-1),
        }
        if tile_weights is not None:
            cols["tile_weights"] = tile_weights
        return pd.DataFrame(cols)

    @staticmethod
    def _divergence_frame(names, times, window: int, stride: int, res: dict) -> pd.DataFrame:
        """The pairwise viewer divergence as a DataFrame, one row per window: the ``divergence`` cell of row r is the [U, U] view
        ``res["divergence"][r]`` (no copy), the ``samples`` cell the [U] samples of the row; ``attrs["users"]`` names the
        viewers in matrix order."""
        div = res["divergence"]
        R = div.shape[0]
        first = np.arange(R, dtype=np.int64) * stride
        times = np.asarray(times)
        per_row = np.ascontiguousarray(res["samples"].T)
        d_col, s_col = np.empty(R, dtype=object), np.empty(R, dtype=object)
        for r in range(R):
            d_col[r], s_col[r] = div[r], per_row[r]
        df = pd.DataFrame({"time": times[first], "time_end": times[first + window - 1], "divergence": d_col, "samples": s_col})
        df.attrs["users"] = list(names)
        return df

    @staticmethod
    def _crowd_frame(names, times, window: int, stride: int, res: dict) -> pd.DataFrame:
        """The viewer-to-crowd divergence as a DataFrame, user-major: one row per (user, r) in the order of ``res``'s [U][R]
        arrays; ``attrs["rows"]`` is the per-window DataFrame of the decomposition pooled = within + between,
        ``attrs["users"]`` names the viewers."""
        U, R = res["divergence"].shape
        row_first = np.arange(R, dtype=np.int64) * stride
        first = np.tile(row_first, U)
        times = np.asarray(times)
        df = pd.DataFrame({
            "user": np.repeat(np.asarray(list(names), dtype=object), R),
            "time": times[first],
            "time_end": times[first + window - 1],
            "divergence": res["divergence"].reshape(-1),
            "samples": res["samples"].reshape(-1),
        })
        df.attrs["rows"] = pd.DataFrame({
            "time": times[row_first], "time_end": times[row_first + window - 1],
            "samples": res["samples"].sum(axis=0, dtype=np.int64),
            "pooled": res["rows"][0], "within": res["rows"][1], "between": res["rows"][2],
        })
        df.attrs["users"] = list(names)
        return df

    @staticmethod
    def _lag_args(max_lag, window: int, stride: int, n_frames: int) -> int:
        """max_lag as an int; ``ValueError`` unless 1 <= max_lag <= rows - 1."""
        if isinstance(max_lag, bool) or not isinstance(max_lag, (int, np.integer)):
            raise ValueError(f"max_lag must be an integer number of rows (got {max_lag!r})")
        rows = (n_frames - window) // stride + 1
        if not 1 <= int(max_lag) <= rows - 1:
            raise ValueError(f"max_lag must be between 1 and rows - 1 = {rows - 1} (got {max_lag}; window={window}, "
                             f"stride={stride} give {rows} rows of {n_frames} frames)")
        return int(max_lag)

    @staticmethod
    def _window_divergence_frame(times, window: int, stride: int, res: dict) -> pd.DataFrame:
        """The window-to-window divergence as a DataFrame, one row per window: ``shift`` is the lag-1 value, the ``divergence``
        cell of row r the [L] view ``res["divergence"][r]`` (no copy); ``attrs["lags"]`` / ``attrs["lag_frames"]`` give the lags
        in rows and in frames."""
        div = res["divergence"]
        R, L = div.shape
        first = np.arange(R, dtype=np.int64) * stride
        times = np.asarray(times)
        d_col = np.empty(R, dtype=object)
        for r in range(R):
            d_col[r] = div[r]
        df = pd.DataFrame({"time": times[first], "time_end": times[first + window - 1], "samples": res["samples"],
                           "shift": div[:, 0], "divergence": d_col})
        df.attrs["lags"] = list(range(1, L + 1))
        df.attrs["lag_frames"] = [stride * l for l in range(1, L + 1)]
        return df

    @staticmethod
    def _coverage_args(fractions, max_lag, window: int, stride: int, n_frames: int):
        """(fractions as a tuple of floats, max_lag as an int); ``ValueError`` unless there are 1 to 8 fractions, each a number in
        (0, 1], strictly increasing, and 0 <= max_lag <= rows - 1."""
        if isinstance(fractions, (str, bytes)) or not hasattr(fractions, "__len__"):
            raise ValueError(f"fractions must be a sequence of numbers in (0, 1] (got {fractions!r})")
        vals = list(fractions)
        if not 1 <= len(vals) <= 8:
            raise ValueError(f"need 1 to 8 fractions (got {len(vals)})")
        for v in vals:
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 < float(v) <= 1.0:
                raise ValueError(f"fractions must be numbers in (0, 1] (got {v!r})")
        vals = [float(v) for v in vals]
        if any(b <= a for a, b in zip(vals, vals[1:])):
            raise ValueError(f"fractions must be strictly increasing (got {vals})")
        if isinstance(max_lag, bool) or not isinstance(max_lag, (int, np.integer)):
            raise ValueError(f"max_lag must be an integer number of rows (got {max_lag!r})")
        rows = (n_frames - window) // stride + 1
        if not 0 <= int(max_lag) <= rows - 1:
            raise ValueError(f"max_lag must be between 0 and rows - 1 = {rows - 1} (got {max_lag}; window={window}, "
                             f"stride={stride} give {rows} rows of {n_frames} frames)")
        return tuple(vals), int(max_lag)

    @staticmethod
    def _coverage_frame(times, window: int, stride: int, res: dict, fractions, n_tiles: int) -> pd.DataFrame:
        """The coverage as a DataFrame, one row per window: ``tiles`` is the [Q] view ``res["tiles"][r]``, ``share`` =
        ``tiles / n_tiles`` (a share of the tiles, not of the sphere's area), ``covered`` the [Q] view ``res["hit"][r, 0]``,
        ``forecast`` the [L, Q] view ``res["hit"][r, 1:]`` and, where ``res`` holds it, ``order`` the [n] view
        ``res["order"][r]`` (no copies); ``attrs`` hold ``fractions``, ``lags`` / ``lag_frames`` (lags 1 .. L in rows and in
        frames) and ``n_tiles``."""
        tiles, hit = res["tiles"], res["hit"]
        R, L = hit.shape[0], hit.shape[1] - 1
        first = np.arange(R, dtype=np.int64) * stride
        times = np.asarray(times)
        share = tiles / float(n_tiles)
        names = ["tiles", "share", "covered", "forecast"] + (["order"] if res.get("order") is not None else [])
        cells = {name: np.empty(R, dtype=object) for name in names}
        for r in range(R):
            cells["tiles"][r], cells["share"][r] = tiles[r], share[r]
            cells["covered"][r], cells["forecast"][r] = hit[r, 0], hit[r, 1:]
            if "order" in cells:
                cells["order"][r] = res["order"][r]
        df = pd.DataFrame({"time": times[first], "time_end": times[first + window - 1], "samples": res["samples"], **cells})
        df.attrs.update(fractions=tuple(fractions), lags=list(range(1, L + 1)), lag_frames=[stride * l for l in range(1, L + 1)],
                        n_tiles=int(n_tiles))
        return df

    def _coverage(self, window, stride, fractions, max_lag, keep_order, n_tiles) -> pd.DataFrame:
        """``compute_coverage`` of the two spatial analyzers: the arguments are checked before the engine is touched.
        ``n_tiles()``: the tiles of lattice 0 (asked after the call)."""
        times, names, call = self._row_call("spatial_coverage")
        window, stride = self._window_args(window, stride, len(times))
        fractions, max_lag = self._coverage_args(fractions, max_lag, window, stride, len(times))
        res = call(window=window, stride=stride, max_lag=max_lag, fractions=fractions, want_order=bool(keep_order), check=False)
        if res["code"] == _native.VET_ERR_RANGE:
            raise ValidationError("Normalized coordinates must be between 0 and 1")
        return self._coverage_frame(times, window, stride, res, fractions, n_tiles())

    @staticmethod
    def _bootstrap_args(replicates, confidence, seed):
        """(replicates, confidence, seed) checked; ``ValueError`` unless 1 <= replicates <= 4096 (an integer), 0 < confidence < 1
        and seed is an integer in [0, 2^64)."""
        for name, v in (("replicates", replicates), ("seed", seed)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"{name} must be an integer (got {v!r})")
        if not 1 <= int(replicates) <= 4096:
            raise ValueError(f"replicates must be between 1 and 4096 (got {replicates})")
        if not 0 <= int(seed) < 1 << 64:
            raise ValueError(f"seed must be an unsigned 64-bit integer (got {seed})")
        if isinstance(confidence, bool) or not isinstance(confidence, (int, float, np.integer, np.floating)) \
                or not 0.0 < float(confidence) < 1.0:
            raise ValueError(f"confidence must be a number inside (0, 1) (got {confidence!r})")
        return int(replicates), float(confidence), int(seed)

    @staticmethod
    def _bootstrap_frame(times, window: int, stride: int, point: dict, res: dict, replicates: int, seed: int,
                         confidence: float) -> pd.DataFrame:
        """The bootstrap as a DataFrame, one row per window: ``entropy`` / ``samples`` of the point estimate (``point``: the
        ``spatial_windowed`` result) beside ``mean``, ``sd``, ``lo``, ``hi`` and ``valid`` of the replicates; where ``res`` holds
        the replicates, the ``replicates`` cell of row r is the [B] view ``res["replicates"][r]`` (no copy)."""
        R = len(point["entropy"])
        first = np.arange(R, dtype=np.int64) * stride
        times = np.asarray(times)
        mean, sd, lo, hi = res["summary"]
        cols = {"time": times[first], "time_end": times[first + window - 1], "entropy": point["entropy"],
                "samples": point["samples"], "mean": mean, "sd": sd, "lo": lo, "hi": hi, "valid": res["valid"]}
        if res.get("replicates") is not None:
            r_col = np.empty(R, dtype=object)
            for r in range(R):
                r_col[r] = res["replicates"][r]
            cols["replicates"] = r_col
        df = pd.DataFrame(cols)
        df.attrs.update(replicates=replicates, seed=seed, confidence=confidence)
        return df

    def _entropy_bootstrap(self, window, stride, replicates, confidence, seed, keep_replicates) -> pd.DataFrame:
        """``compute_entropy_bootstrap`` of the two spatial analyzers: the arguments are checked before the engine is touched;
        the point estimate is the existing ``spatial_windowed`` call (rows without a sample are NaN here, not an error)."""
        times, names, point_call = self._row_call("spatial_windowed")
        _, _, boot_call = self._row_call("spatial_bootstrap")
        window, stride = self._window_args(window, stride, len(times))
        replicates, confidence, seed = self._bootstrap_args(replicates, confidence, seed)
        point = point_call(window=window, stride=stride, check=False)
        if point["code"] == _native.VET_ERR_RANGE:
            raise ValidationError("Normalized coordinates must be between 0 and 1")
        res = boot_call(window=window, stride=stride, replicates=replicates, seed=seed, confidence=confidence,
                        want_replicates=bool(keep_replicates))
        return self._bootstrap_frame(times, window, stride, point, res, replicates, seed, confidence)

    @staticmethod
    def _group_labels(groups, names):
        """(int8 [U] of 0 / 1 / -1 in the order of ``names``, (label A, label B)) from ``groups``: a sequence aligned with
        ``names`` or a mapping from user name to label (a user it does not name is excluded).  ``None`` / NaN is excluded; there
        must be exactly two distinct other labels, in sorted order the first is audience A.  ``ValueError`` otherwise."""
        names = list(names)
        if isinstance(groups, Mapping):
            unknown = [k for k in groups if k not in set(names)]
            if unknown:
                raise ValueError(f"groups names users that are not loaded: {unknown[:5]}")
            labels = [groups.get(name) for name in names]
        else:
            if groups is None or isinstance(groups, (str, bytes)) or not hasattr(groups, "__len__"):
                raise ValueError("groups must be a sequence aligned with the users, or a mapping from user name to label")
            labels = list(groups)
            if len(labels) != len(names):
                raise ValueError(f"groups has {len(labels)} entries for {len(names)} users")

        def missing(v):
            return v is None or (isinstance(v, (float, np.floating)) and np.isnan(v))

        try:
            distinct = sorted({v for v in labels if not missing(v)})
        except TypeError:
            raise ValueError("the group labels cannot be ordered (mixed types)")
        if len(distinct) != 2:
            raise ValueError(f"need exactly two distinct group labels (got {distinct[:5]})")
        code = np.array([-1 if missing(v) else distinct.index(v) for v in labels], dtype=np.int8)
        return code, (distinct[0], distinct[1])

    @staticmethod
    def _group_frame(times, names, window: int, stride: int, code, labels, res: dict, permutations: int, seed: int,
                     confidence: float) -> pd.DataFrame:
        """The permutation test as a DataFrame, one row per window; where ``res`` holds the null distribution, the ``null`` cell
        of row r is the [P] view ``res["null"][r]`` (no copy)."""
        observed, p_value, p_adjusted, null_mean, null_crit = res["summary"]
        R = len(observed)
        first = np.arange(R, dtype=np.int64) * stride
        times = np.asarray(times)
        cols = {"time": times[first], "time_end": times[first + window - 1], "samples_a": res["samples"][0],
                "samples_b": res["samples"][1], "divergence": observed, "p_value": p_value, "p_adjusted": p_adjusted,
                "null_mean": null_mean, "null_crit": null_crit, "valid": res["valid"]}
        if res.get("null") is not None:
            n_col = np.empty(R, dtype=object)
            for r in range(R):
                n_col[r] = res["null"][r]
            cols["null"] = n_col
        df = pd.DataFrame(cols)
        names = list(names)
        df.attrs.update(groups=labels, sizes=(int((code == 0).sum()), int((code == 1).sum())),
                        users=([n for n, c in zip(names, code) if c == 0], [n for n, c in zip(names, code) if c == 1]),
                        permutations=permutations, seed=seed, confidence=confidence)
        return df

    def _group_divergence(self, groups, window, stride, permutations, confidence, seed, keep_null) -> pd.DataFrame:
        """``compute_group_divergence`` of the two spatial analyzers: the arguments are checked before the engine is touched."""
        times, names, call = self._row_call("spatial_group_divergence")
        code, labels = self._group_labels(groups, names)
        window, stride = self._window_args(len(times) if window is None else window, stride, len(times))
        try:
            permutations, confidence, seed = self._bootstrap_args(permutations, confidence, seed)
        except ValueError as e:
            raise ValueError(str(e).replace("replicates", "permutations"))
        res = call(groups=code, window=window, stride=stride, permutations=permutations, seed=seed, confidence=confidence,
                   want_null=bool(keep_null), check=False)
        if res["code"] == _native.VET_ERR_RANGE:
            raise ValidationError("Normalized coordinates must be between 0 and 1")
        return self._group_frame(times, names, window, stride, code, labels, res, permutations, seed, confidence)

    @staticmethod
    def _motion_args(quantiles, bins_deg):
        """(quantiles as a tuple of floats, bins_deg as a tuple of floats or None); ``ValueError`` unless there are at most 8
        quantiles, each a number in [0, 1], strictly increasing, and 2 to 65 finite, strictly ascending bin edges in degrees."""
        def numbers(values, what):
            if values is None or isinstance(values, (str, bytes)) or not hasattr(values, "__len__"):
                raise ValueError(f"{what} must be a sequence of numbers (got {values!r})")
            vals = list(values)
            for v in vals:
                if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
                    raise ValueError(f"{what} must be finite numbers (got {v!r})")
            return [float(v) for v in vals]
        q = numbers(() if quantiles is None else quantiles, "quantiles")
        if len(q) > 8:
            raise ValueError(f"need at most 8 quantiles (got {len(q)})")
        if any(not 0.0 <= v <= 1.0 for v in q):
            raise ValueError(f"quantiles must be numbers in [0, 1] (got {q})")
        if any(b <= a for a, b in zip(q, q[1:])):
            raise ValueError(f"quantiles must be strictly increasing (got {q})")
        if bins_deg is None:
            return tuple(q), None
        e = numbers(bins_deg, "bins_deg")
        if not 2 <= len(e) <= 65:
            raise ValueError(f"need 2 to 65 bin edges, 1 to 64 bins (got {len(e)})")
        if any(b <= a for a, b in zip(e, e[1:])):
            raise ValueError(f"bins_deg must be strictly ascending (got {e})")
        return tuple(q), tuple(e)

    @staticmethod
    def _motion_frame(times, names, window: int, stride: int, lag: int, per_user: bool, res: dict, quantiles, bins_deg) -> pd.DataFrame:
        """The head-motion statistics as a DataFrame in DEGREES, one row per window (``per_user``: per (user, window), user-major,
        ``user`` first): the ``quantiles`` cell of a row is the [Q] view of its quantiles and, where ``res`` holds it, ``hist`` the
        [B] view ``res["hist"][row]`` (no copy of the counts).  ``times``: every frame's time; a pair's time is its later frame's."""
        times = np.asarray(times)
        stats = np.degrees(np.asarray(res["stats"], dtype=np.float64)).reshape(4, -1)
        samples, still = np.asarray(res["samples"]).reshape(-1), np.asarray(res["still"]).reshape(-1)
        rows = len(samples)
        R = rows // len(names) if per_user else rows
        first = np.arange(R, dtype=np.int64) * stride
        if per_user:
            first = np.tile(first, len(names))
        pair_time = times[lag:]
        cols = {}
        if per_user:
            cols["user"] = np.repeat(np.asarray(list(names), dtype=object), R)
        with np.errstate(invalid="ignore", divide="ignore"):
            share = np.where(samples > 0, still / np.maximum(samples, 1), np.nan)
        cols.update(time=pair_time[first], time_end=pair_time[first + window - 1], samples=samples, still=still, still_share=share,
                    mean=stats[0], sd=stats[1], max=stats[2], total=stats[3])
        q_deg = np.degrees(res["quantiles"]).reshape(rows, -1) if res.get("quantiles") is not None else np.empty((rows, 0))
        q_col = np.empty(rows, dtype=object)
        for r in range(rows):
            q_col[r] = q_deg[r]
        cols["quantiles"] = q_col
        if res.get("hist") is not None:
            hist = np.asarray(res["hist"]).reshape(rows, -1)
            h_col = np.empty(rows, dtype=object)
            for r in range(rows):
                h_col[r] = hist[r]
            cols["hist"] = h_col
        df = pd.DataFrame(cols)
        steps = times[lag:] - times[:-lag]
        df.attrs.update(lag=lag, lag_frames=lag, quantiles=tuple(quantiles), bins_deg=None if bins_deg is None else tuple(bins_deg),
                        users=list(names), pair_seconds=float(np.median(steps)) if len(steps) else float("nan"))
        return df

    def compute_head_motion(self, window: Optional[int] = None, stride: int = 1, lag: int = 1, per_user: bool = False,
                            quantiles=(0.5, 0.9, 0.99), bins_deg=None) -> pd.DataFrame:
        """How fast heads turn: pair f is (frame f, frame f + lag); a (pair, viewer) with a sample in both frames is a sample, its
        angle the great-circle angle between the two viewing directions (the reference's ``vector_angle_distance``; exactly 0 for
        two samples with the same Vector, which count as ``still``).  Row r pools the samples of the pairs
        [r * stride, r * stride + window) over all viewers, or with ``per_user`` each viewer's own.  ``window`` and ``stride``
        count pairs; ``window=None`` is the whole video.  Independent of the tiling.

        Uses the data ``process_directory`` cached.  Returns a new DataFrame in DEGREES (``compute_entropy``'s results are left
        alone), one row per window — user-major with ``user`` first when ``per_user``: ``time`` / ``time_end`` (the later frame of
        the row's first / last pair), ``samples``, ``still``, ``still_share``, ``mean``, ``sd`` (ddof = 1), ``max``, ``total`` (the
        path travelled), ``quantiles`` (a [Q] view: linear interpolation between exact order statistics) and, with ``bins_deg``
        (ascending edges in degrees, half-open bins), ``hist`` (a [B] view of counts).  ``attrs`` hold ``lag``, ``lag_frames``,
        ``quantiles``, ``bins_deg``, ``users`` and ``pair_seconds`` (the median of time[f + lag] - time[f]): degrees per second is
        one division.  A window without a sample is NaN with ``samples`` 0 — returned, never raised.  Raises ``ValidationError``
        before data is loaded and for samples outside [0, 1], ``ValueError`` for an illegal ``window`` / ``stride`` / ``lag`` /
        ``quantiles`` / ``bins_deg``."""
        times, names, call = self._row_call("head_motion")
        lag = _native.Plan._pair_lag(lag, len(times))
        n_pairs = len(times) - lag
        window, stride = self._window_args(n_pairs if window is None else window, stride, n_pairs)
        quantiles, bins_deg = self._motion_args(quantiles, bins_deg)
        res = call(window=window, stride=stride, lag=lag, per_user=bool(per_user), quantiles=quantiles,
                   edges=None if bins_deg is None else np.radians(bins_deg), check=False)
        if res["code"] == _native.VET_ERR_RANGE:
            raise ValidationError("Normalized coordinates must be between 0 and 1")
        return self._motion_frame(times, names, window, stride, lag, bool(per_user), res, quantiles, bins_deg)

    @staticmethod
    def _dispersion_frame(times, names, window: int, stride: int, per_user: bool, res: dict, bins_deg) -> pd.DataFrame:
        """The dispersion statistics as a DataFrame in DEGREES, one row per window (``per_user``: per (user, window), user-major,
        ``user`` first): ``center`` of a row is the [3] view of its mean direction (NaN where the centroid is zero) and, where
        ``res`` holds it, ``hist`` the [B] view ``res["hist"][row]`` (no copy of the counts)."""
        times = np.asarray(times)
        stats = np.degrees(np.asarray(res["stats"], dtype=np.float64)).reshape(3, -1)
        counts = np.asarray(res["counts"]).reshape(4, -1)
        samples, same, present = counts[0], counts[1], counts[3]
        centroid = np.asarray(res["centroid"], dtype=np.float64).reshape(-1, 3)
        rows = len(samples)
        R = rows // len(names) if per_user else rows
        first = np.arange(R, dtype=np.int64) * stride
        if per_user:
            first = np.tile(first, len(names))
        cols = {}
        if per_user:
            cols["user"] = np.repeat(np.asarray(list(names), dtype=object), R)
        length = np.sqrt((centroid * centroid).sum(axis=1))
        with np.errstate(invalid="ignore", divide="ignore"):
            share = np.where(samples > 0, same / np.maximum(samples, 1), np.nan)
            resultant = np.where(present > 0, np.minimum(length / np.maximum(present, 1), 1.0), np.nan)
            center = np.where(length[:, None] > 0, centroid / length[:, None], np.nan)
        c_col = np.empty(rows, dtype=object)
        for r in range(rows):
            c_col[r] = center[r]
        cols.update(time=times[first], time_end=times[first + window - 1], samples=samples, same=same, same_share=share,
                    mean=stats[0], max=stats[1], nearest=stats[2], present=present, resultant=resultant, center=c_col)
        if res.get("hist") is not None:
            hist = np.asarray(res["hist"]).reshape(rows, -1)
            h_col = np.empty(rows, dtype=object)
            for r in range(rows):
                h_col[r] = hist[r]
            cols["hist"] = h_col
        df = pd.DataFrame(cols)
        df.attrs.update(bins_deg=None if bins_deg is None else tuple(bins_deg), users=list(names), window=window, stride=stride)
        return df

    def compute_dispersion(self, window: Optional[int] = 1, stride: int = 1, per_user: bool = False, bins_deg=None) -> pd.DataFrame:
        """How tightly the audience looks together: a pair sample is two viewers present in the same frame, its angle the
        great-circle angle between their viewing directions (the reference's ``vector_angle_distance``; exactly 0 for two samples
        with the same Vector, which count as ``same``).  Row r pools the pair samples of the frames
        [r * stride, r * stride + window), or with ``per_user`` holds them from each viewer's own side.  ``window`` and ``stride``
        count frames; ``window=None`` is the whole video.  Independent of the tiling.

        Uses the data ``process_directory`` cached.  Returns a new DataFrame in DEGREES (``compute_entropy``'s results are left
        alone), one row per window — user-major with ``user`` first when ``per_user``: ``time`` / ``time_end`` (the first / last
        frame of the row), ``samples`` (pairs; per viewer: partners), ``same``, ``same_share``, ``mean``, ``max`` (the audience's
        angular diameter; per viewer: the farthest partner), ``nearest`` (the mean angle to the nearest partner: small for a
        clustered crowd), ``present``, ``resultant`` (the length of the mean unit vector, in [0, 1]: 1 = everybody looks one way;
        per viewer: the viewer stays put), ``center`` (a [3] unit-vector view of the mean direction, NaN where it is undefined)
        and, with ``bins_deg`` (ascending edges in degrees, half-open bins; pooled only), ``hist`` (a [B] view of counts).
        ``attrs`` hold ``bins_deg``, ``users``, ``window`` and ``stride``.  A window that never has two viewers in one frame is
        NaN with ``samples`` 0 — returned, never raised.  Raises ``ValidationError`` before data is loaded and for samples outside
        [0, 1], ``ValueError`` for an illegal ``window`` / ``stride`` / ``bins_deg`` and for ``per_user`` with ``bins_deg``."""
        times, names, call = self._row_call("dispersion")
        window, stride = self._window_args(len(times) if window is None else window, stride, len(times))
        _, bins_deg = self._motion_args((), bins_deg)
        if per_user and bins_deg is not None:
            raise ValueError("bins_deg: the per-viewer layout has no histogram (pass bins_deg=None with per_user)")
        res = call(window=window, stride=stride, per_user=bool(per_user), edges=None if bins_deg is None else np.radians(bins_deg),
                   check=False)
        if res["code"] == _native.VET_ERR_RANGE:
            raise ValidationError("Normalized coordinates must be between 0 and 1")
        return self._dispersion_frame(times, names, window, stride, bool(per_user), res, bins_deg)

    CLUSTER_KEEP_LIMIT = 4 << 30     # bytes of per-viewer arrays that compute_viewer_clusters(keep_*=True) hands back at most

    @staticmethod
    def _clusters_frame(times, names, window: int, stride: int, res: dict, threshold_deg: float, min_share: float,
                        fractions) -> pd.DataFrame:
        """The viewer clusters as a DataFrame, one row per window; ``streams``, ``labels``, ``sizes``, ``centroids`` and
        ``links_bits`` of a row are views into the result arrays (no copy)."""
        times = np.asarray(times)
        counts = np.asarray(res["counts"]).reshape(5, -1)
        stats = np.asarray(res["stats"], dtype=np.float64).reshape(3, -1)
        R, U = counts.shape[1], len(names)
        first = np.arange(R, dtype=np.int64) * stride

        def views(a, shape):
            a = np.asarray(a).reshape((R,) + shape)
            col = np.empty(R, dtype=object)
            for r in range(R):
                col[r] = a[r]
            return col
        cols = dict(time=times[first], time_end=times[first + window - 1], viewers=counts[0], clusters=counts[1], largest=counts[2],
                    largest_share=stats[2], singletons=counts[3], links=counts[4], entropy=stats[0], entropy_norm=stats[1])
        top = res.get("top")
        cols["streams"] = views(top if top is not None else np.empty((R, 0), dtype=np.int32), (len(fractions),))
        if res.get("labels") is not None:
            cols["labels"] = views(res["labels"], (U,))
            cols["sizes"] = views(res["sizes"], (U,))
        if res.get("centroids") is not None:
            cols["centroids"] = views(res["centroids"], (U, 3))
        if res.get("links") is not None:
            cols["links_bits"] = views(res["links"], (U, (U + 63) // 64))
        df = pd.DataFrame(cols)
        df.attrs.update(threshold_deg=float(threshold_deg), cos_threshold=float(res["cos_threshold"]), min_share=float(min_share),
                        fractions=tuple(fractions), window=window, stride=stride, users=list(names))
        return df

    def compute_viewer_clusters(self, window: Optional[int] = 1, stride: int = 1, threshold_deg: float = 30.0, min_share: float = 1.0,
                                fractions=(0.5, 0.8, 0.95), keep_labels: bool = True, keep_centroids: bool = False,
                                keep_links: bool = False) -> pd.DataFrame:
        """Who looks together: in a frame two present viewers are near when the great-circle angle between their viewing directions
        is at most ``threshold_deg``; in the window of frames [r * stride, r * stride + window) two viewers are linked when they
        are near in at least ``min_share`` of the frames both are in (1.0: whenever both are there, the segment rule of the
        clustering literature), and the window's clusters are the connected components of the linked viewers: the groups that
        could share one viewport stream.  A viewer without a link is a cluster of one.  ``window`` and ``stride`` count frames;
        ``window=None`` is the whole video.  Independent of the tiling.  ``threshold_deg = 30.0`` is a choice for head-direction
        data, not taken from the reference, which has no such call.

        Uses the data ``process_directory`` cached.  Returns a new DataFrame, one row per window: ``time`` / ``time_end`` (the
        first / last frame of the row), ``viewers`` (present in at least one frame), ``clusters``, ``largest``,
        ``largest_share``, ``singletons``, ``links`` (linked pairs), ``entropy`` (of the partition, bits), ``entropy_norm``
        (over log2 viewers), ``streams`` (a [Q] view: the fewest clusters, largest first, that hold ``fractions[i]`` of the
        viewers) and, with ``keep_labels``, ``labels`` (a [U] view in the analyzer's user order: clusters are numbered by their
        first member, -1 = not in the window) and ``sizes`` (a [U] view: the members of cluster k); with ``keep_centroids``,
        ``centroids`` (a [U, 3] view: the sum of the members' unit vectors per cluster; divide by its norm for the direction);
        with ``keep_links``, ``links_bits`` (a [U, ceil(U / 64)] uint64 view: bit v of row u).  ``attrs`` hold ``threshold_deg``,
        ``cos_threshold`` (what decided the links), ``min_share``, ``fractions``, ``window``, ``stride`` and ``users``.  A window
        without a viewer has labels -1, zero counts and NaN statistics — returned, never raised.  Raises ``ValidationError``
        before data is loaded and for samples outside [0, 1], ``ValueError`` for illegal arguments and for kept arrays beyond
        4 GiB; more than 8192 viewers are refused by the engine (``NativeError``, VET_ERR_UNSUPPORTED)."""
        times, names, call = self._row_call("viewer_clusters")
        window, stride = self._window_args(len(times) if window is None else window, stride, len(times))
        if fractions is None or isinstance(fractions, (str, bytes)) or not hasattr(fractions, "__len__"):
            raise ValueError(f"fractions must be a sequence of numbers in (0, 1] (got {fractions!r})")
        fractions = tuple(fractions)
        _native.Plan._cluster_args(threshold_deg, min_share, fractions)
        U, R = len(names), (len(times) - window) // stride + 1
        kept = R * U * ((8 if keep_labels else 0) + (24 if keep_centroids else 0) + (((U + 63) // 64) * 8 if keep_links else 0))
        if kept > self.CLUSTER_KEEP_LIMIT:
            raise ValueError(f"{R} rows of {U} viewers keep {kept / 2 ** 30:.1f} GiB of labels, centroids and link bits, beyond 4 GiB: "
                             "use a larger stride, or keep_labels=False, keep_centroids=False, keep_links=False")
        res = call(window=window, stride=stride, threshold_deg=float(threshold_deg), min_share=float(min_share), fractions=fractions,
                   want_labels=bool(keep_labels), want_centroids=bool(keep_centroids), want_links=bool(keep_links), check=False)
        if res["code"] == _native.VET_ERR_RANGE:
            raise ValidationError("Normalized coordinates must be between 0 and 1")
        return self._clusters_frame(times, names, window, stride, res, float(threshold_deg), float(min_share), fractions)

    FIXATION_MAX_STEP_DEG = 2.0      # the defaults of compute_fixations: choices for head-direction data on the default grid
    FIXATION_MIN_FRAMES = 5

    @staticmethod
    def _fixation_step_args(max_step_deg, velocity_deg_s, min_frames, min_seconds, frame_seconds: float):
        """(max_step_deg, min_frames) as the engine takes them.  ``velocity_deg_s`` replaces ``max_step_deg`` (step = velocity *
        frame_seconds) and ``min_seconds`` replaces ``min_frames`` (max(1, ceil(min_seconds / frame_seconds))); ``ValueError`` when
        both of a pair are given (the frame-based one moved off its default), for a value that is not a finite number >= 0 (seconds:
        > 0) and for a seconds-based value on data without a frame period."""
        def number(v, what, positive):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v < 0 or \
                    (positive and v <= 0):
                raise ValueError(f"{what} must be a finite number {'above' if positive else 'of at least'} 0 (got {v!r})")
            return float(v)

        def period(what):
            if not np.isfinite(frame_seconds) or frame_seconds <= 0:
                raise ValueError(f"{what} needs frame times that advance (the median frame period is {frame_seconds!r})")
        base = _EntropyAnalyzerBase
        if velocity_deg_s is not None:
            if max_step_deg is not None and max_step_deg != base.FIXATION_MAX_STEP_DEG:
                raise ValueError("give max_step_deg or velocity_deg_s, not both")
            period("velocity_deg_s")
            max_step_deg = number(velocity_deg_s, "velocity_deg_s", False) * float(frame_seconds)
        if min_seconds is not None:
            if min_frames is not None and min_frames != base.FIXATION_MIN_FRAMES:
                raise ValueError("give min_frames or min_seconds, not both")
            period("min_seconds")
            min_frames = max(1, int(np.ceil(number(min_seconds, "min_seconds", True) / float(frame_seconds))))
        return max_step_deg, min_frames

    @staticmethod
    def _fixation_bins(bins_frames):
        """bins_frames as a tuple of ints or None; ``ValueError`` unless they are 2 to 65 integers >= 1, strictly ascending."""
        if bins_frames is None:
            return None
        e = _native.Plan._fixation_args(0.0, 1, bins_frames)[2]
        return tuple(int(v) for v in e)

    @staticmethod
    def _fixation_frame(times, names, window: int, stride: int, per_user: bool, res: dict, by: str, max_step_deg: float,
                        min_frames: int, bins_frames) -> pd.DataFrame:
        """The fixation (or dwell) statistics as a DataFrame, one row per window (``per_user``: per (user, window), user-major,
        ``user`` first); where ``res`` holds them, ``hist`` of a row is the [B] view ``res["hist"][row]``, ``attrs["labels"]`` the
        [T, U] transposed view of the labels and ``attrs["events"]`` the event list as a DataFrame (no copy of the arrays)."""
        times = np.asarray(times, dtype=np.float64)
        counts = np.asarray(res["counts"]).reshape(5, -1)
        samples, fix, events, sum_len, max_len = counts
        rows = counts.shape[1]
        R = rows // len(names) if per_user else rows
        first = np.arange(R, dtype=np.int64) * stride
        if per_user:
            first = np.tile(first, len(names))
        steps = np.diff(times)
        frame_seconds = float(np.median(steps)) if len(steps) else float("nan")
        cols = {}
        if per_user:
            cols["user"] = np.repeat(np.asarray(list(names), dtype=object), R)
        with np.errstate(invalid="ignore", divide="ignore"):
            share = np.where(samples > 0, fix / np.maximum(samples, 1), np.nan)
            mean = np.where(events > 0, sum_len / np.maximum(events, 1), np.nan)
        cols.update(time=times[first], time_end=times[first + window - 1], samples=samples, fix_frames=fix, fix_share=share,
                    events=events, mean_frames=mean, max_frames=max_len, mean_seconds=mean * frame_seconds)
        if res.get("hist") is not None:
            hist = np.asarray(res["hist"]).reshape(rows, -1)
            h_col = np.empty(rows, dtype=object)
            for r in range(rows):
                h_col[r] = hist[r]
            cols["hist"] = h_col
        df = pd.DataFrame(cols)
        df.attrs.update(by=by, max_step_deg=float(max_step_deg), cos_threshold=float(res["cos_threshold"]), min_frames=int(min_frames),
                        frame_seconds=frame_seconds, users=list(names), window=window, stride=stride,
                        bins_frames=None if bins_frames is None else tuple(bins_frames))
        if res.get("labels") is not None:
            df.attrs["labels"] = np.asarray(res["labels"]).T
        if res.get("events") is not None:
            ev = np.asarray(res["events"]).reshape(-1, 4)
            start, frames = ev[:, 1].astype(np.int64), ev[:, 2].astype(np.int64)
            ecols = dict(user=np.asarray(list(names), dtype=object)[ev[:, 0]] if len(ev) else np.empty(0, dtype=object), frame=ev[:, 1],
                         time=times[start], time_end=times[start + frames - 1] if len(ev) else times[:0], frames=ev[:, 2],
                         seconds=frames * frame_seconds)
            if res.get("centroids") is not None:
                c = np.asarray(res["centroids"], dtype=np.float64).reshape(-1, 3)
                length = np.sqrt((c * c).sum(axis=1))
                with np.errstate(invalid="ignore", divide="ignore"):
                    ok = length > 0
                    ecols["lon"] = np.where(ok, np.degrees(np.arctan2(c[:, 1], c[:, 0])), np.nan)
                    ecols["lat"] = np.where(ok, np.degrees(np.arcsin(np.clip(c[:, 2] / np.where(ok, length, 1.0), -1.0, 1.0))), np.nan)
            ecols["dir"] = ev[:, 3]
            df.attrs["events"] = pd.DataFrame(ecols)
        return df

    def compute_fixations(self, window: Optional[int] = None, stride: int = 1, by: str = "angle", max_step_deg: float = 2.0,
                          velocity_deg_s: Optional[float] = None, min_frames: int = 5, min_seconds: Optional[float] = None,
                          per_user: bool = False, bins_frames=None, keep_labels: bool = False, keep_events: bool = False) -> pd.DataFrame:
        """When a viewer holds still, and for how long — or, with ``by="tile"``, how long a viewer stays on one tile.  Two
        consecutive frames of a viewer HOLD when the viewer has a sample in both and the great-circle angle between the two viewing
        directions is at most ``max_step_deg`` (``by="angle"``: the velocity-threshold rule, I-VT; the same Vector always holds), or
        both samples have the same nearest tile of the first tile count (``by="tile"``: tile dwell).  A run is a maximal stretch of
        frames whose pairs all hold; a run of at least ``min_frames`` frames is an event — a fixation, or a dwell — and belongs to
        the window that holds its first frame, with its full length (runs are never cut at window boundaries).
        ``velocity_deg_s`` (degrees per second) and ``min_seconds`` are exclusive alternatives to ``max_step_deg`` and
        ``min_frames``, converted with ``frame_seconds``, the median of ``diff(times)``: step = velocity * frame_seconds,
        ``min_frames = max(1, ceil(min_seconds / frame_seconds))``; leave the frame-based one at its default then.
        ``max_step_deg = 2`` and ``min_frames = 5`` are choices for head-direction data on the default grid, not taken from the
        reference, which has no such call.  ``window`` and ``stride`` count frames; ``window=None`` is the whole video.

        Uses the data ``process_directory`` cached.  Returns a new DataFrame (``compute_entropy``'s results are left alone), one row
        per window — user-major with ``user`` first when ``per_user``: ``time`` / ``time_end`` (the first / last frame of the row),
        ``samples``, ``fix_frames`` (the samples that lie in an event, wherever it started), ``fix_share``, ``events`` (that start
        in the row), ``mean_frames``, ``max_frames``, ``mean_seconds`` and, with ``bins_frames`` (ascending integer edges >= 1 in
        frames, half-open bins of the events' lengths), ``hist`` (a [B] view of counts).  Ratios are NaN where the denominator is 0.
        ``attrs`` hold ``by``, ``max_step_deg``, ``cos_threshold`` (what decided the holds), ``min_frames``, ``frame_seconds``,
        ``users``, ``window``, ``stride``; with ``keep_labels``, ``labels`` ([T, U], aligned with the cached samples: the length of
        the sample's event, 0 outside an event, -1 absent — ``labels > 0`` masks the fixation samples for ``compute_saliency`` and
        its scores); with ``keep_events``, ``events``: a DataFrame of ``user``, ``frame``, ``time``, ``time_end``, ``frames``,
        ``seconds``, ``lon``, ``lat`` (degrees, of the mean direction; NaN for a zero sum) and ``dir`` (the direction id of the
        middle sample).  A window without a sample has zero counts — returned, never raised.  Raises ``ValidationError`` before data
        is loaded and for samples outside [0, 1], ``ValueError`` for illegal arguments."""
        times, names, call = self._row_call("fixations")
        window, stride = self._window_args(len(times) if window is None else window, stride, len(times))
        _native.Plan._fixation_mode(by)
        steps = np.diff(np.asarray(times, dtype=np.float64))
        frame_seconds = float(np.median(steps)) if len(steps) else float("nan")
        max_step_deg, min_frames = self._fixation_step_args(max_step_deg, velocity_deg_s, min_frames, min_seconds, frame_seconds)
        bins_frames = self._fixation_bins(bins_frames)
        _native.Plan._fixation_args(max_step_deg, min_frames, bins_frames)
        res = call(window=window, stride=stride, by=by, max_step_deg=float(max_step_deg), min_frames=int(min_frames),
                   per_user=bool(per_user), edges=bins_frames, keep_labels=bool(keep_labels), keep_events=bool(keep_events),
                   keep_centroids=bool(keep_events), check=False)
        if res["code"] == _native.VET_ERR_RANGE:
            raise ValidationError("Normalized coordinates must be between 0 and 1")
        return self._fixation_frame(times, names, window, stride, bool(per_user), res, by, float(max_step_deg), int(min_frames),
                                    bins_frames)

    SALIENCY_MAP_LIMIT = 4 << 30     # bytes of maps that compute_saliency(keep_maps=True) hands back at most

    @staticmethod
    def _saliency_frame(times, names, window: int, stride: int, per_user: bool, res: dict, sigma_deg: float, width: int, height: int,
                        normalize: str) -> pd.DataFrame:
        """The saliency statistics as a DataFrame, one row per window (``per_user``: per (user, window), user-major, ``user``
        first); where ``res`` holds the maps, ``map`` of a row is the [H, W] view of its map (no copy)."""
        times = np.asarray(times)
        stats = np.asarray(res["stats"], dtype=np.float64).reshape(4, -1)
        counts = np.asarray(res["counts"]).reshape(2, -1)
        peak = np.asarray(res["peak"]).reshape(-1)
        rows = len(peak)
        R = rows // len(names) if per_user else rows
        first = np.arange(R, dtype=np.int64) * stride
        if per_user:
            first = np.tile(first, len(names))
        cols = {}
        if per_user:
            cols["user"] = np.repeat(np.asarray(list(names), dtype=object), R)
        has = peak >= 0
        py, px = np.divmod(np.where(has, peak, 0), width)
        cols.update(time=times[first], time_end=times[first + window - 1], samples=counts[0], distinct=counts[1], mass=stats[0],
                    peak=stats[1], peak_lon=np.where(has, (px + 0.5) / width * 360.0 - 180.0, np.nan),
                    peak_lat=np.where(has, 90.0 - (py + 0.5) / height * 180.0, np.nan), entropy=stats[2], area=stats[3])
        if res.get("map") is not None:
            maps = np.asarray(res["map"]).reshape(rows, height, width)
            m_col = np.empty(rows, dtype=object)
            for r in range(rows):
                m_col[r] = maps[r]
            cols["map"] = m_col
        df = pd.DataFrame(cols)
        df.attrs.update(sigma_deg=float(sigma_deg), kappa=1.0 / min(float(np.radians(sigma_deg)), float(np.pi)) ** 2, width=width, height=height,
                        normalize=normalize, window=window, stride=stride, users=list(names))
        return df

    def compute_saliency(self, window: Optional[int] = 1, stride: int = 1, sigma_deg: float = 5.0, width: int = 180, height: int = 90,
                         per_user: bool = False, normalize: str = "density", keep_maps: bool = True) -> pd.DataFrame:
        """Saliency maps: the continuous density of viewing directions on the sphere per window of frames — the von Mises-Fisher
        kernel density (for small angles the Gaussian of width ``sigma_deg``) of the samples of frames
        [r * stride, r * stride + window) on a ``width`` x ``height`` equirectangular map (row 0 at the top, as the heatmaps),
        pooled over the viewers or with ``per_user`` each viewer's own.  ``window`` and ``stride`` count frames; ``window=None`` is
        the whole video.  Independent of the tiling.  ``sigma_deg = 5.0`` is a choice for head-direction data, not taken from the
        reference, which has no such call.  ``normalize``: "none" (the sum of the kernels), "mean" (divided by the samples) or
        "density" (per steradian; the map integrates to 1 over the sphere).

        Uses the data ``process_directory`` cached.  Returns a new DataFrame, one row per window — user-major with ``user`` first
        when ``per_user``: ``time`` / ``time_end`` (the first / last frame of the row), ``samples``, ``distinct`` (directions),
        ``mass`` (the map's mean over the sphere: 4 pi * mass is near 1 with "density" when the map resolves sigma), ``peak`` and its cell
        centre ``peak_lon`` / ``peak_lat`` in degrees, ``entropy`` (bits, against the uniform sphere: 0 = uniform, negative =
        concentrated), ``area`` (2 ** entropy: the effective share of the sphere looked at; per viewer the exploration ratio)
        and, with ``keep_maps``, ``map`` (an [H, W] view into the one result array).  ``attrs`` hold ``sigma_deg``, ``kappa``,
        ``width``, ``height``, ``normalize``, ``window``, ``stride`` and ``users``.  A window without a sample has a zero map and
        NaN statistics — returned, never raised.  Raises ``ValidationError`` before data is loaded and for samples outside
        [0, 1], ``ValueError`` for illegal arguments and, with ``keep_maps``, for maps beyond 4 GiB."""
        times, names, call = self._row_call("saliency")
        window, stride = self._window_args(len(times) if window is None else window, stride, len(times))
        if not isinstance(normalize, str) or normalize not in _native.SALIENCY_SCALES:
            raise ValueError(f"normalize must be one of {sorted(_native.SALIENCY_SCALES)} (got {normalize!r})")
        _native.Plan._saliency_args(sigma_deg, width, height, normalize)
        rows = ((len(times) - window) // stride + 1) * (len(names) if per_user else 1)
        if keep_maps and rows * int(width) * int(height) * 8 > self.SALIENCY_MAP_LIMIT:
            raise ValueError(f"{rows} maps of {width} x {height} are {rows * int(width) * int(height) * 8 / 2 ** 30:.1f} GiB, beyond 4 GiB: "
                             "use a larger stride, a coarser map (width, height), or keep_maps=False")
        res = call(window=window, stride=stride, per_user=bool(per_user), sigma_deg=float(sigma_deg), width=int(width),
                   height=int(height), scale=normalize, want_map=bool(keep_maps), check=False)
        if res["code"] == _native.VET_ERR_RANGE:
            raise ValidationError("Normalized coordinates must be between 0 and 1")
        return self._saliency_frame(times, names, window, stride, bool(per_user), res, float(sigma_deg), int(width), int(height),
                                    normalize)

    @staticmethod
    def _saliency_similarity_frame(times, names, window: int, stride: int, code, labels, res: dict, sigma_deg: float, width: int,
                                   height: int) -> pd.DataFrame:
        """The saliency similarity as a DataFrame, one row per window; where ``res`` holds the maps, ``map_a`` / ``map_b`` of a row
        are the [H, W] views of its two maps in the one [2][R][H][W] array (no copy)."""
        times = np.asarray(times)
        stats = np.asarray(res["stats"], dtype=np.float64).reshape(9, -1)
        counts = np.asarray(res["counts"]).reshape(4, -1)
        R = stats.shape[1]
        first = np.arange(R, dtype=np.int64) * stride
        cols = dict(time=times[first], time_end=times[first + window - 1], samples_a=counts[0], samples_b=counts[1],
                    distinct_a=counts[2], distinct_b=counts[3])
        cols.update(zip(_native.SALIENCY_SIMILARITY_STATS, stats))
        if res.get("maps") is not None:
            maps = np.asarray(res["maps"]).reshape(2, R, height, width)
            for g, name in enumerate(("map_a", "map_b")):
                m_col = np.empty(R, dtype=object)
                for r in range(R):
                    m_col[r] = maps[g, r]
                cols[name] = m_col
        df = pd.DataFrame(cols)
        names = list(names)
        df.attrs.update(groups=labels, sizes=(int((code == 0).sum()), int((code == 1).sum())),
                        users=([n for n, c in zip(names, code) if c == 0], [n for n, c in zip(names, code) if c == 1]),
                        sigma_deg=float(sigma_deg), kappa=1.0 / min(float(np.radians(sigma_deg)), float(np.pi)) ** 2, width=width,
                        height=height, window=window, stride=stride)
        return df

    def compute_saliency_similarity(self, groups, window: Optional[int] = 1, stride: int = 1, sigma_deg: float = 5.0, width: int = 180,
                                    height: int = 90, keep_maps: bool = False) -> pd.DataFrame:
        """How alike two audiences look at the video, on the tiling-free saliency maps: per window of frames
        [r * stride, r * stride + window) (``window=None``: the whole video) the density maps of ``compute_saliency``
        ("density", the same ``sigma_deg``, ``width``, ``height``) of audience A's and of audience B's samples, and the metrics
        saliency benchmarks report between two maps.

        ``groups`` is ``compute_group_divergence``'s argument: a sequence aligned with the analyzer's user order, or a mapping from
        user name to label; exactly two distinct labels, the first in sorted order is audience A; ``None`` / NaN (and users a
        mapping does not name) are excluded.

        Uses the data ``process_directory`` cached.  Returns a new DataFrame, one row per window: ``time`` / ``time_end``,
        ``samples_a`` / ``samples_b``, ``distinct_a`` / ``distinct_b`` (directions), ``cc`` (Pearson's correlation of the two maps,
        area-weighted), ``sim`` (histogram intersection of the maps as distributions over the sphere, 1 = the same), ``jsd``
        (Jensen-Shannon divergence, bits, 0 .. 1), ``kl_ab`` / ``kl_ba`` (Kullback-Leibler divergence of A from B and of B from
        A, bits; +inf where one audience has weight on a cell in which the other's density underflowed to zero — small
        ``sigma_deg``), ``nss_ab`` / ``nss_ba`` (normalised scanpath saliency: B's standardised density at A's samples and the
        reverse, the density evaluated at the samples' directions; positive = they look where the other audience's density is
        above its sphere average), ``mass_a`` / ``mass_b`` (each map's mean over the sphere, 4 pi * mass near 1 when the map
        resolves sigma) and, with ``keep_maps``, ``map_a`` / ``map_b`` ([H, W] views into one result array).  ``attrs`` hold
        ``groups`` (the two labels), ``sizes``, ``users``, ``sigma_deg``, ``kappa``, ``width``, ``height``, ``window`` and
        ``stride``.  A window in which an audience has no sample has NaN metrics — returned, never raised.  Raises
        ``ValidationError`` before data is loaded and for samples outside [0, 1], ``ValueError`` for illegal arguments and, with
        ``keep_maps``, for maps beyond 4 GiB."""
        times, names, call = self._row_call("saliency_similarity")
        code, labels = self._group_labels(groups, names)
        window, stride = self._window_args(len(times) if window is None else window, stride, len(times))
        _native.Plan._saliency_args(sigma_deg, width, height, "density")
        rows = 2 * ((len(times) - window) // stride + 1)
        if keep_maps and rows * int(width) * int(height) * 8 > self.SALIENCY_MAP_LIMIT:
            raise ValueError(f"{rows} maps of {width} x {height} are {rows * int(width) * int(height) * 8 / 2 ** 30:.1f} GiB, beyond 4 GiB: "
                             "use a larger stride, a coarser map (width, height), or keep_maps=False")
        res = call(groups=code, window=window, stride=stride, sigma_deg=float(sigma_deg), width=int(width), height=int(height),
                   want_maps=bool(keep_maps), check=False)
        if res["code"] == _native.VET_ERR_RANGE:
            raise ValidationError("Normalized coordinates must be between 0 and 1")
        return self._saliency_similarity_frame(times, names, window, stride, code, labels, res, float(sigma_deg), int(width),
                                               int(height))

    @staticmethod
    def _saliency_score_frame(times, names, window: int, stride: int, res: dict, sigma_deg: float, width: int, height: int,
                              static: bool, distribution: bool) -> pd.DataFrame:
        """The saliency scores as a DataFrame, one row per window; where ``res`` holds the audience's maps, ``map`` of a row is the
        [H, W] view of its map in the one [R][H][W] array (no copy)."""
        times = np.asarray(times)
        stats = np.asarray(res["stats"], dtype=np.float64).reshape(9, -1)
        counts = np.asarray(res["counts"]).reshape(2, -1)
        R = stats.shape[1]
        first = np.arange(R, dtype=np.int64) * stride
        cols = dict(time=times[first], time_end=times[first + window - 1], samples=counts[0], distinct=counts[1])
        cols.update(zip(_native.SALIENCY_SCORE_STATS, stats))
        if res.get("map") is not None:
            maps = np.asarray(res["map"]).reshape(R, height, width)
            m_col = np.empty(R, dtype=object)
            for r in range(R):
                m_col[r] = maps[r]
            cols["map"] = m_col
        df = pd.DataFrame(cols)
        df.attrs.update(sigma_deg=float(sigma_deg), kappa=1.0 / min(float(np.radians(sigma_deg)), float(np.pi)) ** 2, width=width,
                        height=height, window=window, stride=stride, users=list(names), static=bool(static),
                        distribution=bool(distribution))
        return df

    def compute_saliency_score(self, maps, window: Optional[int] = 1, stride: int = 1, sigma_deg: float = 5.0,
                               distribution: bool = True, keep_maps: bool = False) -> pd.DataFrame:
        """How well a saliency map from elsewhere — a model's prediction, another dataset's ground truth, a centre or equator bias,
        last segment's map — predicts where this audience looked, per window of frames [r * stride, r * stride + window)
        (``window=None``: the whole video).  ``maps`` is a float64 array, finite and non-negative in any scale, laid out as
        ``compute_saliency``'s maps (row 0 at the top, column c centred at lon (c + 0.5) / W * 360 - 180): [H, W], one static map
        for every window, or [R, H, W], one per window.  The map's size is taken from its shape.  Independent of the tiling.

        Uses the data ``process_directory`` cached.  Returns a new DataFrame, one row per window: ``time`` / ``time_end``,
        ``samples``, ``distinct`` (directions); the location metrics, from the map sampled at the samples' directions by bilinear
        interpolation — ``auc`` (the probability that the map is higher at a sample than at a uniformly drawn point of the sphere,
        ties a half: the Mann-Whitney form of AUC-Judd with the whole sphere as negatives, area-weighted; 0.5 = chance), ``nss``
        (the map standardised by its area-weighted mean and variance, averaged over the samples), ``info_gain`` (mean log2 of the
        map at a sample over the map's sphere mean, bits; -inf where the map is 0 at a sample); with ``distribution`` the
        distribution metrics of the audience's own density map (``compute_saliency``, "density", ``sigma_deg``) against the
        prediction — ``cc``, ``sim``, ``jsd``, ``kl`` (the audience from the prediction, bits; +inf where the audience has weight on
        a cell the map holds 0 in) and ``mass`` (the audience map's) — NaN without it, and no density is evaluated then;
        ``mass_pred`` (the predicted map's mean over the sphere) and, with ``keep_maps``, ``map`` (the audience's map, an [H, W]
        view into one result array).  ``attrs`` hold ``sigma_deg``, ``kappa``, ``width``, ``height``, ``window``, ``stride``,
        ``users``, ``static`` and ``distribution``.  A window without a sample is NaN but for ``mass_pred`` — returned, never
        raised.  Raises ``ValidationError`` before data is loaded and for samples outside [0, 1], ``ValueError`` for illegal
        arguments, a map of the wrong rank, dtype or number, a negative or non-finite map value and, with ``keep_maps``, for maps
        beyond 4 GiB."""
        times, names, call = self._row_call("saliency_score")
        window, stride = self._window_args(len(times) if window is None else window, stride, len(times))
        R = (len(times) - window) // stride + 1
        pred, _, width, height = _native.Plan._score_maps(maps, R, True)
        _native.Plan._saliency_args(sigma_deg, width, height, "density")
        if keep_maps and R * width * height * 8 > self.SALIENCY_MAP_LIMIT:
            raise ValueError(f"{R} maps of {width} x {height} are {R * width * height * 8 / 2 ** 30:.1f} GiB, beyond 4 GiB: "
                             "use a larger stride, a coarser map (width, height), or keep_maps=False")
        res = call(maps=pred, window=window, stride=stride, sigma_deg=float(sigma_deg), distribution=bool(distribution),
                   want_map=bool(keep_maps), check=False)
        if res["code"] == _native.VET_ERR_RANGE:
            raise ValidationError("Normalized coordinates must be between 0 and 1")
        return self._saliency_score_frame(times, names, window, stride, res, float(sigma_deg), width, height, pred.ndim == 2,
                                          bool(distribution))

    @staticmethod
    def _congruency_frame(times, names, window: int, stride: int, res: dict, sigma_deg: float) -> pd.DataFrame:
        """The viewer congruency as a DataFrame, user-major; ``attrs["rows"]`` is the per-window frame."""
        times = np.asarray(times)
        names = list(names)
        U = len(names)
        stats = np.asarray(res["stats"], dtype=np.float64).reshape(3, U, -1)
        counts = np.asarray(res["counts"]).reshape(3, U, -1)
        per_row = np.asarray(res["rows"], dtype=np.float64).reshape(4, -1)
        R = stats.shape[2]
        first = np.arange(R, dtype=np.int64) * stride
        df = pd.DataFrame(dict(user=np.repeat(np.asarray(names, dtype=object), R), time=np.tile(times[first], U),
                               time_end=np.tile(times[first + window - 1], U), samples=counts[0].reshape(-1),
                               distinct=counts[1].reshape(-1), others=counts[2].reshape(-1),
                               **{k: stats[i].reshape(-1) for i, k in enumerate(_native.CONGRUENCY_STATS)}))
        rows = pd.DataFrame(dict(time=times[first], time_end=times[first + window - 1], scored=per_row[0].astype(np.int64),
                                 **{k: per_row[1 + i] for i, k in enumerate(_native.CONGRUENCY_STATS)}))
        df.attrs.update(rows=rows, users=names, sigma_deg=float(sigma_deg),
                        kappa=1.0 / min(float(np.radians(sigma_deg)), float(np.pi)) ** 2, window=window, stride=stride)
        return df

    def compute_congruency(self, window: Optional[int] = None, stride: int = 1, sigma_deg: float = 5.0, nss: bool = True) -> pd.DataFrame:
        """Inter-observer congruency: how well the rest of the audience predicts where each viewer looks, per window of frames
        [r * stride, r * stride + window) (``window=None``: the whole video).  The kernel density of ``compute_saliency``
        (``sigma_deg``) of everyone else's samples is evaluated at the viewer's own directions — leave-one-out, no map, independent
        of the tiling.  The noise ceiling for a saliency model, and an outlier detector for viewers.

        Uses the data ``process_directory`` cached.  Returns a new DataFrame, user-major: ``user``, ``time`` / ``time_end`` (the
        first / last frame of the row), ``samples`` and ``distinct`` (the viewer's own), ``others`` (everyone else's samples),
        ``lift`` (the others' density at the viewer's samples relative to the uniform sphere: 1 = chance), ``info_gain`` (the mean
        log2 of that ratio, bits; -inf where the others' density underflowed to zero at a sample — small ``sigma_deg``) and
        ``nss`` (the density at the samples, standardised by its mean and variance over the sphere in closed form; NaN with
        ``nss=False``, which spares its arithmetic).  ``attrs["rows"]`` is the per-window frame — ``time``, ``time_end``,
        ``scored`` (viewers with a sample and company) and the means ``lift``, ``info_gain``, ``nss`` over them: the segment's
        congruency; ``attrs`` also hold ``users``, ``sigma_deg``, ``kappa``, ``window`` and ``stride``.  A viewer without a sample
        in a window, or alone in it, is NaN — returned, never raised.  Raises ``ValidationError`` before data is loaded and for
        samples outside [0, 1], ``ValueError`` for illegal arguments and fewer than two viewers."""
        times, names, call = self._row_call("congruency")
        window, stride = self._window_args(len(times) if window is None else window, stride, len(times))
        _native.Plan._saliency_args(sigma_deg, 2, 1, "density")
        if len(names) < 2:
            raise ValueError(f"congruency needs at least two viewers (got {len(names)})")
        res = call(window=window, stride=stride, sigma_deg=float(sigma_deg), nss=bool(nss), check=False)
        if res["code"] == _native.VET_ERR_RANGE:
            raise ValidationError("Normalized coordinates must be between 0 and 1")
        return self._congruency_frame(times, names, window, stride, res, float(sigma_deg))

    def compute_entropy(self) -> pd.DataFrame:  # pragma: no cover - overridden
        raise NotImplementedError
