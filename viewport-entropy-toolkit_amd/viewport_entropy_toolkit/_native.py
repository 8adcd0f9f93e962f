"""ctypes binding of the HIP engine's C-ABI (include/vet.h, libvet_hip.so).

This module is the only place the package touches native code.  It has no CPU fallback: if
the shared library has not been built, or no gfx950 device is visible, every compute entry
point raises ``NativeUnavailable`` with the reason.
"""

from __future__ import annotations

import ctypes as C
import math
import os
import threading
from pathlib import Path
from typing import Optional, Sequence

import numpy as np

from . import _quantiser

_PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("VET_HIP_LIBRARY", _PKG_DIR.parent / "lib" / "libvet_hip.so"))

VET_OK, VET_ERR_INVALID, VET_ERR_DEVICE, VET_ERR_RANGE, VET_ERR_EMPTY, VET_ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -5
KERNEL_IDS = {"k_grid_dirs": 0, "k_nearest_lut": 1, "k_spatial": 2, "k_transition": 3, "k_finalize": 4,
              "k_wtab": 5, "k_weights": 6}


class NativeUnavailable(RuntimeError):
    """The HIP extension is missing or no MI355X is visible."""


class NativeError(RuntimeError):
    """A C-ABI call failed; ``code`` is the VET_ERR_* value."""

    def __init__(self, code: int, message: str):
        super().__init__(message)
        self.code = code


class Video(C.Structure):
    """include/vet.h: vet_video (device pointers of one video of a batch)."""
    _fields_ = [("d_mu", C.c_void_p), ("d_mv", C.c_void_p), ("n_users", C.c_int), ("n_frames", C.c_int),
                ("d_entropy", C.c_void_p), ("d_assign", C.c_void_p), ("d_present", C.c_void_p)]


class Track(C.Structure):
    """include/vet.h: vet_track (one parsed CSV file, host memory owned by the library)."""
    _fields_ = [("time", C.POINTER(C.c_double)), ("mu", C.POINTER(C.c_double)), ("mv", C.POINTER(C.c_double)),
                ("n_rows", C.c_int64), ("status", C.c_int)]


VET_CSV_OK, VET_CSV_FALLBACK, VET_CSV_IO = 0, 1, 2


class _PlanDesc(C.Structure):
    _fields_ = [
        ("video_width", C.c_int), ("video_height", C.c_int),
        ("h_lon_cos", C.c_void_p), ("h_lon_sin", C.c_void_p),
        ("h_lat_sin", C.c_void_p), ("h_lat_cos", C.c_void_p),
        ("h_dir_table", C.c_void_p), ("n_dirs", C.c_int64),
        ("n_lattices", C.c_int), ("n_tiles", C.c_void_p),
        ("h_tiles", C.c_void_p), ("h_max_entropy", C.c_void_p),
        ("fov_angle", C.c_double), ("max_angular_distance", C.c_double),
        ("power_factor", C.c_double), ("use_weight_distribution", C.c_int),
        ("h_bin_lut", C.c_void_p), ("n_norm_tiles", C.c_void_p),
    ]


# name -> (restype, argtypes); also the list tests check against include/vet.h
_P, _I, _I64, _D, _SZ, _U64 = C.c_void_p, C.c_int, C.c_int64, C.c_double, C.c_size_t, C.c_uint64
SIGNATURES = {
    "vet_version": (_I, []),
    "vet_last_error": (C.c_char_p, []),
    "vet_device_count": (_I, []),
    "vet_create": (_I, [_I, C.POINTER(_P)]),
    "vet_destroy": (_I, [_P]),
    "vet_synchronize": (_I, [_P]),
    "vet_device_pci_bus_id": (_I, [_P, C.c_char_p, _I]),
    "vet_profile_enable": (_I, [_P, _I]),
    "vet_test_no_row_cap": (_I, [_P, _I]),
    "vet_test_rec8": (_I, [_P, _I]),
    "vet_test_user_transition_hash": (_I, [_P, _I]),
    "vet_test_divergence_chunk_rows": (_I, [_P, _I]),
    "vet_test_window_divergence_chunk_rows": (_I, [_P, _I]),
    "vet_test_crowd_divergence_chunk_rows": (_I, [_P, _I]),
    "vet_test_bootstrap_chunk_rows": (_I, [_P, _I]),
    "vet_test_group_chunk_rows": (_I, [_P, _I]),
    "vet_test_coverage_chunk_rows": (_I, [_P, _I]),
    "vet_test_markov_chunk_rows": (_I, [_P, _I]),
    "vet_test_motion_lds_values": (_I, [_P, _I]),
    "vet_test_dispersion_tile": (_I, [_P, _I]),
    "vet_test_saliency_tile": (_I, [_P, _I]),
    "vet_test_cluster_tile": (_I, [_P, _I, _I]),
    "vet_test_fixation_chunk": (_I, [_P, _I]),
    "vet_profile_reset": (_I, [_P]),
    "vet_profile_get": (_I, [_P, _I, C.POINTER(_D), C.POINTER(_I64)]),
    "vet_kernel_name": (C.c_char_p, [_I]),
    "vet_malloc": (_I, [_P, _SZ, C.POINTER(_P)]),
    "vet_free": (_I, [_P, _P]),
    "vet_memcpy_h2d": (_I, [_P, _P, _P, _SZ]),
    "vet_memcpy_d2h": (_I, [_P, _P, _P, _SZ]),
    "vet_plan_create": (_I, [_P, C.POINTER(_PlanDesc), C.POINTER(_P)]),
    "vet_plan_destroy": (_I, [_P]),
    "vet_plan_n_dirs": (_I64, [_P]),
    "vet_plan_set_table_policy": (_I, [_P, _I]),
    "vet_plan_set_fp64": (_I, [_P, _I]),
    "vet_plan_set_raw_weights": (_I, [_P, _I]),
    "vet_plan_table_stride": (_I, [_P, _I]),
    "vet_plan_table_rows": (_I64, [_P]),
    "vet_plan_table_cap": (_I, [_P, _I, C.POINTER(_I64)]),
    "vet_plan_record_bytes": (_I, [_P]),
    "vet_plan_read_records": (_I, [_P, _P]),
    "vet_plan_last_formulation": (_I, [_P, _I]),
    "vet_plan_last_table_kernel": (C.c_uint32, [_P]),
    "vet_plan_error_bounds": (_I, [_P, _I, C.POINTER(_D), C.POINTER(_D)]),
    "vet_plan_read_dirs": (_I, [_P, _P]),
    "vet_plan_read_nearest": (_I, [_P, _I, _P]),
    "vet_plan_read_table": (_I, [_P, _I, _P, _P, _P, _P, _P, _P]),
    "vet_spatial_entropy": (_I, [_P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P]),
    "vet_spatial_entropy_ids": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _P, _P]),
    "vet_window_rows": (_I64, [_I, _I, _I]),
    "vet_spatial_entropy_windowed": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "vet_spatial_entropy_windowed_ids": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "vet_spatial_entropy_windowed_host": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "vet_user_entropy": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "vet_user_entropy_ids": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "vet_user_entropy_host": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "vet_transition_entropy_windowed": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "vet_transition_entropy_windowed_ids": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "vet_transition_entropy_windowed_host": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "vet_user_transition_entropy": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "vet_user_transition_entropy_ids": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "vet_user_transition_entropy_host": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "vet_transition_markov": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "vet_transition_markov_ids": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "vet_transition_markov_host": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P]),
    "vet_head_motion": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P]),
    "vet_head_motion_ids": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P]),
    "vet_head_motion_host": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _I, _P, _I, _P, _P, _P, _P, _P]),
    "vet_dispersion": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P]),
    "vet_dispersion_ids": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P]),
    "vet_dispersion_host": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _P, _P, _P, _P]),
    "vet_viewer_clusters": (_I, [_P, _P, _P, _I, _I, _I, _I, _D, _D, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "vet_viewer_clusters_ids": (_I, [_P, _P, _I, _I, _I, _I, _D, _D, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "vet_viewer_clusters_host": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _D, _D, _P, _I, _P, _P, _P, _P, _P, _P, _P]),
    "vet_viewer_clusters_sweeps": (_I, [_P, _P]),
    "vet_fixations": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _D, _I, _I, _P, _I, _I64, _P, _P, _P, _P, _P, _P, _P, _P]),
    "vet_fixations_ids": (_I, [_P, _P, _I, _I, _I, _I, _I, _D, _I, _I, _P, _I, _I64, _P, _P, _P, _P, _P, _P, _P, _P]),
    "vet_fixations_host": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _D, _I, _I, _P, _I, _I64, _P, _P, _P, _P, _P, _P]),
    "vet_saliency": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _D, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "vet_saliency_ids": (_I, [_P, _P, _I, _I, _I, _I, _I, _D, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "vet_saliency_host": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _D, _I, _I, _I, _P, _P, _P, _P]),
    "vet_saliency_similarity": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _D, _I, _I, _P, _P, _P, _P, _P]),
    "vet_saliency_similarity_ids": (_I, [_P, _P, _I, _I, _I, _I, _P, _D, _I, _I, _P, _P, _P, _P, _P]),
    "vet_saliency_similarity_host": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _D, _I, _I, _P, _P, _P]),
    "vet_saliency_score": (_I, [_P, _P, _P, _I, _I, _I, _I, _D, _I, _I, _P, _I, _I, _P, _P, _P, _P, _P]),
    "vet_saliency_score_ids": (_I, [_P, _P, _I, _I, _I, _I, _D, _I, _I, _P, _I, _I, _P, _P, _P, _P, _P]),
    "vet_saliency_score_host": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _D, _I, _I, _P, _I, _I, _P, _P, _P]),
    "vet_congruency": (_I, [_P, _P, _P, _I, _I, _I, _I, _D, _I, _P, _P, _P, _P, _P]),
    "vet_congruency_ids": (_I, [_P, _P, _I, _I, _I, _I, _D, _I, _P, _P, _P, _P, _P]),
    "vet_congruency_host": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _D, _I, _P, _P, _P]),
    "vet_user_divergence": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P]),
    "vet_user_divergence_ids": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P]),
    "vet_user_divergence_host": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "vet_window_divergence": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "vet_window_divergence_ids": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "vet_window_divergence_host": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "vet_coverage": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P]),
    "vet_coverage_ids": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P]),
    "vet_coverage_host": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _P, _P, _P, _P]),
    "vet_crowd_divergence": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "vet_crowd_divergence_ids": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "vet_crowd_divergence_host": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "vet_bootstrap_entropy": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _U64, _D, _P, _P, _P, _P, _P, _P]),
    "vet_bootstrap_entropy_ids": (_I, [_P, _P, _I, _I, _I, _I, _I, _U64, _D, _P, _P, _P, _P, _P, _P]),
    "vet_bootstrap_entropy_host": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _U64, _D, _P, _P, _P, _P]),
    "vet_bootstrap_counts_host": (_I, [_P, _I, _I, _U64, _P]),
    "vet_group_divergence": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _I, _U64, _D, _P, _P, _P, _P, _P, _P, _P]),
    "vet_group_divergence_ids": (_I, [_P, _P, _I, _I, _I, _I, _P, _I, _U64, _D, _P, _P, _P, _P, _P, _P, _P]),
    "vet_group_divergence_host": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _U64, _D, _P, _P, _P, _P, _P]),
    "vet_group_labels_host": (_I, [_P, _I, _P, _I, _U64, _P]),
    "vet_transition_entropy": (_I, [_P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P]),
    "vet_transition_entropy_ids": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _P, _P]),
    "vet_spatial_entropy_batch": (_I, [_P, _I, _P, _P, _P]),
    "vet_spatial_entropy_batch_host": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P]),
    "vet_transition_entropy_batch": (_I, [_P, _I, _P, _P, _P]),
    "vet_transition_entropy_batch_host": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P]),
    "vet_spatial_entropy_host": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _P, _P]),
    "vet_transition_entropy_host": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _P, _P]),
    "vet_spatial_entropy_host_resident": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, C.POINTER(_P)]),
    "vet_transition_entropy_host_resident": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, C.POINTER(_P)]),
    "vet_result_fetch": (_I, [_P, _I, _I64, _I64, _P]),
    "vet_result_free": (_I, [_P]),
    "vet_fb_tile_boundaries": (_I, [_P, _P, _I, _I, _P, _P]),
    "vet_angular_distances": (_I, [_P, _P, _I64, _P, _I, _P]),
    "vet_heatmap_create": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, C.POINTER(_P)]),
    "vet_heatmap_destroy": (_I, [_P]),
    "vet_heatmap_read_map": (_I, [_P, _P]),
    "vet_heatmap_render": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _P]),
    "vet_heatmap_render_result": (_I, [_P, _P, _P, _P, _P, _I, _I64, _I64, _P]),
    "vet_heatmap_render_counts": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _P]),
    "vet_heatmap_render_transition_result": (_I, [_P, _P, _P, _P, _P, _I, _I64, _I64, _P]),
    "vet_heatmap_create_latlon": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, C.POINTER(_P)]),
    "vet_heatmap_render_binned": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P]),
    "vet_heatmap_render_binned_host": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "vet_tiling_create": (_I, [_P, _P, _I, _P, _I, _I, _I, C.POINTER(_P)]),
    "vet_tiling_destroy": (_I, [_P]),
    "vet_tiling_render": (_I, [_P, _P, _I, _P, _P, _P]),
    "vet_tiling_render_host": (_I, [_P, _P, _I, _P, _P]),
    "vet_csv_read_tracks": (_I, [_I, C.POINTER(C.c_char_p), C.POINTER(Track), _I]),
    "vet_csv_free_tracks": (None, [_I, C.POINTER(Track)]),
}

# vet_plan_last_formulation codes (include/vet.h)
FORMULATIONS = {0: "table", 1: "sweep", 2: "precise", 3: "ftable", 4: "dtable"}

_lib = None
_lib_lock = threading.Lock()


def _preload_hip_runtime() -> Optional[str]:
    """One HIP runtime per process.  libvet_hip.so needs ``libamdhip64.so.7``; a PyTorch-ROCm wheel ships its own
    copy (``torch/lib/libamdhip64.so``, same SONAME) and a process that ends up with both — this library first,
    ``torch.cuda`` later — fails in torch's ``_cuda_init`` with "No HIP GPUs are available".  So when torch is
    installed its runtime is loaded first, globally, and the dynamic linker binds libvet_hip.so to it by SONAME
    (torch is NOT imported; if it already is, this is the runtime it loaded).  ``VET_HIP_RUNTIME=system`` keeps the
    system runtime.  Returns the path that was preloaded, or None."""
    if os.environ.get("VET_HIP_RUNTIME", "").lower() == "system":
        return None
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return None
    cand = Path(spec.origin).parent / "lib" / "libamdhip64.so"
    if not cand.exists():
        return None
    try:
        C.CDLL(str(cand), mode=C.RTLD_GLOBAL)
    except OSError:
        return None
    return str(cand)


HIP_RUNTIME_PRELOADED: Optional[str] = None


def load_library():
    """dlopen libvet_hip.so and declare every prototype; raises NativeUnavailable."""
    global _lib, HIP_RUNTIME_PRELOADED
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not LIB_PATH.exists():
            raise NativeUnavailable(
                f"HIP extension not found at {LIB_PATH}. Build it with "
                f"`make -C {_PKG_DIR.parent / 'csrc'}` (or __graft_entry__.build()); "
                "this package has no CPU compute path.")
        HIP_RUNTIME_PRELOADED = _preload_hip_runtime()
        try:
            lib = C.CDLL(str(LIB_PATH))
        except OSError as e:  # missing ROCm runtime etc.
            raise NativeUnavailable(f"cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
        return lib


def read_tracks(paths: Sequence, n_threads: int = 0):
    """vet_csv_read_tracks over ``paths``: list of ``(status, time, mu, mv)`` with one FP64 entry per
    data row (NaN = missing); arrays are ``None`` unless status is VET_CSV_OK.  Host code only."""
    lib = load_library()
    n = len(paths)
    if n == 0:
        return []
    c_paths = (C.c_char_p * n)(*[os.fsencode(str(p)) for p in paths])
    tracks = (Track * n)()
    rc = lib.vet_csv_read_tracks(n, c_paths, tracks, int(n_threads))
    if rc != VET_OK:
        raise NativeError(rc, "vet_csv_read_tracks failed")
    try:
        out = []
        for t in tracks:
            if t.status == VET_CSV_OK:
                m = int(t.n_rows)
                cols = [np.frombuffer(C.string_at(ptr, m * 8), dtype=np.float64).copy() if m else np.empty(0)
                        for ptr in (t.time, t.mu, t.mv)]
                out.append((VET_CSV_OK, *cols))
            else:
                out.append((int(t.status), None, None, None))
        return out
    finally:
        lib.vet_csv_free_tracks(n, tracks)


def _check(lib, rc: int):
    if rc != VET_OK:
        msg = lib.vet_last_error()
        raise NativeError(rc, (msg or b"").decode("utf-8", "replace") or f"vet error {rc}")


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


VET_STREAM_LEGACY = 1
TABLE_SAMPLES_PER_DIRECTION = 2      # include/vet.h: VET_TABLE_SAMPLES_PER_DIRECTION (policy 0: table iff samples >= this x directions)


def _stream(handle):
    """hipStream_t handle -> the C-ABI's ``stream`` argument: ``None`` = the engine's own stream;
    0 (torch's default stream) = the legacy null stream; anything else is the stream itself."""
    if handle is None:
        return None
    return C.c_void_p(VET_STREAM_LEGACY if int(handle) == 0 else int(handle))


class Engine:
    """One device context (stream + scratch).  ``Engine.default()`` is per process."""

    _default = None
    _default_lock = threading.Lock()

    def __init__(self, device_id: int = 0):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.vet_create(device_id, C.byref(h))
        if rc == VET_ERR_DEVICE:
            raise NativeUnavailable((self.lib.vet_last_error() or b"").decode())
        _check(self.lib, rc)
        self.handle = h
        self.device_id = device_id

    @staticmethod
    def default_device_id(n_devices: int) -> int:
        """Device of the per-process default engine: ``VET_DEVICE``, else ``LOCAL_RANK`` (one process per GPU), else 0.
        A value that names no visible device RAISES: falling back to device 0 would silently stack the ranks of a
        multi-GPU job on one GPU."""
        for var in ("VET_DEVICE", "LOCAL_RANK"):
            raw = os.environ.get(var)
            if raw is None:
                continue
            try:
                dev = int(raw)
            except ValueError:
                raise NativeUnavailable(f"{var}={raw!r} is not a device index") from None
            if not 0 <= dev < n_devices:
                raise NativeUnavailable(
                    f"{var}={dev} names no visible device ({n_devices} visible): refusing to fall back to device 0 "
                    "(the ranks of a multi-GPU job would share one GPU); fix the launcher's device visibility or set VET_DEVICE")
            return dev
        return 0

    @classmethod
    def default(cls) -> "Engine":
        with cls._default_lock:
            if cls._default is None:
                n = load_library().vet_device_count()
                if n <= 0:
                    raise NativeUnavailable("no HIP device available; this package has no CPU compute path")
                cls._default = cls(cls.default_device_id(n))
            return cls._default

    def pci_bus_id(self) -> str:
        """PCI bus id of the device this context computes on (include/vet.h: vet_device_pci_bus_id)."""
        buf = C.create_string_buffer(64)
        _check(self.lib, self.lib.vet_device_pci_bus_id(self.handle, buf, 64))
        return buf.value.decode()

    def close(self):
        if getattr(self, "handle", None):
            self.lib.vet_destroy(self.handle)
            self.handle = None

    def synchronize(self):
        _check(self.lib, self.lib.vet_synchronize(self.handle))

    def fb_tile_boundaries(self, tiles: np.ndarray, max_edges: int = 16):
        """k_fb_boundaries: (edges [n, max_edges, 2, 3] NaN padded, count [n]) for lattice Vectors ``tiles`` [n, 3]."""
        tiles = np.ascontiguousarray(tiles, dtype=np.float64).reshape(-1, 3)
        n = len(tiles)
        edges = np.empty((n, max_edges, 2, 3), dtype=np.float64)
        count = np.empty(n, dtype=np.int32)
        _check(self.lib, self.lib.vet_fb_tile_boundaries(self.handle, _ptr(tiles), n, max_edges, _ptr(edges), _ptr(count)))
        return edges, count

    # --- profiling -------------------------------------------------------
    def angular_distances(self, vectors: np.ndarray, tiles: np.ndarray) -> np.ndarray:
        """[m, n] arccos(clip(dot(v/|v|, t/|t|))) — vector_angle_distance of the reference for every pair."""
        vectors = np.ascontiguousarray(vectors, dtype=np.float64).reshape(-1, 3)
        tiles = np.ascontiguousarray(tiles, dtype=np.float64).reshape(-1, 3)
        out = np.empty((len(vectors), len(tiles)), dtype=np.float64)
        if out.size:
            _check(self.lib, self.lib.vet_angular_distances(self.handle, _ptr(vectors), len(vectors), _ptr(tiles), len(tiles), _ptr(out)))
        return out

    def test_no_row_cap(self, on: bool = True):
        """Test switch: plans of this engine build their tables with every row whole (include/vet.h: vet_test_no_row_cap)."""
        _check(self.lib, self.lib.vet_test_no_row_cap(self.handle, int(on)))

    def test_rec8(self, on: bool = True):
        """Test switch: table launches of this engine's plans read the 8-byte direction record (include/vet.h: vet_test_rec8)."""
        _check(self.lib, self.lib.vet_test_rec8(self.handle, int(on)))

    def test_user_transition_hash(self, on: bool = True):
        """Test switch: per-viewer transition rows of up to 64 pairs run the hash kernel of the longer rows
        (include/vet.h: vet_test_user_transition_hash)."""
        _check(self.lib, self.lib.vet_test_user_transition_hash(self.handle, int(on)))

    def test_divergence_chunk_rows(self, rows: int = 0):
        """Test switch: the viewer divergence builds its histograms ``rows`` rows at a time (0: the default budget); results do
        not depend on it (include/vet.h: vet_test_divergence_chunk_rows)."""
        _check(self.lib, self.lib.vet_test_divergence_chunk_rows(self.handle, int(rows)))

    def test_window_divergence_chunk_rows(self, rows: int = 0):
        """Test switch: the window divergence takes ``rows`` pair rows per histogram chunk (0: the default budget); results do
        not depend on it (include/vet.h: vet_test_window_divergence_chunk_rows)."""
        _check(self.lib, self.lib.vet_test_window_divergence_chunk_rows(self.handle, int(rows)))

    def test_bootstrap_chunk_rows(self, rows: int = 0):
        """Test switch: the bootstrap builds the viewers' histograms ``rows`` rows at a time (0: the default budget); results do
        not depend on it (include/vet.h: vet_test_bootstrap_chunk_rows)."""
        _check(self.lib, self.lib.vet_test_bootstrap_chunk_rows(self.handle, int(rows)))

    def test_group_chunk_rows(self, rows: int = 0):
        """Test switch: the group divergence builds the viewers' histograms ``rows`` rows at a time (0: the default budget);
        results do not depend on it (include/vet.h: vet_test_group_chunk_rows)."""
        _check(self.lib, self.lib.vet_test_group_chunk_rows(self.handle, int(rows)))

    def test_coverage_chunk_rows(self, rows: int = 0):
        """Test switch: the coverage call takes ``rows`` rows per histogram chunk (0: the default budget); results do not depend
        on it (include/vet.h: vet_test_coverage_chunk_rows)."""
        _check(self.lib, self.lib.vet_test_coverage_chunk_rows(self.handle, int(rows)))

    def test_markov_chunk_rows(self, rows: int = 0):
        """Test switch: the chunked shape of the Markov transition call builds the matrices of ``rows`` rows per pass (0: the
        default budget); results do not depend on it (include/vet.h: vet_test_markov_chunk_rows)."""
        _check(self.lib, self.lib.vet_test_markov_chunk_rows(self.handle, int(rows)))

    def test_motion_lds_values(self, n: int = 0):
        """Test switch: one workgroup of the head-motion call takes rows of at most ``n`` values (a multiple of 1024; 0: the default,
        16384), longer rows run the chunked shape; results do not depend on it (include/vet.h: vet_test_motion_lds_values)."""
        _check(self.lib, self.lib.vet_test_motion_lds_values(self.handle, int(n)))

    def test_dispersion_tile(self, n: int = 0):
        """Test switch: the pair kernel of the dispersion call stages at most ``n`` viewers of a frame in LDS at a time (0: the
        default, 1024); results do not depend on it (include/vet.h: vet_test_dispersion_tile)."""
        _check(self.lib, self.lib.vet_test_dispersion_tile(self.handle, int(n)))

    def test_cluster_tile(self, rows: int = 0, tile: int = 0):
        """Test switch: the viewer-clusters call takes at most ``rows`` rows per pass (0: the default budget) and its link kernel at
        most ``tile`` partners per workgroup (0: the default, 128); results do not depend on them (include/vet.h:
        vet_test_cluster_tile)."""
        _check(self.lib, self.lib.vet_test_cluster_tile(self.handle, int(rows), int(tile)))

    def test_fixation_chunk(self, n: int = 0):
        """Test switch: the walk of the fixations call over a viewer's frames takes chunks of ``n`` frames (a multiple of 4; 0: the
        default, 1024); results do not depend on it (include/vet.h: vet_test_fixation_chunk)."""
        _check(self.lib, self.lib.vet_test_fixation_chunk(self.handle, int(n)))

    def test_saliency_tile(self, n: int = 0):
        """Test switch: the map kernel of the saliency call stages at most ``n`` list entries of a row in LDS at a time (0: the
        default, 1024); results do not depend on it (include/vet.h: vet_test_saliency_tile)."""
        _check(self.lib, self.lib.vet_test_saliency_tile(self.handle, int(n)))

    def test_crowd_divergence_chunk_rows(self, rows: int = 0):
        """Test switch: the crowd divergence takes ``rows`` rows per chunk (0: the default budget); results do not depend on
        it (include/vet.h: vet_test_crowd_divergence_chunk_rows)."""
        _check(self.lib, self.lib.vet_test_crowd_divergence_chunk_rows(self.handle, int(rows)))

    def profile_enable(self, on: bool = True):
        _check(self.lib, self.lib.vet_profile_enable(self.handle, int(on)))

    def profile_reset(self):
        _check(self.lib, self.lib.vet_profile_reset(self.handle))

    def profile_get(self, kernel: str):
        ms, n = C.c_double(), C.c_int64()
        _check(self.lib, self.lib.vet_profile_get(self.handle, KERNEL_IDS[kernel], C.byref(ms), C.byref(n)))
        return ms.value, n.value


class DeviceResult:
    """Optional outputs of one run, resident in device memory (include/vet.h: vet_result).  ``rows(which, r0, n)``
    copies rows [r0, r0+n) of output ``which`` (0 = assignments / pairs, 1 = weights / source counts)."""

    def __init__(self, lib, handle, n_rows, shapes, dtypes, engine=None):
        self.lib, self.handle, self.n_rows = lib, handle, int(n_rows)
        self.shapes, self.dtypes = shapes, dtypes
        self.engine = engine           # keeps the device context alive as long as the rows can be fetched

    def rows(self, which: int, row0: int, n: int) -> np.ndarray:
        if self.handle is None:
            raise RuntimeError("the device-resident result has been released")
        out = np.empty((n,) + tuple(self.shapes[which]), dtype=self.dtypes[which])
        _check(self.lib, self.lib.vet_result_fetch(self.handle, which, row0, n, _ptr(out)))
        return out

    def close(self):
        if getattr(self, "handle", None):
            self.lib.vet_result_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


_F64, _I32, _NP_I64 = np.float64, np.int32, np.int64
# The eleven row calls.  Plan method -> (C symbol stem: the (mu, mv) device entry, + "_ids", + "_host"; window and stride count
# frame pairs, not frames (T - 1 of them, or T - lag for the call that takes a lag between the two frames of a pair); window=None is
# all of them; VET_ERR_EMPTY is a result (check=False); outputs).  An output is
# (result key, dims, dtype, optional); dims: U users, R rows, n tiles of lattice 0, L max_lag, M max_lag + 1 (a band that starts at
# lag 0: max_lag may be 0), Q fractions, B replicates, P permutations, 2, 3, 4, 5.  A call's extra arguments (max_lag; replicates, seed, confidence; the host array groups, permutations, seed, confidence) follow
# stride in the C signatures; ``_row_host`` takes them as ``extra``.  (transition_markov's extra is ``lag``.)
_ROW_CALLS = {
    "spatial_windowed": ("vet_spatial_entropy_windowed", False, False, True,
                         (("entropy", "R", _F64, False), ("weights", "Rn", _F64, True), ("samples", "R", _I32, False))),
    "spatial_per_user": ("vet_user_entropy", False, True, False,
                         (("entropy", "UR", _F64, False), ("weights", "URn", _F64, True), ("samples", "UR", _I32, False))),
    "spatial_user_divergence": ("vet_user_divergence", False, True, False,
                                (("divergence", "RUU", _F64, False), ("samples", "UR", _I32, False))),
    "spatial_crowd_divergence": ("vet_crowd_divergence", False, True, False,
                                 (("divergence", "UR", _F64, False), ("rows", "3R", _F64, False), ("samples", "UR", _I32, False))),
    "spatial_window_divergence": ("vet_window_divergence", False, False, False,
                                  (("divergence", "RL", _F64, False), ("samples", "R", _I32, False))),
    "spatial_coverage": ("vet_coverage", False, False, False,
                         (("tiles", "RQ", _I32, False), ("hit", "RMQ", _F64, False), ("order", "Rn", _I32, True),
                          ("samples", "R", _I32, False))),
    "spatial_bootstrap": ("vet_bootstrap_entropy", False, True, False,
                          (("summary", "4R", _F64, False), ("replicates", "RB", _F64, True), ("weights", "RBn", _F64, True),
                           ("valid", "R", _I32, False))),
    "spatial_group_divergence": ("vet_group_divergence", False, True, False,
                                 (("summary", "5R", _F64, False), ("null", "RP", _F64, True), ("weights", "R2n", _F64, True),
                                  ("samples", "2R", _I32, False), ("valid", "R", _I32, False))),
    "transition_windowed": ("vet_transition_entropy_windowed", True, False, True,
                            (("entropy", "R", _F64, False), ("srccount", "Rn", _I32, True), ("samples", "R", _I32, False))),
    "transition_per_user": ("vet_user_transition_entropy", True, True, False,
                            (("entropy", "UR", _F64, False), ("srccount", "URn", _I32, True), ("samples", "UR", _I32, False))),
    "transition_markov": ("vet_transition_markov", True, True, False,
                          (("stats", "5R", _F64, False), ("matrix", "Rnn", _I32, True), ("samples", "R", _I32, False))),
}

# The head-motion call, in a table of its own: a descriptor of the same form for each layout (per_user False / True; dims: Q
# fractions, H histogram bins).  Its extra arguments are lag, per_user and the two host arrays with their lengths.
_MOTION_CALLS = {
    False: ("vet_head_motion", True, True, False,
            (("stats", "4R", _F64, False), ("quantiles", "RQ", _F64, True), ("hist", "RH", _I32, True), ("still", "R", _I32, False),
             ("samples", "R", _I32, False))),
    True: ("vet_head_motion", True, True, False,
           (("stats", "4UR", _F64, False), ("quantiles", "URQ", _F64, True), ("hist", "URH", _I32, True), ("still", "UR", _I32, False),
            ("samples", "UR", _I32, False))),
}

# The dispersion call, in a table of its own: a descriptor of the same form for each layout (per_user False / True; dim H:
# histogram bins).  Rows count frames; its extra arguments are per_user and the host edges with their number of bins.
_DISPERSION_CALLS = {
    False: ("vet_dispersion", False, True, False,
            (("stats", "3R", _F64, False), ("centroid", "R3", _F64, False), ("hist", "RH", _NP_I64, True), ("counts", "4R", _NP_I64, False))),
    True: ("vet_dispersion", False, True, False,
           (("stats", "3UR", _F64, False), ("centroid", "UR3", _F64, False), ("hist", "URH", _NP_I64, True),
            ("counts", "4UR", _NP_I64, False))),
}

# The viewer-clusters call, in a table of its own: one descriptor of the same form (dims Q: fractions, W: the 64-bit words of a row
# of link bits).  Rows count frames; its extra arguments are cos_threshold, min_share and the host fractions with their number.
_CLUSTERS_CALL = ("vet_viewer_clusters", False, True, False,
                  (("labels", "RU", _I32, True), ("sizes", "RU", _I32, True), ("counts", "5R", _NP_I64, False), ("top", "RQ", _I32, True),
                   ("stats", "3R", _F64, False), ("centroids", "RU3", _F64, True), ("links", "RUW", np.uint64, True)))

# The fixations call, in a table of its own: a descriptor of the same form for each layout (per_user False / True; dims H: histogram
# bins, T: frames, V: viewers + 1, E: the listed events).  Rows count frames; its extra arguments are the mode, cos_threshold,
# min_frames, per_user, the host edges with their number of bins and max_events.
_FIXATION_CALLS = {
    False: ("vet_fixations", False, True, False,
            (("counts", "5R", _NP_I64, False), ("hist", "RH", _I32, True), ("labels", "UT", _I32, True), ("offsets", "V", _NP_I64, True),
             ("events", "E4", _I32, True), ("centroids", "E3", _F64, True))),
    True: ("vet_fixations", False, True, False,
           (("counts", "5UR", _NP_I64, False), ("hist", "URH", _I32, True), ("labels", "UT", _I32, True), ("offsets", "V", _NP_I64, True),
            ("events", "E4", _I32, True), ("centroids", "E3", _F64, True))),
}
FIXATION_MODES = {"angle": 0, "tile": 1}
FIXATION_COUNTS = ("samples", "fix_frames", "events", "sum_len", "max_len")

# The saliency call, in a table of its own: a descriptor of the same form for each layout (per_user False / True; dims Y, X: the
# map's rows and columns).  Rows count frames; its extra arguments are per_user, sigma in radians, the map's size and the scale.
_SALIENCY_CALLS = {
    False: ("vet_saliency", False, True, False,
            (("map", "RYX", _F64, True), ("stats", "4R", _F64, False), ("peak", "R", _I32, False), ("counts", "2R", _NP_I64, False))),
    True: ("vet_saliency", False, True, False,
           (("map", "URYX", _F64, True), ("stats", "4UR", _F64, False), ("peak", "UR", _I32, False), ("counts", "2UR", _NP_I64, False))),
}
SALIENCY_SCALES = {"none": 0, "mean": 1, "density": 2}

# The saliency similarity call, in a table of its own: one descriptor of the same form (dims Y, X: the map's rows and columns; 9
# statistics: cc, sim, jsd, kl_ab, kl_ba, nss_ab, nss_ba, mass_a, mass_b; 4 counts: samples_a, samples_b, distinct_a, distinct_b).
# Rows count frames; its extra arguments are the host array groups, sigma in radians and the map's size.
_SALIENCY_SIMILARITY_CALL = ("vet_saliency_similarity", False, True, False,
                             (("maps", "2RYX", _F64, True), ("stats", "9R", _F64, False), ("counts", "4R", _NP_I64, False)))
SALIENCY_SIMILARITY_STATS = ("cc", "sim", "jsd", "kl_ab", "kl_ba", "nss_ab", "nss_ba", "mass_a", "mass_b")

# The saliency scoring call, in a table of its own: one descriptor of the same form (dims Y, X: the map's rows and columns; 9
# statistics: auc, nss, info_gain, cc, sim, jsd, kl, mass, mass_pred; 2 counts: samples, distinct).  Rows count frames; its extra
# arguments are sigma in radians, the map's size, the predicted maps with their number and want_dist.
_SALIENCY_SCORE_CALL = ("vet_saliency_score", False, True, False,
                        (("map", "RYX", _F64, True), ("stats", "9R", _F64, False), ("counts", "2R", _NP_I64, False)))
SALIENCY_SCORE_STATS = ("auc", "nss", "info_gain", "cc", "sim", "jsd", "kl", "mass", "mass_pred")

# The congruency call, in a table of its own: one descriptor of the same form (3 statistics per viewer and row: lift, info_gain,
# nss; 3 counts: samples, distinct, others; 4 values per row: scored, mean lift, mean info_gain, mean nss).  Rows count frames; its
# extra arguments are sigma in radians and want_nss.
_CONGRUENCY_CALL = ("vet_congruency", False, True, False,
                    (("stats", "3UR", _F64, False), ("counts", "3UR", _NP_I64, False), ("rows", "4R", _F64, False)))
CONGRUENCY_STATS = ("lift", "info_gain", "nss")


class Plan:
    """Device tables of one analyzer configuration (quantiser, lattices, nearest LUTs)."""

    def __init__(self, engine: Engine, tile_xyz: Sequence[np.ndarray], fov_angle: float, power_factor: float,
                 use_weight_distribution: bool, video_width: int = 0, video_height: int = 0,
                 dir_table: Optional[np.ndarray] = None, bin_luts: Optional[Sequence] = None,
                 bin_counts: Optional[Sequence[int]] = None, bin_max_entropy: Optional[Sequence[float]] = None,
                 bin_norm_tiles: Optional[Sequence[int]] = None):
        """``tile_xyz``: one [n,3] array per lattice.  A *binned* lattice k (naive lat/lon tiling)
        passes ``tile_xyz[k] = None`` with ``bin_luts[k]`` (uint16 [n_dirs] direction -> bin),
        ``bin_counts[k]`` bins and the normaliser ``bin_max_entropy[k]``."""
        self.engine = engine
        self.lib = engine.lib
        bin_luts = list(bin_luts) if bin_luts is not None else [None] * len(tile_xyz)
        self.tiles = [np.ascontiguousarray(t, dtype=np.float64) if t is not None else np.zeros((1, 3))
                      for t in tile_xyz]
        self.n_tiles = [len(t) if b is None else int(bin_counts[k])
                        for k, (t, b) in enumerate(zip(self.tiles, bin_luts))]
        self.weighted = bool(use_weight_distribution)
        self.width, self.height = int(video_width), int(video_height)
        d = _PlanDesc()
        keep = []
        if dir_table is None:
            axes = _quantiser.axis_trig(self.width, self.height)
            keep.extend(axes)
            d.video_width, d.video_height = self.width, self.height
            d.h_lon_cos, d.h_lon_sin, d.h_lat_sin, d.h_lat_cos = (a.ctypes.data for a in axes)
        else:
            tab = np.ascontiguousarray(dir_table, dtype=np.float64).reshape(-1, 3)
            keep.append(tab)
            d.h_dir_table, d.n_dirs = tab.ctypes.data, len(tab)
        n_arr = np.asarray(self.n_tiles, dtype=np.int32)
        ptrs = (C.c_void_p * len(self.tiles))(*[t.ctypes.data for t in self.tiles])
        hmax = np.asarray([_quantiser.max_entropy(n) if b is None else float(bin_max_entropy[k])
                           for k, (n, b) in enumerate(zip(self.n_tiles, bin_luts))], dtype=np.float64)
        keep.extend([n_arr, ptrs, hmax])
        if any(b is not None for b in bin_luts):
            luts = [None if b is None else np.ascontiguousarray(b, dtype=np.uint16).reshape(-1) for b in bin_luts]
            lut_ptrs = (C.c_void_p * len(luts))(*[None if b is None else b.ctypes.data for b in luts])
            norm = np.asarray([n if b is None else int(bin_norm_tiles[k])
                               for k, (n, b) in enumerate(zip(self.n_tiles, bin_luts))], dtype=np.int32)
            keep.extend([luts, lut_ptrs, norm])
            d.h_bin_lut = C.cast(lut_ptrs, C.c_void_p)
            d.n_norm_tiles = norm.ctypes.data
        d.n_lattices = len(self.tiles)
        d.n_tiles = n_arr.ctypes.data
        d.h_tiles = C.cast(ptrs, C.c_void_p)
        d.h_max_entropy = hmax.ctypes.data
        d.fov_angle = float(fov_angle)
        d.max_angular_distance = float(np.radians(fov_angle / 2.0))
        d.power_factor = float(power_factor)
        d.use_weight_distribution = int(self.weighted)
        h = C.c_void_p()
        _check(self.lib, self.lib.vet_plan_create(engine.handle, C.byref(d), C.byref(h)))
        self.handle = h
        self.n_dirs = int(self.lib.vet_plan_n_dirs(h))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.vet_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):  # plans are small; free device tables with the Python object
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def set_table_policy(self, policy: int):
        """0 auto, 1 always use the direction weight table, -1 never (brute-force sweep)."""
        _check(self.lib, self.lib.vet_plan_set_table_policy(self.handle, int(policy)))

    def set_fp64(self, on: bool = True):
        """FP64 arithmetic end to end for the weighted Fibonacci lattices: the ``dtable`` formulation (exact FP64 weight rows,
        FP64 histograms) where the table policy asks for a table, ``precise`` otherwise (include/vet.h: vet_plan_set_fp64)."""
        _check(self.lib, self.lib.vet_plan_set_fp64(self.handle, 1 if on else 0))

    def set_raw_weights(self, on: bool = True):
        """Diagnostic: ``weights`` = the formulation's own histogram (table / sweep resolution) instead of the reference's
        values from the weights-only pass of the precise sweep (include/vet.h: vet_plan_set_raw_weights)."""
        _check(self.lib, self.lib.vet_plan_set_raw_weights(self.handle, 1 if on else 0))

    def table_stride(self, lattice: int = 0) -> int:
        return int(self.lib.vet_plan_table_stride(self.handle, lattice))

    def table_rows(self) -> int:
        """Rows of the plan's weight tables: distinct directions up to the lattices' mirror symmetry (0 before a table exists)."""
        return int(self.lib.vet_plan_table_rows(self.handle))

    def table_cap(self, lattice: int = 0):
        """(cap, overflow rows) of the lattice's own table: entries per main row, rows that continue in the overflow table
        (include/vet.h: vet_plan_table_cap); (0, 0) before the table exists."""
        n = C.c_int64()
        return int(self.lib.vet_plan_table_cap(self.handle, lattice, C.byref(n))), int(n.value)

    def record_bytes(self) -> int:
        """4 where the plan's table launches gather the compact direction record, 8 otherwise, 0 before the table exists
        (include/vet.h: vet_plan_record_bytes)."""
        return int(self.lib.vet_plan_record_bytes(self.handle))

    def read_records(self) -> np.ndarray:
        """The compact direction records [n_dirs] (include/vet.h: vet_plan_read_records)."""
        out = np.empty(self.n_dirs, dtype=np.uint32)
        _check(self.lib, self.lib.vet_plan_read_records(self.handle, _ptr(out)))
        return out

    def last_formulation(self, lattice: int = 0) -> str:
        """'table' | 'sweep' | 'precise' | 'ftable' | 'dtable' of the last weighted call ('' before any)."""
        return FORMULATIONS.get(int(self.lib.vet_plan_last_formulation(self.handle, lattice)), "")

    def last_table_kernel(self) -> dict:
        """The table kernel and geometry of the plan's last table launch (include/vet.h: vet_plan_last_table_kernel, VET_TK_*);
        {} before any.  ``fpw`` and ``chunked`` are per video in a batch launch and 0 / False there."""
        w = int(self.lib.vet_plan_last_table_kernel(self.handle))
        if not w & 1:
            return {}
        return dict(nb=(w >> 1) & 3, rec32=bool(w & 0x8), bucketed=bool(w & 0x10), dedup=bool(w & 0x20), il=bool(w & 0x40),
                    occ8=bool(w & 0x80), fp_table=bool(w & 0x100), fused=bool(w & 0x200), narrow=bool(w & 0x400),
                    from_ids=bool(w & 0x800), batch=bool(w & 0x1000), chunked=bool(w & 0x2000), fpw=(w >> 16) & 0xFF)

    def error_bounds(self, lattice: int = 0):
        """(table bound, sweep bound): proven worst-case relative entropy error of the integer formulations."""
        a, b = C.c_double(), C.c_double()
        _check(self.lib, self.lib.vet_plan_error_bounds(self.handle, lattice, C.byref(a), C.byref(b)))
        return a.value, b.value

    # --- parity hooks ---------------------------------------------------------
    def read_dirs(self) -> np.ndarray:
        out = np.empty((self.n_dirs, 3), dtype=np.float64)
        _check(self.lib, self.lib.vet_plan_read_dirs(self.handle, _ptr(out)))
        return out

    def read_nearest(self, lattice: int = 0) -> np.ndarray:
        out = np.empty(self.n_dirs, dtype=np.int32)
        _check(self.lib, self.lib.vet_plan_read_nearest(self.handle, lattice, _ptr(out)))
        return out

    def read_table(self, lattice: int = 0) -> dict:
        """The lattice's own weight table as built on the device: w / tile [rows+1, stride], meta [rows+1] and, for a capped
        table, ovf_w / ovf_tile [overflow rows + 1, 64] and ovf_of_row [rows] (include/vet.h: vet_plan_read_table)."""
        cap, n_ovf = self.table_cap(lattice)
        if cap <= 0:
            raise ValueError("the lattice has no table of its own (yet)")
        rows = self.table_rows()
        out = {"w": np.empty((rows + 1, cap), np.uint32), "tile": np.empty((rows + 1, cap), np.uint16),
               "meta": np.empty(rows + 1, np.uint32)}
        if n_ovf:
            out.update(ovf_w=np.empty((n_ovf + 1, 64), np.uint32), ovf_tile=np.empty((n_ovf + 1, 64), np.uint16),
                       ovf_of_row=np.empty(rows, np.uint32))
        _check(self.lib, self.lib.vet_plan_read_table(self.handle, lattice, _ptr(out["w"]), _ptr(out["tile"]), _ptr(out["meta"]),
                                                      _ptr(out["ovf_w"]) if "ovf_w" in out else None,
                                                      _ptr(out["ovf_tile"]) if "ovf_tile" in out else None,
                                                      _ptr(out["ovf_of_row"]) if "ovf_of_row" in out else None))
        return out

    # --- host-buffer runs (what the analyzers use) ---------------------------
    @staticmethod
    def _samples(mu, mv, ids):
        if ids is not None:
            ids = np.ascontiguousarray(ids, dtype=np.int32)
            return None, None, ids, ids.shape
        mu = np.ascontiguousarray(mu, dtype=np.float64)
        mv = np.ascontiguousarray(mv, dtype=np.float64)
        if mu.shape != mv.shape or mu.ndim != 2:
            raise ValueError("mu and mv must be [n_frames, n_users] arrays of equal shape")
        return mu, mv, None, mu.shape

    def _row_host(self, call, mu, mv, ids, window, stride, want_optional, check, max_lag=None, extra=(), extra_dims=None,
                  pair_lag=1):
        """The host wrapper of row call ``call`` (a name in _ROW_CALLS, or a descriptor of that form): arguments, outputs, the
        ``_host`` entry, the result dict.
        ``want_optional``: one bool for every optional output, or the set of the wanted keys.  ``extra``: the call's scalars behind
        stride (after max_lag, where the call has one), passed as they are; ``extra_dims``: the output dimensions they define.
        ``pair_lag``: the frames between the two frames of a pair (a call over pairs has T - pair_lag of them)."""
        stem, pairs, whole, empty_ok, outputs = _ROW_CALLS[call] if isinstance(call, str) else call
        mu, mv, ids, (T, U) = self._samples(mu, mv, ids)
        n, unit, bound = (T - pair_lag, "frame pairs", f"n_frames - {pair_lag}") if pairs else (T, "frames", "n_frames")
        if window is None and not whole:
            raise ValueError(f"window (a number of {unit}) is required")
        window, stride = n if window is None else int(window), int(stride)
        axes = "".join(shape for _, shape, _, _ in outputs)
        lag = (int(max_lag),) if "L" in axes or "M" in axes else ()     # an output with a lag axis: the call takes max_lag
        lag_min = 0 if "M" in axes else 1                         # M: the band holds lag 0 too
        R = int(self.lib.vet_window_rows(n, window, stride))
        if R < 0:
            raise ValueError(f"need 1 <= window <= {bound} and stride >= 1 (got window={window}, stride={stride}, {T} frames)")
        if lag and not lag_min <= lag[0] <= R - 1:
            raise ValueError(f"need {lag_min} <= max_lag <= rows - 1 = {R - 1} (got max_lag={lag[0]}; window={window}, stride={stride}, "
                             f"{T} frames give {R} rows)")
        dims = {"U": U, "R": R, "n": self.n_tiles[0], "L": lag[0] if lag else 0, "M": lag[0] + 1 if lag else 1, "3": 3, "4": 4,
                **(extra_dims or {})}
        wanted = (lambda key: key in want_optional) if isinstance(want_optional, (set, frozenset)) else (lambda key: want_optional)
        out = {key: None if optional and not wanted(key) else np.empty(tuple(dims[d] for d in shape), dtype=dtype)
               for key, shape, dtype, optional in outputs}
        rc = getattr(self.lib, stem + "_host")(self.handle, _ptr(mu), _ptr(mv), _ptr(ids), U, T, window, stride, *lag, *extra,
                                               *(_ptr(a) for a in out.values()))
        if rc not in (VET_OK, VET_ERR_RANGE) + ((VET_ERR_EMPTY,) if empty_ok else ()) or (check and rc != VET_OK):
            _check(self.lib, rc)
        return dict(out, code=rc)

    def _row_device(self, call, d_mu, d_mv, d_ids, n_users, n_frames, scalars, d_out, d_optional, stream):
        """The device wrapper of row call ``call`` (a name in _ROW_CALLS, or a descriptor of that form): the ``_ids`` entry when
        ``d_ids`` is given, else the (mu, mv) entry."""
        stem = (_ROW_CALLS[call] if isinstance(call, str) else call)[0]
        entry, samples = (getattr(self.lib, stem + "_ids"), (d_ids,)) if d_ids else (getattr(self.lib, stem), (d_mu, d_mv))
        _check(self.lib, entry(self.handle, *samples, n_users, n_frames, *(v if isinstance(v, float) else int(v) for v in scalars), d_out,
                               *(p or None for p in d_optional), _stream(stream)))

    def spatial(self, mu=None, mv=None, ids=None, want_assign=True, want_weights=False, check=True):
        """Returns dict(entropy[T], assign[T,U]|None, weights[T,n0]|None, present[T], code)."""
        mu, mv, ids, (T, U) = self._samples(mu, mv, ids)
        ent = np.empty(T, dtype=np.float64)
        assign = np.empty((T, U), dtype=np.int32) if want_assign else None
        weights = np.empty((T, self.n_tiles[0]), dtype=np.float64) if want_weights else None
        present = np.empty(T, dtype=np.int32)
        rc = self.lib.vet_spatial_entropy_host(self.handle, _ptr(mu), _ptr(mv), _ptr(ids), U, T, _ptr(ent),
                                               _ptr(assign), _ptr(weights), _ptr(present))
        if rc not in (VET_OK, VET_ERR_EMPTY, VET_ERR_RANGE) or (check and rc != VET_OK):
            _check(self.lib, rc)
        return dict(entropy=ent, assign=assign, weights=weights, present=present, code=rc)

    def spatial_windowed(self, mu=None, mv=None, ids=None, window=None, stride=1, want_weights=False, check=True):
        """Pooled entropy of sliding frame windows (include/vet.h: vet_spatial_entropy_windowed): row r pools every present
        sample of frames [r * stride, r * stride + window) into one histogram per lattice.  ``window`` and ``stride`` count
        frames.  Returns dict(entropy[R], weights[R,n0]|None, samples[R], code), R = (T - window) // stride + 1."""
        return self._row_host("spatial_windowed", mu, mv, ids, window, stride, want_weights, check)

    def spatial_per_user(self, mu=None, mv=None, ids=None, window=None, stride=1, want_weights=False, check=True):
        """Each user's own tile histogram over time (include/vet.h: vet_user_entropy): row (u, r) pools user u's present
        samples of frames [r * stride, r * stride + window) into one histogram per lattice.  ``window=None`` is the whole
        video (one row per user).  Returns dict(entropy[U,R], weights[U,R,n0]|None, samples[U,R], code),
        R = (T - window) // stride + 1.  Rows in which the user has no sample are NaN with ``samples`` 0 — data, never an
        error; ``code`` is VET_OK or VET_ERR_RANGE."""
        return self._row_host("spatial_per_user", mu, mv, ids, window, stride, want_weights, check)

    def spatial_user_divergence(self, mu=None, mv=None, ids=None, window=None, stride=1, check=True):
        """Do viewers look at the same places (include/vet.h: vet_user_divergence): for every row r — frames
        [r * stride, r * stride + window), ``window=None`` the whole video — the U x U matrix of mass-weighted Jensen-Shannon
        divergences, in bits, between the viewers' tile histograms of the row (``spatial_per_user``'s ``weights``), averaged
        over the lattices.  Returns dict(divergence[R,U,U], samples[U,R], code), R = (T - window) // stride + 1.  The matrix
        is symmetric with a +0.0 diagonal; the rows and columns of a viewer without a sample in the row are NaN with
        ``samples`` 0 — data, never an error; ``code`` is VET_OK or VET_ERR_RANGE."""
        return self._row_host("spatial_user_divergence", mu, mv, ids, window, stride, False, check)

    def spatial_crowd_divergence(self, mu=None, mv=None, ids=None, window=None, stride=1, check=True):
        """How typical each viewer is of the audience (include/vet.h: vet_crowd_divergence): for every row r — frames
        [r * stride, r * stride + window), ``window=None`` the whole video — and viewer u the Kullback-Leibler divergence, in
        bits, of the viewer's tile histogram (``spatial_per_user``'s ``weights``) from the row's pooled histogram
        (``spatial_windowed``'s ``weights``), averaged over the lattices: 0 = the crowd's places in the crowd's proportions,
        log2(W_r / W_u) = no tile shared with anybody.  Returns dict(divergence[U,R], rows[3,R], samples[U,R], code),
        R = (T - window) // stride + 1; ``rows`` holds pooled = S(P_r), within = sum_u (W_u / W_r) S(h_u) and
        between = sum_u (W_u / W_r) D(u, r), pooled = within + between.  A viewer without a sample in the row is NaN with
        ``samples`` 0 — data, never an error; ``code`` is VET_OK or VET_ERR_RANGE."""
        return self._row_host("spatial_crowd_divergence", mu, mv, ids, window, stride, False, check)

    def spatial_window_divergence(self, mu=None, mv=None, ids=None, window=None, stride=1, max_lag=1, check=True):
        """When does the audience's attention move (include/vet.h: vet_window_divergence): for every row r — frames
        [r * stride, r * stride + window) — and every lag l = 1 .. max_lag the mass-weighted Jensen-Shannon divergence, in bits,
        between the pooled tile histograms of rows r and r + l (``spatial_windowed``'s ``weights``), averaged over the lattices.
        Returns dict(divergence[R,L], samples[R], code), R = (T - window) // stride + 1, ``divergence[r, l - 1] = D(r, l)``.
        Entries with r + l >= R are NaN, and so is every pair with a window that has no sample (``samples`` 0) — data, never an
        error; ``code`` is VET_OK or VET_ERR_RANGE."""
        return self._row_host("spatial_window_divergence", mu, mv, ids, window, stride, False, check, max_lag)

    @staticmethod
    def _fraction_array(fractions):
        """``fractions`` as the C entry takes it: float64 [Q], 1 <= Q <= 8, each in (0, 1], strictly increasing; ``ValueError``
        otherwise."""
        try:
            f = np.ascontiguousarray(fractions, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"fractions must be a sequence of numbers (got {fractions!r})")
        if f.ndim != 1 or not 1 <= f.size <= 8:
            raise ValueError(f"need 1 to 8 fractions in a one-dimensional sequence (got shape {f.shape})")
        if not ((f > 0.0) & (f <= 1.0)).all():
            raise ValueError(f"fractions must lie in (0, 1] (got {f.tolist()})")
        if not (np.diff(f) > 0.0).all():
            raise ValueError(f"fractions must be strictly increasing (got {f.tolist()})")
        return f

    def spatial_coverage(self, mu=None, mv=None, ids=None, window=None, stride=1, max_lag=0, fractions=(0.5, 0.8, 0.95),
                         want_order=False, check=True):
        """Which tiles hold the audience's attention, and for how long (include/vet.h: vet_coverage): for every row r — frames
        [r * stride, r * stride + window) — lattice 0's tiles are ranked by the row's pooled weight (``spatial_windowed``'s
        ``weights`` by absolute value; descending, equal weights by tile index) and ``tiles[r, i]`` is the smallest number of
        top-ranked tiles whose running sum reaches ``fractions[i]`` of the row's mass; ``hit[r, l, i]`` is the share of row
        r + l's mass that those tiles hold, l = 0 .. max_lag (lag 0: the coverage reached; later lags: the forecast).  Returns
        dict(tiles[R,Q], hit[R,L+1,Q], order[R,n0]|None, samples[R], code), R = (T - window) // stride + 1.  A row without mass
        has ``tiles`` 0 and NaN ``hit``; entries with r + l >= R and lags that reach a row without mass are NaN — data, never an
        error; ``code`` is VET_OK or VET_ERR_RANGE."""
        f = self._fraction_array(fractions)
        return self._row_host("spatial_coverage", mu, mv, ids, window, stride, bool(want_order), check, max_lag,
                              extra=(_ptr(f), int(f.size)), extra_dims={"Q": int(f.size)})

    @staticmethod
    def _bootstrap_scalars(replicates, seed, confidence):
        """(replicates, seed, confidence) as the C entry takes them; ``ValueError`` outside [1, 4096], [0, 2^64) and (0, 1)."""
        replicates, seed, confidence = int(replicates), int(seed), float(confidence)
        if not 1 <= replicates <= 4096:
            raise ValueError(f"replicates must be between 1 and 4096 (got {replicates})")
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"seed must be an unsigned 64-bit integer (got {seed})")
        if not 0.0 < confidence < 1.0:
            raise ValueError(f"confidence must be inside (0, 1) (got {confidence})")
        return replicates, seed, confidence

    def spatial_bootstrap(self, mu=None, mv=None, ids=None, window=None, stride=1, replicates=200, seed=0, confidence=0.95,
                          want_replicates=False, want_weights=False, check=True):
        """Bootstrap confidence bands over viewers (include/vet.h: vet_bootstrap_entropy): the audience is resampled with
        replacement ``replicates`` times — the same resample for every row: a viewer's trajectory stays together — and every row
        of ``spatial_windowed`` (frames [r * stride, r * stride + window), ``window=None`` the whole video) is recomputed for each
        resample.  Returns dict(summary[4,R] (mean, sd, lo, hi over the finite replicates), replicates[R,B]|None,
        weights[R,B,n0]|None (lattice 0's replicate histograms, plain values), valid[R], code), R = (T - window) // stride + 1.
        A replicate whose drawn viewers have no sample in the row is NaN — data, never an error; ``code`` is VET_OK or
        VET_ERR_RANGE."""
        replicates, seed, confidence = self._bootstrap_scalars(replicates, seed, confidence)
        want = {k for k, on in (("replicates", want_replicates), ("weights", want_weights)) if on}
        return self._row_host("spatial_bootstrap", mu, mv, ids, window, stride, want, check,
                              extra=(replicates, seed, confidence), extra_dims={"B": replicates})

    def bootstrap_counts(self, n_users: int, replicates: int, seed: int = 0) -> np.ndarray:
        """The bootstrap's draw alone, computed on the device: counts[replicates, n_users] uint16, how often replicate b picked
        viewer u (include/vet.h: vet_bootstrap_counts_host)."""
        replicates, seed, _ = self._bootstrap_scalars(replicates, seed, 0.5)
        out = np.empty((replicates, int(n_users)), dtype=np.uint16)
        _check(self.lib, self.lib.vet_bootstrap_counts_host(self.handle, int(n_users), replicates, seed, _ptr(out)))
        return out

    @staticmethod
    def _group_array(groups, n_users=None):
        """``groups`` as the C entry takes it: int8 [U] of 0 (audience A), 1 (audience B), -1 (excluded), both audiences with a
        viewer; ``ValueError`` otherwise."""
        g = np.asarray(groups)
        if g.ndim != 1 or g.size == 0 or g.dtype.kind not in "iu":
            raise ValueError("groups must be a one-dimensional integer array: 0 = audience A, 1 = audience B, -1 = excluded")
        if n_users is not None and g.size != n_users:
            raise ValueError(f"groups has {g.size} entries for {n_users} users")
        if not np.isin(g, (-1, 0, 1)).all():
            raise ValueError("groups holds values outside {-1, 0, 1}")
        if not (g == 0).any() or not (g == 1).any():
            raise ValueError("both audiences need a viewer")
        return np.ascontiguousarray(g, dtype=np.int8)

    @staticmethod
    def _group_scalars(permutations, seed, confidence):
        """(permutations, seed, confidence) as the C entry takes them; ``ValueError`` outside [1, 4096], [0, 2^64) and (0, 1)."""
        permutations, seed, confidence = int(permutations), int(seed), float(confidence)
        if not 1 <= permutations <= 4096:
            raise ValueError(f"permutations must be between 1 and 4096 (got {permutations})")
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"seed must be an unsigned 64-bit integer (got {seed})")
        if not 0.0 < confidence < 1.0:
            raise ValueError(f"confidence must be inside (0, 1) (got {confidence})")
        return permutations, seed, confidence

    def spatial_group_divergence(self, mu=None, mv=None, ids=None, groups=None, window=None, stride=1, permutations=999, seed=0,
                                 confidence=0.95, want_null=False, want_weights=False, check=True):
        """The two-audience permutation test (include/vet.h: vet_group_divergence): ``groups`` [U] is 0 (audience A), 1 (audience
        B) or -1 (excluded); every row of ``spatial_windowed`` (frames [r * stride, r * stride + window), ``window=None`` the
        whole video) gets the mass-weighted Jensen-Shannon divergence between the two audiences' pooled histograms, in bits, and
        its place among ``permutations`` relabellings of the included viewers — the same relabelling for every row: a viewer's
        trajectory stays together.  Returns dict(summary[5,R] (observed, p_value, p_adjusted, null_mean, null_crit),
        null[R,P]|None, weights[R,2,n0]|None (lattice 0's histograms of A and B, plain values), samples[2,R], valid[R], code),
        R = (T - window) // stride + 1.  A row in which an audience has no sample is NaN — data, never an error; ``code`` is
        VET_OK or VET_ERR_RANGE."""
        permutations, seed, confidence = self._group_scalars(permutations, seed, confidence)
        first = ids if ids is not None else mu
        g = self._group_array(groups, np.shape(first)[1] if np.ndim(first) == 2 else None)
        want = {k for k, on in (("null", want_null), ("weights", want_weights)) if on}
        return self._row_host("spatial_group_divergence", mu, mv, ids, window, stride, want, check,
                              extra=(_ptr(g), permutations, seed, confidence), extra_dims={"P": permutations, "2": 2, "5": 5})

    def group_labels(self, groups, permutations: int, seed: int = 0) -> np.ndarray:
        """The permutation test's draw alone, computed on the device: labels[permutations + 1, U] uint8 (0 = A, 1 = B, 255 =
        excluded); row 0 is ``groups`` itself, row b + 1 permutation b (include/vet.h: vet_group_labels_host)."""
        permutations, seed, _ = self._group_scalars(permutations, seed, 0.5)
        g = self._group_array(groups)
        out = np.empty((permutations + 1, g.size), dtype=np.uint8)
        _check(self.lib, self.lib.vet_group_labels_host(self.handle, int(g.size), _ptr(g), permutations, seed, _ptr(out)))
        return out

    def transition(self, mu=None, mv=None, ids=None, want_pairs=True, want_srccount=False, check=True):
        """Returns dict(entropy[T-1], pairs[T-1,U,2]|None, srccount[T-1,n0]|None, common[T-1], code)."""
        mu, mv, ids, (T, U) = self._samples(mu, mv, ids)
        R = max(T - 1, 0)
        ent = np.empty(R, dtype=np.float64)
        pairs = np.empty((R, U, 2), dtype=np.int32) if want_pairs else None
        src = np.empty((R, self.n_tiles[0]), dtype=np.int32) if want_srccount else None
        common = np.empty(R, dtype=np.int32)
        rc = self.lib.vet_transition_entropy_host(self.handle, _ptr(mu), _ptr(mv), _ptr(ids), U, T, _ptr(ent),
                                                  _ptr(pairs), _ptr(src), _ptr(common))
        if rc not in (VET_OK, VET_ERR_EMPTY, VET_ERR_RANGE) or (check and rc != VET_OK):
            _check(self.lib, rc)
        return dict(entropy=ent, pairs=pairs, srccount=src, common=common, code=rc)

    def transition_windowed(self, mu=None, mv=None, ids=None, window=None, stride=1, want_srccount=False, check=True):
        """Pooled transition entropy of sliding windows of frame pairs (include/vet.h: vet_transition_entropy_windowed): row r
        pools the transitions of pairs [r * stride, r * stride + window), pair f = (frame f, frame f + 1).  ``window`` and
        ``stride`` count frame pairs.  Returns dict(entropy[R], srccount[R,n0]|None, samples[R], code),
        R = (T - 1 - window) // stride + 1."""
        return self._row_host("transition_windowed", mu, mv, ids, window, stride, want_srccount, check)

    @staticmethod
    def _pair_lag(lag, n_frames=None):
        """``lag`` as an int; ``ValueError`` unless it is an integer with 1 <= lag <= n_frames - 1."""
        if isinstance(lag, bool) or not isinstance(lag, (int, np.integer)):
            raise ValueError(f"lag must be an integer number of frames (got {lag!r})")
        if lag < 1 or (n_frames is not None and lag > n_frames - 1):
            raise ValueError(f"need 1 <= lag <= n_frames - 1 (got lag={lag}" + (f", {n_frames} frames)" if n_frames is not None else ")"))
        return int(lag)

    def transition_markov(self, mu=None, mv=None, ids=None, window=None, stride=1, lag=1, want_matrix=False, check=True):
        """Tile-to-tile transition statistics of sliding windows of frame pairs (include/vet.h: vet_transition_markov): pair f is
        (frame f, frame f + lag), row r pools the (pair, user) samples of pairs [r * stride, r * stride + window) present in both
        frames into integer counts n_pc per (source tile, destination tile).  ``window`` and ``stride`` count pairs;
        ``window=None`` is all T - lag pairs (one row: the whole video).  Returns dict(stats[5,R] (rate = H(next | current),
        stationary = H(current), dest = H(next), mutual = dest - rate, stay; bits, mean over the lattices), matrix[R,n0,n0]|None
        (lattice 0's counts, source-major), samples[R], code), R = (T - lag - window) // stride + 1.  A row without a pooled sample
        is NaN with ``samples`` 0 and a zero matrix — data, never an error; ``code`` is VET_OK or VET_ERR_RANGE."""
        first = ids if ids is not None else mu
        lag = self._pair_lag(lag, np.shape(first)[0] if np.ndim(first) == 2 else None)
        return self._row_host("transition_markov", mu, mv, ids, window, stride, bool(want_matrix), check, extra=(lag,),
                              extra_dims={"5": 5}, pair_lag=lag)

    @staticmethod
    def _motion_arrays(quantiles, edges):
        """(fractions float64 [Q] or None, edges float64 [B + 1] or None) as the C entry takes them; ``ValueError`` unless 0 <= Q <= 8
        fractions in [0, 1], strictly increasing, and 1 <= B <= 64 bins between finite, strictly ascending edges."""
        def array(values, what):
            try:
                a = np.ascontiguousarray(values, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"{what} must be a sequence of numbers (got {values!r})")
            if a.ndim != 1:
                raise ValueError(f"{what} must be a one-dimensional sequence (got shape {a.shape})")
            return a
        f = e = None
        if quantiles is not None and len(quantiles):
            f = array(quantiles, "quantiles")
            if f.size > 8:
                raise ValueError(f"need at most 8 quantiles (got {f.size})")
            if not ((f >= 0.0) & (f <= 1.0)).all():
                raise ValueError(f"quantiles must lie in [0, 1] (got {f.tolist()})")
            if not (np.diff(f) > 0.0).all():
                raise ValueError(f"quantiles must be strictly increasing (got {f.tolist()})")
        if edges is not None:
            e = array(edges, "edges")
            if not 2 <= e.size <= 65:
                raise ValueError(f"need 2 to 65 histogram edges, 1 to 64 bins (got {e.size})")
            if not np.isfinite(e).all() or not (np.diff(e) > 0.0).all():
                raise ValueError(f"edges must be finite and strictly ascending (got {e.tolist()})")
        return f, e

    def head_motion(self, mu=None, mv=None, ids=None, window=None, stride=1, lag=1, per_user=False, quantiles=(0.5, 0.9, 0.99),
                    edges=None, check=True):
        """How fast heads turn (include/vet.h: vet_head_motion): pair f is (frame f, frame f + lag); a (pair, viewer) present in both
        frames is a sample, its angle (radians) the reference's ``vector_angle_distance`` of the two Vectors, +0.0 exactly where they
        are the same Vector (still).  Row r pools the samples of pairs [r * stride, r * stride + window) over all viewers, or with
        ``per_user`` row (u, r) holds viewer u's own (outputs user-major, a leading U axis).  ``window`` and ``stride`` count pairs;
        ``window=None`` is all T - lag pairs.  Returns dict(stats[4,R] (mean, sd with ddof = 1, max, total), quantiles[R,Q]|None
        (linear interpolation between exact order statistics), hist[R,B]|None (``edges``: B + 1 ascending values in radians, bins
        half-open), still[R], samples[R], code), R = (T - lag - window) // stride + 1.  A row without a sample is NaN with ``samples``
        0 — data, never an error; ``code`` is VET_OK or VET_ERR_RANGE."""
        first = ids if ids is not None else mu
        lag = self._pair_lag(lag, np.shape(first)[0] if np.ndim(first) == 2 else None)
        f, e = self._motion_arrays(quantiles, edges)
        Q, B = (0 if f is None else int(f.size)), (0 if e is None else int(e.size) - 1)
        want = {key for key, a in (("quantiles", f), ("hist", e)) if a is not None}
        return self._row_host(_MOTION_CALLS[bool(per_user)], mu, mv, ids, window, stride, want, check,
                              extra=(lag, int(bool(per_user)), _ptr(f), Q, _ptr(e), B), extra_dims={"Q": Q, "H": B}, pair_lag=lag)

    @staticmethod
    def _dispersion_edges(edges, per_user=False):
        """edges float64 [B + 1] or None, as the C entry takes them; ``ValueError`` unless there are 1 <= B <= 64 bins between finite,
        strictly ascending edges, and none with ``per_user`` (the per-viewer layout has no histogram)."""
        if edges is None:
            return None
        if per_user:
            raise ValueError("edges: the per-viewer layout has no histogram (pass edges=None with per_user)")
        return Plan._motion_arrays(None, edges)[1]

    def dispersion(self, mu=None, mv=None, ids=None, window=1, stride=1, per_user=False, edges=None, check=True):
        """How tightly the audience looks together (include/vet.h: vet_dispersion): a pair sample is two viewers present in the same
        frame, its angle (radians) the great-circle angle between their directions — the reference's ``vector_angle_distance``, +0.0
        exactly where the two Vectors are the same.  Row r pools the pair samples of frames [r * stride, r * stride + window), or
        with ``per_user`` row (u, r) holds them from viewer u's side (outputs user-major, a leading U axis).  ``window=None`` is
        the whole video.  Returns dict(stats[3,R] (mean, max, nearest: the mean angle to the nearest partner), centroid[R,3] (the
        sum of the present viewers' unit vectors), hist[R,B]|None (``edges``: B + 1 ascending values in radians, bins half-open;
        pooled only), counts[4,R] int64 (samples, same, slots, present), code), R = (T - window) // stride + 1.  A row that never
        has two viewers in one frame is NaN with ``samples`` 0 — data, never an error; ``code`` is VET_OK or VET_ERR_RANGE."""
        e = self._dispersion_edges(edges, per_user)
        B = 0 if e is None else int(e.size) - 1
        return self._row_host(_DISPERSION_CALLS[bool(per_user)], mu, mv, ids, window, stride, {"hist"} if e is not None else set(),
                              check, extra=(int(bool(per_user)), _ptr(e), B), extra_dims={"H": B})

    @staticmethod
    def _cluster_args(threshold_deg, min_share, fractions):
        """(cos_threshold, min_share, fractions float64 [Q] or None) as the C entry takes them; ``ValueError`` unless threshold_deg
        is a finite number of degrees in [0, 180], 0 < min_share <= 1 and there are at most 16 fractions, each in (0, 1]."""
        def number(v):
            return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(v)
        if not number(threshold_deg) or not 0.0 <= float(threshold_deg) <= 180.0:
            raise ValueError(f"threshold_deg must be a finite number of degrees in [0, 180] (got {threshold_deg!r})")
        if not number(min_share) or not 0.0 < float(min_share) <= 1.0:
            raise ValueError(f"min_share must be a number in (0, 1] (got {min_share!r})")
        f = None
        if fractions is not None and len(fractions):
            try:
                f = np.ascontiguousarray(fractions, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"fractions must be a sequence of numbers (got {fractions!r})")
            if f.ndim != 1 or f.size > 16:
                raise ValueError(f"need at most 16 fractions in a one-dimensional sequence (got shape {f.shape})")
            if not ((f > 0.0) & (f <= 1.0)).all():
                raise ValueError(f"fractions must lie in (0, 1] (got {f.tolist()})")
        cos_threshold = min(1.0, max(-1.0, math.cos(math.radians(float(threshold_deg)))))
        return cos_threshold, float(min_share), f

    def viewer_clusters(self, mu=None, mv=None, ids=None, window=1, stride=1, threshold_deg=30.0, min_share=1.0,
                        fractions=(0.5, 0.8, 0.95), want_labels=True, want_centroids=False, want_links=False, cos_threshold=None,
                        check=True):
        """Who looks together (include/vet.h: vet_viewer_clusters): in a frame two present viewers are NEAR when the angle between
        their directions is at most ``threshold_deg`` (decided on the cosine, ``math.cos(math.radians(threshold_deg))``, or
        ``cos_threshold`` itself where that is given; the same Vector is always near); in row r — frames
        [r * stride, r * stride + window), ``window=None`` the whole video — a pair is LINKED when it is NEAR in at least
        ``min_share`` of the frames both are in, and the row's clusters are the connected components of the LINKED graph, numbered
        by their smallest member.  ``threshold_deg = 30`` is a choice for head-direction data, not taken from the reference, which
        has no such call.  Returns dict(labels[R,U]|None (-1: not in the row), sizes[R,U]|None (both ``want_labels``),
        counts[5,R] int64 (viewers, clusters, largest, singletons, links), top[R,Q]|None (the fewest clusters, largest first, that
        hold ``fractions[i]`` of the row's viewers), stats[3,R] (partition entropy in bits, the same over log2 viewers, largest /
        viewers), centroids[R,U,3]|None (``want_centroids``: per cluster the sum of its members' unit vectors), links[R,U,ceil(U /
        64)] uint64|None (``want_links``: bit v of row u), cos_threshold, code), R = (T - window) // stride + 1.  A row without a
        viewer has labels -1, zero counts and NaN stats — data, never an error; ``code`` is VET_OK or VET_ERR_RANGE."""
        c, share, f = self._cluster_args(threshold_deg, min_share, fractions)
        if cos_threshold is not None:
            c = float(cos_threshold)
        Q = 0 if f is None else int(f.size)
        first = ids if ids is not None else mu
        U = int(np.shape(first)[1]) if np.ndim(first) == 2 else 0
        want = {key for key, on in (("labels", want_labels), ("sizes", want_labels), ("top", Q > 0), ("centroids", want_centroids),
                                    ("links", want_links)) if on}
        res = self._row_host(_CLUSTERS_CALL, mu, mv, ids, window, stride, want, check, extra=(c, share, _ptr(f), Q),
                             extra_dims={"Q": Q, "5": 5, "W": (U + 63) // 64})
        return dict(res, cos_threshold=c)

    @staticmethod
    def _fixation_args(max_step_deg, min_frames, edges):
        """(cos_threshold, min_frames, edges int32 [B + 1] or None) as the C entry takes them; ``ValueError`` unless max_step_deg is
        a finite number of degrees in [0, 180], min_frames an integer >= 1, and the edges (where given) 2 to 65 integers >= 1,
        strictly ascending."""
        def number(v):
            return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(v)

        def integer(v):
            return not isinstance(v, bool) and isinstance(v, (int, np.integer))
        if not number(max_step_deg) or not 0.0 <= float(max_step_deg) <= 180.0:
            raise ValueError(f"max_step_deg must be a finite number of degrees in [0, 180] (got {max_step_deg!r})")
        if not integer(min_frames) or int(min_frames) < 1:
            raise ValueError(f"min_frames must be an integer number of frames, at least 1 (got {min_frames!r})")
        e = None
        if edges is not None:
            if isinstance(edges, (str, bytes)) or not hasattr(edges, "__len__"):
                raise ValueError(f"edges must be a sequence of integers (got {edges!r})")
            vals = list(edges)
            if not all(integer(v) for v in vals):
                raise ValueError(f"edges must be integer numbers of frames (got {vals!r})")
            if not 2 <= len(vals) <= 65:
                raise ValueError(f"need 2 to 65 edges, 1 to 64 bins (got {len(vals)})")
            if any(not 1 <= int(v) <= 2 ** 31 - 1 for v in vals) or any(int(b) <= int(a) for a, b in zip(vals, vals[1:])):
                raise ValueError(f"edges must be at least 1 frame and strictly ascending (got {vals!r})")
            e = np.ascontiguousarray(vals, dtype=np.int32)
        cos_threshold = min(1.0, max(-1.0, math.cos(math.radians(float(max_step_deg)))))
        return cos_threshold, int(min_frames), e

    @staticmethod
    def _fixation_mode(by):
        if by not in FIXATION_MODES:
            raise ValueError(f"by must be one of {sorted(FIXATION_MODES)} (got {by!r})")
        return FIXATION_MODES[by]

    def fixations(self, mu=None, mv=None, ids=None, window=None, stride=1, by="angle", max_step_deg=2.0, min_frames=5, per_user=False,
                  edges=None, keep_labels=False, keep_events=False, keep_centroids=False, check=True):
        """When a viewer holds still, or stays on one tile, and for how long (include/vet.h: vet_fixations).  The pair (f, f + 1) of
        a viewer HOLDS when the viewer is present in both frames and, ``by="angle"``, the angle between the two directions is at
        most ``max_step_deg`` (decided on the cosine, ``math.cos(math.radians(max_step_deg))``; the same Vector always holds) or,
        ``by="tile"``, both samples have the same nearest tile of lattice 0.  A run is a maximal stretch of present frames whose
        pairs all hold; a run of at least ``min_frames`` frames is an event (a fixation, or a dwell) and belongs to the row that
        holds its first frame, with its full length L.  Row r takes frames [r * stride, r * stride + window) of all viewers, or
        with ``per_user`` row (u, r) viewer u's own (outputs user-major, a leading U axis); ``window=None`` is the whole video.
        ``max_step_deg = 2`` and ``min_frames = 5`` are choices for head-direction data on the default grid, not taken from the
        reference, which has no such call.  Returns dict(counts[5,R] int64 (samples, fix_frames: the samples that lie in an event,
        events, sum_len, max_len), hist[R,B]|None (``edges``: B + 1 ascending integers >= 1, bins half-open, of L), labels[U,T]|None
        (``keep_labels``: L of the sample's event, 0 outside an event, -1 absent), offsets[U+1] int64|None, events[N,4]|None
        (``keep_events``: viewer, start, L, the direction id of the middle sample; by viewer, then start), centroids[N,3]|None
        (``keep_centroids``, with ``keep_events``: the sum of the event's unit vectors), cos_threshold, code), R = (T - window) //
        stride + 1.  With ``keep_events`` the engine is called twice: the first call gives N = offsets[U].  A row without a sample
        has zero counts — data, never an error; ``code`` is VET_OK or VET_ERR_RANGE."""
        mode = self._fixation_mode(by)
        c, m, e = self._fixation_args(max_step_deg, min_frames, edges)
        if keep_centroids and not keep_events:
            raise ValueError("keep_centroids needs keep_events (the centroids are those of the listed events)")
        B = 0 if e is None else int(e.size) - 1
        first = ids if ids is not None else mu
        T = int(np.shape(first)[0]) if np.ndim(first) == 2 else 0
        U = int(np.shape(first)[1]) if np.ndim(first) == 2 else 0
        call = _FIXATION_CALLS[bool(per_user)]

        def run(want, max_events):
            return self._row_host(call, mu, mv, ids, window, stride, want, check,
                                  extra=(mode, c, m, int(bool(per_user)), _ptr(e), B, int(max_events)),
                                  extra_dims={"5": 5, "H": B, "T": T, "V": U + 1, "E": int(max_events)})
        want = {key for key, on in (("hist", e is not None), ("labels", keep_labels), ("offsets", keep_events)) if on}
        res = run(want, 0)
        if keep_events:
            n = int(res["offsets"][U])
            if n:
                second = run({"events"} | ({"centroids"} if keep_centroids else set()), n)
                res.update(events=second["events"], centroids=second["centroids"], code=res["code"] or second["code"])
            else:
                res.update(events=np.empty((0, 4), dtype=np.int32), centroids=np.empty((0, 3)) if keep_centroids else None)
        return dict(res, cos_threshold=c)

    def viewer_clusters_sweeps(self):
        """(most, total): the label-propagation sweeps of the rows of the last viewer-clusters call on this plan's engine
        (include/vet.h: vet_viewer_clusters_sweeps)."""
        out = np.zeros(2, dtype=np.int64)
        _check(self.lib, self.lib.vet_viewer_clusters_sweeps(self.handle, _ptr(out)))
        return int(out[0]), int(out[1])

    @staticmethod
    def _saliency_args(sigma_deg, width, height, scale):
        """(sigma in radians, W, H, the C scale 0 / 1 / 2) as the C entry takes them; ``ValueError`` unless sigma_deg is a finite
        number in (0, 180], 2 <= width <= 4096 and 1 <= height <= 2048 are integers and scale is "none", "mean" or "density"."""
        if isinstance(sigma_deg, bool) or not isinstance(sigma_deg, (int, float, np.integer, np.floating)) \
                or not np.isfinite(sigma_deg) or not 0.0 < float(sigma_deg) <= 180.0:
            raise ValueError(f"sigma_deg must be a finite number of degrees in (0, 180] (got {sigma_deg!r})")
        for name, v, lo, hi in (("width", width, 2, 4096), ("height", height, 1, 2048)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
                raise ValueError(f"{name} must be an integer in [{lo}, {hi}] (got {v!r})")
        if not isinstance(scale, str) or scale not in SALIENCY_SCALES:
            raise ValueError(f"scale must be one of {sorted(SALIENCY_SCALES)} (got {scale!r})")
        return min(float(np.radians(float(sigma_deg))), float(np.pi)), int(width), int(height), SALIENCY_SCALES[scale]

    def saliency(self, mu=None, mv=None, ids=None, window=1, stride=1, per_user=False, sigma_deg=5.0, width=180, height=90,
                 scale="density", want_map=True, check=True):
        """Saliency maps (include/vet.h: vet_saliency): the von Mises-Fisher kernel density, kappa = 1 / sigma^2, of the viewing
        directions of frames [r * stride, r * stride + window) on a ``width`` x ``height`` equirectangular map (row 0 at the top,
        laid out as the heatmaps), pooled over the viewers, or with ``per_user`` each viewer's own (outputs user-major, a leading
        U axis).  ``window=None`` is the whole video.  ``sigma_deg = 5.0`` is a choice for head-direction data (about the spread
        of gaze around the head direction), not taken from the reference, which has no such call.  ``scale``: "none" (the sum of
        the kernels), "mean" (divided by the samples) or "density" (per steradian, integral 1).  Returns dict(map[R,H,W]|None
        (``want_map``), stats[4,R] (mass = the map's mean over the sphere, 1 / (4 pi) for a resolved "density" map; peak; entropy in bits against the uniform sphere, area = 2 ** entropy: the effective
        share of the sphere), peak[R] int32 (the peak's pixel index, -1 for a row without a sample), counts[2,R] int64 (samples,
        distinct directions), code), R = (T - window) // stride + 1.  A row without a sample has a zero map and NaN statistics —
        data, never an error; ``code`` is VET_OK or VET_ERR_RANGE."""
        sigma, W, H, sc = self._saliency_args(sigma_deg, width, height, scale)
        return self._row_host(_SALIENCY_CALLS[bool(per_user)], mu, mv, ids, window, stride, {"map"} if want_map else set(), check,
                              extra=(int(bool(per_user)), sigma, W, H, sc), extra_dims={"Y": H, "X": W, "2": 2})

    def saliency_similarity(self, mu=None, mv=None, ids=None, groups=None, window=1, stride=1, sigma_deg=5.0, width=180, height=90,
                            want_maps=False, check=True):
        """Saliency similarity of two audiences (include/vet.h: vet_saliency_similarity): ``groups`` [U] is 0 (audience A), 1
        (audience B) or -1 (excluded); for every row of ``saliency`` (frames [r * stride, r * stride + window), ``window=None`` the
        whole video) the density maps of the two audiences' samples are compared.  Returns dict(maps[2,R,H,W]|None
        (``want_maps``: A's maps, then B's), stats[9,R] (cc = Pearson's correlation, sim = histogram intersection, jsd and kl_ab /
        kl_ba in bits, nss_ab / nss_ba = A's samples on B's standardised density and the reverse, by evaluating the density at the
        samples' directions, mass_a, mass_b), counts[4,R] int64 (samples_a, samples_b, distinct_a, distinct_b), code),
        R = (T - window) // stride + 1.  A row in which an audience has no sample is NaN — data, never an error; kl is +inf where
        one audience has weight on a cell in which the other's density underflowed to zero; ``code`` is VET_OK or VET_ERR_RANGE."""
        sigma, W, H, _ = self._saliency_args(sigma_deg, width, height, "density")
        first = ids if ids is not None else mu
        g = self._group_array(groups, np.shape(first)[1] if np.ndim(first) == 2 else None)
        return self._row_host(_SALIENCY_SIMILARITY_CALL, mu, mv, ids, window, stride, {"maps"} if want_maps else set(), check,
                              extra=(_ptr(g), sigma, W, H), extra_dims={"Y": H, "X": W, "2": 2, "9": 9})

    @staticmethod
    def _score_maps(maps, rows, check):
        """The predicted maps as the C entry takes them: (contiguous float64 array, n_pred, W, H).  ``ValueError`` unless ``maps``
        is a float64 array [H, W] (one static map) or [rows, H, W] (``rows``: the rows of the call, None where the window is refused
        later) and, with ``check``, finite and non-negative."""
        if not isinstance(maps, np.ndarray) or maps.dtype != np.float64:
            raise ValueError(f"maps must be a float64 array [H, W] or [rows, H, W] (got {type(maps).__name__}"
                             f"{' of ' + str(maps.dtype) if isinstance(maps, np.ndarray) else ''})")
        if maps.ndim not in (2, 3):
            raise ValueError(f"maps must be [H, W] (one static map) or [rows, H, W] (got {maps.ndim} dimensions)")
        if maps.ndim == 3 and rows is not None and maps.shape[0] != rows:
            raise ValueError(f"maps holds {maps.shape[0]} maps for {rows} rows: pass one map per row, or one [H, W] map for all")
        if check and (not np.isfinite(maps).all() or (maps < 0).any()):
            raise ValueError("maps must be finite and non-negative")
        return np.ascontiguousarray(maps), (1 if maps.ndim == 2 else int(maps.shape[0])), int(maps.shape[-1]), int(maps.shape[-2])

    def saliency_score(self, mu=None, mv=None, ids=None, maps=None, window=1, stride=1, sigma_deg=5.0, distribution=True,
                       want_map=False, check=True):
        """Saliency scoring (include/vet.h: vet_saliency_score): how well the predicted ``maps`` — float64 [H, W], one static map
        for every row, or [R, H, W], one per row; finite, non-negative, any scale, laid out as ``saliency``'s maps — predict where the
        audience looked in frames [r * stride, r * stride + window) (``window=None``: the whole video).  Returns dict(map[R,H,W]|None
        (``want_map``: the audience's own density map), stats[9,R] (auc = the area-weighted Mann-Whitney AUC of the map's values at
        the samples against the whole sphere, nss, info_gain in bits over the uniform sphere — the map sampled at the samples'
        directions by bilinear interpolation — and, with ``distribution``, cc, sim, jsd, kl of the audience's density map
        (``sigma_deg``) against the prediction and mass, the audience map's; mass_pred), counts[2,R] int64 (samples, distinct
        directions), code), R = (T - window) // stride + 1.  A row without a sample is NaN but for mass_pred — data, never an error;
        info_gain is -inf where the map is 0.0 at a sample, kl +inf where the audience has weight on a cell the map holds 0.0 in;
        without ``distribution`` cc .. mass are NaN and no density is evaluated.  ``check`` also refuses a negative or non-finite
        map value.  ``code`` is VET_OK or VET_ERR_RANGE."""
        first = ids if ids is not None else mu
        T = np.shape(first)[0] if np.ndim(first) == 2 else None
        w = T if window is None else window
        ok = T is not None and isinstance(w, (int, np.integer)) and isinstance(stride, (int, np.integer)) and 1 <= w <= T and stride >= 1
        pred, n_pred, W, H = self._score_maps(maps, (T - int(w)) // int(stride) + 1 if ok else None, check)
        sigma, W, H, _ = self._saliency_args(sigma_deg, W, H, "density")
        return self._row_host(_SALIENCY_SCORE_CALL, mu, mv, ids, window, stride, {"map"} if want_map else set(), check,
                              extra=(sigma, W, H, _ptr(pred), n_pred, int(bool(distribution))), extra_dims={"Y": H, "X": W, "2": 2, "9": 9})

    def congruency(self, mu=None, mv=None, ids=None, window=None, stride=1, sigma_deg=5.0, nss=True, check=True):
        """Viewer congruency (include/vet.h: vet_congruency): for every viewer and every row of ``saliency`` (frames
        [r * stride, r * stride + window), ``window=None`` the whole video) the kernel density of everyone else's samples, evaluated
        at the viewer's own directions — no map.  Returns dict(stats[3,U,R] (lift = the others' density at the viewer's samples over
        the uniform sphere's, info_gain = the mean log2 of that ratio in bits, nss = the density standardised by its closed-form
        mean and variance over the sphere; NaN without ``nss``), counts[3,U,R] int64 (samples, distinct directions, the others'
        samples), rows[4,R] (scored viewers, mean lift, mean info_gain, mean nss over them), code), R = (T - window) // stride + 1.
        A viewer without a sample in a row, or alone in it, is NaN — data, never an error; info_gain is -inf where the others'
        density underflowed to zero at a sample; ``code`` is VET_OK or VET_ERR_RANGE."""
        sigma, _, _, _ = self._saliency_args(sigma_deg, 2, 1, "density")
        return self._row_host(_CONGRUENCY_CALL, mu, mv, ids, window, stride, set(), check, extra=(sigma, int(bool(nss))))

    def transition_per_user(self, mu=None, mv=None, ids=None, window=None, stride=1, want_srccount=False, check=True):
        """Each user's own tile moves over time (include/vet.h: vet_user_transition_entropy): row (u, r) pools user u's
        transitions of pairs [r * stride, r * stride + window), pair f = (frame f, frame f + 1), into one call of the
        reference's ``compute_transition_entropy``.  ``window`` and ``stride`` count frame pairs; ``window=None`` is all
        T - 1 pairs (one row per user).  Returns dict(entropy[U,R], srccount[U,R,n0]|None, samples[U,R], code),
        R = (T - 1 - window) // stride + 1.  Rows in which the user has no pair present in both frames are NaN with
        ``samples`` 0 — data, never an error; ``code`` is VET_OK or VET_ERR_RANGE."""
        return self._row_host("transition_per_user", mu, mv, ids, window, stride, want_srccount, check)

    def spatial_resident(self, mu=None, mv=None, ids=None, check=True):
        """Like ``spatial`` but only entropy[T] and present[T] come back; the tile assignments and weights stay
        on the device in ``result`` (a ``DeviceResult``) and are fetched by row on demand."""
        mu, mv, ids, (T, U) = self._samples(mu, mv, ids)
        ent = np.empty(T, dtype=np.float64)
        present = np.empty(T, dtype=np.int32)
        h = C.c_void_p()
        rc = self.lib.vet_spatial_entropy_host_resident(self.handle, _ptr(mu), _ptr(mv), _ptr(ids), U, T, _ptr(ent),
                                                        _ptr(present), C.byref(h))
        result = DeviceResult(self.lib, h, T, [(U,), (self.n_tiles[0],)], [np.int32, np.float64], self.engine) if h.value else None
        if rc not in (VET_OK, VET_ERR_EMPTY, VET_ERR_RANGE) or (check and rc != VET_OK):
            if result is not None:
                result.close()
            _check(self.lib, rc)
        return dict(entropy=ent, present=present, result=result, code=rc)

    def transition_resident(self, mu=None, mv=None, ids=None, check=True):
        """Like ``transition`` with the tile pairs and source-tile counts kept on the device."""
        mu, mv, ids, (T, U) = self._samples(mu, mv, ids)
        R = max(T - 1, 0)
        ent = np.empty(R, dtype=np.float64)
        common = np.empty(R, dtype=np.int32)
        h = C.c_void_p()
        rc = self.lib.vet_transition_entropy_host_resident(self.handle, _ptr(mu), _ptr(mv), _ptr(ids), U, T, _ptr(ent),
                                                           _ptr(common), C.byref(h))
        result = DeviceResult(self.lib, h, R, [(U, 2), (self.n_tiles[0],)], [np.int32, np.int32], self.engine) if h.value else None
        if rc not in (VET_OK, VET_ERR_EMPTY, VET_ERR_RANGE) or (check and rc != VET_OK):
            if result is not None:
                result.close()
            _check(self.lib, rc)
        return dict(entropy=ent, common=common, result=result, code=rc)

    def spatial_batch(self, videos, want_assign=False, check=True):
        """Many videos, one launch.  ``videos``: sequence of (mu[T,U], mv[T,U]).  Returns a list of
        dict(entropy[T], assign[T,U]|None, present[T]) in the same order."""
        mus = [np.ascontiguousarray(m, dtype=np.float64) for m, _ in videos]
        mvs = [np.ascontiguousarray(v, dtype=np.float64) for _, v in videos]
        T = np.asarray([m.shape[0] for m in mus], dtype=np.int32)
        U = np.asarray([m.shape[1] for m in mus], dtype=np.int32)
        mu = np.concatenate([m.ravel() for m in mus])
        mv = np.concatenate([v.ravel() for v in mvs])
        ent = np.empty(int(T.sum()), dtype=np.float64)
        present = np.empty(int(T.sum()), dtype=np.int32)
        assign = np.empty(mu.size, dtype=np.int32) if want_assign else None
        rc = self.lib.vet_spatial_entropy_batch_host(self.handle, len(mus), _ptr(U), _ptr(T), _ptr(mu), _ptr(mv),
                                                     _ptr(ent), _ptr(assign), _ptr(present))
        if rc not in (VET_OK, VET_ERR_EMPTY, VET_ERR_RANGE) or (check and rc != VET_OK):
            _check(self.lib, rc)
        out, so, ro = [], 0, 0
        for t, u in zip(T.tolist(), U.tolist()):
            out.append(dict(entropy=ent[ro:ro + t], present=present[ro:ro + t],
                            assign=assign[so:so + t * u].reshape(t, u) if want_assign else None))
            so += t * u
            ro += t
        return out

    def transition_batch(self, videos, want_pairs=False, check=True):
        """Transition mode, many videos, one launch per lattice.  ``videos``: sequence of (mu[T,U], mv[T,U]), T >= 2.
        Returns a list of dict(entropy[T-1], pairs[T-1,U,2]|None, common[T-1]) in the same order."""
        mus = [np.ascontiguousarray(m, dtype=np.float64) for m, _ in videos]
        mvs = [np.ascontiguousarray(v, dtype=np.float64) for _, v in videos]
        T = np.asarray([m.shape[0] for m in mus], dtype=np.int32)
        U = np.asarray([m.shape[1] for m in mus], dtype=np.int32)
        mu = np.concatenate([m.ravel() for m in mus])
        mv = np.concatenate([v.ravel() for v in mvs])
        R = int((T - 1).sum())
        ent = np.empty(R, dtype=np.float64)
        common = np.empty(R, dtype=np.int32)
        pairs = np.empty(int(((T - 1) * U).sum()) * 2, dtype=np.int32) if want_pairs else None
        rc = self.lib.vet_transition_entropy_batch_host(self.handle, len(mus), _ptr(U), _ptr(T), _ptr(mu), _ptr(mv),
                                                        _ptr(ent), _ptr(pairs), _ptr(common))
        if rc not in (VET_OK, VET_ERR_EMPTY, VET_ERR_RANGE) or (check and rc != VET_OK):
            _check(self.lib, rc)
        out, po, ro = [], 0, 0
        for t, u in zip(T.tolist(), U.tolist()):
            out.append(dict(entropy=ent[ro:ro + t - 1], common=common[ro:ro + t - 1],
                            pairs=pairs[po:po + (t - 1) * u * 2].reshape(t - 1, u, 2) if want_pairs else None))
            po += (t - 1) * u * 2
            ro += t - 1
        return out

    def transition_batch_device(self, videos, d_status: int = 0, stream=None):
        """``videos``: ctypes array of ``Video`` (device pointers: d_entropy [T-1], d_assign = pairs, d_present = common)."""
        _check(self.lib, self.lib.vet_transition_entropy_batch(self.handle, len(videos), videos, d_status or None,
                                                               _stream(stream)))

    def spatial_batch_device(self, videos, d_status: int = 0, stream=None):
        """``videos``: ctypes array of ``Video`` (device pointers); asynchronous on ``stream``
        (``None`` = the engine's own stream, 0 = the legacy null stream, else a hipStream_t handle)."""
        _check(self.lib, self.lib.vet_spatial_entropy_batch(self.handle, len(videos), videos, d_status or None,
                                                            _stream(stream)))

    # --- device-pointer runs (inputs resident in HBM; asynchronous on ``stream``) ----
    def spatial_device(self, d_mu: int, d_mv: int, n_users: int, n_frames: int, d_entropy: int, d_assign: int = 0,
                       d_weights: int = 0, d_present: int = 0, d_status: int = 0, stream=None):
        _check(self.lib, self.lib.vet_spatial_entropy(self.handle, d_mu, d_mv, n_users, n_frames, d_entropy,
                                                      d_assign or None, d_weights or None, d_present or None,
                                                      d_status or None, _stream(stream)))

    def spatial_windowed_device(self, d_mu: int, d_mv: int, n_users: int, n_frames: int, window: int, stride: int,
                                d_entropy: int, d_weights: int = 0, d_samples: int = 0, d_status: int = 0, stream=None):
        self._row_device("spatial_windowed", d_mu, d_mv, 0, n_users, n_frames,
                         (window, stride), d_entropy, (d_weights, d_samples, d_status), stream)

    def spatial_per_user_device(self, d_mu: int, d_mv: int, n_users: int, n_frames: int, window: int, stride: int,
                                d_entropy: int, d_weights: int = 0, d_samples: int = 0, d_status: int = 0, stream=None):
        """Outputs are user-major: d_entropy [U][R], d_weights [U][R][n0], d_samples [U][R] (include/vet.h: vet_user_entropy)."""
        self._row_device("spatial_per_user", d_mu, d_mv, 0, n_users, n_frames,
                         (window, stride), d_entropy, (d_weights, d_samples, d_status), stream)

    def spatial_user_divergence_device(self, d_mu: int, d_mv: int, n_users: int, n_frames: int, window: int, stride: int,
                                       d_div: int, d_samples: int = 0, d_status: int = 0, stream=None):
        """d_div [R][U][U]; d_samples [U][R] (include/vet.h: vet_user_divergence)."""
        self._row_device("spatial_user_divergence", d_mu, d_mv, 0, n_users, n_frames,
                         (window, stride), d_div, (d_samples, d_status), stream)

    def spatial_crowd_divergence_device(self, d_mu: int, d_mv: int, n_users: int, n_frames: int, window: int, stride: int,
                                        d_div: int, d_rows: int = 0, d_samples: int = 0, d_status: int = 0, stream=None,
                                        d_ids: int = 0):
        """d_div [U][R]; d_rows [3][R]; d_samples [U][R] (include/vet.h: vet_crowd_divergence; ``d_ids``:
        vet_crowd_divergence_ids)."""
        self._row_device("spatial_crowd_divergence", d_mu, d_mv, d_ids, n_users, n_frames,
                         (window, stride), d_div, (d_rows, d_samples, d_status), stream)

    def spatial_bootstrap_device(self, d_mu: int, d_mv: int, n_users: int, n_frames: int, window: int, stride: int,
                                 replicates: int, seed: int, confidence: float, d_summary: int, d_replicates: int = 0,
                                 d_weights: int = 0, d_valid: int = 0, d_status: int = 0, stream=None, d_ids: int = 0):
        """d_summary [4][R]; d_replicates [R][B]; d_weights [R][B][n0]; d_valid [R] (include/vet.h: vet_bootstrap_entropy;
        ``d_ids``: vet_bootstrap_entropy_ids)."""
        self._row_device("spatial_bootstrap", d_mu, d_mv, d_ids, n_users, n_frames,
                         (window, stride, replicates, seed, float(confidence)), d_summary,
                         (d_replicates, d_weights, d_valid, d_status), stream)

    def spatial_group_divergence_device(self, d_mu: int, d_mv: int, n_users: int, n_frames: int, window: int, stride: int, groups,
                                        permutations: int, seed: int, confidence: float, d_summary: int, d_null: int = 0,
                                        d_weights: int = 0, d_samples: int = 0, d_valid: int = 0, d_status: int = 0, stream=None,
                                        d_ids: int = 0):
        """``groups``: the host array [U]; d_summary [5][R]; d_null [R][P]; d_weights [R][2][n0]; d_samples [2][R]; d_valid [R]
        (include/vet.h: vet_group_divergence; ``d_ids``: vet_group_divergence_ids)."""
        g = self._group_array(groups, n_users)
        self._row_device("spatial_group_divergence", d_mu, d_mv, d_ids, n_users, n_frames,
                         (window, stride, g.ctypes.data, permutations, seed, float(confidence)), d_summary,
                         (d_null, d_weights, d_samples, d_valid, d_status), stream)

    def spatial_window_divergence_device(self, d_mu: int, d_mv: int, n_users: int, n_frames: int, window: int, stride: int,
                                         max_lag: int, d_div: int, d_samples: int = 0, d_status: int = 0, stream=None,
                                         d_ids: int = 0):
        """d_div [R][max_lag]; d_samples [R] (include/vet.h: vet_window_divergence; ``d_ids``: vet_window_divergence_ids)."""
        self._row_device("spatial_window_divergence", d_mu, d_mv, d_ids, n_users, n_frames,
                         (window, stride, max_lag), d_div, (d_samples, d_status), stream)

    def spatial_coverage_device(self, d_mu: int, d_mv: int, n_users: int, n_frames: int, window: int, stride: int, max_lag: int,
                                fractions, d_tiles: int, d_hit: int, d_order: int = 0, d_samples: int = 0, d_status: int = 0,
                                stream=None, d_ids: int = 0):
        """``fractions``: the host sequence [Q]; d_tiles i32 [R][Q]; d_hit f64 [R][max_lag + 1][Q]; d_order i32 [R][n0];
        d_samples [R] (include/vet.h: vet_coverage; ``d_ids``: vet_coverage_ids)."""
        f = self._fraction_array(fractions)
        self._row_device("spatial_coverage", d_mu, d_mv, d_ids, n_users, n_frames,
                         (window, stride, max_lag, f.ctypes.data, f.size), d_tiles, (d_hit, d_order, d_samples, d_status), stream)

    def transition_windowed_device(self, d_mu: int, d_mv: int, n_users: int, n_frames: int, window: int, stride: int,
                                   d_entropy: int, d_srccount: int = 0, d_samples: int = 0, d_status: int = 0, stream=None):
        self._row_device("transition_windowed", d_mu, d_mv, 0, n_users, n_frames,
                         (window, stride), d_entropy, (d_srccount, d_samples, d_status), stream)

    def transition_markov_device(self, d_mu: int, d_mv: int, n_users: int, n_frames: int, window: int, stride: int, lag: int,
                                 d_stats: int, d_matrix: int = 0, d_samples: int = 0, d_status: int = 0, stream=None, d_ids: int = 0):
        """d_stats f64 [5][R]; d_matrix i32 [R][n0][n0]; d_samples [R] (include/vet.h: vet_transition_markov; ``d_ids``:
        vet_transition_markov_ids)."""
        self._row_device("transition_markov", d_mu, d_mv, d_ids, n_users, n_frames,
                         (window, stride, lag), d_stats, (d_matrix, d_samples, d_status), stream)

    def head_motion_device(self, d_mu: int, d_mv: int, n_users: int, n_frames: int, window: int, stride: int, lag: int, per_user: bool,
                           quantiles, edges, d_stats: int, d_quantiles: int = 0, d_hist: int = 0, d_still: int = 0, d_samples: int = 0,
                           d_status: int = 0, stream=None, d_ids: int = 0):
        """``quantiles`` / ``edges``: the host sequences [Q] / [B + 1] (or None); d_stats f64 [4][Rows]; d_quantiles f64 [Rows][Q];
        d_hist i32 [Rows][B]; d_still, d_samples i32 [Rows]; Rows = R, or U * R user-major with ``per_user`` (include/vet.h:
        vet_head_motion; ``d_ids``: vet_head_motion_ids)."""
        f, e = self._motion_arrays(quantiles, edges)
        self._row_device(_MOTION_CALLS[bool(per_user)], d_mu, d_mv, d_ids, n_users, n_frames,
                         (window, stride, lag, int(bool(per_user)), f.ctypes.data if f is not None else 0, 0 if f is None else f.size,
                          e.ctypes.data if e is not None else 0, 0 if e is None else e.size - 1), d_stats,
                         (d_quantiles, d_hist, d_still, d_samples, d_status), stream)

    def dispersion_device(self, d_mu: int, d_mv: int, n_users: int, n_frames: int, window: int, stride: int, per_user: bool, edges,
                          d_stats: int = 0, d_centroid: int = 0, d_hist: int = 0, d_counts: int = 0, d_status: int = 0, stream=None,
                          d_ids: int = 0):
        """``edges``: the host sequence [B + 1] in radians (or None); d_stats f64 [3][Rows]; d_centroid f64 [Rows][3]; d_hist i64
        [Rows][B]; d_counts i64 [4][Rows]; Rows = R, or U * R user-major with ``per_user``; every output may be 0 (include/vet.h:
        vet_dispersion; ``d_ids``: vet_dispersion_ids)."""
        e = self._dispersion_edges(edges, per_user)
        self._row_device(_DISPERSION_CALLS[bool(per_user)], d_mu, d_mv, d_ids, n_users, n_frames,
                         (window, stride, int(bool(per_user)), e.ctypes.data if e is not None else 0, 0 if e is None else e.size - 1),
                         d_stats or None, (d_centroid, d_hist, d_counts, d_status), stream)

    def viewer_clusters_device(self, d_mu: int, d_mv: int, n_users: int, n_frames: int, window: int, stride: int, cos_threshold: float,
                               min_share: float, fractions, d_labels: int = 0, d_sizes: int = 0, d_counts: int = 0, d_top: int = 0,
                               d_stats: int = 0, d_centroids: int = 0, d_links: int = 0, d_status: int = 0, stream=None,
                               d_ids: int = 0):
        """``fractions``: the host sequence [Q] (or None); d_labels, d_sizes i32 [R][U]; d_counts i64 [5][R]; d_top i32 [R][Q];
        d_stats f64 [3][R]; d_centroids f64 [R][U][3]; d_links u64 [R][U][ceil(U / 64)]; every output may be 0 (include/vet.h:
        vet_viewer_clusters; ``d_ids``: vet_viewer_clusters_ids).  The C entry checks cos_threshold, min_share and the fractions."""
        f = None if fractions is None or not len(fractions) else np.ascontiguousarray(fractions, dtype=np.float64)
        self._row_device(_CLUSTERS_CALL, d_mu, d_mv, d_ids, n_users, n_frames,
                         (window, stride, float(cos_threshold), float(min_share), f.ctypes.data if f is not None else 0,
                          0 if f is None else f.size), d_labels or None,
                         (d_sizes, d_counts, d_top, d_stats, d_centroids, d_links, d_status), stream)

    def fixations_device(self, d_mu: int, d_mv: int, n_users: int, n_frames: int, window: int, stride: int, by: str,
                         cos_threshold: float, min_frames: int, per_user: bool, edges=None, max_events: int = 0, d_counts: int = 0,
                         d_hist: int = 0, d_labels: int = 0, d_offsets: int = 0, d_events: int = 0, d_centroids: int = 0,
                         d_status: int = 0, stream=None, d_ids: int = 0):
        """``edges``: the host sequence [B + 1] of integers (or None); d_counts i64 [5][Rows]; d_hist i32 [Rows][B]; d_labels i32
        [U][T]; d_offsets i64 [U + 1]; d_events i32 [max_events][4]; d_centroids f64 [max_events][3]; Rows = R, or U * R user-major
        with ``per_user``; every output may be 0 (include/vet.h: vet_fixations; ``d_ids``: vet_fixations_ids).  The C entry checks
        cos_threshold, min_frames, the edges and max_events."""
        e = None if edges is None else np.ascontiguousarray(edges, dtype=np.int32)
        self._row_device(_FIXATION_CALLS[bool(per_user)], d_mu, d_mv, d_ids, n_users, n_frames,
                         (window, stride, self._fixation_mode(by), float(cos_threshold), int(min_frames), int(bool(per_user)),
                          e.ctypes.data if e is not None else 0, 0 if e is None else e.size - 1, int(max_events)), d_counts or None,
                         (d_hist, d_labels, d_offsets, d_events, d_centroids, d_status), stream)

    def saliency_device(self, d_mu: int, d_mv: int, n_users: int, n_frames: int, window: int, stride: int, per_user: bool,
                        sigma_deg: float = 5.0, width: int = 180, height: int = 90, scale: str = "density", d_map: int = 0,
                        d_stats: int = 0, d_peak: int = 0, d_counts: int = 0, d_status: int = 0, stream=None, d_ids: int = 0):
        """d_map f64 [Rows][H][W]; d_stats f64 [4][Rows]; d_peak i32 [Rows]; d_counts i64 [2][Rows]; Rows = R, or U * R user-major
        with ``per_user``; every output may be 0 — without d_map no map leaves the workspace (include/vet.h: vet_saliency;
        ``d_ids``: vet_saliency_ids)."""
        sigma, W, H, sc = self._saliency_args(sigma_deg, width, height, scale)
        self._row_device(_SALIENCY_CALLS[bool(per_user)], d_mu, d_mv, d_ids, n_users, n_frames,
                         (window, stride, int(bool(per_user)), sigma, W, H, sc), d_map or None,
                         (d_stats, d_peak, d_counts, d_status), stream)

    def saliency_similarity_device(self, d_mu: int, d_mv: int, n_users: int, n_frames: int, window: int, stride: int, groups,
                                   sigma_deg: float = 5.0, width: int = 180, height: int = 90, d_maps: int = 0, d_stats: int = 0,
                                   d_counts: int = 0, d_status: int = 0, stream=None, d_ids: int = 0):
        """``groups``: the host array [U]; d_maps f64 [2][R][H][W]; d_stats f64 [9][R]; d_counts i64 [4][R]; every output may be 0 —
        without d_maps no map leaves the workspace (include/vet.h: vet_saliency_similarity; ``d_ids``:
        vet_saliency_similarity_ids)."""
        sigma, W, H, _ = self._saliency_args(sigma_deg, width, height, "density")
        g = self._group_array(groups, n_users)
        self._row_device(_SALIENCY_SIMILARITY_CALL, d_mu, d_mv, d_ids, n_users, n_frames,
                         (window, stride, g.ctypes.data, sigma, W, H), d_maps or None, (d_stats, d_counts, d_status), stream)

    def saliency_score_device(self, d_mu: int, d_mv: int, n_users: int, n_frames: int, window: int, stride: int, d_pred: int,
                              n_pred: int, width: int, height: int, sigma_deg: float = 5.0, distribution: bool = True, d_map: int = 0,
                              d_stats: int = 0, d_counts: int = 0, d_status: int = 0, stream=None, d_ids: int = 0):
        """d_pred f64 [n_pred][H][W] on the device, read in place (finite and non-negative: a precondition, not checked); n_pred 1 or
        R; d_map f64 [R][H][W]; d_stats f64 [9][R]; d_counts i64 [2][R]; every output may be 0 (include/vet.h: vet_saliency_score;
        ``d_ids``: vet_saliency_score_ids)."""
        sigma, W, H, _ = self._saliency_args(sigma_deg, width, height, "density")
        self._row_device(_SALIENCY_SCORE_CALL, d_mu, d_mv, d_ids, n_users, n_frames,
                         (window, stride, sigma, W, H, int(d_pred), int(n_pred), int(bool(distribution))), d_map or None,
                         (d_stats, d_counts, d_status), stream)

    def congruency_device(self, d_mu: int, d_mv: int, n_users: int, n_frames: int, window: int, stride: int, sigma_deg: float = 5.0,
                          nss: bool = True, d_stats: int = 0, d_counts: int = 0, d_rows: int = 0, d_status: int = 0, stream=None,
                          d_ids: int = 0):
        """d_stats f64 [3][U][R]; d_counts i64 [3][U][R]; d_rows f64 [4][R]; every output may be 0 (include/vet.h: vet_congruency;
        ``d_ids``: vet_congruency_ids)."""
        sigma, _, _, _ = self._saliency_args(sigma_deg, 2, 1, "density")
        self._row_device(_CONGRUENCY_CALL, d_mu, d_mv, d_ids, n_users, n_frames, (window, stride, sigma, int(bool(nss))),
                         d_stats or None, (d_counts, d_rows, d_status), stream)

    def transition_per_user_device(self, d_mu: int, d_mv: int, n_users: int, n_frames: int, window: int, stride: int,
                                   d_entropy: int, d_srccount: int = 0, d_samples: int = 0, d_status: int = 0, stream=None):
        """Outputs are user-major: d_entropy [U][R], d_srccount [U][R][n0], d_samples [U][R]
        (include/vet.h: vet_user_transition_entropy)."""
        self._row_device("transition_per_user", d_mu, d_mv, 0, n_users, n_frames,
                         (window, stride), d_entropy, (d_srccount, d_samples, d_status), stream)

    def transition_device(self, d_mu: int, d_mv: int, n_users: int, n_frames: int, d_entropy: int, d_pairs: int = 0,
                          d_srccount: int = 0, d_common: int = 0, d_status: int = 0, stream=None):
        _check(self.lib, self.lib.vet_transition_entropy(self.handle, d_mu, d_mv, n_users, n_frames, d_entropy,
                                                         d_pairs or None, d_srccount or None, d_common or None,
                                                         d_status or None, _stream(stream)))


class Heatmap:
    """Per-frame tile-attention heatmaps of one lattice (include/vet.h: vet_heatmap): ``width`` x ``height`` uint8 RGB
    frames, equirectangular (row 0 = latitude +90), every pixel coloured by its nearest tile's
    ``tile_weights / users present`` as the reference's animation colours tiles, with black viewport markers of side
    ``2 * marker_radius + 1``.  The pixel -> tile map is built on the device once, here."""

    def __init__(self, engine: Engine, tiles: np.ndarray, width: int, height: int, video_width: int, video_height: int,
                 marker_radius: int = 2):
        self.engine, self.lib = engine, engine.lib
        tiles = np.ascontiguousarray(tiles, dtype=np.float64).reshape(-1, 3)
        self.n_tiles, self.width, self.height = len(tiles), int(width), int(height)
        self.video_width, self.video_height, self.marker_radius = int(video_width), int(video_height), int(marker_radius)
        h = C.c_void_p()
        _check(self.lib, self.lib.vet_heatmap_create(engine.handle, _ptr(tiles), self.n_tiles, self.width, self.height,
                                                     self.video_width, self.video_height, self.marker_radius, C.byref(h)))
        self.handle = h

    @classmethod
    def latlon(cls, engine: Engine, tile_width: int, tile_height: int, width: int, height: int, video_width: int,
               video_height: int, marker_radius: int = 2) -> "Heatmap":
        """The heatmap of a naive plan's ``tile_height`` x ``tile_width`` degree lat/lon cells
        (include/vet.h: vet_heatmap_create_latlon): every pixel centre's cell, find_naive_tile_index's arithmetic, in the
        plan's bin numbering ((360 / tile_width + 1) * (180 / tile_height + 1) cells).  Render it with ``render_binned``."""
        self = cls.__new__(cls)
        self.engine, self.lib = engine, engine.lib
        self.tile_width, self.tile_height = int(tile_width), int(tile_height)
        self.width, self.height = int(width), int(height)
        self.video_width, self.video_height, self.marker_radius = int(video_width), int(video_height), int(marker_radius)
        h = C.c_void_p()
        _check(self.lib, self.lib.vet_heatmap_create_latlon(engine.handle, self.tile_width, self.tile_height, self.width,
                                                            self.height, self.video_width, self.video_height,
                                                            self.marker_radius, C.byref(h)))
        self.handle = h
        self.n_tiles = (360 // self.tile_width + 1) * (180 // self.tile_height + 1)
        return self

    def close(self):
        if getattr(self, "handle", None):
            self.lib.vet_heatmap_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def map(self) -> np.ndarray:
        """int32 [height, width]: the tile of every pixel."""
        out = np.empty((self.height, self.width), dtype=np.int32)
        _check(self.lib, self.lib.vet_heatmap_read_map(self.handle, _ptr(out)))
        return out

    def render_device(self, d_weights: int, d_present: int, n_frames: int, d_rgb: int, d_mu: int = 0, d_mv: int = 0,
                      n_users: int = 0, stream=None):
        """Frames [0, n_frames) from device pointers (weights f64 [T, n_tiles], present i32 [T], optional samples f64
        [T, U]) into ``d_rgb`` (uint8 [T, H, W, 3], 4-byte aligned); asynchronous on ``stream`` as ``Plan.spatial_device``."""
        _check(self.lib, self.lib.vet_heatmap_render(self.handle, d_weights, d_present, d_mu or None, d_mv or None,
                                                     int(n_users), int(n_frames), d_rgb, _stream(stream)))

    def render_counts_device(self, d_counts: int, d_present: int, n_frames: int, d_rgb: int, d_mu: int = 0, d_mv: int = 0,
                             n_users: int = 0, stream=None):
        """``render_device`` with i32 user counts per tile [T, n_tiles] (a transition result's source-tile counts) in
        place of the f64 weights; ``present`` and the samples are those of each row's prior frame."""
        _check(self.lib, self.lib.vet_heatmap_render_counts(self.handle, d_counts, d_present, d_mu or None, d_mv or None,
                                                            int(n_users), int(n_frames), d_rgb, _stream(stream)))

    def render_binned_device(self, plan: "Plan", d_mu: int, d_mv: int, n_users: int, n_frames: int, d_rgb: int,
                             markers: bool = True, stream=None):
        """Frames [0, n_frames) of a lat/lon heatmap from device samples (f64 [T, U] each) through ``plan``'s binned
        lattice 0 into ``d_rgb`` (uint8 [T, H, W, 3], 4-byte aligned); asynchronous on ``stream`` as
        ``Plan.spatial_device``."""
        _check(self.lib, self.lib.vet_heatmap_render_binned(self.handle, plan.handle, d_mu, d_mv, int(n_users),
                                                            int(n_frames), int(bool(markers)), d_rgb, _stream(stream)))

    def _out(self, n: int, out: Optional[np.ndarray]) -> np.ndarray:
        shape = (n, self.height, self.width, 3)
        if out is None:
            return np.empty(shape, dtype=np.uint8)
        if out.shape != shape or out.dtype != np.uint8 or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous uint8 array of shape {shape}")
        return out

    def render_binned(self, plan: "Plan", mu: np.ndarray, mv: np.ndarray, row0: int = 0, n: Optional[int] = None,
                      markers: bool = True, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Frames [row0, row0 + n) of the samples ``mu`` / ``mv`` (f64 [T, U], NaN = absent) of a lat/lon heatmap ->
        uint8 [n, H, W, 3] (into ``out`` when given).  Each cell's colour is its users (through ``plan``'s own quantiser
        and LUT) over the users present in the frame; ``markers=False`` draws no viewport markers."""
        mu = np.ascontiguousarray(mu, dtype=np.float64)
        mv = np.ascontiguousarray(mv, dtype=np.float64)
        if mu.ndim != 2 or mu.shape != mv.shape:
            raise ValueError("mu and mv must be [n_frames, n_users] arrays of equal shape")
        T, U = mu.shape
        row0 = int(row0)
        n = T - row0 if n is None else int(n)
        if row0 < 0 or n < 0 or row0 + n > T:
            raise ValueError(f"frames [{row0}, {row0 + n}) outside the samples' {T} frames")
        out = self._out(n, out)
        _check(self.lib, self.lib.vet_heatmap_render_binned_host(self.handle, plan.handle, _ptr(mu[row0:row0 + n]),
                                                                 _ptr(mv[row0:row0 + n]), U, n, int(bool(markers)),
                                                                 _ptr(out)))
        return out

    def _render_rows(self, entry, result, present, mu, mv, row0, n, out) -> np.ndarray:
        n = result.n_rows - row0 if n is None else int(n)
        present = np.ascontiguousarray(present, dtype=np.int32).reshape(-1)
        if len(present) != n:
            raise ValueError(f"present holds {len(present)} rows, expected {n}")
        U = 0
        if mu is not None:
            mu = np.ascontiguousarray(mu, dtype=np.float64)
            mv = np.ascontiguousarray(mv, dtype=np.float64)
            if mu.ndim != 2 or mu.shape != mv.shape or len(mu) != n:
                raise ValueError(f"mu and mv must be [{n}, n_users] arrays of equal shape")
            U = mu.shape[1]
        out = self._out(n, out)
        _check(self.lib, entry(self.handle, result.handle, _ptr(present), _ptr(mu), _ptr(mv), U, int(row0), n, _ptr(out)))
        return out

    def render_result(self, result: "DeviceResult", present: np.ndarray, mu: Optional[np.ndarray] = None,
                      mv: Optional[np.ndarray] = None, row0: int = 0, n: Optional[int] = None,
                      out: Optional[np.ndarray] = None) -> np.ndarray:
        """Frames [row0, row0 + n) of a spatial ``DeviceResult`` -> uint8 [n, H, W, 3] (into ``out`` when given: a
        C-contiguous uint8 array of that shape).  ``present``, ``mu``, ``mv`` hold those frames' rows only; without
        ``mu`` / ``mv`` no markers are drawn.  The weight rows stay on the device."""
        return self._render_rows(self.lib.vet_heatmap_render_result, result, present, mu, mv, row0, n, out)

    def render_transition_result(self, result: "DeviceResult", present: np.ndarray, mu: Optional[np.ndarray] = None,
                                 mv: Optional[np.ndarray] = None, row0: int = 0, n: Optional[int] = None,
                                 out: Optional[np.ndarray] = None) -> np.ndarray:
        """Rows [row0, row0 + n) of a transition ``DeviceResult`` (row r: the pair of frames r -> r+1) -> uint8
        [n, H, W, 3], as ``render_result``.  Row r's colours are its source-tile counts over ``present[r]``, the users
        present in frame r (not the common users), and its markers are frame r's samples: ``present``, ``mu``, ``mv`` are
        the frame table's rows row0 .. row0 + n - 1.  The count rows stay on the device."""
        return self._render_rows(self.lib.vet_heatmap_render_transition_result, result, present, mu, mv, row0, n, out)


class Tiling:
    """A tiling drawn on the unit sphere (include/vet.h: vet_tiling): ``arcs`` [n, 2, 3] great-circle arcs, each drawn as 49
    black chords, optional ``centres`` [m, 3] drawn as red squares, over a translucent grey unit sphere, seen through a
    parallel projection.  The chord points are computed on the device once, here; every render takes one camera (P, U, F)
    per frame."""

    def __init__(self, engine: Engine, arcs: np.ndarray, centres: Optional[np.ndarray], width: int, height: int):
        self.engine, self.lib = engine, engine.lib
        arcs = np.ascontiguousarray(arcs, dtype=np.float64).reshape(-1, 2, 3)
        centres = None if centres is None else np.ascontiguousarray(centres, dtype=np.float64).reshape(-1, 3)
        self.n_arcs, self.n_centres = len(arcs), 0 if centres is None else len(centres)
        self.width, self.height = int(width), int(height)
        h = C.c_void_p()
        _check(self.lib, self.lib.vet_tiling_create(engine.handle, _ptr(arcs), self.n_arcs,
                                                    _ptr(centres) if self.n_centres else None, self.n_centres,
                                                    self.width, self.height, C.byref(h)))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self.lib.vet_tiling_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    @staticmethod
    def _inputs(cameras, background):
        cameras = np.ascontiguousarray(cameras, dtype=np.float64).reshape(-1, 9)
        bg = np.ascontiguousarray(background, dtype=np.uint8).reshape(3)
        return cameras, bg

    def render(self, cameras: np.ndarray, background=(255, 255, 255), out: Optional[np.ndarray] = None) -> np.ndarray:
        """cameras [n, 3, 3] (P, U, F per frame) -> uint8 [n, H, W, 3] on the host (into ``out`` when given: a C-contiguous
        uint8 array of that shape); synchronous."""
        cameras, bg = self._inputs(cameras, background)
        shape = (len(cameras), self.height, self.width, 3)
        if out is None:
            out = np.empty(shape, dtype=np.uint8)
        elif out.shape != shape or out.dtype != np.uint8 or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous uint8 array of shape {shape}")
        _check(self.lib, self.lib.vet_tiling_render_host(self.handle, _ptr(cameras), len(cameras), _ptr(bg), _ptr(out)))
        return out

    def render_device(self, cameras: np.ndarray, d_rgb: int, background=(255, 255, 255), stream=None):
        """The frames of ``cameras`` [n, 3, 3] into ``d_rgb`` (device, uint8 [n, H, W, 3], 4-byte aligned); asynchronous on
        ``stream`` as ``Plan.spatial_device``."""
        cameras, bg = self._inputs(cameras, background)
        _check(self.lib, self.lib.vet_tiling_render(self.handle, _ptr(cameras), len(cameras), _ptr(bg), d_rgb,
                                                    _stream(stream)))
