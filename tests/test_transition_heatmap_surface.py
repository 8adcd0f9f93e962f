"""Heatmaps of transition results, the parts that run without a GPU: the C-ABI surface, the analyzer's checks before
compute_entropy, and the denominator of the colours (the users present in each row's prior frame)."""
import ctypes

import numpy as np
import pandas as pd
import pytest

from tests.test_cabi_symbols import header_functions

ENTRIES = ["vet_heatmap_render_counts", "vet_heatmap_render_transition_result"]


# --------------------------------------------------------------------------- C-ABI
def test_header_library_and_signatures():
    from viewport_entropy_toolkit import _native
    fns = header_functions()
    assert set(ENTRIES) <= set(fns)
    lib = ctypes.CDLL(str(_native.LIB_PATH))
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert set(ENTRIES) <= set(_native.SIGNATURES)
    assert _native.SIGNATURES["vet_heatmap_render_counts"] == _native.SIGNATURES["vet_heatmap_render"]
    assert _native.SIGNATURES["vet_heatmap_render_transition_result"] == _native.SIGNATURES["vet_heatmap_render_result"]
    assert _native.load_library().vet_version() == 141


def test_null_arguments_are_invalid_without_a_device():
    """Argument checks come before any device call."""
    from viewport_entropy_toolkit import _native
    lib = _native.load_library()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.vet_heatmap_render_counts(None, None, None, None, None, 0, 0, None, None) == _native.VET_ERR_INVALID
    assert lib.vet_heatmap_render_counts(None, p, p, None, None, 0, 1, p, None) == _native.VET_ERR_INVALID
    assert lib.vet_heatmap_render_transition_result(None, None, None, None, None, 0, 0, 0, None) == _native.VET_ERR_INVALID
    assert lib.vet_heatmap_render_transition_result(p, None, p, None, None, 0, 0, 1, p) == _native.VET_ERR_INVALID
    assert b"NULL" in lib.vet_last_error()


# --------------------------------------------------------------------------- the analyzer
def test_heatmaps_before_compute_entropy(tmp_path):
    import viewport_entropy_toolkit as vt
    from viewport_entropy_toolkit.config import AnalyzerConfig
    from viewport_entropy_toolkit.data_types import ValidationError
    an = vt.TransitionEntropyAnalyzer(AnalyzerConfig(output_dir=tmp_path / "out"))
    with pytest.raises(ValidationError, match="No entropy results. Call compute_entropy first."):
        an.render_heatmaps()
    with pytest.raises(ValidationError, match="No entropy results. Call compute_entropy first."):
        an.save_heatmaps(tmp_path / "h.npy")
    assert not (tmp_path / "h.npy").exists()


def test_spatial_and_transition_share_one_implementation():
    import viewport_entropy_toolkit as vt
    from viewport_entropy_toolkit.analyzers._heatmaps import _HeatmapMixin
    for name in ("render_heatmaps", "save_heatmaps", "_frame_range", "_heatmap", "_heatmap_job", "_render_block"):
        assert getattr(vt.SpatialEntropyAnalyzer, name) is getattr(_HeatmapMixin, name)
        assert getattr(vt.TransitionEntropyAnalyzer, name) is getattr(_HeatmapMixin, name)
    assert vt.SpatialEntropyAnalyzer._heatmap_entry == "render_result"
    assert vt.TransitionEntropyAnalyzer._heatmap_entry == "render_transition_result"


# --------------------------------------------------------------------------- the denominator
# user -> frames present (of 0 .. 6; the ingest starts every track at time 0): u0 everywhere, u1 leaves after frame 2,
# u2 leaves after frame 0 and joins again at frame 3, u3 has a gap at 3, u4 is present in frames 0 and 5.
TRACKS = {"u0": range(7), "u1": range(3), "u2": [0, 3, 4, 5, 6], "u3": [0, 1, 2, 4, 5, 6], "u4": [0, 5]}


def _video(tmp_path):
    d = tmp_path / "video"
    d.mkdir()
    rng = np.random.default_rng(3)
    for name, frames in TRACKS.items():
        frames = np.asarray(list(frames))
        pd.DataFrame({"time": frames * 0.2, "2dmu": rng.uniform(0.05, 0.95, len(frames)),
                      "2dmv": rng.uniform(0.05, 0.95, len(frames)), "x": 1}).to_csv(d / f"{name}.csv", index=False)
    return d


def _reference_points_count(points_data):
    """len(points_list) of PlotManager.update_frame (utilities/visualization_utils.py:124-133) for every row."""
    from viewport_entropy_toolkit.data_types import RadialPoint
    out = []
    for i in range(len(points_data)):
        row = points_data.iloc[i]
        out.append(sum(1 for c in points_data.columns if c != "time" and row[c] is not None and isinstance(row[c], RadialPoint)))
    return np.array(out)


def test_prior_frame_presence_is_the_reference_denominator(tmp_path):
    import viewport_entropy_toolkit as vt
    from viewport_entropy_toolkit.config import AnalyzerConfig
    an = vt.TransitionEntropyAnalyzer(AnalyzerConfig(tile_counts=[20], output_dir=tmp_path / "out"))
    an.process_directory(_video(tmp_path))
    points = an._data_cache["points"]
    ref = _reference_points_count(points)
    assert sorted(ref.tolist()) == [2, 3, 3, 3, 3, 4, 5]            # frames in first-appearance (glob) order
    kind, times, a, b, _ = an._samples()
    assert kind == "grid" and np.array_equal(times, points["time"].to_numpy(dtype=np.float64))
    got = an._prior_frame_present(kind, a, b)
    assert got.dtype == np.int32 and got.tolist() == ref[:-1].tolist()           # row r <-> frame r, T-1 rows
    present = an._presence(kind, a, b)
    common = (present[:-1] & present[1:]).sum(axis=1)
    assert (got >= common).all() and (got != common).any()                      # not the common-user count
    # the ids path (a hand-assigned frame table) counts the same users
    an._data_cache["vectors"] = an._data_cache["vectors"]
    kind, _, ids, _, _ = an._samples()
    assert kind == "ids"
    assert an._prior_frame_present(kind, ids, None).tolist() == ref[:-1].tolist()
