"""Viewer clusters (who looks together, per window), CPU side: the C-ABI surface, the analyzers' method and its defaults, the
DataFrame glue, and the numpy oracle of tests/_cluster_oracle.py on hand-made cases whose answer is known without it.  No GPU."""
import ctypes
import inspect
import math
import re
from pathlib import Path

import numpy as np
import pytest

from tests import _cluster_oracle as co

W, H = 200, 100                      # 200 columns of 1.8 degrees, 100 rows: a viewer on the equator is (px, H // 2)
SYMBOLS = ("vet_viewer_clusters", "vet_viewer_clusters_ids", "vet_viewer_clusters_host")
COS10 = math.cos(math.radians(10.0))


def equator(cols):
    """direction ids [T][U] of viewers on the equator at the given columns (None: absent); cols is [T][U] or [U].  Column c is
    pixel c + 1: the quantiser's pixel 0 is longitude 0, not -180 (the reference's rule), so the columns start beside it"""
    cols = np.atleast_2d(np.array([[-1 if c is None else c for c in row] for row in np.atleast_2d(np.asarray(cols, dtype=object))]))
    return np.where(cols >= 0, (H // 2) * (W + 1) + cols + 1, -1).astype(np.int32)


def solve(ids, window=1, stride=1, cos_threshold=COS10, min_share=1.0, fractions=(0.5, 0.8, 0.95)):
    table = co.grid_table(W, H)
    near, c = co.frame_near(table, ids, cos_threshold)
    assert co.margin(c, cos_threshold) > 1e-9
    return co.rows(near, ids, table, window, stride, min_share, fractions)


def test_entry_points_are_in_the_ctypes_table_with_the_headers_arity():
    from viewport_entropy_toolkit import _native
    header = (Path(__file__).resolve().parent.parent / "include" / "vet.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in SYMBOLS + ("vet_test_cluster_tile",):
        assert name in _native.SIGNATURES, name
        args = re.search(rf"\b{name}\s*\(([^)]*)\)", text).group(1)
        assert len(args.split(",")) == len(_native.SIGNATURES[name][1]), name
    i, p, d = ctypes.c_int, ctypes.c_void_p, ctypes.c_double
    for tail, at in (("", 7), ("_ids", 6), ("_host", 8)):      # the leading arguments of the other row calls, then the call's own
        mine = _native.SIGNATURES["vet_viewer_clusters" + tail]
        assert mine[1][:at] == _native.SIGNATURES["vet_dispersion" + tail][1][:at], tail
        assert mine[1][at:at + 4] == [d, d, p, i], tail
        assert mine[1][at + 4:] == [p] * (7 if tail == "_host" else 9), tail       # seven outputs (+ status, stream)
    lib = ctypes.CDLL(str(_native.LIB_PATH))
    for name in SYMBOLS + ("vet_test_cluster_tile",):
        assert hasattr(lib, name), f"{name} is not exported"
    for name in ("viewer_clusters", "viewer_clusters_device"):
        assert hasattr(_native.Plan, name)
    assert hasattr(_native.Engine, "test_cluster_tile")
    assert _native.load_library().vet_version() == 141
    for phrase in ("NEAR", "LINKED", "cos_threshold", "min_share", "ALL ORDERED PAIRS", "Not built", "complete-linkage",
                   "not taken from the reference", "8192"):
        assert phrase in header, phrase


def test_analyzers_have_the_method_with_the_stated_defaults():
    from viewport_entropy_toolkit.analyzers import NaiveSpatialEntropyAnalyzer, SpatialEntropyAnalyzer, TransitionEntropyAnalyzer
    for cls in (SpatialEntropyAnalyzer, NaiveSpatialEntropyAnalyzer, TransitionEntropyAnalyzer):
        sig = inspect.signature(cls.compute_viewer_clusters)
        got = {k: v.default for k, v in sig.parameters.items() if k != "self"}
        assert got == dict(window=1, stride=1, threshold_deg=30.0, min_share=1.0, fractions=(0.5, 0.8, 0.95), keep_labels=True,
                           keep_centroids=False, keep_links=False), cls.__name__


def test_argument_checks_of_the_python_layer():
    from viewport_entropy_toolkit import _native
    ok = _native.Plan._cluster_args(30.0, 1.0, (0.5, 0.8, 0.95))
    assert ok[0] == math.cos(math.radians(30.0)) and ok[1] == 1.0 and ok[2].tolist() == [0.5, 0.8, 0.95]
    assert _native.Plan._cluster_args(0.0, 0.5, ())[0] == 1.0 and _native.Plan._cluster_args(180.0, 0.5, None)[0] == -1.0
    for bad in ((-1.0, 1.0, (0.5,)), (181.0, 1.0, (0.5,)), (float("nan"), 1.0, (0.5,)), (True, 1.0, (0.5,)), (30.0, 0.0, (0.5,)),
                (30.0, 1.5, (0.5,)), (30.0, float("nan"), (0.5,)), (30.0, 1.0, (0.0,)), (30.0, 1.0, (1.1,)),
                (30.0, 1.0, (float("nan"),)), (30.0, 1.0, (0.5,) * 17), (30.0, 1.0, "x")):
        with pytest.raises(ValueError):
            _native.Plan._cluster_args(*bad)


def test_two_far_groups_and_a_loner():
    res = solve(equator([0, 5, 50, 55, 120]))
    assert res["labels"].tolist() == [[0, 0, 1, 1, 2]]
    assert res["sizes"].tolist() == [[2, 2, 1, 0, 0]]
    assert res["counts"][:, 0].tolist() == [5, 3, 2, 1, 2]
    assert res["top"].tolist() == [[2, 2, 3]]                   # 2.5, 4.0 and 4.75 of 5 viewers: sizes 2, 2, 1 in that order
    H_want = math.log2(5) - (2 * 1 + 2 * 1) / 5
    assert res["stats"][:, 0] == pytest.approx([H_want, H_want / math.log2(5), 0.4], rel=1e-15)
    assert res["links"].tolist() == [[[0b00010], [0b00001], [0b01000], [0b00100], [0]]]
    # cluster 0's centroid: the two unit vectors on the equator, 9 degrees apart (the quantiser rounds its Vectors to 6 decimals)
    assert np.linalg.norm(res["centroids"][0, 0]) == pytest.approx(2 * math.cos(math.radians(4.5)), rel=1e-6)
    assert (res["centroids"][0, 3:] == 0).all()


def test_a_chain_is_one_cluster_although_its_ends_are_not_near():
    ids = equator([0, 5, 10])
    near, _ = co.frame_near(co.grid_table(W, H), ids, COS10)
    assert near[0, 0, 1] and near[0, 1, 2] and not near[0, 0, 2]
    res = solve(ids)
    assert res["labels"].tolist() == [[0, 0, 0]] and res["counts"][:, 0].tolist() == [3, 1, 3, 0, 2]
    assert res["stats"][:, 0] == pytest.approx([0.0, 0.0, 1.0], abs=1e-15)


def test_min_share_over_a_four_frame_window():
    # viewers 0 and 1 are near in two of the four frames both are in; viewer 2 is near viewer 1 in one of its two frames with it
    cols = [[0, 5, None], [0, 5, 10], [0, 7, 14], [0, 7, None]]
    ids = equator(cols)
    full = solve(ids, window=4, min_share=1.0)
    half = solve(ids, window=4, min_share=0.5)
    low = solve(ids, window=4, min_share=0.51)
    assert full["labels"].tolist() == [[0, 1, 2]] and full["counts"][4, 0] == 0
    assert half["labels"].tolist() == [[0, 0, 0]] and half["counts"][4, 0] == 2          # 2 >= 0.5 * 4 and 1 >= 0.5 * 2
    assert low["labels"].tolist() == [[0, 1, 2]]
    per_frame = solve(ids, window=1)
    assert per_frame["labels"].tolist() == [[0, 0, -1], [0, 0, 0], [0, 1, 2], [0, 1, -1]]


def test_a_viewer_present_in_no_frame_and_a_window_with_nobody():
    ids = equator([[0, None, 5], [0, None, 5], [None, None, None]])
    res = solve(ids, window=2)
    assert res["labels"].tolist() == [[0, -1, 0], [0, -1, 0]]
    assert res["counts"][:, 0].tolist() == [2, 1, 2, 0, 1]
    assert (res["links"][:, 1] == 0).all()
    empty = solve(ids[2:], window=1)
    assert empty["labels"].tolist() == [[-1, -1, -1]] and (empty["counts"] == 0).all() and np.isnan(empty["stats"]).all()
    assert (empty["top"] == 0).all() and (empty["sizes"] == 0).all() and (empty["centroids"] == 0).all()


def test_never_co_present_viewers_are_not_linked_even_on_one_direction():
    res = solve(equator([[3, None], [None, 3]]), window=2)
    assert res["labels"].tolist() == [[0, 1]] and res["counts"][:, 0].tolist() == [2, 2, 1, 2, 0]


def test_frame_glue_builds_the_stated_columns():
    from viewport_entropy_toolkit.analyzers._base import _EntropyAnalyzerBase as Base
    ids = equator([[0, 5, 50, 55, 120]] * 3)
    res = solve(ids, window=2)
    names, times = ["a", "b", "c", "d", "e"], np.array([0.0, 0.5, 1.0])
    df = Base._clusters_frame(times, names, 2, 1, dict(res, cos_threshold=COS10, code=0), 10.0, 1.0, (0.5, 0.8, 0.95))
    assert list(df.columns) == ["time", "time_end", "viewers", "clusters", "largest", "largest_share", "singletons", "links",
                                "entropy", "entropy_norm", "streams", "labels", "sizes", "centroids", "links_bits"]
    assert df["time"].tolist() == [0.0, 0.5] and df["time_end"].tolist() == [0.5, 1.0]
    assert df["streams"][0].tolist() == [2, 2, 3] and df["labels"][1].tolist() == [0, 0, 1, 1, 2]
    assert df["centroids"][0].shape == (5, 3) and df["links_bits"][0].shape == (5, 1) and df["links_bits"][0].dtype == np.uint64
    assert np.shares_memory(df["labels"][0], res["labels"])
    assert df.attrs == dict(threshold_deg=10.0, cos_threshold=COS10, min_share=1.0, fractions=(0.5, 0.8, 0.95), window=2, stride=1,
                            users=names)
    slim = Base._clusters_frame(times, names, 2, 1, dict(res, labels=None, sizes=None, centroids=None, links=None,
                                                         cos_threshold=COS10, code=0), 10.0, 1.0, (0.5, 0.8, 0.95))
    assert list(slim.columns)[-1] == "streams"
