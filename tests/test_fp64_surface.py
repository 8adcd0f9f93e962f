"""The FP64 formulation's surface (no GPU): the C-ABI entry point vet_plan_set_fp64, Plan.set_fp64, the formulation code
of `dtable` and the analyzer's keyword-only switch."""
import ctypes
import inspect
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "vet.h"


def test_header_declares_set_fp64_and_the_library_exports_it():
    from viewport_entropy_toolkit import _native
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert re.search(r"\bint\s+vet_plan_set_fp64\s*\(\s*vet_plan\s*\*\s*plan\s*,\s*int\s+on\s*\)\s*;", text)
    assert hasattr(ctypes.CDLL(str(_native.LIB_PATH)), "vet_plan_set_fp64")
    assert _native.SIGNATURES["vet_plan_set_fp64"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])
    # the header documents formulation 4
    assert re.search(r"\*\s+4 dtable\b", HEADER.read_text())


def test_plan_has_set_fp64():
    from viewport_entropy_toolkit import _native
    assert callable(getattr(_native.Plan, "set_fp64", None))
    assert list(inspect.signature(_native.Plan.set_fp64).parameters) == ["self", "on"]


def test_formulation_map_knows_dtable():
    from viewport_entropy_toolkit import _native
    assert _native.FORMULATIONS == {0: "table", 1: "sweep", 2: "precise", 3: "ftable", 4: "dtable"}


def test_analyzer_fp64_switch_constructs_without_a_device(tmp_path):
    from viewport_entropy_toolkit import SpatialEntropyAnalyzer, AnalyzerConfig
    an = SpatialEntropyAnalyzer(AnalyzerConfig(output_dir=tmp_path), fp64=True)
    assert an._fp64 is True and an._plan is None           # no plan (and no device) until compute_entropy
    plain = SpatialEntropyAnalyzer(AnalyzerConfig(output_dir=tmp_path))
    assert plain._fp64 is False and plain._plan is None
    # keyword-only: the reference-shaped positional call has one parameter
    params = inspect.signature(SpatialEntropyAnalyzer.__init__).parameters
    assert params["fp64"].kind is inspect.Parameter.KEYWORD_ONLY
    try:
        SpatialEntropyAnalyzer(AnalyzerConfig(output_dir=tmp_path), True)
    except TypeError:
        pass
    else:
        raise AssertionError("fp64 must not be accepted positionally")

