"""The trace kernels and their lookup are generated from one table of builds and one list of forms (kernels.hip FT_TRACE_BUILDS, FT_TRACE_FORMS).
What the lookup answers, and which kernels exist, against the table recorded from the library before that (tests/golden/trace_kernel_matrix.json,
written by tests/golden/make_trace_kernel_matrix.py: the grid is keys() there): every family, every carved kind and values that are none, with and
without EXTENSION, glibc math and views, every shade form and one that is none.

No GPU is needed and none is touched: ft_trace_kernel_for only returns the address of a kernel handle, which is named by the library's own exported
symbols."""
import json
import os
import sys

from fraytracer_amd import _lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_trace_kernel_matrix as matrix  # noqa: E402


def test_the_table_covers_the_grid_and_every_kernel():
    table = json.load(open(matrix.TABLE))
    assert table["recorded_from_commit"] == "9934c09"               # the parent of the refactor: not the code under test
    assert "static" in table["header"] and "extern" in table["header"]
    names = [matrix.key_name(k) for k in matrix.keys()]
    assert len(names) == 1120 == len(set(names)) and sorted(table["answers"]) == sorted(names)
    assert len(table["kernels"]) == 56 == len(set(table["kernels"]))
    assert set(table["answers"].values()) == set(table["kernels"]) | {"null"}      # every kernel is reached, and only kernels are


def test_the_library_exports_exactly_the_recorded_kernels():
    assert matrix.exported_handles(_lib.LIB_PATH) == json.load(open(matrix.TABLE))["kernels"]


def test_every_key_resolves_to_the_recorded_kernel():
    want = json.load(open(matrix.TABLE))["answers"]
    got = matrix.run(_lib.lib)
    wrong = [(k, "got " + got[k], "recorded " + want[k]) for k in want if got[k] != want[k]]
    assert not wrong, f"{len(wrong)} of {len(want)} keys differ; the first: {wrong[:5]}"
