"""The status every render and ray-buffer entry point returns for refused calls, on a host-only context and with a NULL context, against the
table recorded from the library before the entry points were routed through one path (tests/golden/refusal_matrix.json, written by
tests/golden/make_refusal_matrix.py: the grid is cases() there).  The statuses show which check comes first — FT_ERR_INVALID before
FT_ERR_NO_DEVICE or after it, the 2^32 job limit before the device is asked for — and the sixteen forms differ in that on purpose.

No GPU is needed and none is touched: a host-only context never calls HIP, the scene is NULL, every call is refused and no buffer is read or
written (their addresses are plain integers).  What the table cannot show: the ray-buffer forms ask for the device before they look at n, so
n = 0 (FT_OK) and n >= 0xFFFF0000 (FT_ERR_UNSUPPORTED) are visible only with a GPU (tests/test_gpu_parity.py, tests/test_gpu_rays_device.py)."""
import json
import os
import sys

from fraytracer_amd import _lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_refusal_matrix as matrix  # noqa: E402
import make_refusal_matrix_records_field as records_field  # noqa: E402

ENTRY_POINTS = sorted(list(matrix.FRAMES) + list(matrix.RAY_FORMS))


def test_the_table_covers_the_sixteen_entry_points():
    table = json.load(open(matrix.TABLE))
    assert len(ENTRY_POINTS) == 16 and sorted(table["rows"]) == ENTRY_POINTS
    assert table["recorded_from_commit"] == "5de1cdf"               # the parent of the refactor: not the code under test
    cases = matrix.cases()
    assert table["calls"] == len(cases) == sum(len(r) for r in table["rows"].values())
    for name in ENTRY_POINTS:
        assert len(table["rows"][name]) == sum(1 for n, _ in cases if n == name), name
    seen = set("".join(table["rows"].values()))
    assert {"I", "N", "U"} <= seen and "O" not in seen and "H" not in seen          # every call is refused, and the table discriminates


def test_every_refused_call_returns_the_recorded_status():
    want = json.load(open(matrix.TABLE))["rows"]
    got = matrix.run(_lib)
    at = dict.fromkeys(ENTRY_POINTS, 0)
    wrong = []
    for name, case in matrix.cases():
        i = at[name]
        at[name] += 1
        if got[name][i] != want[name][i]:
            wrong.append((name, case, "got " + got[name][i], "recorded " + want[name][i]))
    assert not wrong, f"{len(wrong)} of {sum(at.values())} calls differ; the first: {wrong[:5]}"


def test_the_record_and_field_forms_return_the_recorded_status_and_message():
    """The second table (tests/golden/refusal_matrix_records_field.json, the grid is cases() of make_refusal_matrix_records_field.py): the eleven record
    and field entry points, recorded before they were routed through the shared host path.  Here a call can also have nothing to do (n = 0: FT_OK),
    the scene varies (the context's own, one under 33 lights, NULL, another context's) and every refusal's ft_last_error text is pinned too."""
    table = json.load(open(records_field.TABLE))
    assert table["recorded_from_commit"] == "bad71da"               # the parent of the refactor: not the code under test
    cases = records_field.cases()
    assert len(records_field.FORMS) == 11 and sorted(table["rows"]) == sorted(records_field.FORMS)
    assert table["calls"] == len(cases) < 20000
    seen = set("".join(r["status"] for r in table["rows"].values()))
    assert {"I", "N", "U", "O"} <= seen and "H" not in seen
    got, messages = records_field.run(_lib)
    at = dict.fromkeys(records_field.FORMS, 0)
    wrong = []
    for name, case in cases:
        i = at[name]
        at[name] += 1
        want_row, got_row = table["rows"][name], got[name]
        want = (want_row["status"][i], None if want_row["message"][i] < 0 else table["messages"][want_row["message"][i]])
        have = (got_row["status"][i], None if got_row["message"][i] < 0 else messages[got_row["message"][i]])
        if have != want:
            wrong.append((name, case, "got", have, "recorded", want))
    assert all(at[name] == len(table["rows"][name]["status"]) == len(table["rows"][name]["message"]) for name in at)
    assert not wrong, f"{len(wrong)} of {len(cases)} calls differ; the first: {wrong[:5]}"
