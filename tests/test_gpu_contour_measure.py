"""Contour measures on the GPU (ft_slices_measure): every record bit for bit against the restatement of the rule
(tests/contour_measure_restatement.py) — through the internal entry on contours no slicer would write (every run shape of a wave, closing segments
across waves and workgroups, tiny polylines, all axes, scattered slices, non-finite and extreme coordinates, wrapping low words, every grid, the eager
variant, guard words) and through the public path (a torus on every axis, refined, open polylines, device memory, tensors, lifetimes)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import _lib
from helpers import options_left_at_defaults  # noqa: F401  (a fixture)

import contour_measure_cases as cases
import contour_measure_restatement as rule
import mesh_cases

pytestmark = pytest.mark.gpu

L = _lib.lib
OK, INVALID = _lib.FT_OK, _lib.FT_ERR_INVALID
POLY = L.ft_ctx_measure_polylines                                                          # internal: not in the header
POLY.restype, POLY.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
GRID = L.ft_ctx_contour_measure_grid
GRID.restype, GRID.argtypes = C.c_int, [C.c_void_p, C.c_int32]
PROBE = L.ft_ctx_contour_measure_probe
PROBE.restype, PROBE.argtypes = C.c_int, [C.c_void_p, C.c_int32]


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def measure(gpu, p, rec, axis, n_slices, want_polylines=True, want_slices=True):
    """both record arrays through the internal entry, each between guard words"""
    p, rec = np.ascontiguousarray(p, np.float32), np.ascontiguousarray(rec, np.int32)
    raw_p, raw_s = np.full(len(rec) * 7 + 8, 7.25), np.full(n_slices * 9 + 8, 7.25)        # 56 and 72 bytes per record, guard words behind them
    rc = POLY(gpu._ctx, ptr(p), len(p), ptr(rec), len(rec), axis, n_slices, ptr(raw_p) if want_polylines else None, ptr(raw_s) if want_slices else None)
    assert rc == OK, _lib.last_error()
    assert (raw_p[len(rec) * 7 if want_polylines else 0:] == 7.25).all() and (raw_s[n_slices * 9 if want_slices else 0:] == 7.25).all()
    return raw_p[:len(rec) * 7].view(rule.RECORD), raw_s[:n_slices * 9].view(rule.SLICE_RECORD)


def assert_same_records(got, want, what):
    dtype = want.dtype
    g = got if isinstance(got, np.ndarray) and got.dtype == dtype else np.ascontiguousarray(got).view(dtype).reshape(-1)
    assert g.shape == want.shape, (what, g.shape, want.shape)
    for name in dtype.names:
        a, b = np.ascontiguousarray(g[name]), np.ascontiguousarray(want[name])
        kind = {8: np.uint64, 4: np.uint32}[a.dtype.itemsize]
        same = a.view(kind) == b.view(kind)
        assert same.all(), (what, name, int((~same).sum()), a[~same][:3], b[~same][:3])
    assert rule.same_bytes(g, want), what


def assert_both(got, want, what):
    assert_same_records(got[0], want[0], what + ": polylines")
    assert_same_records(got[1], want[1], what + ": slices")


# ---- contours no slicer would write ----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("closed", [True, False])
@pytest.mark.parametrize("n", cases.SINGLE_COUNTS)
def test_one_polyline(gpu, n, closed):
    p, rec, axis, n_slices = cases.single(n, closed)
    got = measure(gpu, p, rec, axis, n_slices)
    assert_both(got, rule.measure(p, rec, axis, n_slices), f"{n} points, closed {closed}")
    if n >= 3:
        assert got[0]["length"][0] > 0 and (got[0]["area"][0] > 0 or not closed) and got[1]["n_outer"][0] == int(closed)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_cases(gpu, name):
    p, rec, axis, n_slices = cases.case(name)
    got = measure(gpu, p, rec, axis, n_slices)
    want = rule.measure(p, rec, axis, n_slices)
    assert_both(got, want, name)
    lines, per = got
    if name == "straddling":
        assert lines["area"][1] > 0 and per["n_outer"][0] == 2
    elif name == "triangles64":
        assert (np.sign(lines["area"]) == np.where(np.arange(64) % 2 == 0, 1, -1)).all() and per["n_polylines"].tolist() == [22, 21, 21]
    elif name == "tiny_counts":
        assert lines["extent_exponent"][0] == 10 and np.isinf(lines["bbox_min"][[0, 3, 5]]).all() and per["n_polylines"].tolist() == [3, 3]
    elif name.startswith("permuted"):
        assert lines["area"].tolist() == [18.0, -1.0] and per["area"].tolist() == [17.0] and lines["length"].tolist() == [22.0, 4.0]
        assert (per["n_outer"][0], per["n_holes"][0]) == (1, 1)
    elif name == "scattered_slices":
        assert per["n_polylines"].tolist() == [2, 2, 1, 0] and np.isinf(per["bbox_min"][3]).all() and per["length"][3] == 0
    elif name == "non_finite":
        assert lines["n_unmeasured"].tolist() == [7, 4, 0] and per["n_unmeasured"].tolist() == [11, 0]      # the last polyline: non-finite along the axis only
        assert np.isfinite(lines["bbox_max"][0]).all() and lines["bbox_min"][1, 1] == np.inf and np.isfinite(lines["bbox_min"][1, 0])
    elif name == "huge_E128":
        assert lines["extent_exponent"][0] == 128 and np.isfinite(lines["moment"]).all() and (lines["length"] > 1e38).all()
    elif name.startswith("denormal"):
        assert lines["extent_exponent"][0] == int(name.split("E")[1]) and (lines["length"] > 0).all() and (lines["area"] != 0).all()
    elif name == "wrapping":
        sums, _ = rule.integer_sums(p, rec, axis)
        assert sums[0][1] < 0 and sums[1][1] > 2 ** 64 and sums[2][1] < -(2 ** 64) and lines["area"][0] < 0 < lines["area"][1]
    elif name == "ties":
        assert lines["length"][:3].tolist() == [0.0, 2.0 ** -87, 2.0 ** -87]


def test_either_output_alone(gpu):
    p, rec, axis, n_slices = cases.case("scattered_slices")
    want = rule.measure(p, rec, axis, n_slices)
    assert_same_records(measure(gpu, p, rec, axis, n_slices, want_slices=False)[0], want[0], "polylines alone")
    assert_same_records(measure(gpu, p, rec, axis, n_slices, want_polylines=False)[1], want[1], "slices alone")
    none = np.zeros((0, 4), np.int32)                                                      # points without polylines: the extent, and empty slices
    got = measure(gpu, p, none, axis, n_slices)
    assert_both(got, rule.measure(p, none, axis, n_slices), "no polylines")
    assert got[1]["extent_exponent"].tolist() == [want[0]["extent_exponent"][0]] * n_slices and np.isinf(got[1]["bbox_min"]).all()


@pytest.mark.parametrize("name", ["mixed", "wrapping", "triangles64", "straddling"])
def test_every_grid_and_the_eager_variant_give_the_same_bytes(gpu, name):
    p, rec, axis, n_slices = cases.case(name)
    want = rule.measure(p, rec, axis, n_slices)
    try:
        for grid in (1, 2, 7, 0):                                                          # 0: as many workgroups as fill the device
            assert GRID(gpu._ctx, grid) == OK
            for eager in (0, 1):
                assert PROBE(gpu._ctx, eager) == OK
                assert_both(measure(gpu, p, rec, axis, n_slices), want, f"{name}, grid {grid}, eager {eager}")
    finally:
        assert GRID(gpu._ctx, 0) == OK and PROBE(gpu._ctx, 0) == OK


def test_internal_entry_validates_on_the_host(gpu):
    p, rec, axis, n_slices = cases.case("scattered_slices")
    out_p, out_s = np.zeros(len(rec), rule.RECORD), np.zeros(n_slices, rule.SLICE_RECORD)
    for row, col, value in ((0, 0, -1), (4, 1, 34), (1, 1, -1), (2, 2, 4), (2, 2, -1), (2, 0, 39)):      # outside the points, outside the slices, overlapping
        bad = np.array(rec)
        bad[row, col] = value
        assert POLY(gpu._ctx, ptr(p), len(p), ptr(bad), len(bad), axis, n_slices, ptr(out_p), ptr(out_s)) == INVALID, (row, col, value)
    assert POLY(gpu._ctx, ptr(p), len(p), ptr(np.array(rec)), len(rec), 3, n_slices, ptr(out_p), ptr(out_s)) == INVALID
    assert POLY(gpu._ctx, ptr(p), len(p), ptr(np.array(rec)), len(rec), axis, n_slices, ptr(out_p), ptr(out_p)) == INVALID
    assert POLY(gpu._ctx, ptr(p), len(p), ptr(np.array(rec)), len(rec), axis, n_slices, None, None) == INVALID


# ---- the public path -----------------------------------------------------------------------------------------------------------------------------


def want_of(c):
    return rule.measure(ft.Mesh._host(c.points), ft.Mesh._host(c.polylines), c.axis, c.slices)


def torus(axis):
    return ft.SdfForm.Primitive.torus((0.0, 0.0, 0.0), cases.torus_normal(axis), cases.TORUS_MAJOR, cases.TORUS_MINOR)


@pytest.mark.parametrize("refine", [None, 6])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_torus(gpu, axis, refine):
    origin, step, counts = cases.torus_lattice(axis)
    c = ft.SdfForm.slice(torus(axis), origin, step, counts, axis=axis, device=gpu, refine=refine, measures=True)
    assert c.slices == 5 and isinstance(c.measures, ft.ContourMeasures) and len(c.measures) == len(c.polylines) and len(c.layer_measures) == 5
    want = want_of(c)
    assert_both((c.measures.records, c.layer_measures.records), want, f"torus, axis {axis}, refine {refine}")
    per = c.layer_measures
    middle = np.flatnonzero(c.polylines[:, 2] == 2)
    assert per.n_outer[2] == 1 and per.n_holes[2] == 1 and per.n_polylines[2] == 2 and len(middle) == 2 and c.polylines[middle, 3].tolist() == [1, 1]
    a = c.measures.area[middle]
    assert a[0] * a[1] < 0 and per.area[2] == want[1]["area"][2] and per.n_unmeasured.sum() == 0
    R, r = cases.TORUS_MAJOR, cases.TORUS_MINOR
    annulus = np.pi * ((R + r) ** 2 - (R - r) ** 2)
    assert abs(per.area[2] - annulus) < (0.05 if refine is None else 0.02)
    assert np.abs(per.centroid[2]).max() < 1e-6 and per.n_polylines[[0, 4]].tolist() == [0, 0] and np.isinf(per.bbox_min[0]).all()
    assert abs(per.length[2] - 2 * np.pi * 2 * R) < 0.05                                   # both circles: 2 pi (R + r) + 2 pi (R - r)
    plain = ft.SdfForm.slice(torus(axis), origin, step, counts, axis=axis, device=gpu, refine=refine)      # the default: today's result
    assert plain.measures is None and plain.layer_measures is None and np.array_equal(plain.points, c.points)


def test_open_polylines_of_a_scene_lattice_with_non_finite_values(gpu, oracle):
    origin, step, d = mesh_cases.oracle_lattice(oracle, "c3_64")
    d = np.array(d)
    d[10, :, :] = np.nan                                                                   # two slabs of non-finite values through the body: in every plane
    d[:, :, 11] = np.inf                                                                   # of axis 0 and 2 a line of them cuts the contours open
    for axis in (0, 2):
        c = gpu.slice_values(d, origin, step, axis, measures=True)
        assert c.skipped > 0 and (c.polylines[:, 3] == 0).any() and (c.polylines[:, 3] == 1).any()
        assert_both((c.measures.records, c.layer_measures.records), want_of(c), f"c3_64 with holes in the lattice, axis {axis}")
        assert c.layer_measures.n_polylines.sum() == len(c.polylines) and c.layer_measures.n_closed.sum() == c.closed


@pytest.fixture(scope="module")
def hip():
    h = C.CDLL("libamdhip64.so.7")             # the runtime the library is linked against (already loaded: same instance)
    h.hipMalloc.argtypes, h.hipMemcpy.argtypes, h.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p]
    return h


def test_device_records_host_records_and_contours_that_outlive_their_scene(gpu, hip):
    """records in device memory between guard words, then one synchronisation: the same bytes as host records; a misaligned address
    and one address for both are refused; the scene is destroyed before its contours are measured"""
    axis = 1
    origin, step, counts = cases.torus_lattice(axis)
    lat, _ = ft.api._lattice(origin, step, counts)
    ds = ft.api._form_scene(torus(axis), gpu)
    h = C.c_void_p()
    assert L.ft_slice_lattice(gpu._ctx, ds._scene, C.byref(lat), axis, 0.0, 0.0, 0, C.byref(h)) == OK
    ds.close()                                                                             # the contours outlive their scene
    try:
        info = _lib.SlicesInfo()
        assert L.ft_slices_get_info(h, C.byref(info)) == OK
        nL, nW = int(info.n_polylines), int(info.n_slices)
        points, rec = np.zeros((int(info.n_points), 3), np.float32), np.zeros((nL, 4), np.int32)
        assert L.ft_slices_read(h, ptr(points), ptr(rec), None, None) == OK
        want = rule.measure(points, rec, axis, nW)
        host_p, host_s = np.zeros(nL, np.dtype(_lib.CONTOUR_MEASURE_DTYPE)), np.zeros(nW, np.dtype(_lib.SLICE_MEASURE_DTYPE))
        assert L.ft_slices_measure(h, ptr(host_p), ptr(host_s)) == OK
        assert_both((host_p, host_s), want, "host records after the scene is gone")
        one = (_lib.SliceMeasure * nW)()
        assert L.ft_slices_measure(h, None, one) == OK and one[2].n_outer == 1 and one[2].n_holes == 1 and one[2].area == want[1]["area"][2]
        words = 8 + 7 * nL + 9 * nW + 8
        guard = np.full(words, 7.25)
        base = C.c_void_p()
        assert hip.hipMalloc(C.byref(base), C.c_size_t(guard.nbytes)) == 0
        try:
            assert hip.hipMemcpy(base, ptr(guard), C.c_size_t(guard.nbytes), 1) == 0
            d_p, d_s = base.value + 64, base.value + 64 + 56 * nL                           # 56 nL is a multiple of 8
            for off in (1, 2, 4, 7):
                assert L.ft_slices_measure(h, C.c_void_p(d_p + off), C.c_void_p(d_s)) == INVALID and "aligned" in _lib.last_error()
                assert L.ft_slices_measure(h, C.c_void_p(d_p), C.c_void_p(d_s + off)) == INVALID
            assert L.ft_slices_measure(h, C.c_void_p(d_p), C.c_void_p(d_p)) == INVALID and "same address" in _lib.last_error()
            assert L.ft_slices_measure(h, None, None) == INVALID
            assert L.ft_slices_measure(h, C.c_void_p(d_p), C.c_void_p(d_s)) == OK
            assert hip.hipDeviceSynchronize() == 0                                         # the one synchronisation: the call itself made none
            back = np.empty_like(guard)
            assert hip.hipMemcpy(ptr(back), base, C.c_size_t(back.nbytes), 2) == 0
            assert (back[:8] == 7.25).all() and (back[-8:] == 7.25).all()                  # nothing outside the records
            assert_both((back[8:8 + 7 * nL], back[8 + 7 * nL:-8]), want, "device records")
        finally:
            assert hip.hipFree(base) == 0
    finally:
        L.ft_slices_destroy(h)


TENSOR_PATH = r"""
import json, sys
import numpy as np
import torch                              # before the library: torch's HIP runtime is the one the process loads first
import fraytracer_amd as ft
sys.path.insert(0, "tests")
import contour_measure_cases as cases
import contour_measure_restatement as rule
host = lambda t: np.ascontiguousarray(t.detach().cpu().numpy())
dev = ft.Device(0)
r = {}
axis = 2
origin, step, counts = cases.torus_lattice(axis)
form = ft.SdfForm.Primitive.torus((0.0, 0.0, 0.0), cases.torus_normal(axis), cases.TORUS_MAJOR, cases.TORUS_MINOR)
like = torch.empty(1, device="cuda")
c = ft.SdfForm.slice(form, origin, step, counts, axis=axis, device=dev, measures=True)
want = rule.measure(c.points, c.polylines, axis, counts[axis])
t = ft.api._form_scene(form, dev).slice_lattice(origin, step, counts, axis=axis, like=like, measures=True)
torch.cuda.synchronize()
rec, per = t.measures.records, t.layer_measures.records
r["tensors"] = bool(rec.is_cuda and per.is_cuda and tuple(rec.shape) == (len(want[0]), 14) and tuple(per.shape) == (5, 18) and rec.dtype == torch.float32 and t.points.is_cuda)
r["aligned"] = rec.data_ptr() % 8 == 0 and per.data_ptr() % 8 == 0
r["polylines"] = rule.same_bytes(t.measures.host(), want[0])
r["slices"] = rule.same_bytes(t.layer_measures.host(), want[1])
r["properties"] = bool(np.array_equal(t.layer_measures.area, want[1]["area"]) and t.layer_measures.n_holes[2] == 1 and t.measures.bbox_min.dtype == np.float32)
side = torch.cuda.Stream()                # a lattice of values made by torch on a side stream: the stream hand-over
side.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(side):
    vals = torch.from_numpy(cases.torus_distances(axis)).cuda() + 0
    v = dev.slice_values(vals, origin, step, axis, measures=True)
side.synchronize()
r["values on a side stream"] = bool(v.measures.records.is_cuda and rule.same_bytes(v.measures.host(), rule.measure(host(v.points), host(v.polylines), axis, 5)[0])
                                    and rule.same_bytes(v.layer_measures.host(), rule.measure(host(v.points), host(v.polylines), axis, 5)[1]))
dev.close()
print(json.dumps(r))
"""


def test_tensor_path_in_a_process_that_loads_torch_first():
    """device tensors in, device records out, on the caller's stream: in a child process that loads torch before the library"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", TENSOR_PATH], cwd=root, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    failed = [k for k, v in r.items() if v is not True]
    assert not failed, failed
