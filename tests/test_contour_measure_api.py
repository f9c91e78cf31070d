"""Contour measures (ft_slices_measure), the parts that need no GPU: the ABI, the header's statement of the rule, every refusal that comes before the
device is asked for and their order on a host-only context, empty contours, the internal entry's host validation, the Python surface, the build's
new translation unit, the C++ and F# mirrors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import _lib
from helpers import HEADER, ROOT, assert_cpp_compiles, assert_declared_exported_bound, dev_ptr as _p, host_ptr as ptr

import contour_measure_restatement as rule

INVALID, NO_DEVICE, OK = _lib.FT_ERR_INVALID, _lib.FT_ERR_NO_DEVICE, _lib.FT_OK
L = _lib.lib


def test_symbols_structs_and_the_abi_version():
    assert_declared_exported_bound(("ft_slices_measure",))
    assert C.sizeof(_lib.ContourMeasure) == 56 and C.sizeof(_lib.SliceMeasure) == 72
    assert np.dtype(_lib.CONTOUR_MEASURE_DTYPE).itemsize == 56 and np.dtype(_lib.SLICE_MEASURE_DTYPE).itemsize == 72
    assert np.dtype(_lib.CONTOUR_MEASURE_DTYPE) == rule.RECORD and np.dtype(_lib.SLICE_MEASURE_DTYPE) == rule.SLICE_RECORD
    assert [n for n, _ in _lib.SliceMeasure._fields_] == list(rule.SLICE_RECORD.names) and [n for n, _ in _lib.ContourMeasure._fields_] == list(rule.RECORD.names)
    assert L.ft_abi_version() == 5                                                         # additive: the ABI version stays
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert "#define FT_ABI_VERSION 5" in text and "ft_ctx_measure_polylines" not in text    # the internal entry is exported, not declared
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for name in ("ft_ctx_measure_polylines", "ft_ctx_contour_measure_grid", "ft_ctx_contour_measure_probe"):
        assert re.search(r"\bT " + name + r"\b", out), name
    assert ft.ContourMeasures is ft.api.ContourMeasures and "ContourMeasures" in ft.__all__


def test_header_is_still_plain_c99(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER])
    src = tmp_path / "use.c"
    src.write_text('#include "fraytracer_hip.h"\n'
                   "typedef char polyline_record_is_56_bytes[sizeof(ft_contour_measure) == 56 ? 1 : -1];\n"
                   "typedef char slice_record_is_72_bytes[sizeof(ft_slice_measure) == 72 ? 1 : -1];\n"
                   "double f(const ft_slices* s) {\n"
                   "    ft_contour_measure p[2]; ft_slice_measure w[2];\n"
                   "    int rc = ft_slices_measure(s, p, w) + ft_slices_measure(s, 0, w) + ft_slices_measure(s, p, 0);\n"
                   "    return rc + p[0].length + p[0].area + p[1].moment[1] + p[0].bbox_min[0] + p[0].bbox_max[1] + p[0].n_unmeasured + p[0].extent_exponent\n"
                   "           + w[0].length + w[0].area + w[1].moment[0] + w[0].bbox_min[1] + w[0].n_polylines + w[0].n_closed + w[0].n_outer + w[0].n_holes\n"
                   "           + w[0].n_unmeasured + w[0].extent_exponent;\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_header_states_the_rule_once():
    text = open(HEADER).read()
    m = re.search(r"/\* Contour measures:(?:(?!\*/).)*?\*/\s*typedef struct ft_contour_measure", text, flags=re.S)
    assert m and text.count("/* Contour measures:") == 1 and text.index("/* Measures:") < m.start()
    doc = " ".join(re.sub(r"\n \*", "\n", m.group(0)).split())
    for phrase in ("u = (a + 1) % 3 and v = (a + 2) % 3", "Nothing reads the coordinate along a, except the extent", "the closing segment (P_m-1, P_0)",
                   "iff its four in-plane coordinates are finite", "Zero-length segments are measured", "du = Q.u - P.u, dv = Q.v - P.v", "L_t = sqrt(du du + dv dv)",
                   "C_t = P.u Q.v - Q.u P.v", "M_t,u = C_t (P.u + Q.u)", "M_t,v = C_t (P.v + Q.v)", "B_L = E + 2", "B_C = 2E + 2", "B_M = 3E + 3", "s_K = 90 - B_K",
                   "area = S_C / 2.0", "moment[0] = S_M,u / 6.0 and moment[1] = S_M,v / 6.0", "the centroid is moment / area", "a closed hole area < 0",
                   "over the closed ones only", "n_outer counts the closed polylines with Q_C > 0", "n_holes those with Q_C < 0", "+inf / -inf box",
                   "Either output may be NULL, but not both, unless nothing would be written", "for a misaligned device pointer",
                   "for out_polylines identical to out_slices", "empty contours: FT_OK", "then FT_ERR_NO_DEVICE", "84 B per polyline", "100 B per slice"):
        assert phrase in doc, phrase


@pytest.fixture(scope="module")
def host_ctx_():
    dev = ft.Device(-1)
    yield dev._ctx
    dev.close()


def empty_slices(ctx, axis=0, counts=(4, 1, 3)):
    """an ft_slices of a host-only context: a lattice without cells in the planes of `axis`"""
    lat = _lib.Lattice(_lib.Vec3(0, 0, 0), _lib.Vec3(1, 1, 1), *counts)
    vals = np.zeros(int(np.prod(counts)), np.float32)
    out = C.c_void_p()
    assert L.ft_slice_values(ctx, C.byref(lat), ptr(vals), axis, 0.0, C.byref(out)) == OK and out.value
    return out


def test_refusals_in_order_and_empty_contours_on_a_host_only_context(host_ctx_):
    h = empty_slices(host_ctx_)                                                            # no polylines, four slices
    lines, per = np.full(7, 7.0), np.full(4 * 9 + 4, 7.0)
    try:
        assert L.ft_slices_measure(None, ptr(lines), ptr(per)) == INVALID and L.ft_slices_measure(None, None, None) == INVALID
        assert L.ft_slices_measure(h, None, None) == INVALID and "null" in _lib.last_error()      # four slice records would be written
        assert L.ft_slices_measure(h, ptr(per), ptr(per)) == INVALID and "same address" in _lib.last_error()
        assert (per == 7.0).all()
        # empty contours: FT_OK without a device; the slice records of zeros are still written, nothing else
        assert L.ft_slices_measure(h, ptr(lines), None) == OK and (lines == 7.0).all()
        assert L.ft_slices_measure(h, ptr(lines), ptr(per)) == OK and (lines == 7.0).all() and (per[36:] == 7.0).all()
        got = per[:36].view(rule.SLICE_RECORD)
        want = rule.measure(np.zeros((0, 3), np.float32), np.zeros((0, 4), np.int32), 0, 4)[1]
        assert rule.same_bytes(got, want) and got["bbox_min"].tolist() == [[np.inf, np.inf]] * 4 and got["bbox_max"].tolist() == [[-np.inf, -np.inf]] * 4
        assert got["length"].tolist() == [0] * 4 and got["n_polylines"].tolist() == [0] * 4 and got["extent_exponent"].tolist() == [0] * 4
        one = (_lib.SliceMeasure * 4)()
        assert L.ft_slices_measure(h, None, one) == OK and one[3].area == 0 and one[3].bbox_min[0] == np.inf
    finally:
        L.ft_slices_destroy(h)


def test_the_internal_entry_refuses_before_the_device(host_ctx_):
    ctx = host_ctx_
    poly = L.ft_ctx_measure_polylines
    poly.restype, poly.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
    grid, probe = L.ft_ctx_contour_measure_grid, L.ft_ctx_contour_measure_probe
    grid.restype, grid.argtypes, probe.restype, probe.argtypes = C.c_int, [C.c_void_p, C.c_int32], C.c_int, [C.c_void_p, C.c_int32]
    p = np.zeros((6, 3), np.float32)
    rec = np.array([[0, 3, 0, 1], [3, 3, 1, 0]], np.int32)
    lines, per = np.zeros(2, rule.RECORD), np.zeros(2, rule.SLICE_RECORD)
    call = lambda r, nP=6, nL=2, axis=2, nW=2, a=lines, b=per, c=ctx, pts=p: poly(c, ptr(pts), nP, ptr(r), nL, axis, nW, ptr(a), ptr(b))
    assert call(rec, c=None) == INVALID and call(rec, pts=None) == INVALID and poly(ctx, ptr(p), 6, None, 2, 2, 2, ptr(lines), ptr(per)) == INVALID
    for kw in (dict(nP=-1), dict(nL=-1), dict(nW=-1), dict(nP=2 ** 31), dict(nW=2 ** 31), dict(axis=-1), dict(axis=3), dict(a=None, b=None), dict(b=lines)):
        assert call(rec, **kw) == INVALID, kw
    for row, col, value in ((0, 0, -1), (1, 1, 4), (1, 1, -1), (0, 2, 2), (0, 2, -1), (1, 0, 2)):      # outside the points, outside the slices, overlapping
        bad = np.array(rec)
        bad[row, col] = value
        assert call(bad) == INVALID, (row, col, value)
    assert call(rec, nW=1) == INVALID                                                      # slice 1 of one slice
    assert call(rec) == NO_DEVICE and call(rec, a=None) == NO_DEVICE and call(rec, b=None) == NO_DEVICE
    assert call(rec, nL=0) == NO_DEVICE                                                    # points without polylines still have an extent
    # nothing at all: FT_OK without a device, zeroed slice records if asked for
    per[:] = rule.measure(p, rec, 2, 2)[1]
    assert poly(ctx, None, 0, None, 0, 1, 2, None, ptr(per)) == OK and per["n_polylines"].tolist() == [0, 0] and np.isinf(per["bbox_max"]).all()
    assert poly(ctx, None, 0, None, 0, 1, 0, None, None) == OK
    assert [grid(ctx, g) for g in (1, 2, 7, 1024, 0)] == [OK] * 5 and grid(ctx, -1) == INVALID and grid(None, 1) == INVALID
    assert [probe(ctx, e) for e in (1, 0)] == [OK, OK] and probe(ctx, 2) == INVALID and probe(None, 0) == INVALID


def test_python_surface_on_empty_contours():
    dev = ft.Device(-1)
    try:
        flat = np.zeros((3, 1, 4), np.float32)
        c = dev.slice_values(flat, (0, 0, 0), (1, 1, 1), axis=2, measures=True)
        assert c.polylines.shape == (0, 4) and c.slices == 4
        assert isinstance(c.measures, ft.ContourMeasures) and len(c.measures) == 0 and not c.measures.per_slice
        assert isinstance(c.layer_measures, ft.ContourMeasures) and len(c.layer_measures) == 4 and c.layer_measures.per_slice
        per = c.layer_measures
        assert per.area.tolist() == [0] * 4 and per.length.dtype == np.float64 and per.moment.shape == (4, 2) and per.bbox_min.dtype == np.float32
        assert per.n_outer.tolist() == [0] * 4 and per.n_holes.tolist() == [0] * 4 and per.n_polylines.dtype == np.int32 and per.extent_exponent == 0
        assert per.centroid.shape == (4, 2) and np.isnan(per.centroid).all() and c.measures.centroid.shape == (0, 2) and c.measures.area.shape == (0,)
        plain = dev.slice_values(flat, (0, 0, 0), (1, 1, 1), axis=2)
        assert plain.measures is None and plain.layer_measures is None                     # the default: today's result
        import inspect
        for fn in (ft.DeviceScene.slice_lattice, ft.Device.slice_values, ft.SdfForm.slice):
            assert inspect.signature(fn).parameters["measures"].default is False
    finally:
        dev.close()


def test_the_build_knows_the_new_translation_unit():
    csrc = os.path.join(ROOT, "fraytracer_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^contour_measure\.o: contour_measure\.hip ft_contour_measure\.h$", mk, flags=re.M)
    assert re.search(r"^\$\(OUT\):.*\bcontour_measure\.o\b", mk, flags=re.M) and re.search(r"^capi\.o:.*\bft_contour_measure\.h\b", mk, flags=re.M)
    assert mk.count("measure.hip contour_measure.hip scene.cpp") == 2                      # the profile and experiment builds
    import importlib.util
    spec = importlib.util.spec_from_file_location("source_hash", os.path.join(csrc, "source_hash.py"))
    sh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sh)
    assert "fraytracer_amd/csrc/contour_measure.hip" in sh.FILES and "fraytracer_amd/csrc/ft_contour_measure.h" in sh.FILES
    src = open(os.path.join(csrc, "contour_measure.hip")).read()
    assert "asm" not in re.sub(r"//[^\n]*", "", src) and "#pragma clang fp contract(off)" in src


def test_cpp_and_fsharp_mirrors(tmp_path):
    assert_cpp_compiles(tmp_path, "contour_measures.cpp",
                        "double f(const FrayTracer::SdfScene& scene, const ft_lattice& lat, ft_ctx* ctx, const std::vector<float>& values) {\n"
                        "    FrayTracer::Slice::Request r; r.measures = true; r.axis = 1;\n"
                        "    FrayTracer::Slice::Contours a = FrayTracer::Slice::ofLattice(scene, lat, r);\n"
                        "    FrayTracer::Slice::Contours b = FrayTracer::Slice::ofValues(ctx, lat, values, 2, 0.0f, true);\n"
                        "    const ft_contour_measure& p = a.measures.at(0); const ft_slice_measure& w = b.layerMeasures.at(0);\n"
                        "    return p.length + p.area + p.moment[1] + w.area + w.n_outer + w.n_holes + w.moment[0] / w.area;\n"
                        "}\n")
    fs = open(os.path.join(ROOT, "host", "fsharp", "FrayTracer.Hip.fs")).read()
    assert re.search(r"extern int ft_slices_measure\(nativeint \w+, nativeint \w+, nativeint \w+\)", fs)
    for name, fields in (("FtContourMeasure", 10), ("FtSliceMeasure", 14)):
        m = re.search(r"type\s+" + name + r"\s*=\s*\{(.*?)\}", fs, flags=re.S)
        assert m and len(re.findall(r"(\w+)\s*:\s*([\w.]+)", m.group(1))) == fields, name
