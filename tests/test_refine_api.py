"""Refinement (ft_mesh_lattice_refined, ft_slice_lattice_refined, ft_refine_segments, ft_refine_segments_device): the parts that need no GPU — the
ABI, the header's statement of the rule, every refusal that comes before the device is asked for, what succeeds without a device, the build's
bookkeeping, the C++ and F# mirrors, the examples."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import _lib
from fraytracer_amd import synthetic as syn
from helpers import HEADER, ROOT, assert_cpp_compiles, assert_declared_exported_bound, dev_ptr as _p, host_ptr as ptr

NAMES = ("ft_mesh_lattice_refined", "ft_slice_lattice_refined", "ft_refine_segments", "ft_refine_segments_device")
INVALID, UNSUPPORTED, NO_DEVICE, OK = _lib.FT_ERR_INVALID, _lib.FT_ERR_UNSUPPORTED, _lib.FT_ERR_NO_DEVICE, _lib.FT_OK
L = _lib.lib
CSRC = os.path.join(ROOT, "fraytracer_amd", "csrc")


def test_symbols_are_declared_exported_and_bound():
    assert_declared_exported_bound(NAMES)
    assert L.ft_abi_version() == 5                                                         # additive: the ABI version stays
    assert callable(ft.SdfForm.crossings) and callable(ft.DeviceScene.refine_segments) and callable(ft.DeviceScene.refine_segments_device)
    import inspect
    for fn in (ft.DeviceScene.mesh_lattice, ft.DeviceScene.slice_lattice, ft.SdfForm.mesh, ft.SdfForm.slice):
        assert inspect.signature(fn).parameters["refine"].default is None
    sig = inspect.signature(ft.DeviceScene.refine_segments).parameters
    assert sig["iso"].default == 0.0 and sig["steps"].default == 8


def test_header_is_still_plain_c99(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER])
    src = tmp_path / "use.c"
    src.write_text('#include "fraytracer_hip.h"\n'
                   "int f(ft_ctx* c, const ft_scene* s, const ft_vec3* a, const ft_vec3* b, void* d, ft_vec3* p, int32_t* st) {\n"
                   "    ft_lattice lat = {{0.0f, 0.0f, 0.0f}, {1.0f, 1.0f, 1.0f}, 2, 3, 4};\n"
                   "    ft_mesh* m = 0; ft_slices* r = 0;\n"
                   "    int rc = ft_mesh_lattice_refined(c, s, &lat, 0.0f, 0.001f, FT_MESH_NORMAL, 8, &m)\n"
                   "           + ft_slice_lattice_refined(c, s, &lat, 2, 0.0f, 0.001f, FT_SLICE_MATERIAL, 8, &r)\n"
                   "           + ft_refine_segments(c, s, a, b, 4, 0.0f, 8, p, st) + ft_refine_segments_device(c, s, d, d, 4, 0.0f, 8, d, d);\n"
                   "    ft_mesh_destroy(m); ft_slices_destroy(r);\n"
                   "    return rc;\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_header_states_the_rule_once():
    text = open(HEADER).read()
    m = re.search(r"/\* Refinement:(?:(?!\*/).)*?\*/\s*int ft_mesh_lattice_refined", text, flags=re.S)
    assert m and text.count("/* Refinement:") == 1
    assert text.index("void ft_slices_destroy(ft_slices*);") < m.start()                   # after the slicer's declarations
    doc = " ".join(re.sub(r"\n \*", "\n", m.group(0)).split())
    for phrase in ("two points A, B (float32 x 3) with signed values sA, sB", "Both values are finite and exactly one of sA < 0, sB < 0 holds", "mesher's s < 0",
                   "Round, repeated R times", "M = (A + B) * 0.5f per coordinate: one float32 sum, rounded, then one product, rounded", "sM = D(M) - iso",
                   "the bits ft_eval_distance / ft_sample_points give for M", "one float32 subtraction", "If sM is not finite the bracket stays as it is",
                   "if (sM < 0) == (sA < 0) then (A, sA) = (M, sM), else (B, sB) = (M, sM)", "no other stopping rule", "a fixed point of this rule",
                   "t = sA / (sA - sB), v = A + t * (B - A)", "rounded one by one, never fused, always from A towards B",
                   "A = p(q), the owner, B = p(q'), sA = s[q] and sB = s[q']", "With R = 0", "bit-equal to the unrefined one", "refined once and shared",
                   "bit for bit the refined mesh vertex on the same edge", "n_skipped are those of the unrefined result, word for word",
                   "|D(v) - iso| <= L * 2^-R", "between the vertex emit and whatever reads the vertices", "taken at the refined positions",
                   "0 .. 32", "checked right after the flag bits", "They add no synchronisation", "the mesher still synchronises once, the slicer twice",
                   "1 + 2 R launches", "48 B per vertex", "no refined *_values forms", "finds A crossing, not the first one", "the point is three NaN",
                   "Either output may be NULL, but not both", "ft_sample_points / ft_sample_points_device", "n >= 0xFFFF0000", "n = 0: FT_OK, nothing launched",
                   "stages through the context's scratch", "52 B per segment"):
        assert phrase in doc, phrase
    # the "Meshing" and "Slicing" comments and the #define behind each are where they were
    assert re.search(r"/\* Meshing:(?:(?!\*/).)*?\*/\s*#define FT_MESH_NORMAL", text, flags=re.S)
    assert re.search(r"/\* Slicing:(?:(?!\*/).)*?\*/\s*#define FT_SLICE_NORMAL", text, flags=re.S)


@pytest.fixture(scope="module")
def host_scene():
    """a scene on a host-only context: what a call on it returns other than FT_ERR_NO_DEVICE comes from a check made before any device work"""
    dev = ft.Device(-1)
    ds = dev.scene(syn.config3(n=8)[0])
    yield dev._ctx, ds._scene
    dev.close()


def lattice(nx=2, ny=3, nz=4):
    return _lib.Lattice(_lib.Vec3(0, 0, 0), _lib.Vec3(1, 1, 1), nx, ny, nz)


def test_the_constructors_refuse_before_the_device_in_their_parents_order(host_scene):
    ctx, sc = host_scene
    lat = lattice()
    out = C.c_void_p(0xDEAD)
    o = C.byref(out)

    def refused(rc, want, word=None):
        assert rc == want and out.value is None, (rc, want, out.value)                     # *out is NULL on any failure
        assert word is None or word in L.ft_last_error(), (word, L.ft_last_error())
        out.value = 0xDEAD

    mesh = lambda c=ctx, s=sc, l=lat, flags=0, steps=8, out_=o: L.ft_mesh_lattice_refined(c, s, None if l is None else C.byref(l), 0.0, 0.001, flags, steps, out_)
    slc = lambda c=ctx, s=sc, l=lat, axis=2, flags=0, steps=8, out_=o: L.ft_slice_lattice_refined(c, s, None if l is None else C.byref(l), axis, 0.0, 0.001, flags, steps, out_)
    for steps in (0, 1, 8, 32):                                                            # the arguments pass: only then is the device missed
        refused(mesh(steps=steps), NO_DEVICE)
        refused(mesh(steps=steps, flags=3), NO_DEVICE)
        for axis in (0, 1, 2):
            refused(slc(steps=steps, axis=axis, flags=3), NO_DEVICE)
    for fn in (mesh, slc):
        refused(fn(c=None), INVALID)
        refused(fn(s=None), INVALID)
        refused(fn(l=None), INVALID)
        assert fn(out_=None) == INVALID
        for bad in (lattice(0, 3, 4), lattice(2, 3, 16777217)):
            refused(fn(l=bad), INVALID, b"count")
        for flags in (4, 0x80000000):
            refused(fn(flags=flags), INVALID, b"flag")
        for steps in (-1, 33, -2 ** 31, 2 ** 31 - 1):
            refused(fn(steps=steps), INVALID, b"refine_steps")
        for huge in (lattice(65536, 65536, 2), lattice(65536, 32768, 2)):
            refused(fn(l=huge), UNSUPPORTED)
        # the order: counts, (axis,) flag bits, refine_steps, then unsupported
        refused(fn(l=lattice(0, 3, 4), flags=4, steps=40), INVALID, b"count")
        refused(fn(flags=4, steps=40), INVALID, b"flag")
        refused(fn(l=lattice(65536, 65536, 2), steps=40), INVALID, b"refine_steps")
    refused(slc(axis=3, flags=4, steps=40), INVALID, b"axis")
    refused(slc(l=lattice(0, 3, 4), axis=3), INVALID, b"count")
    other = ft.Device(-1)
    try:
        foreign = other.scene(syn.config3(n=8)[0])._scene
        refused(mesh(s=foreign), INVALID)
        refused(slc(s=foreign), INVALID)
    finally:
        other.close()


def test_the_segment_forms_refuse_before_the_device_in_the_stated_order(host_scene):
    ctx, sc = host_scene
    a, b = np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32)
    pts, st = np.zeros((4, 3), np.float32), np.zeros(4, np.int32)
    host = lambda c=ctx, s=sc, a_=ptr(a), b_=ptr(b), n=4, steps=8, p=ptr(pts), q=ptr(st): L.ft_refine_segments(c, s, a_, b_, n, 0.0, steps, p, q)
    dev = lambda c=ctx, s=sc, a_=_p(4096), b_=_p(8192), n=4, steps=8, p=_p(12288), q=_p(16384): L.ft_refine_segments_device(c, s, a_, b_, n, 0.0, steps, p, q)

    def said(rc, want, word=None):
        assert rc == want, (rc, want)
        assert word is None or word in L.ft_last_error(), (word, L.ft_last_error())

    for fn in (host, dev):
        for steps in (0, 1, 32):
            said(fn(steps=steps), NO_DEVICE)
        said(fn(p=None), NO_DEVICE)                                                        # either output may be NULL ...
        said(fn(q=None), NO_DEVICE)
        said(fn(p=None, q=None), INVALID, b"no output")                                    # ... but not both
        said(fn(c=None), INVALID)
        said(fn(s=None), INVALID)
        said(fn(a_=None), INVALID, b"null segment ends")
        said(fn(b_=None), INVALID, b"null segment ends")
        said(fn(n=-1), INVALID, b"negative count")
        for steps in (-1, 33, 2 ** 31 - 1):
            said(fn(steps=steps), INVALID, b"steps")
        for n in (0xFFFF0000, 2 ** 40):
            said(fn(n=n), UNSUPPORTED)
        said(fn(n=0), OK)                                                                  # nothing to do: no device needed
        said(fn(n=0xFFFF0000 - 1), NO_DEVICE)
        # the order: no output, steps, the ends, (alignment, identical pointers,) unsupported, n = 0
        said(fn(p=None, q=None, steps=40, a_=None), INVALID, b"no output")
        said(fn(steps=40, a_=None, n=2 ** 40), INVALID, b"steps")
        said(fn(a_=None, n=2 ** 40), INVALID, b"null segment ends")
        said(fn(n=0, steps=33), INVALID, b"steps")
    # identical pointers
    said(host(p=ptr(a)), INVALID, b"overlap")
    said(host(p=ptr(b)), INVALID, b"overlap")
    said(host(q=ptr(a)), INVALID, b"overlap")
    said(dev(p=_p(4096)), INVALID, b"overlap")
    said(dev(q=_p(8192)), INVALID, b"overlap")
    said(dev(p=_p(12288), q=_p(12288)), INVALID, b"overlap")
    said(dev(b_=_p(4096)), NO_DEVICE)                                                      # a == b is a segment of length 0, not an overlap
    # a misaligned device buffer, before the overlap and the count
    for k in range(4):
        for off in (1, 2, 3):
            addr = [4096, 8192, 12288, 16384]
            addr[k] += off
            said(dev(a_=_p(addr[0]), b_=_p(addr[1]), p=_p(addr[2]), q=_p(addr[3])), INVALID, b"aligned")
    said(dev(a_=_p(4097), p=_p(4097), n=2 ** 40), INVALID, b"aligned")
    said(dev(p=_p(4096), n=2 ** 40), INVALID, b"overlap")
    other = ft.Device(-1)
    try:
        foreign = other.scene(syn.config3(n=8)[0])._scene
        said(host(s=foreign), INVALID)
        said(dev(s=foreign), INVALID)
    finally:
        other.close()


def test_what_needs_no_device(host_scene):
    ctx, sc = host_scene
    # a lattice without cells: an empty result, whatever the rounds
    for lat in (lattice(1, 1, 1), lattice(1, 70, 1), lattice(7, 1, 10)):
        out = C.c_void_p()
        assert L.ft_mesh_lattice_refined(ctx, sc, C.byref(lat), 0.0, 0.001, 3, 8, C.byref(out)) == OK and out.value
        info = _lib.MeshInfo()
        assert L.ft_mesh_get_info(out, C.byref(info)) == OK
        assert (info.n_vertices, info.n_triangles, info.n_skipped, info.has_normal, info.has_material) == (0, 0, 0, 1, 1)
        L.ft_mesh_destroy(out)
    for lat, axis in ((lattice(1, 1, 1), 0), (lattice(7, 1, 10), 2), (lattice(5, 14, 1), 1)):
        out = C.c_void_p()
        assert L.ft_slice_lattice_refined(ctx, sc, C.byref(lat), axis, 0.0, 0.001, 1, 8, C.byref(out)) == OK and out.value
        info = _lib.SlicesInfo()
        assert L.ft_slices_get_info(out, C.byref(info)) == OK
        assert (info.n_points, info.n_polylines, info.axis, info.has_normal, info.has_material) == (0, 0, axis, 1, 0)
        L.ft_slices_destroy(out)
    dev = ft.Device(-1)
    try:
        ds = dev.scene(syn.config3(n=8)[0])
        m = ds.mesh_lattice((0, 0, 0), (1, 1, 1), (4, 1, 4), refine=8)
        assert m.vertices.shape == (0, 3) and m.triangles.shape == (0, 3)
        c = ds.slice_lattice((0, 0, 0), (1, 1, 1), (4, 1, 4), axis=0, refine=0)
        assert c.points.shape == (0, 3) and c.polylines.shape == (0, 4)
        points, status = ds.refine_segments(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
        assert points.shape == (0, 3) and points.dtype == np.float32 and status.shape == (0,) and status.dtype == np.int32
        points, status = ds.refine_segments(np.zeros((2, 0, 3), np.float32), np.zeros((2, 0, 3), np.float32), iso=0.5, steps=0)
        assert points.shape == (2, 0, 3) and status.shape == (2, 0)
        for call in (lambda: ds.mesh_lattice((0, 0, 0), (1, 1, 1), (2, 2, 2), refine=0), lambda: ds.slice_lattice((0, 0, 0), (1, 1, 1), (2, 2, 2), refine=4),
                     lambda: ds.refine_segments([[0, 0, 0]], [[1, 1, 1]])):
            with pytest.raises(ft.FrayTracerError) as e:
                call()
            assert e.value.code == NO_DEVICE
        for call in (lambda: ds.mesh_lattice((0, 0, 0), (1, 1, 1), (2, 2, 2), refine=33), lambda: ds.slice_lattice((0, 0, 0), (1, 1, 1), (2, 2, 2), refine=-1),
                     lambda: ds.refine_segments([[0, 0, 0]], [[1, 1, 1]], steps=40)):
            with pytest.raises(ft.FrayTracerError) as e:
                call()
            assert e.value.code == INVALID
        with pytest.raises(ValueError, match="same"):
            ds.refine_segments(np.zeros((3, 3)), np.zeros((4, 3)))
        with pytest.raises(ValueError, match=r"\[..., 3\]"):
            ds.refine_segments(np.zeros((3, 2)), np.zeros((3, 2)))
        form = syn.config3(n=8)[0].Object.kids[1]
        points, status = ft.SdfForm.crossings(form, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), 0.0, 8, device=dev)
        assert points.shape == (0, 3) and status.shape == (0,)
    finally:
        dev.close()


def test_internal_entry_points_are_not_in_the_header(host_scene):
    ctx, _ = host_scene
    text = open(HEADER).read()
    rnd = L.ft_ctx_refine_round                                                            # internal: one round on caller-given brackets (tests/test_gpu_refine.py)
    rnd.restype, rnd.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_int32, C.c_void_p]
    assert rnd(ctx, _p(4096), 4, _p(8192), _p(12288), 4, 0.0, 0, None) == NO_DEVICE and rnd(None, _p(4096), 4, _p(8192), _p(12288), 4, 0.0, 0, None) == INVALID
    probe = L.ft_ctx_refine_probe                                                          # internal (tools/refine_probe.py)
    probe.restype, probe.argtypes = C.c_int, [C.c_void_p, C.c_int32]
    assert [probe(ctx, v) for v in (1, 0)] == [OK, OK] and [probe(ctx, v) for v in (-1, 2)] == [INVALID, INVALID] and probe(None, 0) == INVALID
    assert "ft_ctx_refine_round" not in text and "ft_ctx_refine_probe" not in text


def test_the_build_knows_the_new_translation_unit():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule_ = re.search(r"^refine\.o:(.*)$", mk, flags=re.M).group(1).split()
    inc = set(re.findall(r'^\s*#include\s+"([^"]+)"', open(os.path.join(CSRC, "refine.hip")).read(), flags=re.M))
    assert inc == {"ft_refine.h"} and set(rule_) == {"refine.hip", "ft_refine.h"}          # every header it includes is listed
    assert not re.findall(r'^\s*#include\s+"([^"]+)"', open(os.path.join(CSRC, "ft_refine.h")).read(), flags=re.M)
    assert "ft_refine.h" in re.search(r"^capi\.o:(.*)$", mk, flags=re.M).group(1).split()
    assert re.search(r"^\$\(OUT\):.*\brefine\.o\b", mk, flags=re.M)
    for target in ("profile", "experiment"):
        assert "refine.hip" in re.search(r"^%s:.*\n\t(.*)$" % target, mk, flags=re.M).group(1), target
    files = re.search(r"^FILES = \[(.*?)\]", open(os.path.join(CSRC, "source_hash.py")).read(), flags=re.M | re.S).group(1)
    assert {"fraytracer_amd/csrc/refine.hip", "fraytracer_amd/csrc/ft_refine.h"} <= set(re.findall(r'"([^"]+)"', files))
    # the older units and what they include do not know the refinement
    for f in ("kernels.hip", "ft_kernels.h", "ft_device.h", "ft_math.h", "ft_libm.h", "mesh.hip", "ft_mesh.h", "slice.hip", "ft_slice.h"):
        assert not re.search(r"ft_refine|refine\.hip|refinement", open(os.path.join(CSRC, f)).read(), flags=re.I), f
    # no atomics: the order is the rule's; and the unit evaluates no distance of its own
    src = open(os.path.join(CSRC, "refine.hip")).read()
    assert "atomic" not in src.replace("no atomics", "")
    assert os.path.exists(os.path.join(ROOT, "profiles", "refine_kernel_resources.txt"))


def test_the_edge_tables_are_the_headers_directions():
    """ft_refine.h's corner codes per mask bit against the header's e: the mesher's seven, and per slice axis e 0, 1, 2 / 0, 3, 4 / 1, 3, 5"""
    text = open(os.path.join(CSRC, "ft_refine.h")).read()
    mesh = int(re.search(r"#define FT_REFINE_EDGES_MESH (0x[0-9a-f]+)u", text).group(1), 16)
    assert [(mesh >> (3 * b)) & 7 for b in range(8)] == [1, 2, 3, 4, 5, 6, 7, 0]
    words = [int(w, 16) for w in re.findall(r"0x[0-9a-f]+", re.search(r"#define FT_REFINE_EDGES_SLICE \{(.*?)\}", text).group(1))]
    assert [[((w >> (3 * b)) & 7) - 1 for b in range(3)] for w in words] == [[0, 1, 2], [0, 3, 4], [1, 3, 5]] and all(w >> 9 == 0 for w in words)


def test_cpp_mirror_compiles(tmp_path):
    assert_cpp_compiles(tmp_path, "refine.cpp",
                        "int f(const FrayTracer::SdfScene& s, const std::vector<ft_vec3>& a, const std::vector<ft_vec3>& b) {\n"
                        "    FrayTracer::Mesh::Request m; m.refineSteps = 8; m.normal = true; m.normalEpsilon = 0.00125f;\n"
                        "    FrayTracer::Slice::Request r; r.axis = 1; r.refineSteps = 4;\n"
                        "    static_assert(FrayTracer::Mesh::Request{}.refineSteps == -1 && FrayTracer::Slice::Request{}.refineSteps == -1, \"unrefined by default\");\n"
                        "    ft_lattice l{{0.0f, 0.0f, 0.0f}, {0.1f, 0.1f, 0.1f}, 4, 5, 6};\n"
                        "    FrayTracer::Mesh::Triangles t = FrayTracer::Mesh::ofLattice(s, l, m);\n"
                        "    FrayTracer::Slice::Contours c = FrayTracer::Slice::ofLattice(s, l, r);\n"
                        "    FrayTracer::Field::Crossings x = FrayTracer::Field::refineSegments(s, a, b, 0.25f, 12);\n"
                        "    return (int)(t.vertices.size() + c.points.size() + x.points.size()) + x.status[0];\n"
                        "}\n")


def test_fsharp_binding_imports_the_four_names():
    fs = open(os.path.join(ROOT, "host", "fsharp", "FrayTracer.Hip.fs")).read()
    for name in NAMES:
        assert re.search(r"\[<DllImport\(Lib\)>\] extern int " + name + r"\(", fs), name
    assert re.search(r"extern int ft_mesh_lattice_refined\([^)]*uint32 flags, int refineSteps, nativeint mesh\)", fs)
    assert re.search(r"extern int ft_slice_lattice_refined\([^)]*int axis, float32 iso[^)]*uint32 flags, int refineSteps, nativeint slices\)", fs)
    for name in ("ft_refine_segments", "ft_refine_segments_device"):
        assert re.search(r"extern int " + name + r"\([^)]*int64 n, float32 iso, int steps, nativeint \w+, nativeint \w+\)", fs), name


def test_examples_parse_and_know_the_option():
    for name in ("mesh.py", "slice.py"):
        path = os.path.join(ROOT, "examples", name)
        text = open(path).read()
        compile(text, path, "exec")
        assert '"--refine"' in text and "refine=args.refine" in text
