"""The measures' C ABI and Python surface without a GPU (ft_shells_measure, ft_mesh_measure): the record's layout, the refusals in their order on a
host-only context, empty input, shells of another mesh, the keep="bodies" mask, the header's rule text, the build's new translation unit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import _lib
from helpers import HEADER, ROOT, assert_cpp_compiles, assert_declared_exported_bound, dev_ptr as _p, host_ptr as ptr

import measure_restatement as rule

NAMES = ("ft_shells_measure", "ft_mesh_measure")
INTERNAL = ("ft_ctx_measure_triangles", "ft_ctx_measure_finish", "ft_ctx_measure_grid")
INVALID, NO_DEVICE, OK = _lib.FT_ERR_INVALID, _lib.FT_ERR_NO_DEVICE, _lib.FT_OK
L = _lib.lib
FIELDS = (("area", 0, 8), ("volume", 8, 8), ("moment", 16, 24), ("bbox_min", 40, 12), ("bbox_max", 52, 12), ("n_unmeasured", 64, 4), ("extent_exponent", 68, 4))


def test_symbols_are_declared_exported_and_bound():
    assert_declared_exported_bound(NAMES)
    assert L.ft_abi_version() == 5                                                         # additive: the ABI version stays
    assert ft.Measures is ft.api.Measures and "Measures" in ft.__all__
    for internal in INTERNAL:                                                              # not in the header, like ft_ctx_shells_tile
        getattr(L, internal)
        assert internal not in open(HEADER).read()


def test_record_layout_in_c_ctypes_and_numpy(tmp_path):
    """sizeof / offsetof of ft_shell_measure as a C compiler sees the header, against the ctypes twin, the numpy dtype and the restatement's"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fraytracer_hip.h"\n'
                   "int main(void) {\n"
                   '    printf("%zu", sizeof(ft_shell_measure));\n'
                   + "".join(f'    printf(" %zu %zu", offsetof(ft_shell_measure, {n}), sizeof(((ft_shell_measure*)0)->{n}));\n' for n, _, _ in FIELDS)
                   + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got[0] == 72 and list(zip(got[1::2], got[2::2])) == [(o, s) for _, o, s in FIELDS]
    assert C.sizeof(_lib.ShellMeasure) == 72
    dt = np.dtype(_lib.SHELL_MEASURE_DTYPE)
    assert dt.itemsize == 72 and rule.RECORD == dt
    for name, offset, size in FIELDS:
        f = getattr(_lib.ShellMeasure, name)
        assert (f.offset, f.size) == (offset, size), name
        assert (dt.fields[name][1], dt.fields[name][0].itemsize) == (offset, size), name


def test_header_states_the_rule_once():
    text = open(HEADER).read()
    m = re.search(r"/\* Measures:(?:(?!\*/).)*?\*/\s*typedef struct ft_shell_measure", text, flags=re.S)
    assert m and text.count("/* Measures:") == 1 and text.index("/* Shells:") < text.index("/* Measures:")      # behind "Shells"
    doc = " ".join(re.sub(r"\n \*", "\n", m.group(0)).split())
    for phrase in ("rounded ONCE to a multiple of a power of two", "added as integers, where order cannot matter", "used by a triangle or not",
                   "else ilogb(m) + 1", "denormals count by their true exponent", "-148 <= E <= 128", "all nine of its coordinates are finite",
                   "1 to its shell's n_unmeasured", "widened to float64 (exact)", "never fused, operands in the order written", "u = b - a, v = c - a",
                   "A_t = 0.5 * sqrt((n.x n.x + n.y n.y) + n.z n.z)", "sqrt correctly rounded",
                   "W_t = (a.x (b.y c.z - b.z c.y) + a.y (b.z c.x - b.x c.z)) + a.z (b.x c.y - b.y c.x)", "M_t,i = W_t * ((a_i + b_i) + c_i)",
                   "B_A = 2E + 3", "B_W = 3E + 3", "B_M = 4E + 5", "s_K = 90 - B_K", "round-half-to-even(term * 2^s_K)", "|q| <= 2^91",
                   "inside +-2^122", "a 128-bit two's-complement accumulator never overflows", "S_K = fl64(Q_K) * 2^(-s_K)", "rounds half to even",
                   "the scaling is exact", "volume = S_W / 6.0", "moment[i] = S_M,i / 24.0", "the centroid is moment / volume",
                   "a closed body has volume > 0 and a closed cavity volume < 0", "mean nothing geometric", "bits ^ 0x80000000", "~bits", "-0 < +0",
                   "one of the input bit patterns", "+inf / -inf", "72 B", "the same in every record of a call", "needs no device",
                   "the direction is taken from the address", "8-byte aligned", "synchronises the context's stream once", "the device form does not synchronise",
                   "all made before the device is asked for, in this order", "shells of a triangle list measure nothing", "FT_ERR_NO_DEVICE",
                   "A selected mesh (ft_mesh_select) measures like any other"):
        assert phrase in doc, phrase
    assert "ft_measure.h" not in doc


def test_header_is_still_plain_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "fraytracer_hip.h"\n'
                   "typedef char record_is_72_bytes[sizeof(ft_shell_measure) == 72 ? 1 : -1];\n"
                   "double f(const ft_mesh* m, const ft_shells* s) {\n"
                   "    ft_shell_measure r[2];\n"
                   "    int rc = ft_shells_measure(m, s, r) + ft_mesh_measure(m, r);\n"
                   "    return rc + r[0].area + r[0].volume + r[1].moment[2] + r[0].bbox_min[0] + r[0].bbox_max[2] + r[0].n_unmeasured + r[0].extent_exponent;\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


@pytest.fixture(scope="module")
def host_ctx_():
    dev = ft.Device(-1)
    yield dev._ctx
    dev.close()


def empty_mesh(ctx):
    """an ft_mesh of a host-only context: a lattice without cells"""
    lat = _lib.Lattice(_lib.Vec3(0, 0, 0), _lib.Vec3(1, 1, 1), 3, 3, 1)
    vals = np.zeros(9, np.float32)
    out = C.c_void_p()
    assert L.ft_mesh_values(ctx, C.byref(lat), ptr(vals), 0.0, C.byref(out)) == OK and out.value
    return out


def test_refusals_and_empty_input_on_a_host_only_context(host_ctx_):
    ctx = host_ctx_
    mesh, other = empty_mesh(ctx), empty_mesh(ctx)
    sh, generic, generic3 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.ft_mesh_shells(mesh, C.byref(sh)) == OK and L.ft_shells_triangles(ctx, None, 0, 0, C.byref(generic)) == OK
    assert L.ft_shells_triangles(ctx, None, 0, 3, C.byref(generic3)) == OK
    guard = np.full(40, 7.0)
    try:
        # NULL
        assert L.ft_shells_measure(None, sh, ptr(guard)) == INVALID and L.ft_shells_measure(mesh, None, ptr(guard)) == INVALID
        assert L.ft_mesh_measure(None, ptr(guard)) == INVALID
        assert L.ft_shells_measure(None, None, None) == INVALID
        # shells of another mesh (equal counts), shells of a triangle list: before anything about out, and before the device
        assert L.ft_shells_measure(other, sh, ptr(guard)) == INVALID and "not built from this mesh" in _lib.last_error()
        assert L.ft_shells_measure(mesh, generic, ptr(guard)) == INVALID and L.ft_shells_measure(mesh, generic3, ptr(guard)) == INVALID
        assert L.ft_shells_measure(other, sh, None) == INVALID
        # empty input: FT_OK, nothing written, no device needed; out may be NULL because nothing would be written
        assert L.ft_shells_measure(mesh, sh, ptr(guard)) == OK and L.ft_shells_measure(mesh, sh, None) == OK
        assert L.ft_mesh_measure(mesh, ptr(guard)) == OK and L.ft_mesh_measure(mesh, None) == OK
        assert L.ft_shells_measure(mesh, sh, _p(4097)) == OK                               # a host-only context takes every address for host memory
        assert (guard == 7.0).all()
    finally:
        for h in (sh, generic, generic3):
            L.ft_shells_destroy(h)
        for h in (mesh, other):
            L.ft_mesh_destroy(h)


def test_internal_entries_refuse_before_the_device(host_ctx_):
    ctx = host_ctx_
    tri = L.ft_ctx_measure_triangles
    tri.restype, tri.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    fin = L.ft_ctx_measure_finish
    fin.restype, fin.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
    grid = L.ft_ctx_measure_grid
    grid.restype, grid.argtypes = C.c_int, [C.c_void_p, C.c_int32]
    v, t, out = np.zeros((3, 3), np.float32), np.array([[0, 1, 2]], np.int32), np.zeros(1, rule.RECORD)
    assert tri(None, ptr(v), 3, ptr(t), 1, None, None, 1, ptr(out)) == INVALID
    assert tri(ctx, None, 3, ptr(t), 1, None, None, 1, ptr(out)) == INVALID and tri(ctx, ptr(v), 3, None, 1, None, None, 1, ptr(out)) == INVALID
    assert tri(ctx, ptr(v), 3, ptr(t), 1, None, None, 1, None) == INVALID
    for nv, nt, ns in ((-1, 1, 1), (3, -1, 1), (3, 1, -1), (2 ** 31, 1, 1), (3, 2 ** 31, 1)):
        assert tri(ctx, ptr(v), nv, ptr(t), nt, None, None, ns, ptr(out)) == INVALID
    assert tri(ctx, ptr(v), 3, ptr(t), 1, None, None, 0, None) == OK                       # zero shells: nothing written, no device
    assert tri(ctx, ptr(v), 3, ptr(t), 1, None, None, 1, ptr(out)) == NO_DEVICE
    sums, res = np.zeros(2, np.uint64), np.zeros(1)
    assert fin(None, ptr(sums), 1, 0, ptr(res)) == INVALID and fin(ctx, None, 1, 0, ptr(res)) == INVALID and fin(ctx, ptr(sums), 1, 0, None) == INVALID
    assert fin(ctx, ptr(sums), -1, 0, ptr(res)) == INVALID and fin(ctx, None, 0, 0, None) == OK and fin(ctx, ptr(sums), 1, 0, ptr(res)) == NO_DEVICE
    assert [grid(ctx, g) for g in (1, 2, 1024, 0)] == [OK] * 4 and grid(ctx, -1) == INVALID and grid(None, 1) == INVALID


def test_python_surface_on_an_empty_mesh():
    dev = ft.Device(-1)
    try:
        flat = np.zeros((1, 4, 4), np.float32)
        m = dev.mesh_values(flat, (0, 0, 0), (1, 1, 1), measures=True)                     # implies shells
        assert m.triangles.shape == (0, 3) and len(m.shells) == 0 and isinstance(m.shells.measures, ft.Measures) and len(m.shells.measures) == 0
        assert len(m.measure) == 0 and m.shells.measures.volume.shape == (0,) and m.shells.measures.moment.shape == (0, 3)
        assert m.shells.measures.centroid.shape == (0, 3) and m.shells.measures.bbox_min.dtype == np.float32
        for keep in ("bodies", "closed", lambda s: s.closed & (s.measures.volume > 0)):
            kept = dev.mesh_values(flat, (0, 0, 0), (1, 1, 1), keep=keep, measures=True)
            assert kept.vertices.shape == (0, 3) and len(kept.shells.measures) == 0
        assert dev.mesh_values(flat, (0, 0, 0), (1, 1, 1), keep="bodies").shells.measures is None      # kept by the volumes, not asked to carry them
        plain = dev.mesh_values(flat, (0, 0, 0), (1, 1, 1))
        assert plain.shells is None and plain.measure is None                              # the default: today's result
        assert dev.mesh_values(flat, (0, 0, 0), (1, 1, 1), shells=True).shells.measures is None
    finally:
        dev.close()


def test_keep_bodies_mask():
    """closed and of positive volume: shell 1 is open, shell 2 a cavity, shell 3 closed with volume 0"""
    records = np.array([[0, 3, 5, 0], [3, 3, 9, 2], [6, 3, 9, 0], [9, 3, 1, 0]], np.int32)
    rec = np.zeros(4, np.dtype(_lib.SHELL_MEASURE_DTYPE))
    rec["volume"] = [2.5, 7.0, -1.0, 0.0]
    rec["moment"] = [[5.0, 0.0, -2.5], [0, 0, 0], [1, 1, 1], [0, 0, 0]]
    sh = ft.Shells(np.zeros(12, np.int32), np.zeros(24, np.int32), records, {"n_shells": 4}, measures=ft.Measures(rec))
    parse = lambda keep: ft.api._keep_mask(sh, keep).tolist()
    assert parse("bodies") == [1, 0, 0, 0] and parse("closed") == [1, 0, 1, 1]
    assert parse(lambda s: s.closed & (s.measures.volume > 0)) == parse("bodies")
    assert parse(lambda s: s.measures.volume < 0) == [0, 0, 1, 0]
    assert sh.measures.centroid[0].tolist() == [2.0, 0.0, -1.0] and np.isnan(sh.measures.centroid[3]).all() and len(sh.measures) == 4
    bare = ft.Shells(np.zeros(12, np.int32), np.zeros(24, np.int32), records, {"n_shells": 4})
    assert bare.measures is None
    with pytest.raises(ValueError, match="keep"):
        ft.api._keep_mask(bare, "bodies")
    with pytest.raises(ValueError, match="keep"):
        parse("cavities")


def test_the_build_knows_the_new_translation_unit():
    csrc = os.path.join(ROOT, "fraytracer_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    rule_ = re.search(r"^measure\.o:(.*)$", mk, flags=re.M).group(1).split()
    inc = set(re.findall(r'^\s*#include\s+"([^"]+)"', open(os.path.join(csrc, "measure.hip")).read(), flags=re.M))
    assert inc == {"ft_measure.h"} and set(rule_) == {"measure.hip", "ft_measure.h"}
    assert not re.findall(r'^\s*#include\s+"([^"]+)"', open(os.path.join(csrc, "ft_measure.h")).read(), flags=re.M)
    assert "ft_measure.h" in re.search(r"^capi\.o:(.*)$", mk, flags=re.M).group(1).split()
    assert re.search(r"^\$\(OUT\):.*\bmeasure\.o\b", mk, flags=re.M)
    for target in ("profile", "experiment"):
        assert "measure.hip" in re.search(r"^%s:.*\n\t(.*)$" % target, mk, flags=re.M).group(1), target
    files = re.search(r"^FILES = \[(.*?)\]", open(os.path.join(csrc, "source_hash.py")).read(), flags=re.M | re.S).group(1)
    assert {"fraytracer_amd/csrc/measure.hip", "fraytracer_amd/csrc/ft_measure.h"} <= set(re.findall(r'"([^"]+)"', files))
    # the other device units do not know the measures
    for f in ("kernels.hip", "ft_kernels.h", "ft_device.h", "ft_math.h", "ft_libm.h", "mesh.hip", "ft_mesh.h", "slice.hip", "ft_slice.h", "refine.hip", "ft_refine.h",
              "shells.hip", "ft_shells.h"):
        assert "ft_measure" not in open(os.path.join(csrc, f)).read(), f
    listing = open(os.path.join(ROOT, "profiles", "measure_kernel_resources.txt")).read()
    rows = re.findall(r"^(ft_measure_\w+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)\s+threads\s+(\d+)", listing, flags=re.M)
    assert {r[0] for r in rows} == {"ft_measure_extent_kernel", "ft_measure_terms_kernel", "ft_measure_finish_kernel", "ft_measure_convert_kernel"}
    for name, vgpr, _, lds, scratch, threads in rows:
        assert int(scratch) == 0 and int(lds) == 0 and int(threads) == 256, name
        assert int(vgpr) <= 128, name                                                      # four waves per SIMD: a whole workgroup of 256 per SIMD pair and more


def test_mirrors_examples_and_documents_carry_the_feature(tmp_path):
    assert_cpp_compiles(tmp_path, "measure.cpp",
                        "double f(const FrayTracer::SdfScene& s) {\n"
                        "    FrayTracer::Mesh::Request r; r.measures = true; r.keepBodies = true;\n"
                        "    ft_lattice l{{0.0f, 0.0f, 0.0f}, {0.1f, 0.1f, 0.1f}, 4, 5, 6};\n"
                        "    FrayTracer::Mesh::Triangles a = FrayTracer::Mesh::ofLattice(s, l, r);\n"
                        "    const ft_shell_measure& first = a.shellMeasures.at(0);\n"
                        "    return first.area + first.volume + first.moment[0] + first.bbox_min[1] + a.measure.volume + a.measure.n_unmeasured;\n"
                        "}\n")
    fs = open(os.path.join(ROOT, "host", "fsharp", "FrayTracer.Hip.fs")).read()
    for name in NAMES:
        m = re.search(r"\[<DllImport\(Lib\)>\] extern (int|void) " + name + r"\(([^)]*)\)", fs)
        assert m, name
        for a in m.group(2).split(","):                                                    # every pointer is a plain nativeint: no new by-reference type
            assert a.strip().rsplit(" ", 1)[0] == "nativeint", (name, a)
    assert "ShellMeasure" in fs
    path = os.path.join(ROOT, "examples", "mesh.py")
    text = open(path).read()
    compile(text, path, "exec")
    for flag in ("--measure", "--keep-bodies"):
        assert flag in text, flag
    for doc, words in (("README.md", ("ft_shells_measure", "ft_mesh_measure")), ("DESIGN.md", ("Measures", "measure_kernel_resources.txt", "correctly rounded"))):
        body = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in body, (doc, w)
