"""Shells (ft_mesh_shells, ft_shells_triangles, ft_shells_triangles_device, what reads them, ft_mesh_select): the parts that need no GPU — the ABI, the
header's statement of the rule, every refusal that comes before the device is asked for, the empty input, the build's bookkeeping, the C++ and F#
mirrors, the example, keep= parsing and the OBJ groups."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import _lib
from helpers import HEADER, ROOT, assert_cpp_compiles, assert_declared_exported_bound, dev_ptr as _p, host_ptr as ptr

import mesh_restatement as mesh_rule
import shells_restatement as rule

NAMES = ("ft_mesh_shells", "ft_shells_triangles", "ft_shells_triangles_device", "ft_shells_get_info", "ft_shells_device_buffers", "ft_shells_read",
         "ft_shells_destroy", "ft_mesh_select")
INVALID, UNSUPPORTED, NO_DEVICE, OK = _lib.FT_ERR_INVALID, _lib.FT_ERR_UNSUPPORTED, _lib.FT_ERR_NO_DEVICE, _lib.FT_OK
L = _lib.lib
LIMIT = 715827883                                                                          # 3 * LIMIT no longer fits int32


def test_symbols_are_declared_exported_and_bound():
    assert_declared_exported_bound(NAMES)
    assert C.sizeof(_lib.Shell) == 16 and C.sizeof(_lib.ShellsInfo) == 48
    assert L.ft_abi_version() == 5                                                         # additive: the ABI version stays
    assert ft.Shells is ft.api.Shells and "Shells" in ft.__all__
    for internal in ("ft_ctx_shells_tile", "ft_ctx_shells_last"):                          # not in the header, like ft_ctx_mesh_tile
        getattr(L, internal)
        assert internal not in open(HEADER).read()


def test_header_is_still_plain_c99(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER])
    src = tmp_path / "use.c"
    src.write_text('#include "fraytracer_hip.h"\n'
                   "typedef char record_is_16_bytes[sizeof(ft_shell) == 16 ? 1 : -1];\n"
                   "typedef char info_is_48_bytes[sizeof(ft_shells_info) == 48 ? 1 : -1];\n"
                   "int f(ft_ctx* c, const ft_mesh* m, const int32_t* t, void* d, const uint8_t* keep) {\n"
                   "    ft_shells* s = 0; ft_mesh* kept = 0; ft_shells_info i; void* b[3]; int32_t v[4]; ft_shell r[2];\n"
                   "    int rc = ft_mesh_shells(m, &s) + ft_shells_triangles(c, t, 2, 4, &s) + ft_shells_triangles_device(c, d, 2, 4, &s)\n"
                   "           + ft_shells_get_info(s, &i) + ft_shells_device_buffers(s, &b[0], &b[1], &b[2]) + ft_shells_read(s, v, v, r)\n"
                   "           + ft_mesh_select(m, s, keep, 2, &kept);\n"
                   "    ft_shells_destroy(s);\n"
                   "    ft_mesh_destroy(kept);\n"
                   "    return rc + r[0].first_vertex + r[0].n_vertices + r[0].n_triangles + r[0].n_border_edges + (int)i.n_unused_vertices;\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_header_states_the_rule_once():
    text = open(HEADER).read()
    m = re.search(r"/\* Shells:(?:(?!\*/).)*?\*/\s*typedef struct ft_shells ft_shells;", text, flags=re.S)
    assert m and text.count("/* Shells:") == 1
    doc = " ".join(re.sub(r"\n \*", "\n", m.group(0)).split())
    for phrase in ("never a float", "0 <= index < nV", "pairwise different", "a vertex named by at least one triangle", "Connectivity is by shared vertex",
                   "Zero-area triangles connect like any other", "ascending order of their smallest vertex index", "or -1 for an unused vertex",
                   "t0 -> t1, t1 -> t2, t2 -> t0", "iff no triangle has the side b -> a", "Each side is judged on its own",
                   "a side that occurs twice is not a border edge if its reverse occurs once", "closed iff n_border_edges == 0", "715827883",
                   "FT_ERR_UNSUPPORTED", "nT == 0 gives zero shells and every vertex unused", "no device needed", "keep[s] != 0",
                   "in their old relative order", "the rank among the kept", "n_skipped is copied from the source", "The remap is monotone",
                   "first_vertex remapped, in order", "No shell kept gives an empty mesh", "independent of the mesh once built",
                   "all made before the device is asked for, in this order", "validates its indices on the host before it uploads",
                   "at the constructor's first synchronisation", "no kernel indexes anything with an unchecked value", "On any failure *out is NULL",
                   "Shiloach and Vishkin", "floor(log_{3/2} nV) + 2", "never a partial labelling", "ceil(I / 4) + 1 times",
                   "one read of a 4-byte flag per batch of B = 4 iterations", "plus one for the totals", "36 B per vertex, 12 B per triangle",
                   "FT_ERR_NO_DEVICE", "accepts NULL for any part", "equal counts alone do not pass", "It synchronises ONCE, for its two totals",
                   "it outlives the source mesh and the shells"):
        assert phrase in doc, phrase
    assert "ft_shells.h" not in doc


@pytest.fixture(scope="module")
def host_ctx_():
    dev = ft.Device(-1)
    yield dev._ctx
    dev.close()


def empty_mesh(ctx, nz=1):
    """an ft_mesh of a host-only context: a lattice without cells"""
    lat = _lib.Lattice(_lib.Vec3(0, 0, 0), _lib.Vec3(1, 1, 1), 3, 3, nz)
    vals = np.zeros(9 * nz, np.float32)
    out = C.c_void_p()
    assert L.ft_mesh_values(ctx, C.byref(lat), ptr(vals), 0.0, C.byref(out)) == OK and out.value
    return out


def test_every_refusal_comes_before_the_device_is_asked_for(host_ctx_):
    ctx = host_ctx_
    tri = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
    out = C.c_void_p(0xDEAD)
    o = C.byref(out)

    def refused(rc, want):
        assert rc == want and out.value is None, (rc, want, out.value)                     # *out is NULL on any failure
        out.value = 0xDEAD

    # the arguments pass: only then is the device missed
    refused(L.ft_shells_triangles(ctx, ptr(tri), 2, 4, o), NO_DEVICE)
    refused(L.ft_shells_triangles(ctx, ptr(tri), 2, 2 ** 31 - 1, o), NO_DEVICE)
    refused(L.ft_shells_triangles_device(ctx, _p(4096), 2, 4, o), NO_DEVICE)
    refused(L.ft_shells_triangles_device(ctx, _p(4096), LIMIT - 1, 4, o), NO_DEVICE)       # the largest count
    # NULL where none is allowed
    refused(L.ft_shells_triangles(None, ptr(tri), 2, 4, o), INVALID)
    refused(L.ft_shells_triangles(ctx, None, 2, 4, o), INVALID)
    assert L.ft_shells_triangles(ctx, ptr(tri), 2, 4, None) == INVALID
    refused(L.ft_shells_triangles_device(None, _p(4096), 2, 4, o), INVALID)
    refused(L.ft_shells_triangles_device(ctx, None, 2, 4, o), INVALID)
    assert L.ft_shells_triangles_device(ctx, _p(4096), 2, 4, None) == INVALID
    refused(L.ft_mesh_shells(None, o), INVALID)
    # negative counts, n_vertices >= 2^31
    for nt, nv in ((-1, 4), (2, -1), (2, 2 ** 31), (2, 2 ** 40)):
        refused(L.ft_shells_triangles(ctx, ptr(tri), nt, nv, o), INVALID)
        refused(L.ft_shells_triangles_device(ctx, _p(4096), nt, nv, o), INVALID)
    # a misaligned device pointer
    for addr in (4097, 4098, 4099):
        refused(L.ft_shells_triangles_device(ctx, _p(addr), 2, 4, o), INVALID)
    # the triangle limit; invalid before unsupported
    for nt in (LIMIT, LIMIT + 1, 2 ** 40):
        refused(L.ft_shells_triangles_device(ctx, _p(4096), nt, 4, o), UNSUPPORTED)
        refused(L.ft_shells_triangles_device(ctx, _p(4097), nt, 4, o), INVALID)
        refused(L.ft_shells_triangles_device(ctx, _p(4096), nt, -4, o), INVALID)
    # the host form validates its indices itself: out of range, negative, twice in one triangle, triangles without vertices
    for bad, nv in (([[0, 1, 4]], 4), ([[0, -1, 2]], 4), ([[0, 1, 2], [3, 1, 3]], 4), ([[0, 1, 1]], 4), ([[2, 1, 2]], 4), ([[0, 1, 2]], 0)):
        refused(L.ft_shells_triangles(ctx, ptr(np.array(bad, np.int32)), len(bad), nv, o), INVALID)
    refused(L.ft_shells_triangles_device(ctx, _p(4096), 1, 0, o), INVALID)
    # readers: NULL
    info = _lib.ShellsInfo()
    assert L.ft_shells_get_info(None, C.byref(info)) == INVALID and L.ft_shells_read(None, None, None, None) == INVALID
    assert L.ft_shells_device_buffers(None, None, None, None) == INVALID
    L.ft_shells_destroy(None)                                                              # a no-op
    # ft_mesh_select
    mesh, other = empty_mesh(ctx), empty_mesh(ctx)
    sh, generic = C.c_void_p(), C.c_void_p()
    assert L.ft_mesh_shells(mesh, C.byref(sh)) == OK and L.ft_shells_triangles(ctx, None, 0, 0, C.byref(generic)) == OK
    keep = np.zeros(4, np.uint8)
    try:
        refused(L.ft_mesh_select(None, sh, ptr(keep), 0, o), INVALID)
        refused(L.ft_mesh_select(mesh, None, ptr(keep), 0, o), INVALID)
        refused(L.ft_mesh_select(mesh, sh, None, 1, o), INVALID)
        assert L.ft_mesh_select(mesh, sh, ptr(keep), 0, None) == INVALID
        refused(L.ft_mesh_select(other, sh, ptr(keep), 0, o), INVALID)                     # equal counts, another mesh
        refused(L.ft_mesh_select(mesh, generic, ptr(keep), 0, o), INVALID)                 # shells of a triangle list
        refused(L.ft_mesh_select(other, sh, ptr(keep), 1, o), INVALID)                     # the order: the wrong mesh before the wrong count
        for n in (1, -1, 4):
            refused(L.ft_mesh_select(mesh, sh, ptr(keep), n, o), INVALID)
        assert L.ft_mesh_select(mesh, sh, None, 0, o) == OK and out.value                  # nothing to keep: an empty mesh, no device needed
        info = _lib.MeshInfo()
        assert L.ft_mesh_get_info(out, C.byref(info)) == OK and (info.n_vertices, info.n_triangles, info.n_skipped) == (0, 0, 0)
        L.ft_mesh_destroy(out)
    finally:
        for h in (sh, generic):
            L.ft_shells_destroy(h)
        for h in (mesh, other):
            L.ft_mesh_destroy(h)


def test_an_empty_input_gives_empty_shells_without_a_device(host_ctx_):
    ctx = host_ctx_
    mesh = empty_mesh(ctx)
    handles = []
    for make in ("mesh", "host", "host null", "device"):
        out = C.c_void_p()
        if make == "mesh":
            rc, nv = L.ft_mesh_shells(mesh, C.byref(out)), 0
        elif make == "host":
            rc, nv = L.ft_shells_triangles(ctx, ptr(np.zeros((0, 3), np.int32)), 0, 7, C.byref(out)), 7
        elif make == "host null":
            rc, nv = L.ft_shells_triangles(ctx, None, 0, 5, C.byref(out)), 5
        else:
            rc, nv = L.ft_shells_triangles_device(ctx, _p(4096), 0, 3, C.byref(out)), 3
        assert rc == OK and out.value, make
        handles.append(out)
        info = _lib.ShellsInfo()
        assert L.ft_shells_get_info(out, C.byref(info)) == OK and L.ft_shells_get_info(out, None) == INVALID
        assert [getattr(info, k) for k, _ in info._fields_] == [nv, 0, 0, 0, nv, 0], make
        bufs = [C.c_void_p(1) for _ in range(3)]
        assert L.ft_shells_device_buffers(out, *map(C.byref, bufs)) == OK and [b.value for b in bufs] == [None] * 3
        labels = np.full(nv + 2, 7, np.int32)
        assert L.ft_shells_read(out, ptr(labels), None, None) == OK and labels.tolist() == [-1] * nv + [7, 7]      # every vertex unused; nothing beyond
        assert L.ft_shells_read(out, None, None, None) == OK
    for h in handles:
        L.ft_shells_destroy(h)
    L.ft_mesh_destroy(mesh)
    dev = ft.Device(-1)
    try:
        sh = dev.shells(np.zeros((0, 3), np.int32), 4)
        assert isinstance(sh, ft.Shells) and len(sh) == 0 and sh.vertex_shell.tolist() == [-1] * 4 and sh.vertex_shell.dtype == np.int32
        assert sh.triangle_shell.shape == (0,) and sh.records.shape == (0, 4) and sh.closed.shape == (0,) and sh.euler.shape == (0,)
        assert sh.info == {"n_vertices": 4, "n_triangles": 0, "n_shells": 0, "n_closed": 0, "n_unused_vertices": 4, "n_border_edges": 0}
        mesh = dev.mesh_values(np.zeros((1, 4, 4), np.float32), (0, 0, 0), (1, 1, 1), shells=True)
        assert mesh.triangles.shape == (0, 3) and len(mesh.shells) == 0
        for keep in (0, 3, "closed", np.zeros(0, bool), lambda s: s.closed):
            kept = dev.mesh_values(np.zeros((1, 4, 4), np.float32), (0, 0, 0), (1, 1, 1), keep=keep)
            assert kept.vertices.shape == (0, 3) and len(kept.shells) == 0
        assert dev.mesh_values(np.zeros((1, 4, 4), np.float32), (0, 0, 0), (1, 1, 1)).shells is None      # the default: today's result
        with pytest.raises(ValueError, match=r"\[nT, 3\]"):
            dev.shells(np.zeros((4, 2), np.int32), 4)
        with pytest.raises(ValueError, match="like"):
            dev.shells(np.zeros((0, 3), np.int32), 4, like=np.zeros(3))
        with pytest.raises(ft.FrayTracerError) as e:
            dev.shells(np.array([[0, 1, 2]], np.int32), 3)
        assert e.value.code == NO_DEVICE
        with pytest.raises(ft.FrayTracerError) as e:
            dev.shells(np.array([[0, 1, 3]], np.int32), 3)
        assert e.value.code == INVALID
    finally:
        dev.close()


def test_internal_switches(host_ctx_):
    ctx = host_ctx_
    fn = L.ft_ctx_shells_tile
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int32]
    assert [fn(ctx, t) for t in (128, 256, 1024, 512)] == [OK] * 4
    assert [fn(ctx, t) for t in (0, 64, 192, 2048, -256)] == [INVALID] * 5 and fn(None, 256) == INVALID
    last = L.ft_ctx_shells_last
    last.restype, last.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]
    two = (C.c_int64 * 2)(5, 5)
    assert last(ctx, two) == OK and list(two) == [0, 0] and last(None, two) == INVALID and last(ctx, None) == INVALID
    cap = L.ft_shells_iteration_cap                                                       # floor(log_{3/2} n) + 2, in integers
    cap.restype, cap.argtypes = C.c_uint, [C.c_uint64]
    for n in (1, 2, 3, 4, 5, 20002, 2 ** 31 - 1):
        k = 0
        while 3 ** (k + 1) <= n * 2 ** (k + 1):
            k += 1
        assert cap(n) == k + 2, n
    assert cap(20002) == 26 and cap(2 ** 31 - 1) == 54


def test_keep_parsing():
    records = np.array([[0, 3, 5, 0], [3, 3, 9, 2], [6, 3, 9, 0], [9, 3, 1, 0]], np.int32)
    sh = ft.Shells(np.zeros(12, np.int32), np.zeros(24, np.int32), records, {"n_shells": 4})
    parse = lambda keep: ft.api._keep_mask(sh, keep).tolist()
    assert sh.closed.tolist() == [True, False, True, True] and sh.euler.tolist() == [3 - 7 + 5, 3 - 14 + 9, 3 - 13 + 9, 3 - 1 + 1]
    assert parse(0) == [0, 0, 0, 0] and parse(1) == [0, 1, 0, 0] and parse(2) == [0, 1, 1, 0] and parse(3) == [1, 1, 1, 0] and parse(9) == [1, 1, 1, 1]
    assert parse("closed") == [1, 0, 1, 1]
    assert parse(np.array([True, False, False, True])) == [1, 0, 0, 1] and parse([False, True, False, False]) == [0, 1, 0, 0]
    assert parse(lambda s: s.records[:, 2] > 4) == [1, 1, 1, 0] and parse(lambda s: 1) == [0, 1, 0, 0]
    assert ft.api._keep_mask(sh, 2).dtype == np.uint8
    for bad in ("open", np.array([True, False]), np.array([1, 0, 0, 1]), -1, 1.5):
        with pytest.raises(ValueError, match="keep"):
            parse(bad)
    for k in range(6):
        assert parse(k) == rule.largest(records, k).astype(int).tolist()


def test_obj_groups_round_trip(tmp_path):
    d = np.full((2, 2, 5), 1.0, np.float32)
    d[0, 0, 0] = d[1, 1, 4] = -1.0                                                          # two caps in opposite corners
    m = mesh_rule.extract(d, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    want = rule.shells(m.triangles, len(m.vertices))
    assert want.info["n_shells"] == 2
    sh = ft.Shells(want.vertex_shell, want.triangle_shell, want.records, want.info)
    plain, grouped, default = tmp_path / "plain.obj", tmp_path / "grouped.obj", tmp_path / "default.obj"
    ft.Mesh(m.vertices, m.triangles).save_obj(str(plain))
    ft.Mesh(m.vertices, m.triangles, shells=sh).save_obj(str(default))
    assert plain.read_text() == default.read_text() and "\ng " not in plain.read_text()    # the default output is unchanged
    ft.Mesh(m.vertices, m.triangles).save_obj(str(grouped), groups=True)
    assert grouped.read_text() == plain.read_text()                                        # no shells: nothing to group by
    ft.Mesh(m.vertices, m.triangles, shells=sh).save_obj(str(grouped), groups=True)
    faces, group = {}, None
    for line in grouped.read_text().splitlines():
        w = line.split()
        if w[0] == "g":
            group = w[1]
            faces[group] = []
        elif w[0] == "f":
            faces[group].append([int(x) - 1 for x in w[1:]])
    assert list(faces) == ["shell_0", "shell_1"]
    for s in range(2):
        assert np.array_equal(np.array(faces[f"shell_{s}"], np.int32), m.triangles[want.triangle_shell == s])
    assert [l for l in grouped.read_text().splitlines() if l[0] in "v#"] == [l for l in plain.read_text().splitlines() if l[0] in "v#"]


def test_the_build_knows_the_new_translation_unit():
    csrc = os.path.join(ROOT, "fraytracer_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    rule_ = re.search(r"^shells\.o:(.*)$", mk, flags=re.M).group(1).split()
    inc = set(re.findall(r'^\s*#include\s+"([^"]+)"', open(os.path.join(csrc, "shells.hip")).read(), flags=re.M))
    assert inc == {"ft_shells.h"} and set(rule_) == {"shells.hip", "ft_shells.h"}
    assert not re.findall(r'^\s*#include\s+"([^"]+)"', open(os.path.join(csrc, "ft_shells.h")).read(), flags=re.M)
    assert "ft_shells.h" in re.search(r"^capi\.o:(.*)$", mk, flags=re.M).group(1).split()
    assert re.search(r"^\$\(OUT\):.*\bshells\.o\b", mk, flags=re.M)
    for target in ("profile", "experiment"):
        assert "shells.hip" in re.search(r"^%s:.*\n\t(.*)$" % target, mk, flags=re.M).group(1), target
    files = re.search(r"^FILES = \[(.*?)\]", open(os.path.join(csrc, "source_hash.py")).read(), flags=re.M | re.S).group(1)
    assert {"fraytracer_amd/csrc/shells.hip", "fraytracer_amd/csrc/ft_shells.h"} <= set(re.findall(r'"([^"]+)"', files))
    # the other device units do not know the shells, and the device side computes with no float
    for f in ("kernels.hip", "ft_kernels.h", "ft_device.h", "ft_math.h", "ft_libm.h", "mesh.hip", "ft_mesh.h", "slice.hip", "ft_slice.h", "refine.hip", "ft_refine.h"):
        assert "shells" not in open(os.path.join(csrc, f)).read().lower(), f
    code = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "shells.hip")).read() + open(os.path.join(csrc, "ft_shells.h")).read())
    assert not re.search(r"\b(float|double)\b", code)
    # the bound and its source are written down where the algorithm is
    head = open(os.path.join(csrc, "ft_shells.h")).read()
    assert "Shiloach" in head and "Journal of Algorithms 3" in head and "floor(log_{3/2} n) + 2" in head
    listing = open(os.path.join(ROOT, "profiles", "shells_kernel_resources.txt")).read()
    rows = re.findall(r"^(ft_shells_\w+(?:<\d+>)?)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)\s+threads\s+(\d+)", listing, flags=re.M)
    assert len(rows) >= 14 + 8 * 4
    for name, vgpr, _, _, scratch, threads in rows:
        assert int(scratch) == 0, name
        assert int(vgpr) * max(2, int(threads) // 256) <= 512, name                        # resident at two waves per SIMD (512 VGPRs per SIMD lane), or one whole workgroup where that is more


def test_cpp_mesh_mirror_compiles(tmp_path):
    assert_cpp_compiles(tmp_path, "shells.cpp",
                        "FrayTracer::Mesh::Triangles f(const FrayTracer::SdfScene& s) {\n"
                        "    FrayTracer::Mesh::Request r; r.shells = true; r.keepLargest = 2;\n"
                        "    ft_lattice l{{0.0f, 0.0f, 0.0f}, {0.1f, 0.1f, 0.1f}, 4, 5, 6};\n"
                        "    FrayTracer::Mesh::Triangles a = FrayTracer::Mesh::ofLattice(s, l, r);\n"
                        "    const ft_shell& first = a.shells.at(0);\n"
                        "    a.skipped += first.n_border_edges + a.vertexShell.at(0) + a.triangleShell.at(0) + (int)a.shellsInfo.n_closed;\n"
                        "    return a;\n"
                        "}\n")


def test_fsharp_binding_imports_the_shell_forms():
    fs = open(os.path.join(ROOT, "host", "fsharp", "FrayTracer.Hip.fs")).read()
    for name in NAMES:
        m = re.search(r"\[<DllImport\(Lib\)>\] extern (int|void) " + name + r"\(([^)]*)\)", fs)
        assert m, name
        for a in m.group(2).split(","):                                                    # every pointer is a plain nativeint: no new by-reference type
            assert a.strip().rsplit(" ", 1)[0] in ("nativeint", "int64"), (name, a)


def test_example_parses_and_documents_feature():
    path = os.path.join(ROOT, "examples", "mesh.py")
    text = open(path).read()
    compile(text, path, "exec")
    for flag in ("--shells", "--keep-largest", "--keep-closed"):
        assert flag in text, flag
    for doc, words in (("README.md", ("ft_mesh_shells", "ft_mesh_select")), ("DESIGN.md", ("Shells", "Shiloach")), ("INTEGRATION.md", ("ft_mesh_shells", "ft_mesh_select"))):
        body = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in body, (doc, w)
