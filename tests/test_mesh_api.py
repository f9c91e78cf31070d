"""Meshing (ft_mesh_lattice, ft_mesh_values, ft_mesh_values_device and what reads a mesh): the parts that need no GPU — the ABI, the header's
statement of the rule, every refusal that comes before the device is asked for, the empty mesh of a lattice without cells, the orientation table
against the integer geometry, the OBJ / STL writers, the build's bookkeeping, the C++ and F# mirrors."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import _lib
from fraytracer_amd import synthetic as syn
from helpers import HEADER, ROOT, assert_cpp_compiles, assert_declared_exported_bound, dev_ptr as _p, host_ptr as ptr

import mesh_restatement as rule

NAMES = ("ft_mesh_lattice", "ft_mesh_values_device", "ft_mesh_values", "ft_mesh_get_info", "ft_mesh_device_buffers", "ft_mesh_read", "ft_mesh_destroy")
INVALID, UNSUPPORTED, NO_DEVICE, OK = _lib.FT_ERR_INVALID, _lib.FT_ERR_UNSUPPORTED, _lib.FT_ERR_NO_DEVICE, _lib.FT_OK
L = _lib.lib


def test_symbols_are_declared_exported_and_bound():
    assert_declared_exported_bound(NAMES)
    assert C.sizeof(_lib.MeshInfo) == 32 and (_lib.FT_MESH_NORMAL, _lib.FT_MESH_MATERIAL) == (1, 2)
    assert L.ft_abi_version() == 5                                                         # additive: the ABI version stays


def test_header_is_still_plain_c99(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER])
    src = tmp_path / "use.c"
    src.write_text('#include "fraytracer_hip.h"\n'
                   "typedef char info_is_32_bytes[sizeof(ft_mesh_info) == 32 ? 1 : -1];\n"
                   "int f(ft_ctx* c, const ft_scene* s, const float* v, void* d, ft_vec3* p, int32_t* t) {\n"
                   "    ft_lattice l = {{0.0f, 0.0f, 0.0f}, {1.0f, 1.0f, 1.0f}, 2, 3, 4};\n"
                   "    ft_mesh* m = 0; ft_mesh_info i; void* b[4];\n"
                   "    int rc = ft_mesh_lattice(c, s, &l, 0.0f, 0.001f, FT_MESH_NORMAL | FT_MESH_MATERIAL, &m) + ft_mesh_values(c, &l, v, 0.5f, &m)\n"
                   "           + ft_mesh_values_device(c, &l, d, 0.0f, &m) + ft_mesh_get_info(m, &i) + ft_mesh_device_buffers(m, &b[0], &b[1], &b[2], &b[3])\n"
                   "           + ft_mesh_read(m, p, t, p, t);\n"
                   "    ft_mesh_destroy(m);\n"
                   "    return rc;\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_header_states_the_rule_once():
    text = open(HEADER).read()
    m = re.search(r"/\* Meshing:(?:(?!\*/).)*?\*/\s*#define FT_MESH_NORMAL", text, flags=re.S)
    assert m and text.count("/* Meshing:") == 1
    doc = " ".join(re.sub(r"\n \*", "\n", m.group(0)).split())
    for phrase in ("s[q] = d[q] - iso, one float32 subtraction", "inside iff s[q] < 0", "+0, -0 and NaN are not inside", "e = 4 * di + 2 * dj + dk - 1",
                   "owned by q", "both finite and exactly one end is inside", "never a fused multiply-add", "t = s[q] / (s[q] - s[q'])", "one true division",
                   "v = p(q) + t * (p(q') - p(q))", "from the owner towards the far end", "(i * ny + j) * nz + k, then by e", "lexicographic order",
                   "c3 = (i + 1, j + 1, k + 1)", "counted in n_skipped", "(a1 b1, a1 b2, a2 b2, a2 b1)", "never from floats",
                   "counter-clockwise seen from the outside", "smallest vertex index comes first", "(q0, q1, q2), then (q0, q2, q3)",
                   "then by tetrahedron", "in opposite directions", "zero-area triangles", "referenced by no triangle", "FT_ERR_UNSUPPORTED",
                   "never FT_FIELD_BOUNDED", "ft_sample_points_device", "synchronises the context's stream ONCE", "0xFFFF0000", "FT_ERR_NO_DEVICE",
                   "outlives its scene but not its context", "accepts NULL for any part"):
        assert phrase in doc, phrase


@pytest.fixture(scope="module")
def host_scene():
    """a scene on a host-only context: what a call on it returns other than FT_ERR_NO_DEVICE comes from a check made before any device work"""
    dev = ft.Device(-1)
    ds = dev.scene(syn.config3(n=8)[0])
    yield dev._ctx, ds._scene
    dev.close()


def lattice(nx=2, ny=3, nz=4):
    return _lib.Lattice(_lib.Vec3(0, 0, 0), _lib.Vec3(1, 1, 1), nx, ny, nz)


def test_every_refusal_comes_before_the_device_is_asked_for(host_scene):
    ctx, sc = host_scene
    vals = np.zeros(24, np.float32)
    lat = lattice()
    out = C.c_void_p(0xDEAD)
    o = C.byref(out)

    def refused(rc, want):
        assert rc == want and out.value is None, (rc, want, out.value)                     # *out is NULL on any failure
        out.value = 0xDEAD

    # the arguments pass: only then is the device missed
    refused(L.ft_mesh_lattice(ctx, sc, C.byref(lat), 0.0, 0.0, 0, o), NO_DEVICE)
    refused(L.ft_mesh_lattice(ctx, sc, C.byref(lat), 0.25, 0.001, 3, o), NO_DEVICE)
    refused(L.ft_mesh_values(ctx, C.byref(lat), ptr(vals), 0.0, o), NO_DEVICE)
    refused(L.ft_mesh_values_device(ctx, C.byref(lat), _p(4096), 0.0, o), NO_DEVICE)
    big = lattice(16777216, 2, 2)                                                          # the largest count
    refused(L.ft_mesh_values_device(ctx, C.byref(big), _p(4096), 0.0, o), NO_DEVICE)
    # NULL where none is allowed
    refused(L.ft_mesh_lattice(None, sc, C.byref(lat), 0.0, 0.0, 0, o), INVALID)
    refused(L.ft_mesh_lattice(ctx, None, C.byref(lat), 0.0, 0.0, 0, o), INVALID)
    refused(L.ft_mesh_lattice(ctx, sc, None, 0.0, 0.0, 0, o), INVALID)
    assert L.ft_mesh_lattice(ctx, sc, C.byref(lat), 0.0, 0.0, 0, None) == INVALID
    refused(L.ft_mesh_values(None, C.byref(lat), ptr(vals), 0.0, o), INVALID)
    refused(L.ft_mesh_values(ctx, None, ptr(vals), 0.0, o), INVALID)
    refused(L.ft_mesh_values(ctx, C.byref(lat), None, 0.0, o), INVALID)
    assert L.ft_mesh_values(ctx, C.byref(lat), ptr(vals), 0.0, None) == INVALID
    refused(L.ft_mesh_values_device(None, C.byref(lat), _p(4096), 0.0, o), INVALID)
    refused(L.ft_mesh_values_device(ctx, None, _p(4096), 0.0, o), INVALID)
    refused(L.ft_mesh_values_device(ctx, C.byref(lat), None, 0.0, o), INVALID)
    assert L.ft_mesh_values_device(ctx, C.byref(lat), _p(4096), 0.0, None) == INVALID
    # a count < 1 or > 2^24
    for bad in (lattice(0, 3, 4), lattice(2, -1, 4), lattice(2, 3, 0), lattice(16777217, 2, 2), lattice(2, 16777217, 2), lattice(2, 2, 16777217)):
        refused(L.ft_mesh_lattice(ctx, sc, C.byref(bad), 0.0, 0.0, 0, o), INVALID)
        refused(L.ft_mesh_values(ctx, C.byref(bad), ptr(vals), 0.0, o), INVALID)
        refused(L.ft_mesh_values_device(ctx, C.byref(bad), _p(4096), 0.0, o), INVALID)
    # unknown flag bits
    for flags in (4, 7, 0x80000000):
        refused(L.ft_mesh_lattice(ctx, sc, C.byref(lat), 0.0, 0.0, flags, o), INVALID)
    # a misaligned device pointer
    for addr in (4097, 4098, 4099):
        refused(L.ft_mesh_values_device(ctx, C.byref(lat), _p(addr), 0.0, o), INVALID)
    # too many points for one call; the last two are exactly 0xFFFF0000
    for huge in (lattice(65536, 65536, 2), lattice(16777216, 256, 2), lattice(16777216, 16777216, 16777216), lattice(2, 65536, 65536), lattice(65536, 32768, 2),
                 lattice(65535, 32768, 2), lattice(65536, 65535, 1)):
        refused(L.ft_mesh_lattice(ctx, sc, C.byref(huge), 0.0, 0.0, 0, o), UNSUPPORTED)
        refused(L.ft_mesh_values(ctx, C.byref(huge), ptr(vals), 0.0, o), UNSUPPORTED)
        refused(L.ft_mesh_values_device(ctx, C.byref(huge), _p(4096), 0.0, o), UNSUPPORTED)
    refused(L.ft_mesh_values_device(ctx, C.byref(lattice(65535, 32767, 2)), _p(4096), 0.0, o), NO_DEVICE)      # below it
    # the order: invalid before unsupported (a misaligned pointer on a lattice that is too large)
    refused(L.ft_mesh_values_device(ctx, C.byref(lattice(65536, 65536, 2)), _p(4097), 0.0, o), INVALID)
    # a scene of another context
    other = ft.Device(-1)
    try:
        foreign = other.scene(syn.config3(n=8)[0])._scene
        refused(L.ft_mesh_lattice(ctx, foreign, C.byref(lat), 0.0, 0.0, 0, o), INVALID)
    finally:
        other.close()
    # readers of a mesh: NULL
    info = _lib.MeshInfo()
    assert L.ft_mesh_get_info(None, C.byref(info)) == INVALID and L.ft_mesh_read(None, None, None, None, None) == INVALID
    assert L.ft_mesh_device_buffers(None, None, None, None, None) == INVALID
    L.ft_mesh_destroy(None)                                                                # a no-op


def test_a_lattice_without_cells_is_an_empty_mesh_without_a_device(host_scene):
    ctx, sc = host_scene
    vals = np.full(70, -1.0, np.float32)
    for lat, make in ((lattice(1, 1, 1), "values"), (lattice(1, 70, 1), "values"), (lattice(7, 1, 10), "device"), (lattice(5, 14, 1), "scene")):
        out = C.c_void_p()
        if make == "values":
            rc = L.ft_mesh_values(ctx, C.byref(lat), ptr(vals), 0.0, C.byref(out))
        elif make == "device":
            rc = L.ft_mesh_values_device(ctx, C.byref(lat), _p(4096), 0.0, C.byref(out))
        else:
            rc = L.ft_mesh_lattice(ctx, sc, C.byref(lat), 0.0, 0.001, _lib.FT_MESH_NORMAL, C.byref(out))
        assert rc == OK and out.value
        info = _lib.MeshInfo()
        assert L.ft_mesh_get_info(out, C.byref(info)) == OK and L.ft_mesh_get_info(out, None) == INVALID
        assert (info.n_vertices, info.n_triangles, info.n_skipped) == (0, 0, 0)
        assert (info.has_normal, info.has_material) == ((1, 0) if make == "scene" else (0, 0))
        bufs = [C.c_void_p(1) for _ in range(4)]
        assert L.ft_mesh_device_buffers(out, *map(C.byref, bufs)) == OK and [b.value for b in bufs] == [None] * 4
        assert L.ft_mesh_device_buffers(out, None, None, None, None) == OK
        assert L.ft_mesh_read(out, None, None, None, None) == OK
        if make != "scene":
            assert L.ft_mesh_read(out, None, None, ptr(vals), None) == INVALID                 # normals of a mesh built without them
        L.ft_mesh_destroy(out)
    dev = ft.Device(-1)
    try:
        mesh = dev.mesh_values(np.zeros((1, 4, 4), np.float32), (0, 0, 0), (1, 1, 1))
        assert mesh.vertices.shape == (0, 3) and mesh.triangles.shape == (0, 3) and mesh.triangles.dtype == np.int32 and mesh.skipped == 0
        assert mesh.normal is None and mesh.material is None
        with pytest.raises(ValueError, match=r"\[nx, ny, nz\]"):
            dev.mesh_values(np.zeros((4, 4), np.float32), (0, 0, 0), (1, 1, 1))
        with pytest.raises(ft.FrayTracerError) as e:
            dev.mesh_values(np.zeros((2, 2, 2), np.float32), (0, 0, 0), (1, 1, 1))
        assert e.value.code == NO_DEVICE
        ds = dev.scene(syn.config3(n=8)[0])
        with pytest.raises(ValueError, match="like"):
            ds.mesh_lattice((0, 0, 0), (1, 1, 1), (2, 2, 2), like=np.zeros(3))
        with pytest.raises(ValueError, match="counts"):
            ds.mesh_lattice((0, 0, 0), (1, 1, 1), (2, 0, 2))
        with pytest.raises(ft.FrayTracerError) as e:
            ds.mesh_lattice((0, 0, 0), (1, 1, 1), (2, 2, 2), normal_epsilon=0.01, material=True)
        assert e.value.code == NO_DEVICE
        assert callable(ft.SdfForm.mesh) and callable(ft.DeviceScene.mesh_lattice) and callable(ft.Device.mesh_values)
    finally:
        dev.close()


def test_internal_tile_switch_is_per_context(host_scene):
    ctx, _ = host_scene
    fn = L.ft_ctx_mesh_tile                                                                # internal: not in the header
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int32]
    assert [fn(ctx, t) for t in (128, 256, 1024, 512)] == [OK] * 4
    assert [fn(ctx, t) for t in (0, 64, 192, 2048, -256)] == [INVALID] * 5 and fn(None, 256) == INVALID


def test_orientation_table_is_the_integer_geometry():
    """the table the triangle kernel reads (built at compile time, mesh.hip) against the restatement's orientation, slot by slot: entry
    [tetrahedron][inside mask] = triangle count, then (owner corner code << 3 | e) per triangle corner, smallest slot first"""
    fn = L.ft_mesh_table                                                                   # internal: not in the header
    fn.restype = C.POINTER(C.c_uint64)
    table = fn()
    for tet, perm in enumerate(rule.PERMS):
        corners = rule.tetrahedron_corners(perm)
        code = [int(4 * c[0] + 2 * c[1] + c[2]) for c in corners]
        for mask in range(16):
            cyc = rule.oriented_cycle(corners, [bool(mask >> x & 1) for x in range(4)])
            word = int(table[tet * 16 + mask])
            if not cyc:
                assert word == 0, (tet, mask)
                continue
            slots = [(code[x] << 3) | ((code[y] - code[x]) - 1) for x, y in cyc]
            r = slots.index(min(slots))
            slots = slots[r:] + slots[:r]
            want = slots if len(slots) == 3 else [slots[0], slots[1], slots[2], slots[0], slots[2], slots[3]]
            assert word & 3 == len(want) // 3, (tet, mask)
            assert [(word >> (2 + 6 * i)) & 63 for i in range(len(want))] == want, (tet, mask)
            assert word >> (2 + 6 * len(want)) == 0


def small_mesh():
    d = np.array([[[-1.0, 0.5], [0.25, 1.0]], [[0.75, 1.0], [1.0, 2.0]]], np.float32)       # one inside corner: a small cap
    m = rule.extract(d, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    assert len(m.triangles) == 6
    return m


def test_obj_and_stl_round_trip(tmp_path):
    m = small_mesh()
    nrm = (m.vertices / np.linalg.norm(m.vertices, axis=1, keepdims=True)).astype(np.float32)
    for normal in (None, nrm):
        mesh = ft.Mesh(m.vertices, m.triangles, normal=normal)
        path = tmp_path / "m.obj"
        mesh.save_obj(str(path))
        v, vn, f = [], [], []
        for line in path.read_text().splitlines():
            w = line.split()
            if w[0] == "v":
                v.append([float(x) for x in w[1:]])
            elif w[0] == "vn":
                vn.append([float(x) for x in w[1:]])
            elif w[0] == "f":
                f.append([int(x.split("/")[0]) - 1 for x in w[1:]])
                if normal is not None:
                    assert all(x.split("//")[0] == x.split("//")[1] for x in w[1:])
        assert np.array_equal(np.array(v, np.float32).view(np.uint32), m.vertices.view(np.uint32))       # float32 round-trips through 9 digits
        assert np.array_equal(np.array(f, np.int32), m.triangles)
        assert (normal is None and not vn) or np.array_equal(np.array(vn, np.float32).view(np.uint32), nrm.view(np.uint32))
    path = tmp_path / "m.stl"
    ft.Mesh(m.vertices, m.triangles).save_stl(str(path))
    raw = path.read_bytes()
    n, = struct.unpack_from("<I", raw, 80)
    assert n == len(m.triangles) and len(raw) == 84 + 50 * n
    rec = np.frombuffer(raw, np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("attr", "<u2")]), offset=84)
    assert np.array_equal(rec["v"].view(np.uint32), m.vertices[m.triangles.astype(np.int64)].view(np.uint32))
    cross = np.cross(rec["v"][:, 1] - rec["v"][:, 0], rec["v"][:, 2] - rec["v"][:, 0])
    assert np.allclose(np.linalg.norm(rec["n"], axis=1), 1.0, atol=1e-6) and (np.einsum("ij,ij->i", rec["n"], cross) > 0).all()
    assert ft.Mesh(m.vertices, m.triangles, material=np.zeros(len(m.vertices), np.int32), materials={0: "x"}).descriptor(0) == "x"


def test_the_build_knows_the_new_translation_unit():
    csrc = os.path.join(ROOT, "fraytracer_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    rule_ = re.search(r"^mesh\.o:(.*)$", mk, flags=re.M).group(1).split()
    inc = set(re.findall(r'^\s*#include\s+"([^"]+)"', open(os.path.join(csrc, "mesh.hip")).read(), flags=re.M))
    assert inc == {"ft_mesh.h"} and set(rule_) == {"mesh.hip", "ft_mesh.h"}                 # every header it includes is listed
    assert not re.findall(r'^\s*#include\s+"([^"]+)"', open(os.path.join(csrc, "ft_mesh.h")).read(), flags=re.M)
    assert "ft_mesh.h" in re.search(r"^capi\.o:(.*)$", mk, flags=re.M).group(1).split()
    assert re.search(r"^\$\(OUT\):.*\bmesh\.o\b", mk, flags=re.M)
    for target in ("profile", "experiment"):
        assert "mesh.hip" in re.search(r"^%s:.*\n\t(.*)$" % target, mk, flags=re.M).group(1), target
    files = re.search(r"^FILES = \[(.*?)\]", open(os.path.join(csrc, "source_hash.py")).read(), flags=re.M | re.S).group(1)
    assert {"fraytracer_amd/csrc/mesh.hip", "fraytracer_amd/csrc/ft_mesh.h"} <= set(re.findall(r'"([^"]+)"', files))
    # kernels.hip and what it includes do not know the mesher
    for f in ("kernels.hip", "ft_kernels.h", "ft_device.h", "ft_math.h", "ft_libm.h"):
        assert "mesh" not in open(os.path.join(csrc, f)).read().lower(), f


def test_cpp_mesh_mirror_compiles(tmp_path):
    assert_cpp_compiles(tmp_path, "mesh.cpp",
                        "FrayTracer::Mesh::Triangles f(ft_ctx* ctx, const FrayTracer::SdfScene& s, const std::vector<float>& values) {\n"
                        "    FrayTracer::Mesh::Request r; r.iso = 0.125f; r.normal = true; r.normalEpsilon = 0.00125f; r.material = true;\n"
                        "    ft_lattice l{{0.0f, 0.0f, 0.0f}, {0.1f, 0.1f, 0.1f}, 4, 5, 6};\n"
                        "    FrayTracer::Mesh::Triangles a = FrayTracer::Mesh::ofLattice(s, l, r);\n"
                        "    FrayTracer::Mesh::Triangles b = FrayTracer::Mesh::ofValues(ctx, l, values, 0.5f);\n"
                        "    a.triangles.insert(a.triangles.end(), b.triangles.begin(), b.triangles.end());\n"
                        "    a.skipped += b.skipped;\n"
                        "    return a;\n"
                        "}\n")


def test_fsharp_binding_imports_the_mesh_forms():
    fs = open(os.path.join(ROOT, "host", "fsharp", "FrayTracer.Hip.fs")).read()
    for name in NAMES:
        assert re.search(r"\[<DllImport\(Lib\)>\] extern (int|void) " + name + r"\(", fs), name
    # the ft_mesh** out-parameter is a plain nativeint
    for name in ("ft_mesh_lattice", "ft_mesh_values_device", "ft_mesh_values"):
        assert re.search(r"extern int " + name + r"\([^)]*, nativeint mesh\)", fs), name
    m = re.search(r"type\s+FtMeshInfo\s*=\s*\{(.*?)\}", fs, flags=re.S)
    assert m and [(n, t) for n, t in re.findall(r"(\w+)\s*:\s*([\w.]+)", m.group(1))] == \
        [("NVertices", "int64"), ("NTriangles", "int64"), ("NSkipped", "int64"), ("HasNormal", "int"), ("HasMaterial", "int")]


def test_example_exists_and_parses():
    path = os.path.join(ROOT, "examples", "mesh.py")
    compile(open(path).read(), path, "exec")
