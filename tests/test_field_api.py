"""Sampling the distance field on the device (ft_sample_points, ft_sample_lattice and their *_device forms): the parts that need no GPU — the
ABI, the header's statement of the definition, every refusal that comes before the device is asked for, the duck-typed device-tensor check,
the point formula of lattice_points, the C++ and F# mirrors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import _lib, api
from fraytracer_amd import synthetic as syn
from helpers import HEADER, ROOT, assert_cpp_compiles, assert_declared_exported_bound, dev_ptr as _p, host_ptr as ptr

NAMES = ("ft_sample_points", "ft_sample_points_device", "ft_sample_lattice", "ft_sample_lattice_device")
INVALID, UNSUPPORTED, NO_DEVICE, OK = _lib.FT_ERR_INVALID, _lib.FT_ERR_UNSUPPORTED, _lib.FT_ERR_NO_DEVICE, _lib.FT_OK


def test_symbols_are_declared_exported_and_bound():
    assert_declared_exported_bound(NAMES)
    assert C.sizeof(_lib.Lattice) == 36 and _lib.FT_FIELD_BOUNDED == 1
    assert _lib.lib.ft_abi_version() == 5                                                  # additive: the ABI version stays


def test_header_is_still_plain_c99(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER])
    src = tmp_path / "use.c"
    src.write_text('#include "fraytracer_hip.h"\n'
                   "typedef char lattice_is_36_bytes[sizeof(ft_lattice) == 36 ? 1 : -1];\n"
                   "int f(ft_ctx* c, const ft_scene* s, const ft_vec3* p, void* d, float* dist, ft_vec3* nrm, int32_t* m) {\n"
                   "    ft_lattice l = {{0.0f, 0.0f, 0.0f}, {1.0f, 1.0f, 1.0f}, 2, 3, 4};\n"
                   "    return ft_sample_points(c, s, p, 1, 0.0f, FT_FIELD_BOUNDED, dist, nrm, m) + ft_sample_points_device(c, s, d, 1, 0.0f, 0u, d, d, d)\n"
                   "         + ft_sample_lattice(c, s, &l, 0.0f, 0u, dist, nrm, m) + ft_sample_lattice_device(c, s, &l, 0.0f, 0u, d, d, d);\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_header_states_the_definition():
    text = open(HEADER).read()
    m = re.search(r"/\*(?:(?!\*/).)*?\*/\s*typedef struct ft_lattice", text, flags=re.S)
    assert m
    doc = " ".join(re.sub(r"\n \*", "\n", m.group(0)).split())                             # the comment as running text, without its line prefixes
    for phrase in ("origin.x + (float)i * step.x", "one float32 product, rounded, then one float32 sum, rounded", "never a fused multiply-add",
                   "(i * ny + j) * nz + k", "k is contiguous", "1 .. 16777216",
                   "dx = D(p.x + e, p.y, p.z), dy = D(p.x, p.y + e, p.z), dz = D(p.x, p.y, p.z + e), d = D(p)",
                   "sqrt((g.x * g.x + g.y * g.y) + g.z * g.z)", "three true divisions", "the same bits with or without the normal",
                   "FT_FIELD_BOUNDED", "(dx * dx + dy * dy) + dz * dz < Radius * Radius", "the material is -1",
                   "Any output may be NULL, but not all three", "0xFFFF0000", "ft_eval_distance", "FT_ERR_NO_DEVICE"):
        assert phrase in doc, phrase
    m = re.search(r"/\*(?:(?!\*/).)*?\*/\s*int ft_sample_points_device\(", text, flags=re.S)
    assert m and "4-byte aligned" in m.group(0) and "NOT synchronised" in m.group(0) and "only identical pointers are detected" in m.group(0)


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
    L = _lib.lib
    pts, d, nrm, m = np.zeros((4, 3), np.float32), np.empty(4, np.float32), np.empty((4, 3), np.float32), np.empty(4, np.int32)
    lat = lattice()
    # the arguments pass: only then is the device missed
    assert L.ft_sample_points(ctx, sc, ptr(pts), 4, 0.0, 0, ptr(d), ptr(nrm), ptr(m)) == NO_DEVICE
    assert L.ft_sample_points(ctx, sc, ptr(pts), 4, 0.0, 1, None, None, ptr(m)) == NO_DEVICE
    assert L.ft_sample_points_device(ctx, sc, _p(4096), 4, 0.0, 0, _p(8192), None, None) == NO_DEVICE
    assert L.ft_sample_lattice(ctx, sc, C.byref(lat), 0.0, 1, ptr(np.empty(24, np.float32)), None, None) == NO_DEVICE
    assert L.ft_sample_lattice_device(ctx, sc, C.byref(lat), 0.0, 0, None, _p(8192), _p(4096)) == NO_DEVICE
    big = lattice(16777216, 1, 1)                                                          # the largest count
    assert L.ft_sample_lattice_device(ctx, sc, C.byref(big), 0.0, 0, _p(4096), None, None) == NO_DEVICE
    # n = 0: FT_OK, nothing launched (no device needed)
    assert L.ft_sample_points(ctx, sc, ptr(pts), 0, 0.0, 0, ptr(d), None, None) == OK
    assert L.ft_sample_points_device(ctx, sc, _p(4096), 0, 0.0, 0, _p(8192), None, None) == OK
    # NULL where none is allowed
    assert L.ft_sample_points(None, sc, ptr(pts), 4, 0.0, 0, ptr(d), None, None) == INVALID
    assert L.ft_sample_points(ctx, None, ptr(pts), 4, 0.0, 0, ptr(d), None, None) == INVALID
    assert L.ft_sample_points(ctx, sc, None, 4, 0.0, 0, ptr(d), None, None) == INVALID
    assert L.ft_sample_points_device(ctx, sc, None, 4, 0.0, 0, _p(8192), None, None) == INVALID
    assert L.ft_sample_lattice(ctx, sc, None, 0.0, 0, ptr(d), None, None) == INVALID
    assert L.ft_sample_lattice_device(ctx, sc, None, 0.0, 0, _p(4096), None, None) == INVALID
    assert L.ft_sample_lattice_device(ctx, None, C.byref(lat), 0.0, 0, _p(4096), None, None) == INVALID
    # all three outputs NULL
    assert L.ft_sample_points(ctx, sc, ptr(pts), 4, 0.0, 0, None, None, None) == INVALID
    assert L.ft_sample_points_device(ctx, sc, _p(4096), 4, 0.0, 0, None, None, None) == INVALID
    assert L.ft_sample_lattice(ctx, sc, C.byref(lat), 0.0, 0, None, None, None) == INVALID
    assert L.ft_sample_lattice_device(ctx, sc, C.byref(lat), 0.0, 0, None, None, None) == INVALID
    # n < 0; a count < 1 or > 2^24
    assert L.ft_sample_points(ctx, sc, ptr(pts), -1, 0.0, 0, ptr(d), None, None) == INVALID
    assert L.ft_sample_points_device(ctx, sc, _p(4096), -1, 0.0, 0, _p(8192), None, None) == INVALID
    for bad in (lattice(0, 3, 4), lattice(2, -1, 4), lattice(2, 3, 0), lattice(16777217, 1, 1), lattice(1, 16777217, 1), lattice(1, 1, 16777217)):
        assert L.ft_sample_lattice(ctx, sc, C.byref(bad), 0.0, 0, ptr(d), None, None) == INVALID
        assert L.ft_sample_lattice_device(ctx, sc, C.byref(bad), 0.0, 0, _p(4096), None, None) == INVALID
    # unknown flag bits
    for flags in (2, 3, 0x80000000):
        assert L.ft_sample_points(ctx, sc, ptr(pts), 4, 0.0, flags, ptr(d), None, None) == INVALID
        assert L.ft_sample_lattice_device(ctx, sc, C.byref(lat), 0.0, flags, _p(4096), None, None) == INVALID
    # misalignment (device forms), identical input and output
    for args in ((_p(4097), _p(8192), None, None), (_p(4096), _p(8194), None, None), (_p(4096), None, _p(8193), None), (_p(4096), None, None, _p(8195))):
        assert L.ft_sample_points_device(ctx, sc, args[0], 4, 0.0, 0, *args[1:]) == INVALID
    assert L.ft_sample_lattice_device(ctx, sc, C.byref(lat), 0.0, 0, _p(4098), None, None) == INVALID
    assert L.ft_sample_points_device(ctx, sc, _p(4096), 4, 0.0, 0, _p(4096), None, None) == INVALID
    assert L.ft_sample_points_device(ctx, sc, _p(4096), 4, 0.0, 0, None, _p(4096), None) == INVALID
    # too many points for one call
    assert L.ft_sample_points_device(ctx, sc, _p(4096), 0xFFFF0000, 0.0, 0, _p(8192), None, None) == UNSUPPORTED
    assert L.ft_sample_points_device(ctx, sc, _p(4096), 0xFFFF0000 - 1, 0.0, 0, _p(8192), None, None) == NO_DEVICE
    assert L.ft_sample_points(ctx, sc, ptr(pts), 1 << 40, 0.0, 0, ptr(d), None, None) == UNSUPPORTED
    for huge in (lattice(65536, 65536, 1), lattice(16777216, 256, 1), lattice(16777216, 16777216, 16777216), lattice(1, 65536, 65536), lattice(65536, 65535, 1)):     # the last one: exactly 0xFFFF0000
        assert L.ft_sample_lattice(ctx, sc, C.byref(huge), 0.0, 0, ptr(d), None, None) == UNSUPPORTED
        assert L.ft_sample_lattice_device(ctx, sc, C.byref(huge), 0.0, 0, _p(4096), None, None) == UNSUPPORTED
    assert L.ft_sample_lattice_device(ctx, sc, C.byref(lattice(65535, 65535, 1)), 0.0, 0, _p(4096), None, None) == NO_DEVICE      # below it
    # a scene of another context
    other = ft.Device(-1)
    try:
        foreign = other.scene(syn.config3(n=8)[0])._scene
        assert L.ft_sample_points(ctx, foreign, ptr(pts), 4, 0.0, 0, ptr(d), None, None) == INVALID
        assert L.ft_sample_lattice_device(ctx, foreign, C.byref(lat), 0.0, 0, _p(4096), None, None) == INVALID
    finally:
        other.close()


def test_internal_brick_shape_switch_is_per_context(host_scene):
    ctx, _ = host_scene
    fn = _lib.lib.ft_ctx_field_brick                                                       # internal: not in the header
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int32]
    assert [fn(ctx, k) for k in (0, 1, 2)] == [OK, OK, OK]
    assert fn(ctx, 3) == INVALID and fn(ctx, -2) == INVALID and fn(None, 0) == INVALID
    assert fn(ctx, -1) == OK                                                               # the shipped rule: by kernel family


class FakeTensor:
    """what api.is_device_tensor looks for, without torch"""

    def __init__(self, shape=(5, 3), dtype="torch.float32", contiguous=True, is_cuda=True):
        self.shape, self.dtype, self._contiguous, self.is_cuda = shape, dtype, contiguous, is_cuda

    def data_ptr(self): return 4096

    def is_contiguous(self): return self._contiguous


def test_device_point_buffers_are_checked_strictly():
    assert api.check_device_points(FakeTensor()) == (5,)
    assert api.check_device_points(FakeTensor(shape=(4, 6, 3))) == (4, 6)
    assert api.check_device_points(FakeTensor(shape=(0, 3))) == (0,)
    with pytest.raises(ValueError, match="float32"):
        api.check_device_points(FakeTensor(dtype="torch.float64"))
    with pytest.raises(ValueError, match=r"\[\.\.\., 3\]"):
        api.check_device_points(FakeTensor(shape=(5, 4)))
    with pytest.raises(ValueError, match=r"\[\.\.\., 3\]"):
        api.check_device_points(FakeTensor(shape=()))
    with pytest.raises(ValueError, match="contiguous"):
        api.check_device_points(FakeTensor(contiguous=False))
    dev = ft.Device(-1)
    try:
        ds = dev.scene(syn.config3(n=8)[0])
        for bad in (FakeTensor(dtype="torch.float16"), FakeTensor(shape=(5, 8)), FakeTensor(contiguous=False)):
            with pytest.raises(ValueError):
                ds.sample_points(bad)                                                      # refused before anything is allocated or launched
        with pytest.raises(ValueError, match="no output"):
            ds.sample_points(np.zeros((2, 3), np.float32), distance=False)
        with pytest.raises(ValueError, match="like"):
            ds.sample_lattice((0, 0, 0), (1, 1, 1), (2, 2, 2), like=np.zeros(3, np.float32))
        with pytest.raises(ValueError, match="counts"):
            ds.sample_lattice((0, 0, 0), (1, 1, 1), (2, 0, 2))
        with pytest.raises(ValueError, match=r"\[\.\.\., 3\]"):
            ds.sample_points(np.zeros((2, 4), np.float32))
        with pytest.raises(ft.FrayTracerError) as e:                                       # everything passes: the host-only context has no device
            ds.sample_lattice((0, 0, 0), (1, 1, 1), (2, 2, 2), normal_epsilon=0.01, material=True)
        assert e.value.code == NO_DEVICE
    finally:
        dev.close()


def test_python_api_has_the_field_forms():
    for name in ("sample_points", "sample_lattice", "sample_points_device", "sample_lattice_device"):
        assert callable(getattr(ft.DeviceScene, name)), name
    assert callable(ft.SdfForm.normal) and callable(ft.SdfForm.sample) and callable(ft.lattice_points)
    mat = ft.SdfMaterial.createSolid((0.25, 0.5, 0.75))
    fs = ft.FieldSamples(np.zeros(2, np.float32), None, np.array([7, -1], np.int32), {7: mat})
    assert fs.descriptor(7) is mat and fs.descriptor(-1) is None and fs.normal is None


def reference_lattice_points(origin, step, counts):
    """the definition, written as a loop: per coordinate one float32 product, rounded, then one float32 sum, rounded"""
    F = np.float32
    o, s = [F(v) for v in origin], [F(v) for v in step]
    out = np.empty(tuple(counts) + (3,), F)
    with np.errstate(all="ignore"):
        for i in range(counts[0]):
            for j in range(counts[1]):
                for k in range(counts[2]):
                    for a, idx in enumerate((i, j, k)):
                        prod = F(F(idx) * s[a])
                        out[i, j, k, a] = F(o[a] + prod)
    return out


@pytest.mark.parametrize("origin, step, counts", [
    ((-1.5, 0.25, 3.0), (0.1, 0.3, 0.7), (5, 4, 7)),
    ((2.0, 2.0, 2.0), (-0.37, 0.0, 1e-3), (6, 3, 5)),                                      # a negative step, a zero step
    ((1e7, 1e7, -1e7), (0.1, 0.7, 0.3), (9, 8, 11)),                                       # both roundings are visible: the product's, then the sum's at 1e7 (ulp 1)
    ((0.1, 0.2, 0.3), (1.0 / 3.0, 1e-8, 1e30), (3, 1, 4)),
])
def test_lattice_points_is_the_definition(origin, step, counts):
    got = ft.lattice_points(origin, step, counts)
    assert got.dtype == np.float32 and got.shape == tuple(counts) + (3,) and got.flags.c_contiguous
    want = reference_lattice_points(origin, step, counts)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if origin[0] == 1e7:
        # the case separates the definition from its neighbours: a fused multiply-add, and double arithmetic rounded once, give other bits
        i = np.arange(counts[0], dtype=np.float64)
        once = (np.float64(np.float32(origin[0])) + i * np.float64(np.float32(step[0]))).astype(np.float32)
        assert not np.array_equal(once, got[:, 0, 0, 0])                                   # i = 5: 5 * 0.1f rounds to 0.5, and 1e7 + 0.5 is a tie that goes down
        assert got[5, 0, 0, 0] == np.float32(1e7) and once[5] == np.float32(10000001.0)


def test_cpp_field_mirror_compiles(tmp_path):
    assert_cpp_compiles(tmp_path, "field.cpp",
                        "FrayTracer::Field::Samples f(const FrayTracer::SdfScene& s, const std::vector<ft_vec3>& p) {\n"
                        "    FrayTracer::Field::Request r; r.normal = true; r.normalEpsilon = 0.00125f; r.material = true; r.bounded = true;\n"
                        "    ft_lattice l{{0.0f, 0.0f, 0.0f}, {0.1f, 0.1f, 0.1f}, 4, 5, 6};\n"
                        "    FrayTracer::Field::Samples a = FrayTracer::Field::sampleLattice(s, l, r);\n"
                        "    FrayTracer::Field::Samples b = FrayTracer::Field::samplePoints(s, p);\n"
                        "    a.distance.insert(a.distance.end(), b.distance.begin(), b.distance.end());\n"
                        "    return a;\n"
                        "}\n")


def test_fsharp_binding_imports_the_field_forms():
    fs = open(os.path.join(ROOT, "host", "fsharp", "FrayTracer.Hip.fs")).read()
    for name in NAMES:
        assert re.search(r"\[<DllImport\(Lib\)>\] extern int " + name + r"\(", fs), name
    m = re.search(r"type\s+FtLattice\s*=\s*\{(.*?)\}", fs, flags=re.S)
    assert m and [(n, t) for n, t in re.findall(r"(\w+)\s*:\s*([\w.]+)", m.group(1))] == \
        [("Origin", "Vector3"), ("Step", "Vector3"), ("Nx", "int"), ("Ny", "int"), ("Nz", "int")]
