"""Meshing on the GPU (ft_mesh_lattice, ft_mesh_values, ft_mesh_values_device): vertices, triangles and n_skipped bit for bit against the numpy
restatement of the rule (tests/mesh_restatement.py) — every sign pattern of one cell, special values, the lattice shapes that leave tiles and
waves part-filled, every level of the scan, a second tile for every workgroup, the scene form on the CPU oracle's distances with normals and
materials, the options, the glibc arithmetic, the device buffers and the meshes' lifetimes."""
import ctypes as C
import itertools

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import _lib
from helpers import assert_bit_equal, glibc_mode, options, options_left_at_defaults  # noqa: F401  (glibc_mode, options_left_at_defaults: fixtures)

import mesh_cases as cases
import mesh_restatement as rule

pytestmark = pytest.mark.gpu

F = np.float32
L = _lib.lib
TILE = 512                                 # lattice points per workgroup of the count and emit kernels (ft_mesh.h FT_MESH_TILE_DEFAULT)
SCAN_ROUND = 512 * 8                       # tiles per round of the scan kernel (FT_MESH_SCAN_BLOCK * FT_MESH_SCAN_ITEMS)
UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def assert_same_mesh(got, want, what):
    assert got.vertices.dtype == np.float32 and got.triangles.dtype == np.int32, what
    assert got.vertices.shape == want.vertices.shape and got.triangles.shape == want.triangles.shape, (what, got.vertices.shape, want.vertices.shape,
                                                                                                       got.triangles.shape, want.triangles.shape)
    assert np.array_equal(got.vertices.view(np.uint32), want.vertices.view(np.uint32)), what + ": vertices"
    assert np.array_equal(got.triangles, want.triangles), what + ": triangles"
    assert got.skipped == want.skipped, (what, got.skipped, want.skipped)


def check_values(gpu, values, origin=UNIT[0], step=UNIT[1], iso=0.0, what=""):
    got = gpu.mesh_values(values, origin, step, iso)
    want = rule.extract(values, origin, step, iso)
    assert_same_mesh(got, want, what)
    assert got.normal is None and got.material is None
    return want


def test_every_sign_pattern_of_one_cell(gpu):
    rng = np.random.default_rng(7)
    triangles = 0
    for pattern in itertools.product((False, True), repeat=8):
        mag = rng.uniform(0.05, 2.0, (2, 2, 2)).astype(F)
        d = np.where(np.array(pattern).reshape(2, 2, 2), -mag, mag).astype(F)
        triangles += len(check_values(gpu, d, (0.25, -1.5, 3.0), (0.5, 0.75, 1.25), what=str(pattern)).triangles)
    assert triangles == 6 * (8 * 1 + 6 * 2) * 16                                           # each tetrahedron: 8 masks of its corners with 1 triangle, 6 with 2; 2^4 for the other corners


SPECIALS = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, np.inf, -np.inf, np.nan, 3.0e38, -3.0e38, 1.0, -1.0, 0.5, -0.5], F)


@pytest.mark.parametrize("iso", [0.0, 0.5, -1e-40])
def test_special_values(gpu, iso):
    rng = np.random.default_rng(11)
    skipped = vertices = 0
    for shape in ((2, 2, 2), (3, 3, 3), (4, 3, 5)):
        for _ in range(12):
            d = rng.standard_normal(shape).astype(F)
            where = rng.random(shape) < 0.45
            d[where] = rng.choice(SPECIALS, int(where.sum()))
            d[rng.random(shape) < 0.1] = F(iso)                                            # values of exactly iso
            want = check_values(gpu, d, (-1.0, 0.5, 2.0), (0.3, -0.2, 0.0), iso, f"iso {iso} {shape}")      # a negative and a zero step as well
            skipped, vertices = skipped + want.skipped, vertices + len(want.vertices)
    assert skipped > 100 and vertices > 100                                                # the inputs did reach both rules
    whole = np.full((3, 3, 3), np.nan, F)
    assert check_values(gpu, whole, iso=iso).skipped == 6 * 8                              # nothing but NaN: every tetrahedron skipped, no vertex


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 70, 1), (2, 2, 2), (2, 2, 70), (3, 3, 3), (5, 2, 130), (21, 18, 23)])
def test_lattice_shapes(gpu, shape):
    rng = np.random.default_rng(sum(shape))
    d = rng.standard_normal(shape).astype(F)
    want = check_values(gpu, d, (0.1, 0.2, 0.3), (0.01, 0.02, 0.03), what=str(shape))
    assert (len(want.triangles) > 0) == (min(shape) > 1)
    check_values(gpu, d, (0.1, 0.2, 0.3), (0.01, 0.02, 0.03), 0.75, f"{shape} iso 0.75")


def tiles_with_a_crossing(d, iso=0.0):
    """per tile of TILE consecutive points: does a cell or an owned edge at one of its points cross the level (a condition on the input alone)"""
    inside = (d - F(iso)) < 0
    pad = np.pad(inside, ((0, 1), (0, 1), (0, 1)), mode="edge")
    nx, ny, nz = d.shape
    mixed = np.zeros(d.shape, bool)
    for di, dj, dk in rule.DIRS:
        mixed |= pad[di:di + nx, dj:dj + ny, dk:dk + nz] != inside
    flat = np.zeros(-(-d.size // TILE) * TILE, bool)
    flat[:d.size] = mixed.reshape(-1)
    return flat.reshape(-1, TILE).any(axis=1)


def test_tiles_cross_every_level_of_the_scan(gpu):
    """130 x 128 x 130 = 2 163 200 points are 4 225 tiles of 512: the scan kernel's single workgroup takes 512 x 8 = 4 096 tile sums per round, so
    the sums cross a thread's eight items, a wave's 64 threads, the workgroup's 8 waves and the carry into a second round.  Two thin shells
    around i = 8 and i = 126 with nothing in between: empty tiles between non-empty ones, and non-empty ones in both rounds."""
    shape = (130, 128, 130)
    i = np.arange(shape[0], dtype=F)[:, None, None]
    rng = np.random.default_rng(3)
    d = (np.minimum(np.abs(i - F(8.3)), np.abs(i - F(126.4))) - F(1.2) + rng.uniform(-0.2, 0.2, shape).astype(F)).astype(F)
    busy = tiles_with_a_crossing(d)
    assert len(busy) == 4225 and len(busy) > SCAN_ROUND
    idx = np.flatnonzero(busy)
    assert idx[0] < SCAN_ROUND <= idx[-1] and (np.diff(idx) > 1).any()
    assert busy[:SCAN_ROUND].reshape(8, 64, 8).any(axis=(1, 2)).sum() >= 2                # more than one wave of the scan has something to add
    want = check_values(gpu, d, what="scan levels")
    assert len(want.vertices) > 100000


def test_every_workgroup_takes_a_second_tile(gpu):
    """64 x 64 x 66 = 270 336 points are 528 tiles of 512 points: with one workgroup per CU (FT_OPT_MAX_BLOCKS_PER_CU = 1; 256 CUs: 256 workgroups)
    every workgroup of the count and emit kernels comes back for a second tile, and 16 for a third"""
    shape = (64, 64, 66)
    assert -(-np.prod(shape) // TILE) >= 2 * 256
    origin, step = (-1.5,) * 3, (3.0 / 63, 3.0 / 63, 3.0 / 65)
    p = ft.lattice_points(origin, step, shape)
    d = (np.sqrt((p * p).sum(axis=-1, dtype=F)) - F(1.0) + F(0.05) * np.sin(F(9.0) * p[..., 0])).astype(F)
    with options(gpu, max_blocks_per_cu=1):
        want = check_values(gpu, d, origin, step, what="second tile")
    assert rule.is_closed(want.triangles) and rule.euler_characteristic(want) == 2


def test_every_tile_gives_the_same_mesh(gpu):
    tile = L.ft_ctx_mesh_tile                                                              # internal: not in the header
    tile.restype, tile.argtypes = C.c_int, [C.c_void_p, C.c_int32]
    d = np.random.default_rng(5).standard_normal((21, 18, 23)).astype(F)
    d[4, 5, 6], d[10, 10, 10] = np.nan, np.inf
    want = rule.extract(d, *UNIT)
    try:
        for t in (128, 256, 1024, 512):
            assert tile(gpu._ctx, t) == 0
            assert_same_mesh(gpu.mesh_values(d, *UNIT), want, f"tile {t}")
    finally:
        tile(gpu._ctx, TILE)                                                               # the shipped tile


def test_an_empty_mesh(gpu):
    d = np.full((9, 10, 11), 0.5, F)                                                       # all distances positive
    got = gpu.mesh_values(d, *UNIT)
    assert got.vertices.shape == (0, 3) and got.triangles.shape == (0, 3) and got.skipped == 0
    got = gpu.mesh_values(-d, *UNIT)                                                       # all inside: nothing crosses either
    assert got.vertices.shape == (0, 3) and got.triangles.shape == (0, 3)
    ds = gpu.scene(cases.scene_of("c3_64"))
    far = ds.mesh_lattice((100.0, 100.0, 100.0), (0.1, 0.1, 0.1), (5, 6, 7), normal_epsilon=cases.NORMAL_EPS, material=True)
    assert far.vertices.shape == (0, 3) and far.normal.shape == (0, 3) and far.material.shape == (0,) and far.skipped == 6 * 4 * 5 * 6      # +inf there


# ---- the scene form ------------------------------------------------------------------------------------------------------------------------


def numpy_normal(dx, dy, dz, d):
    with np.errstate(all="ignore"):
        g = np.stack([dx - d, dy - d, dz - d], axis=-1).astype(F)
        return (g / np.sqrt((g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2])[..., None]).astype(F)


def oracle_at(oracle, name, pts, eps):
    """SdfForm.normal and the material colour at pts [n, 3] from the CPU oracle"""
    os_ = oracle.Oracle().scene(cases.scene_of(name))
    O = oracle.Oracle()
    form = O.object_form(os_.object)
    with np.errstate(all="ignore"):
        d = O.form_distance(form, pts)
        probes = []
        for a in range(3):
            q = pts.copy()
            q[:, a] = pts[:, a] + F(eps)
            probes.append(O.form_distance(form, q))
    return numpy_normal(*probes, d), np.array([O.object_color(os_.object, p) for p in pts], F)


def material_colors(mesh):
    handles = np.asarray(mesh.material)
    out = np.empty(handles.shape + (3,), F)
    for h in np.unique(handles):
        out[handles == h] = np.asarray(mesh.descriptor(h).args[0], F)
    return out


@pytest.mark.parametrize("name", list(cases.SCENES))
def test_scene_form_matches_the_restatement_on_the_oracle_distances(gpu, oracle, name):
    origin, step, d = cases.oracle_lattice(oracle, name)
    want = rule.extract(d, origin, step)
    assert len(want.vertices) >= 400                                                       # tests/test_mesh_host.py asserts the other input conditions
    ds = gpu.scene(cases.scene_of(name))
    got = ds.mesh_lattice(origin, step, cases.COUNTS, normal_epsilon=cases.NORMAL_EPS, material=True)
    assert_same_mesh(got, want, name)
    nrm, col = oracle_at(oracle, name, want.vertices, cases.NORMAL_EPS)
    assert got.normal.shape == want.vertices.shape and got.material.shape == (len(want.vertices),) and got.material.dtype == np.int32
    assert_bit_equal(got.normal, nrm, name + ": normal")
    assert (got.material >= 0).all()
    assert_bit_equal(material_colors(got), col, name + ": material colour")
    # exactly what sample_points gives for those points
    pts = ds.sample_points(got.vertices, normal_epsilon=cases.NORMAL_EPS, material=True)
    assert_bit_equal(got.normal, pts.normal, name + ": normal against sample_points")
    assert np.array_equal(got.material, pts.material)
    # without the flags: the same mesh, nothing else; another level; the values form on the lattice's distances
    plain = ds.mesh_lattice(origin, step, cases.COUNTS)
    assert_same_mesh(plain, want, name + " without flags")
    assert plain.normal is None and plain.material is None
    only_material = ds.mesh_lattice(origin, step, cases.COUNTS, material=True)
    assert only_material.normal is None and np.array_equal(only_material.material, got.material)
    assert_same_mesh(ds.mesh_lattice(origin, step, cases.COUNTS, iso=0.03), rule.extract(d, origin, step, 0.03), name + " iso 0.03")
    assert_same_mesh(gpu.mesh_values(ds.sample_lattice(origin, step, cases.COUNTS).distance, origin, step), want, name + " values form")
    for opt, values in (("cull", (0, 1)), ("carved", (0, 1)), ("max_blocks_per_cu", (1, 3))):
        for v in values:
            with options(gpu, **{opt: v}):
                other = ds.mesh_lattice(origin, step, cases.COUNTS, normal_epsilon=cases.NORMAL_EPS, material=True)
            assert_same_mesh(other, want, f"{name} {opt} = {v}")
            assert_bit_equal(other.normal, got.normal, f"{name} {opt} = {v}: normal")
            assert np.array_equal(other.material, got.material), (opt, v)


def test_scene_form_under_the_glibc_arithmetic(gpu, oracle, glibc_mode):
    origin, step, d = cases.oracle_lattice(oracle, "c3_64", libm=True)                     # formed under the oracle's libm switch (glibc_mode holds it)
    want = rule.extract(d, origin, step)
    ds = gpu.scene(cases.scene_of("c3_64"))
    got = ds.mesh_lattice(origin, step, cases.COUNTS, normal_epsilon=cases.NORMAL_EPS)
    assert_same_mesh(got, want, "glibc")
    nrm, _ = oracle_at(oracle, "c3_64", want.vertices, cases.NORMAL_EPS)
    assert_bit_equal(got.normal, nrm, "glibc: normal")


def test_sdf_form_mesh(gpu, oracle):
    origin, step, d = cases.oracle_lattice(oracle, "c3_64")
    form = cases.scene_of("c3_64").Object.kids[1]
    got = ft.SdfForm.mesh(form, origin, step, cases.COUNTS, device=gpu)
    assert_same_mesh(got, rule.extract(d, origin, step), "SdfForm.mesh")


# ---- device buffers and lifetimes --------------------------------------------------------------------------------------------------------------

GUARD = 0x5EEDFACE


@pytest.fixture(scope="module")
def hip():
    h = C.CDLL("libamdhip64.so.7")             # the runtime the library is linked against (already loaded: same instance)
    h.hipMalloc.argtypes, h.hipMemcpy.argtypes, h.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p]
    return h


class GuardedBuffer:
    """n_words 4-byte words of device memory between two rows of 64 guard words"""

    def __init__(self, hip, n_words):
        self.hip, self.n = hip, n_words
        self.base = C.c_void_p()
        assert hip.hipMalloc(C.byref(self.base), C.c_size_t(4 * (n_words + 128))) == 0
        self.ptr = self.base.value + 256
        host = np.full(n_words + 128, GUARD, np.uint32)
        host[64:64 + n_words] = 0xFFFFFFFF
        assert hip.hipMemcpy(self.base, host.ctypes.data_as(C.c_void_p), C.c_size_t(host.nbytes), 1) == 0
        assert hip.hipDeviceSynchronize() == 0

    def read(self, dtype):
        host = np.empty(self.n + 128, np.uint32)
        assert self.hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), self.base, C.c_size_t(host.nbytes), 2) == 0
        return host[64:64 + self.n].view(dtype), bool((host[:64] == GUARD).all() and (host[-64:] == GUARD).all())

    def free(self):
        assert self.hip.hipFree(self.base) == 0


def from_device(hip, ptr, shape, dtype):
    out = np.empty(shape, dtype)
    if out.size:
        assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0
    return out


def guarded_host(shape, dtype):
    """a host array between two rows of 16 guard words -> (the array, a check that the guards are intact)"""
    n = int(np.prod(shape))
    raw = np.full(n + 32, GUARD, np.uint32)
    return raw[16:16 + n].view(dtype).reshape(shape), lambda: bool((raw[:16] == GUARD).all() and (raw[-16:] == GUARD).all())


def read_mesh(handle, normals=False, materials=False):
    info = _lib.MeshInfo()
    assert L.ft_mesh_get_info(handle, C.byref(info)) == 0
    nv, nt = info.n_vertices, info.n_triangles
    parts = [guarded_host((nv, 3), np.float32), guarded_host((nt, 3), np.int32), guarded_host((nv, 3), np.float32) if normals else None,
             guarded_host((nv,), np.int32) if materials else None]
    ptrs = [None if p is None else p[0].ctypes.data_as(C.c_void_p) for p in parts]
    assert L.ft_mesh_read(handle, *ptrs) == 0
    assert all(p is None or p[1]() for p in parts)                                         # the guard words behind the caller's buffers
    return info, [None if p is None else p[0] for p in parts]


@pytest.mark.parametrize("name", ["c3_64", "console_200"])
def test_device_buffers_and_the_values_device_form(gpu, oracle, hip, name):
    origin, step, d = cases.oracle_lattice(oracle, name)
    want = rule.extract(d, origin, step)
    ds = gpu.scene(cases.scene_of(name))
    lat, _ = ft.api._lattice(origin, step, cases.COUNTS)
    n = int(np.prod(cases.COUNTS))
    kept = GuardedBuffer(hip, n)
    a, b = C.c_void_p(), C.c_void_p()
    try:
        # a lattice kept from ft_sample_lattice_device, meshed where it lies
        ds.sample_lattice_device(origin, step, cases.COUNTS, kept.ptr)
        assert L.ft_mesh_values_device(gpu._ctx, C.byref(lat), C.c_void_p(kept.ptr), 0.0, C.byref(a)) == 0
        assert L.ft_mesh_lattice(gpu._ctx, ds._scene, C.byref(lat), 0.0, cases.NORMAL_EPS, 3, C.byref(b)) == 0
        values, intact = kept.read(np.float32)
        assert intact and np.array_equal(values.view(np.uint32), d.reshape(-1).view(np.uint32))        # the input lattice is unchanged, its guards too
        (ia, pa), (ib, pb) = read_mesh(a), read_mesh(b, True, True)
        assert (ia.n_vertices, ia.n_triangles, ia.n_skipped, ia.has_normal, ia.has_material) == (len(want.vertices), len(want.triangles), 0, 0, 0)
        assert (ib.n_vertices, ib.n_triangles, ib.has_normal, ib.has_material) == (len(want.vertices), len(want.triangles), 1, 1)
        for parts in (pa, pb):
            assert np.array_equal(parts[0].view(np.uint32), want.vertices.view(np.uint32)) and np.array_equal(parts[1], want.triangles)
        assert L.ft_mesh_read(a, None, None, pb[2].ctypes.data_as(C.c_void_p), None) == _lib.FT_ERR_INVALID          # built without normals
        # ft_mesh_device_buffers = ft_mesh_read
        bufs = [C.c_void_p() for _ in range(4)]
        assert L.ft_mesh_device_buffers(b, *map(C.byref, bufs)) == 0 and all(p.value for p in bufs)
        assert all(p.value % 4 == 0 for p in bufs)
        nv, nt = ib.n_vertices, ib.n_triangles
        for p, shape, dtype, host in zip(bufs, ((nv, 3), (nt, 3), (nv, 3), (nv,)), (np.float32, np.int32, np.float32, np.int32), pb):
            assert np.array_equal(from_device(hip, p.value, shape, dtype).view(np.uint32), host.view(np.uint32))
        bufs_a = [C.c_void_p(1) for _ in range(4)]
        assert L.ft_mesh_device_buffers(a, *map(C.byref, bufs_a)) == 0 and bufs_a[0].value and bufs_a[1].value and not bufs_a[2].value and not bufs_a[3].value
        # parts of a read: any may be NULL
        info, only_triangles = read_mesh(b)
        assert np.array_equal(only_triangles[1], want.triangles)
        assert L.ft_mesh_read(b, None, None, None, None) == 0
    finally:
        L.ft_mesh_destroy(a)
        L.ft_mesh_destroy(b)
        kept.free()


def test_two_meshes_alive_at_once_destroyed_in_either_order(gpu):
    rng = np.random.default_rng(9)
    fields = [rng.standard_normal(shape).astype(F) for shape in ((6, 7, 8), (9, 5, 4))]
    wants = [rule.extract(d, *UNIT) for d in fields]
    for order in ((0, 1), (1, 0)):
        handles = []
        for d in fields:
            lat, _ = ft.api._lattice(*UNIT, d.shape)
            h = C.c_void_p()
            assert L.ft_mesh_values(gpu._ctx, C.byref(lat), d.ctypes.data_as(C.c_void_p), 0.0, C.byref(h)) == 0
            handles.append(h)
        assert handles[0].value != handles[1].value
        first, second = order
        _, parts = read_mesh(handles[second])                                              # each is whole while the other lives ...
        assert np.array_equal(parts[0].view(np.uint32), wants[second].vertices.view(np.uint32)) and np.array_equal(parts[1], wants[second].triangles)
        L.ft_mesh_destroy(handles[first])
        _, parts = read_mesh(handles[second])                                              # ... and after it is gone
        assert np.array_equal(parts[0].view(np.uint32), wants[second].vertices.view(np.uint32)) and np.array_equal(parts[1], wants[second].triangles)
        L.ft_mesh_destroy(handles[second])
    # a mesh outlives its scene
    dev = ft.Device(0)
    try:
        ds = dev.scene(cases.scene_of("c3_64"))
        origin, step = cases.lattice_around(ds.boundary(), cases.SPAN, cases.COUNTS)
        lat, _ = ft.api._lattice(origin, step, cases.COUNTS)
        whole = ds.mesh_lattice(origin, step, cases.COUNTS)
        h = C.c_void_p()
        assert L.ft_mesh_lattice(dev._ctx, ds._scene, C.byref(lat), 0.0, 0.0, 0, C.byref(h)) == 0
        ds.close()
        _, parts = read_mesh(h)
        assert len(parts[0]) > 0 and np.array_equal(parts[0].view(np.uint32), whole.vertices.view(np.uint32)) and np.array_equal(parts[1], whole.triangles)
        L.ft_mesh_destroy(h)
    finally:
        dev.close()


TENSOR_PATH = r"""
import json, sys
import numpy as np
import torch                              # before the library: torch's HIP runtime is the one the process loads first
import fraytracer_amd as ft
sys.path.insert(0, "tests")
import mesh_cases as cases
import mesh_restatement as rule
same = lambda t, a: bool(np.array_equal(np.ascontiguousarray(t.detach().cpu().numpy()).view(np.uint32), np.ascontiguousarray(a).view(np.uint32)))
dev = ft.Device(0)
d = np.random.default_rng(2).standard_normal((21, 18, 23)).astype(np.float32)
want = rule.extract(d, (0, 0, 0), (1, 1, 1), 0.25)
r = {}
side = torch.cuda.Stream()                # on a side stream, behind the torch kernel that makes the values: the stream hand-over
side.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(side):
    t = torch.from_numpy(d).cuda() * 1.0
    m = dev.mesh_values(t, (0, 0, 0), (1, 1, 1), 0.25)
side.synchronize()
r["tensors"] = m.vertices.is_cuda and m.triangles.is_cuda and m.triangles.dtype == torch.int32 and m.normal is None
r["values: vertices"], r["values: triangles"], r["values: skipped"] = same(m.vertices, want.vertices), same(m.triangles, want.triangles), m.skipped == want.skipped
r["input unchanged"] = same(t, d)
ds = dev.scene(cases.scene_of("c3_64"))
origin, step = cases.lattice_around(ds.boundary(), cases.SPAN, cases.COUNTS)
host = ds.mesh_lattice(origin, step, cases.COUNTS, normal_epsilon=cases.NORMAL_EPS, material=True)
like = ds.mesh_lattice(origin, step, cases.COUNTS, normal_epsilon=cases.NORMAL_EPS, material=True, like=t)      # torch's default stream: the side-stream path
torch.cuda.synchronize()
r["like"] = like.vertices.is_cuda and same(like.vertices, host.vertices) and same(like.triangles, host.triangles) and same(like.normal, host.normal) and same(like.material, host.material)
for bad, why in ((t.double(), "float32"), (t[::2], "contiguous")):
    try:
        dev.mesh_values(bad, (0, 0, 0), (1, 1, 1))
        r["refuses " + why] = False
    except ValueError as e:
        r["refuses " + why] = why in str(e)
dev.close()
print(json.dumps(r))
"""


def test_tensor_path_in_a_process_that_loads_torch_first():
    """device tensors in, device tensors out, on the caller's stream: in a child process that loads torch before the library"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", TENSOR_PATH], cwd=root, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    failed = [k for k, v in r.items() if v is not True]
    assert not failed, failed
