"""Shells on the GPU (ft_mesh_shells, ft_shells_triangles, ft_shells_triangles_device, ft_mesh_select): labels, records and info bit for bit against
the restatement of the rule (tests/shells_restatement.py) — the lattices and triangle lists of tests/shells_cases.py, every tile, the scenes with
normals and materials, refined and not, the selection, the device form and its index check, lifetimes, device buffers and tensors."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import _lib
from helpers import options, options_left_at_defaults  # noqa: F401  (options_left_at_defaults: a fixture)

import mesh_cases
import mesh_restatement as mesh_rule
import shells_cases as cases
import shells_restatement as rule

pytestmark = pytest.mark.gpu

L = _lib.lib
OK, INVALID = _lib.FT_OK, _lib.FT_ERR_INVALID
GUARD = 0x5EEDFACE
BATCH = 4                                  # iterations between two reads of the stop flag (ft_shells.h FT_SHELLS_BATCH)


def assert_same_shells(got, want, what):
    assert got.vertex_shell.dtype == np.int32 and got.triangle_shell.dtype == np.int32 and got.records.dtype == np.int32, what
    assert np.array_equal(got.vertex_shell, want.vertex_shell), what + ": vertex labels"
    assert np.array_equal(got.triangle_shell, want.triangle_shell), what + ": triangle labels"
    assert got.records.shape == want.records.shape and np.array_equal(got.records, want.records), (what, got.records[:8], want.records[:8])
    assert got.info == want.info, (what, got.info, want.info)


def assert_same_mesh(got, want, what):
    assert np.array_equal(got.vertices.view(np.uint32), np.ascontiguousarray(want.vertices).view(np.uint32)), what + ": vertices"
    assert got.triangles.dtype == np.int32 and np.array_equal(got.triangles, want.triangles), what + ": triangles"


def last(gpu):
    fn = L.ft_ctx_shells_last                                                              # internal: not in the header
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]
    two = (C.c_int64 * 2)()
    assert fn(gpu._ctx, two) == OK
    return int(two[0]), int(two[1])


def set_tile(gpu, tile):
    fn = L.ft_ctx_shells_tile                                                              # internal: not in the header
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int32]
    assert fn(gpu._ctx, tile) == OK


def check_iterations(gpu, n_vertices, what):
    iterations, syncs = last(gpu)
    bound = 0                                                                              # floor(log_{3/2} n) + 2
    while 3 ** (bound + 1) <= n_vertices * 2 ** (bound + 1):
        bound += 1
    assert 1 <= iterations <= bound + 2 and syncs == -(-iterations // BATCH) + 1, (what, iterations, syncs)
    return iterations


def test_every_sign_pattern_of_one_cell(gpu):
    several = 0
    for d, origin, step in cases.one_cell_patterns():
        got = gpu.mesh_values(d, origin, step, shells=True)
        want = rule.shells(got.triangles, len(got.vertices))
        assert_same_shells(got.shells, want, "one cell")
        several += want.info["n_shells"] > 1
    assert several >= 10


@pytest.mark.parametrize("name", list(cases.LATTICES))
def test_lattices(gpu, name):
    d, origin, step = cases.lattice(name)
    mesh = cases.mesh_of(name)
    got = gpu.mesh_values(d, origin, step, shells=True)
    assert_same_mesh(got, mesh, name)
    assert_same_shells(got.shells, rule.shells(mesh.triangles, len(mesh.vertices)), name)
    check_iterations(gpu, len(mesh.vertices), name)
    assert np.array_equal(got.shells.euler, rule.euler(got.shells.records)) and np.array_equal(got.shells.closed, got.shells.records[:, 3] == 0)
    plain = gpu.mesh_values(d, origin, step)                                               # the defaults: today's result
    assert plain.shells is None and np.array_equal(plain.triangles, got.triangles)


@pytest.mark.parametrize("name", list(cases.LISTS))
def test_triangle_lists(gpu, name):
    tri, nv = cases.triangle_list(name)
    got = gpu.shells(tri, nv)
    assert_same_shells(got, rule.shells(tri, nv), name)
    if len(tri):
        iterations = check_iterations(gpu, nv, name)
        if name == "permuted_strip":
            assert iterations <= 4 * int(np.ceil(np.log2(nv))) == 60, iterations           # plain minimum propagation needs 4 482 rounds here


def test_generic_entry_refuses_bad_indices_on_the_host(gpu):
    for bad in ([[0, 1, 5]], [[0, 1, 2], [3, 3, 4]], [[-1, 1, 2]]):
        with pytest.raises(ft.FrayTracerError) as e:
            gpu.shells(np.array(bad, np.int32), 5)
        assert e.value.code == INVALID


# ---- every tile ------------------------------------------------------------------------------------------------------------------------------------


def test_every_tile_gives_the_same_shells(gpu):
    """tiles of 128 vertices: the 34 208 vertices of the 41^3 egg crate are 268 tiles, the last one part-filled, so with one workgroup per CU (256
    CUs) some workgroups of every tiled kernel take a second tile; the 270 001 vertices of the sparse strips are 2 110 tiles, more than the 512 x 4
    = 2 048 the scan takes per round.  The rod is one shell across every tile."""
    d41, o41, s41 = cases.lattice("egg_crate_41")
    m41, rod = cases.mesh_of("egg_crate_41"), cases.mesh_of("capped_rod")
    tri, nv = cases.triangle_list("sparse_strips")
    assert -(-len(m41.vertices) // 128) > 256 and len(m41.vertices) % 1024 and len(m41.triangles) % 1024 and -(-nv // 128) > 512 * 4 and nv % 1024
    want41, want_rod, want_sparse = rule.shells(m41.triangles, len(m41.vertices)), rule.shells(rod.triangles, len(rod.vertices)), rule.shells(tri, nv)
    keep = np.arange(len(want41.records)) % 3 != 1
    sel_v, sel_t, _, _, _ = rule.select(m41.vertices, m41.triangles, want41, keep)
    try:
        for tile in (128, 256, 1024, 512):
            set_tile(gpu, tile)
            with options(gpu, max_blocks_per_cu=1):
                got = gpu.mesh_values(d41, o41, s41, shells=True)
                assert_same_shells(got.shells, want41, f"egg crate, tile {tile}")
                kept = gpu.mesh_values(d41, o41, s41, keep=keep)
                assert_same_mesh(kept, mesh_rule.Mesh(sel_v, sel_t, 0), f"selection, tile {tile}")
                assert_same_shells(gpu.shells(tri, nv), want_sparse, f"sparse strips, tile {tile}")
            assert_same_shells(gpu.mesh_values(*cases.lattice("capped_rod"), shells=True).shells, want_rod, f"rod, tile {tile}")
    finally:
        set_tile(gpu, 512)                                                                 # the shipped tile


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(mesh_cases.SCENES))
def test_scenes_with_normals_and_materials_refined_and_not(gpu, oracle, name):
    origin, step, d = mesh_cases.oracle_lattice(oracle, name)
    mesh = mesh_rule.extract(d, origin, step)
    want = rule.shells(mesh.triangles, len(mesh.vertices))
    ds = gpu.scene(mesh_cases.scene_of(name))
    kw = dict(normal_epsilon=mesh_cases.NORMAL_EPS, material=True)
    plain = ds.mesh_lattice(origin, step, mesh_cases.COUNTS, **kw)
    got = ds.mesh_lattice(origin, step, mesh_cases.COUNTS, shells=True, **kw)
    assert_same_mesh(got, mesh, name)
    assert_same_shells(got.shells, want, name)
    assert np.array_equal(got.normal.view(np.uint32), plain.normal.view(np.uint32)) and np.array_equal(got.material, plain.material)
    refined = ds.mesh_lattice(origin, step, mesh_cases.COUNTS, shells=True, refine=4, **kw)
    assert np.array_equal(refined.triangles, mesh.triangles)
    assert_same_shells(refined.shells, want, name + " refined")                            # only positions move
    # the largest shell, with its normals and materials gathered
    keep = rule.largest(want.records, 1)
    v, t, n, m, new = rule.select(plain.vertices, plain.triangles, want, keep, plain.normal, plain.material)
    kept = ds.mesh_lattice(origin, step, mesh_cases.COUNTS, keep=1, **kw)
    assert_same_mesh(kept, mesh_rule.Mesh(v, t, 0), name + " largest")
    assert np.array_equal(kept.normal.view(np.uint32), n.view(np.uint32)) and np.array_equal(kept.material, m) and kept.skipped == plain.skipped
    assert_same_shells(kept.shells, rule.shells(t, len(v)), name + " largest: shells")
    assert kept.descriptor(kept.material[0]) is not None
    form = mesh_cases.scene_of(name).Object
    if name == "c3_64":
        via_form = ft.SdfForm.mesh(form.kids[1], origin, step, mesh_cases.COUNTS, device=gpu, shells=True)
        assert_same_shells(via_form.shells, want, "SdfForm.mesh")


# ---- the selection ---------------------------------------------------------------------------------------------------------------------------------


def test_select(gpu):
    name = "egg_crate_shifted"
    d, origin, step = cases.lattice(name)
    mesh = cases.mesh_of(name)
    want = rule.shells(mesh.triangles, len(mesh.vertices))
    S = len(want.records)
    smallest = np.zeros(S, bool)
    smallest[min(range(S), key=lambda s: (int(want.records[s, 2]), s))] = True
    variants = {"none": np.zeros(S, bool), "all": np.ones(S, bool), "every second": np.arange(S) % 2 == 0, "smallest": smallest,
                "closed": want.records[:, 3] == 0, "largest 3": rule.largest(want.records, 3), "largest 200": np.ones(S, bool)}
    asked = {"closed": "closed", "largest 3": 3, "largest 200": 200, "smallest": lambda sh: smallest}
    for what, keep in variants.items():
        v, t, _, _, new = rule.select(mesh.vertices, mesh.triangles, want, keep)
        got = gpu.mesh_values(d, origin, step, keep=asked.get(what, keep))
        assert got.vertices.shape == (len(v), 3) and got.triangles.shape == (len(t), 3), what
        assert_same_mesh(got, mesh_rule.Mesh(v, t, 0), what)
        kept = want.records[keep].copy()
        kept[:, 0] = new[kept[:, 0]]
        assert np.array_equal(got.shells.records, kept), what                              # the kept records, first_vertex remapped, in order
        assert_same_shells(got.shells, rule.shells(t, len(v)), what)
        assert got.normal is None and got.material is None and got.skipped == mesh.skipped
    # the noise: unused vertices are dropped, n_skipped is copied
    d, origin, step = cases.lattice("noise")
    mesh = cases.mesh_of("noise")
    want = rule.shells(mesh.triangles, len(mesh.vertices))
    got = gpu.mesh_values(d, origin, step, keep=np.ones(len(want.records), bool))
    v, t, _, _, _ = rule.select(mesh.vertices, mesh.triangles, want, np.ones(len(want.records), bool))
    assert_same_mesh(got, mesh_rule.Mesh(v, t, 0), "noise, all kept")
    assert len(got.vertices) == len(mesh.vertices) - want.info["n_unused_vertices"] and got.skipped == mesh.skipped > 0 and got.shells.info["n_unused_vertices"] == 0


def make_mesh(gpu, name):
    d, origin, step = cases.lattice(name)
    lat, _ = ft.api._lattice(origin, step, d.shape)
    h = C.c_void_p()
    assert L.ft_mesh_values(gpu._ctx, C.byref(lat), d.ctypes.data_as(C.c_void_p), 0.0, C.byref(h)) == OK
    return h


def guarded_host(shape, dtype):
    n = int(np.prod(shape))
    raw = np.full(n + 32, GUARD, np.uint32)
    return raw[16:16 + n].view(dtype).reshape(shape), lambda: bool((raw[:16] == GUARD).all() and (raw[-16:] == GUARD).all())


def read_shells(handle):
    info = _lib.ShellsInfo()
    assert L.ft_shells_get_info(handle, C.byref(info)) == OK
    parts = [guarded_host((info.n_vertices,), np.int32), guarded_host((info.n_triangles,), np.int32), guarded_host((info.n_shells, 4), np.int32)]
    assert L.ft_shells_read(handle, *[p[0].ctypes.data_as(C.c_void_p) for p in parts]) == OK
    assert all(p[1]() for p in parts)                                                      # the guard words round the caller's buffers
    return ft.Shells(*[p[0] for p in parts], info={k: int(getattr(info, k)) for k, _ in info._fields_})


def read_mesh(handle):
    info = _lib.MeshInfo()
    assert L.ft_mesh_get_info(handle, C.byref(info)) == OK
    v, t = np.empty((info.n_vertices, 3), np.float32), np.empty((info.n_triangles, 3), np.int32)
    assert L.ft_mesh_read(handle, v.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), None, None) == OK
    return mesh_rule.Mesh(v, t, info.n_skipped)


def test_lifetimes_and_shells_of_another_mesh(gpu):
    name = "clipped_plus_whole"
    mesh = cases.mesh_of(name)
    want = rule.shells(mesh.triangles, len(mesh.vertices))
    a, b = make_mesh(gpu, name), make_mesh(gpu, name)                                      # equal counts, equal bits: two meshes all the same
    sa, sel = C.c_void_p(), C.c_void_p(0xDEAD)
    assert L.ft_mesh_shells(a, C.byref(sa)) == OK
    keep = np.array([0, 1], np.uint8)
    assert L.ft_mesh_select(b, sa, keep.ctypes.data_as(C.c_void_p), 2, C.byref(sel)) == INVALID and sel.value is None
    assert L.ft_mesh_select(a, sa, keep.ctypes.data_as(C.c_void_p), 3, C.byref(sel)) == INVALID and sel.value is None
    assert L.ft_mesh_select(a, sa, keep.ctypes.data_as(C.c_void_p), 2, C.byref(sel)) == OK and sel.value
    L.ft_mesh_destroy(b)
    L.ft_mesh_destroy(a)                                                                   # the shells outlive their mesh ...
    assert_same_shells(read_shells(sa), want, "after the mesh")
    L.ft_shells_destroy(sa)                                                                # ... and the selected mesh outlives both
    v, t, _, _, _ = rule.select(mesh.vertices, mesh.triangles, want, keep)
    got = read_mesh(sel)
    assert_same_mesh(got, mesh_rule.Mesh(v, t, 0), "after the mesh and the shells")
    again = C.c_void_p()
    assert L.ft_mesh_shells(sel, C.byref(again)) == OK                                     # a selected mesh is a mesh like any other
    assert_same_shells(read_shells(again), rule.shells(t, len(v)), "shells of the selected mesh")
    L.ft_shells_destroy(again)
    L.ft_mesh_destroy(sel)


# ---- the device form ---------------------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def hip():
    h = C.CDLL("libamdhip64.so.7")             # the runtime the library is linked against (already loaded: same instance)
    h.hipMalloc.argtypes, h.hipMemcpy.argtypes, h.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p]
    return h


class DeviceWords:
    """an int32 array in device memory between two rows of 64 guard words"""

    def __init__(self, hip, array):
        self.hip, self.n = hip, array.size
        self.base = C.c_void_p()
        host = np.full(self.n + 128, GUARD, np.uint32)
        host[64:64 + self.n] = array.reshape(-1).view(np.uint32)
        self.sent = host
        assert hip.hipMalloc(C.byref(self.base), C.c_size_t(host.nbytes)) == 0
        self.ptr = self.base.value + 256
        assert hip.hipMemcpy(self.base, host.ctypes.data_as(C.c_void_p), C.c_size_t(host.nbytes), 1) == 0

    def unchanged(self):
        host = np.empty_like(self.sent)
        assert self.hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), self.base, C.c_size_t(host.nbytes), 2) == 0
        return bool(np.array_equal(host, self.sent))

    def free(self):
        assert self.hip.hipFree(self.base) == 0


def from_device(hip, ptr, shape, dtype):
    out = np.empty(shape, dtype)
    if out.size:
        assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0
    return out


def test_device_form_and_device_buffers(gpu, hip):
    tri, nv = cases.triangle_list("isolated_between")
    mesh = cases.mesh_of("clipped_plus_whole")
    for triangles, n_vertices, what in ((tri, nv, "list"), (mesh.triangles, len(mesh.vertices), "mesh")):
        want = rule.shells(triangles, n_vertices)
        buf = DeviceWords(hip, triangles)
        h = C.c_void_p()
        try:
            assert L.ft_shells_triangles_device(gpu._ctx, C.c_void_p(buf.ptr), len(triangles), n_vertices, C.byref(h)) == OK
            assert buf.unchanged()                                                         # only read
            assert_same_shells(read_shells(h), want, what)
            bufs = [C.c_void_p() for _ in range(3)]
            assert L.ft_shells_device_buffers(h, *map(C.byref, bufs)) == OK and all(p.value and p.value % 4 == 0 for p in bufs)
            assert L.ft_shells_device_buffers(h, None, None, None) == OK
            assert np.array_equal(from_device(hip, bufs[0].value, (n_vertices,), np.int32), want.vertex_shell)
            assert np.array_equal(from_device(hip, bufs[1].value, (len(triangles),), np.int32), want.triangle_shell)
            assert np.array_equal(from_device(hip, bufs[2].value, want.records.shape, np.int32), want.records)
            assert L.ft_shells_read(h, None, None, None) == OK
        finally:
            L.ft_shells_destroy(h)
            buf.free()


@pytest.mark.parametrize("bad", ["out of range", "negative", "twice"])
def test_device_form_checks_its_indices_on_the_device(gpu, hip, bad):
    """the first pass finds the index and the constructor says so at its first synchronisation; nothing was indexed with it: the context labels
    the next list as if nothing had happened, and the input is untouched"""
    tri, nv = cases.triangle_list("open_fan")
    broken = tri.copy()
    broken[1500] = {"out of range": [0, 1500, nv], "negative": [0, -7, 1501], "twice": [0, 1500, 1500]}[bad]
    buf = DeviceWords(hip, broken)
    h = C.c_void_p(0xDEAD)
    try:
        assert L.ft_shells_triangles_device(gpu._ctx, C.c_void_p(buf.ptr), len(broken), nv, C.byref(h)) == INVALID and h.value is None
        assert "index" in _lib.last_error() and buf.unchanged()
        assert last(gpu) == (BATCH, 1)                                                     # reported at the first synchronisation
    finally:
        buf.free()
    assert_same_shells(gpu.shells(tri, nv), rule.shells(tri, nv), "after a refusal")


TENSOR_PATH = r"""
import json, sys
import numpy as np
import torch                              # before the library: torch's HIP runtime is the one the process loads first
import fraytracer_amd as ft
sys.path.insert(0, "tests")
import shells_cases as cases
import shells_restatement as rule
host = lambda t: np.ascontiguousarray(t.detach().cpu().numpy())
def same(got, want):
    return bool(got.vertex_shell.is_cuda and got.records.is_cuda and got.records.dtype == torch.int32 and np.array_equal(host(got.vertex_shell), want.vertex_shell)
                and np.array_equal(host(got.triangle_shell), want.triangle_shell) and np.array_equal(host(got.records), want.records) and got.info == want.info)
dev = ft.Device(0)
r = {}
mesh = cases.mesh_of("egg_crate")
want = rule.shells(mesh.triangles, len(mesh.vertices))
side = torch.cuda.Stream()                # on a side stream, behind the torch kernel that makes the triangles: the stream hand-over
side.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(side):
    t = torch.from_numpy(np.array(mesh.triangles)).cuda() + 0
    got = dev.shells(t, len(mesh.vertices))
side.synchronize()
r["tensor on a side stream"] = same(got, want)
r["input unchanged"] = bool(np.array_equal(host(t), mesh.triangles))
r["like"] = same(dev.shells(mesh.triangles, len(mesh.vertices), like=t), want)          # torch's default stream: the side-stream path
torch.cuda.synchronize()
r["closed, euler"] = bool(got.closed.all() and (got.euler == 2).all())
d, origin, step = cases.lattice("egg_crate")
m = dev.mesh_values(torch.from_numpy(np.array(d)).cuda(), origin, step, shells=True)
torch.cuda.synchronize()
r["mesh_values tensor"] = bool(m.vertices.is_cuda and same(m.shells, want))
keep = np.arange(len(want.records)) % 2 == 0
v, tr, _, _, _ = rule.select(mesh.vertices, mesh.triangles, want, keep)
k = dev.mesh_values(torch.from_numpy(np.array(d)).cuda(), origin, step, keep=torch.from_numpy(keep).cuda())
torch.cuda.synchronize()
r["keep tensor"] = bool(k.triangles.is_cuda and np.array_equal(host(k.triangles), tr) and np.array_equal(host(k.vertices).view(np.uint32), v.view(np.uint32)) and same(k.shells, rule.shells(tr, len(v))))
bad = t.clone(); bad[5, 1] = len(mesh.vertices)
try:
    dev.shells(bad, len(mesh.vertices)); r["refuses an index out of range"] = False
except ft.FrayTracerError as e:
    r["refuses an index out of range"] = e.code == -1
bad = t.clone(); bad[7, 2] = bad[7, 0]
try:
    dev.shells(bad, len(mesh.vertices)); r["refuses an index twice"] = False
except ft.FrayTracerError as e:
    r["refuses an index twice"] = e.code == -1
r["works after the refusals"] = same(dev.shells(t, len(mesh.vertices)), want)
for wrong, why in ((t.long(), "int32"), (t[::2], "contiguous")):
    try:
        dev.shells(wrong, len(mesh.vertices)); r["refuses " + why] = False
    except ValueError as e:
        r["refuses " + why] = why in str(e)
dev.close()
print(json.dumps(r))
"""


def test_tensor_path_in_a_process_that_loads_torch_first():
    """device tensors in, device tensors out, on the caller's stream: in a child process that loads torch before the library"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", TENSOR_PATH], cwd=root, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    failed = [k for k, v in r.items() if v is not True]
    assert not failed, failed
