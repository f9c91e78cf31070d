"""Refinement on the GPU (ft_mesh_lattice_refined, ft_slice_lattice_refined, ft_refine_segments and its device form): bit for bit against the numpy
restatement of the rule (tests/refine_restatement.py) on the CPU oracle's distances — the round kernel alone on special midpoint values, the segment
query, refined meshes and contours with their normals and materials, a second trip for every workgroup, the context's work buffer, the tensor path."""
import ctypes as C

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import _lib
from helpers import assert_bit_equal, glibc_mode, options, options_left_at_defaults  # noqa: F401  (glibc_mode, options_left_at_defaults: fixtures)

import mesh_cases as cases
import refine_cases as rc
import refine_restatement as rule

pytestmark = pytest.mark.gpu

F = np.float32
L = _lib.lib
BLOCK = 256                                # threads per workgroup of the refinement's kernels (ft_refine.h FT_REFINE_BLOCK)
GUARD = 0x5EEDFACE
same_bits = lambda a, b: a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.fixture(scope="module")
def hip():
    h = C.CDLL("libamdhip64.so.7")             # the runtime the library is linked against (already loaded: same instance)
    h.hipMalloc.argtypes, h.hipMemcpy.argtypes, h.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p]
    return h


class GuardedBuffer:
    """a host array's words in device memory between two rows of 64 guard words"""

    def __init__(self, hip, array):
        self.hip = hip
        words = np.ascontiguousarray(array).reshape(-1).view(np.uint32)
        self.n = len(words)
        self.base = C.c_void_p()
        assert hip.hipMalloc(C.byref(self.base), C.c_size_t(4 * (self.n + 128))) == 0
        self.ptr = self.base.value + 256
        host = np.full(self.n + 128, GUARD, np.uint32)
        host[64:64 + self.n] = words
        assert hip.hipMemcpy(self.base, host.ctypes.data_as(C.c_void_p), C.c_size_t(host.nbytes), 1) == 0
        assert hip.hipDeviceSynchronize() == 0

    def read(self, dtype, shape):
        """the words as they are now; asserts that the guard words are"""
        assert self.hip.hipDeviceSynchronize() == 0
        host = np.empty(self.n + 128, np.uint32)
        assert self.hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), self.base, C.c_size_t(host.nbytes), 2) == 0
        assert (host[:64] == GUARD).all() and (host[-64:] == GUARD).all(), "guard words overwritten"
        return host[64:64 + self.n].view(dtype).reshape(shape).copy()

    def free(self):
        assert self.hip.hipFree(self.base) == 0


# ---- the round kernel alone --------------------------------------------------------------------------------------------------------------------

SPECIALS = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, np.inf, -np.inf, np.nan, 3.0e38, -3.0e38], F)
UNTOUCHED = 0xFFFFFFFF


@pytest.mark.parametrize("iso", [0.0, 0.5])
@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097])
def test_one_round_on_special_midpoint_values(gpu, hip, n, last, iso):
    """ft_ctx_refine_round (internal): the rule's non-finite and signed-zero branches, which no scene produces on demand"""
    fn = L.ft_ctx_refine_round
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_int32, C.c_void_p]
    rng = np.random.default_rng(1000 * n + 10 * last + int(iso * 2))
    A, B, M = (rng.uniform(-2.0, 2.0, (n, 3)).astype(F) for _ in range(3))                 # M from the buffer, not recomputed
    mag = rng.uniform(1e-3, 1.5, (2, n)).astype(F)
    a_inside = rng.random(n) < 0.5
    sA, sB = np.where(a_inside, -mag[0], mag[0]).astype(F), np.where(a_inside, mag[1], -mag[1]).astype(F)
    dM = rng.normal(iso, 0.5, n).astype(F)
    special = rng.random(n) < 0.6
    dM[special] = rng.choice(SPECIALS, int(special.sum()))
    dM[rng.random(n) < 0.1] = F(iso)                                                       # sM = +0
    if n >= 63:
        dM[:len(SPECIALS)] = SPECIALS                                                      # every special value reaches the kernel
    old = rule.Brackets(A, B, sA, sB)
    new = rule.round_(old, M, dM, iso)
    state = np.concatenate([A.T.reshape(-1), B.T.reshape(-1), sA, sB])                     # eight arrays of n floats, n apart
    bufs = [GuardedBuffer(hip, state), GuardedBuffer(hip, M), GuardedBuffer(hip, dM), GuardedBuffer(hip, np.full((n, 3), UNTOUCHED, np.uint32))]
    try:
        assert fn(gpu._ctx, bufs[0].ptr, n, bufs[1].ptr, bufs[2].ptr, n, iso, last, bufs[3].ptr) == 0
        got = bufs[0].read(F, (8, n))
        got = rule.Brackets(got[0:3].T, got[3:6].T, got[6], got[7])
        for part, g, w in zip("A B sA sB".split(), got, new):
            assert same_bits(np.ascontiguousarray(g), w), (part, n, last)
        assert same_bits(bufs[2].read(F, (n,)), dM)                                        # the distances are only read
        mid, out = bufs[1].read(F, (n, 3)), bufs[3].read(np.uint32, (n, 3))
        if last:
            assert same_bits(mid, M) and same_bits(out.view(F), rule.finish(new))
        else:
            assert same_bits(mid, rule.midpoint(new.A, new.B)) and (out == UNTOUCHED).all()
    finally:
        for b in bufs:
            b.free()
    stays = ~np.isfinite((dM - F(iso)).astype(F))
    if n >= 63:
        assert stays.any() and (~stays).any()


# ---- segments ------------------------------------------------------------------------------------------------------------------------------

def segment_ends(oracle, name, n, seed):
    """seeded ends: lattice points of the scene's lattice paired at random (crossing, both outside, both inside), some a == b, some with an end far
    outside -> (a, b, the oracle's distances at them)"""
    origin, step, d = cases.oracle_lattice(oracle, name)
    pts = ft.lattice_points(origin, step, cases.COUNTS).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    inside, outside = np.flatnonzero(d.reshape(-1) < 0), np.flatnonzero(d.reshape(-1) > 0)
    pick = lambda idx: pts[rng.choice(idx, n)]
    kind = rng.integers(0, 6, n) if n > 1 else np.zeros(n, np.int64)                       # one segment: a crossing
    jitter = lambda p: (p + rng.uniform(-0.4, 0.4, p.shape).astype(F) * np.asarray(step, F)).astype(F)
    a, b = jitter(pick(outside)), jitter(pick(outside))
    a[kind == 0], b[kind == 1] = pick(inside)[kind == 0], pick(inside)[kind == 1]          # crossing, either end inside
    both = kind == 2
    a[both], b[both] = pick(inside)[both], pick(inside)[both]
    b[kind == 3] = a[kind == 3]                                                            # a == b
    far = kind == 4
    b[far] = (F(100.0) + rng.uniform(0.0, 5.0, (n, 3)).astype(F))[far]                    # far outside: the smooth union is +inf there
    distance = rc.distance_of(oracle, name)
    return np.ascontiguousarray(a), np.ascontiguousarray(b), distance(a), distance(b)


@pytest.mark.parametrize("name", ["c3_64", "console_200"])
def test_segments_host_and_device_forms(gpu, oracle, hip, name):
    ds = gpu.scene(cases.scene_of(name))
    distance = rc.distance_of(oracle, name)
    for n in (0, 1, 65, 1000):
        a, b, dA, dB = segment_ends(oracle, name, n, 40 + n)
        iso = 0.03 if n == 65 else 0.0
        if n == 1000:
            with np.errstate(all="ignore"):
                sA, sB = dA - F(iso), dB - F(iso)
            fin = np.isfinite(sA) & np.isfinite(sB)
            equal = (a == b).all(axis=1)
            assert (fin & ((sA < 0) != (sB < 0))).sum() > 100 and (fin & (sA >= 0) & (sB >= 0) & ~equal).sum() > 100 and (fin & (sA < 0) & (sB < 0)).sum() > 50
            assert equal.sum() > 50
            if name == "c3_64":
                assert (np.isinf(dB) & (dB > 0)).sum() > 50                                # an infinite distance: no bracket, whatever the other end
        for steps in (0, 1, 5, 12):
            want_p, want_s = rule.segments(a, b, dA, dB, distance, iso, steps)
            assert n < 65 or (0 < want_s.sum() < n)
            points, status = ds.refine_segments(a, b, iso=iso, steps=steps)
            assert points.shape == (n, 3) and points.dtype == np.float32 and status.shape == (n,) and status.dtype == np.int32
            assert np.array_equal(status, want_s), (n, steps)
            assert_bit_equal(points, want_p, f"{name} n {n} steps {steps}: points")
            assert np.array_equal(np.isnan(points).all(axis=1), want_s == 0) and np.array_equal(np.isnan(points).any(axis=1), want_s == 0)
            if n == 0:
                continue
            # the device form, each output alone as well
            da, db = GuardedBuffer(hip, a), GuardedBuffer(hip, b)
            dp, dst = GuardedBuffer(hip, np.full((n, 3), UNTOUCHED, np.uint32)), GuardedBuffer(hip, np.full(n, UNTOUCHED, np.uint32))
            try:
                for want_point, want_status in ((True, True), (True, False), (False, True)):
                    ds.refine_segments_device(da.ptr, db.ptr, n, dp.ptr if want_point else None, dst.ptr if want_status else None, iso=iso, steps=steps)
                    if want_point:
                        assert_bit_equal(dp.read(F, (n, 3)), want_p, f"{name} n {n} steps {steps}: device points")
                    if want_status:
                        assert np.array_equal(dst.read(np.int32, (n,)), want_s)
                assert same_bits(da.read(F, (n, 3)), a) and same_bits(db.read(F, (n, 3)), b)       # the inputs are only read
            finally:
                for buf in (da, db, dp, dst):
                    buf.free()
    # other shapes, and SdfForm.crossings
    a, b, dA, dB = segment_ends(oracle, name, 24, 7)
    want_p, want_s = rule.segments(a, b, dA, dB, distance, 0.0, 8)
    points, status = ds.refine_segments(a.reshape(2, 3, 4, 3), b.reshape(2, 3, 4, 3))
    assert points.shape == (2, 3, 4, 3) and status.shape == (2, 3, 4) and np.array_equal(status.reshape(-1), want_s)
    assert_bit_equal(points.reshape(-1, 3), want_p, "leading shape")
    if name == "c3_64":
        form = cases.scene_of(name).Object.kids[1]
        points, status = ft.SdfForm.crossings(form, a, b, 0.0, 8, device=gpu)
        assert np.array_equal(status, want_s)
        assert_bit_equal(points, want_p, "SdfForm.crossings")


# ---- refined meshes ----------------------------------------------------------------------------------------------------------------------------

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
def test_refined_meshes_match_the_restatement_on_the_oracle_distances(gpu, oracle, name):
    origin, step, _ = cases.oracle_lattice(oracle, name)
    ds = gpu.scene(cases.scene_of(name))
    for iso in rc.ISOS:
        plain = ds.mesh_lattice(origin, step, cases.COUNTS, iso=iso)
        for R in (0, 1, 8):
            want = rc.refined(oracle, name, iso, R)
            got = ds.mesh_lattice(origin, step, cases.COUNTS, iso=iso, refine=R)
            assert got.vertices.dtype == np.float32 and same_bits(got.vertices, want), (name, iso, R)
            assert np.array_equal(got.triangles, plain.triangles) and got.skipped == plain.skipped and got.normal is None and got.material is None
            if R == 0:
                assert same_bits(got.vertices, plain.vertices)                             # no round: ft_mesh_lattice's vertices
            else:
                assert not same_bits(got.vertices, plain.vertices)
    # normals and materials are taken at the refined positions
    want = rc.refined(oracle, name, 0.0, 8)
    got = ds.mesh_lattice(origin, step, cases.COUNTS, normal_epsilon=cases.NORMAL_EPS, material=True, refine=8)
    assert same_bits(got.vertices, want)
    pts = ds.sample_points(got.vertices, normal_epsilon=cases.NORMAL_EPS, material=True)
    assert_bit_equal(got.normal, pts.normal, name + ": normal against sample_points")
    assert np.array_equal(got.material, pts.material) and got.material.dtype == np.int32 and (got.material >= 0).all()
    nrm, col = oracle_at(oracle, name, np.array(want), cases.NORMAL_EPS)
    assert_bit_equal(got.normal, nrm, name + ": normal")
    assert_bit_equal(material_colors(got), col, name + ": material colour")
    unrefined = ds.mesh_lattice(origin, step, cases.COUNTS, normal_epsilon=cases.NORMAL_EPS)
    assert not same_bits(got.normal, unrefined.normal)
    for opt, values in (("cull", (0, 1)), ("carved", (0, 1)), ("max_blocks_per_cu", (1, 3))):
        for v in values:
            with options(gpu, **{opt: v}):
                other = ds.mesh_lattice(origin, step, cases.COUNTS, normal_epsilon=cases.NORMAL_EPS, material=True, refine=8)
            assert same_bits(other.vertices, want) and np.array_equal(other.triangles, got.triangles), (opt, v)
            assert_bit_equal(other.normal, got.normal, f"{name} {opt} = {v}: normal")
            assert np.array_equal(other.material, got.material), (opt, v)


def test_refined_mesh_under_the_glibc_arithmetic(gpu, oracle, glibc_mode):
    origin, step, _ = cases.oracle_lattice(oracle, "c3_64", libm=True)                     # formed under the oracle's libm switch (glibc_mode holds it)
    want = rc.refined(oracle, "c3_64", 0.0, 8, None, True)
    got = gpu.scene(cases.scene_of("c3_64")).mesh_lattice(origin, step, cases.COUNTS, normal_epsilon=cases.NORMAL_EPS, refine=8)
    assert same_bits(got.vertices, want)
    nrm, _ = oracle_at(oracle, "c3_64", np.array(want), cases.NORMAL_EPS)
    assert_bit_equal(got.normal, nrm, "glibc: normal")


def test_sdf_form_passes_refine_through(gpu, oracle):
    origin, step, _ = cases.oracle_lattice(oracle, "c3_64")
    form = cases.scene_of("c3_64").Object.kids[1]
    assert same_bits(ft.SdfForm.mesh(form, origin, step, cases.COUNTS, device=gpu, refine=8).vertices, rc.refined(oracle, "c3_64", 0.0, 8))
    got = ft.SdfForm.slice(form, origin, step, cases.COUNTS, axis=1, device=gpu, refine=8)
    assert same_bits(got.points, rc.refined(oracle, "c3_64", 0.0, 8, 1)[rc.slice_order(oracle, "c3_64", 0.0, 1)])


# ---- refined contours --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("axis", [0, 1, 2])
def test_refined_contours_match_the_restatement(gpu, oracle, axis):
    name = "c3_64"
    origin, step, _ = cases.oracle_lattice(oracle, name)
    ds = gpu.scene(cases.scene_of(name))
    for iso in rc.ISOS:
        plain = ds.slice_lattice(origin, step, cases.COUNTS, axis=axis, iso=iso)
        order = rc.slice_order(oracle, name, iso, axis)
        assert len(order) == len(plain.points) >= 100
        for R in (0, 8):
            got = ds.slice_lattice(origin, step, cases.COUNTS, axis=axis, iso=iso, refine=R)
            assert same_bits(got.points, rc.refined(oracle, name, iso, R, axis)[order]), (axis, iso, R)
            assert np.array_equal(got.polylines, plain.polylines) and (got.closed, got.skipped, got.axis, got.slices) == (plain.closed, plain.skipped, plain.axis, plain.slices)
            assert same_bits(got.points, plain.points) == (R == 0)                         # no round: ft_slice_lattice's points
    got = ds.slice_lattice(origin, step, cases.COUNTS, axis=axis, normal_epsilon=cases.NORMAL_EPS, material=True, refine=8)
    pts = ds.sample_points(got.points, normal_epsilon=cases.NORMAL_EPS, material=True)
    assert_bit_equal(got.normal, pts.normal, "normal against sample_points")
    assert np.array_equal(got.material, pts.material)


# ---- every workgroup comes back --------------------------------------------------------------------------------------------------------------------

def test_every_workgroup_takes_a_second_trip(gpu, oracle):
    """with one workgroup per CU (FT_OPT_MAX_BLOCKS_PER_CU = 1; 256 CUs) the refinement's kernels run 256 workgroups of 256 lanes: more than 65 536
    vertices bring every workgroup of the round kernel back, and the 88^3 lattice points every workgroup of the bracket kernel, 10 times"""
    name, counts, iso, R = "console_200", (88, 88, 88), 0.0, 2
    O, _, form = rc.form_of(oracle, name)
    origin, step = cases.lattice_around(O.form_boundary(form), cases.SPAN, counts)
    distance = rc.distance_of(oracle, name)
    d = distance(ft.lattice_points(origin, step, counts).reshape(-1, 3)).reshape(counts)
    br, _ = rule.lattice_brackets(d, origin, step, iso)
    assert len(br.sA) > 256 * BLOCK and d.size > 2 * 256 * BLOCK                            # from the restatement's count
    want = rule.bisect(*br, distance, iso, R)
    ds = gpu.scene(cases.scene_of(name))
    with options(gpu, max_blocks_per_cu=1):
        got = ds.mesh_lattice(origin, step, counts, iso=iso, refine=R)
    assert same_bits(got.vertices, want)
    plain = ds.mesh_lattice(origin, step, counts, iso=iso)
    assert np.array_equal(got.triangles, plain.triangles) and same_bits(plain.vertices, rule.finish(br))


# ---- the context's work buffer, lifetimes ------------------------------------------------------------------------------------------------------

def read_vertices(handle):
    info = _lib.MeshInfo()
    assert L.ft_mesh_get_info(handle, C.byref(info)) == 0
    v = np.empty((info.n_vertices, 3), F)
    assert L.ft_mesh_read(handle, v.ctypes.data_as(C.c_void_p), None, None, None) == 0
    return v


def test_the_work_buffer_grows_and_is_reused(oracle):
    """large, then small, then large on one fresh context; two refined results alive at once, destroyed in either order"""
    name = "console_200"
    origin, step, _ = cases.oracle_lattice(oracle, name)
    want = rc.refined(oracle, name, 0.0, 8)
    small_counts = (6, 5, 7)
    O, _, form = rc.form_of(oracle, name)
    small_origin, small_step = cases.lattice_around(O.form_boundary(form), cases.SPAN, small_counts)
    distance = rc.distance_of(oracle, name)
    small_d = distance(ft.lattice_points(small_origin, small_step, small_counts).reshape(-1, 3)).reshape(small_counts)
    small_br, _ = rule.lattice_brackets(small_d, small_origin, small_step, 0.0)
    small_want = rule.bisect(*small_br, distance, 0.0, 8)
    assert 0 < len(small_want) < len(want) // 4
    dev = ft.Device(0)
    try:
        ds = dev.scene(cases.scene_of(name))
        for counts, o, s, w in ((cases.COUNTS, origin, step, want), (small_counts, small_origin, small_step, small_want), (cases.COUNTS, origin, step, want),
                                (small_counts, small_origin, small_step, small_want)):
            assert same_bits(ds.mesh_lattice(o, s, counts, refine=8).vertices, w)
            assert same_bits(ds.slice_lattice(origin, step, cases.COUNTS, axis=2, refine=8).points,
                             rc.refined(oracle, name, 0.0, 8, 2)[rc.slice_order(oracle, name, 0.0, 2)])
        # a segment query in between uses the same buffer
        points, status = ds.refine_segments(small_br.A, small_br.B)
        assert status.all() and same_bits(points, small_want)
        for order in ((0, 1), (1, 0)):
            handles = []
            for counts, o, s in ((cases.COUNTS, origin, step), (small_counts, small_origin, small_step)):
                lat, _ = ft.api._lattice(o, s, counts)
                h = C.c_void_p()
                assert L.ft_mesh_lattice_refined(dev._ctx, ds._scene, C.byref(lat), 0.0, 0.0, 0, 8, C.byref(h)) == 0
                handles.append(h)
            wants = (want, small_want)
            first, second = order
            assert same_bits(read_vertices(handles[second]), wants[second])                # each is whole while the other lives ...
            L.ft_mesh_destroy(handles[first])
            assert same_bits(read_vertices(handles[second]), wants[second])                # ... and after it is gone
            L.ft_mesh_destroy(handles[second])
    finally:
        dev.close()


TENSOR_PATH = r"""
import json, sys
import numpy as np
import torch                              # before the library: torch's HIP runtime is the one the process loads first
import fraytracer_amd as ft
sys.path.insert(0, "tests")
import mesh_cases as cases
same = lambda t, a: bool(np.array_equal(np.ascontiguousarray(t.detach().cpu().numpy()).view(np.uint32), np.ascontiguousarray(a).view(np.uint32)))
dev = ft.Device(0)
r = {}
ds = dev.scene(cases.scene_of("c3_64"))
origin, step = cases.lattice_around(ds.boundary(), cases.SPAN, cases.COUNTS)
t = torch.zeros(4, device="cuda")
host = ds.mesh_lattice(origin, step, cases.COUNTS, normal_epsilon=cases.NORMAL_EPS, material=True, refine=8)
like = ds.mesh_lattice(origin, step, cases.COUNTS, normal_epsilon=cases.NORMAL_EPS, material=True, like=t, refine=8)
torch.cuda.synchronize()
r["mesh like"] = like.vertices.is_cuda and same(like.vertices, host.vertices) and same(like.triangles, host.triangles) and same(like.normal, host.normal) and same(like.material, host.material)
r["mesh moved"] = not same(like.vertices, ds.mesh_lattice(origin, step, cases.COUNTS).vertices)
hs = ds.slice_lattice(origin, step, cases.COUNTS, axis=0, refine=8)
ls = ds.slice_lattice(origin, step, cases.COUNTS, axis=0, like=t, refine=8)
torch.cuda.synchronize()
r["slice like"] = ls.points.is_cuda and same(ls.points, hs.points) and same(ls.polylines, hs.polylines)
side = torch.cuda.Stream()                # segments on a side stream, behind the torch kernels that make the ends
side.wait_stream(torch.cuda.current_stream())
rng = np.random.default_rng(3)
a = (np.asarray(origin, np.float32) + rng.uniform(0, 1, (300, 3)).astype(np.float32) * np.asarray(step, np.float32) * (np.asarray(cases.COUNTS, np.float32) - 1)).astype(np.float32)
b = a[::-1].copy()
hp, hst = ds.refine_segments(a, b, steps=6)
with torch.cuda.stream(side):
    ta, tb = torch.from_numpy(a).cuda() * 1.0, torch.from_numpy(b).cuda() * 1.0
    tp, tst = ds.refine_segments(ta, tb, steps=6)
side.synchronize()
r["segments"] = tp.is_cuda and tst.dtype == torch.int32 and same(tst, hst) and bool(hst.any()) and not bool(hst.all())
r["segment points"] = bool(np.array_equal(np.isnan(tp.cpu().numpy()), np.isnan(hp))) and same(torch.nan_to_num(tp), np.nan_to_num(hp))
r["inputs unchanged"] = same(ta, a) and same(tb, b)
for bad, why in (((ta.double(), tb.double()), "float32"), ((ta[::2], tb[::2]), "contiguous"), ((ta, tb[:10]), "shapes differ"), ((ta, b), "both ends")):
    try:
        ds.refine_segments(*bad)
        r["refuses " + why] = False
    except ValueError as e:
        r["refuses " + why] = why in str(e)
dev.close()
print(json.dumps(r))
"""


def test_tensor_path_in_a_process_that_loads_torch_first():
    """like= and device tensors, on the caller's stream: in a child process that loads torch before the library"""
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
