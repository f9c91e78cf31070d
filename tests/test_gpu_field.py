"""Sampling the distance field on the device (ft_sample_points, ft_sample_lattice and their *_device forms) on the GPU: distance, normal and
material, bit for bit against the CPU oracle, over every kernel family, the lattice shapes that leave bricks part-filled, the points form,
the agreement of the entries with each other and with ft_eval_distance, the options, edge points, FT_FIELD_BOUNDED and the glibc arithmetic."""
import ctypes as C
import functools

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import _lib
from fraytracer_amd import synthetic as syn
from helpers import assert_bit_equal, glibc_mode, options, options_left_at_defaults  # noqa: F401  (glibc_mode, options_left_at_defaults: fixtures)

pytestmark = pytest.mark.gpu

F = np.float32
NORMAL_EPS = 0.00125
COUNTS = (21, 18, 23)                      # 8 694 points; no count is a multiple of a brick edge (2, 4, 8, 16)

# name -> (scene, half-width of the lattice in boundary radii).  The condition on the inputs, asserted below on the oracle's values alone: at
# least 3 % of the points inside the form and at least 50 % outside.  Every scene meets it at 0.6 (inside: 5.2, 47.4, 10.2, 26.7, 6.5, 3.8, 9.7,
# 4.6, 7.4 and 5.6 % in the order below; c3_300 has 52.6 % outside).
SCENES = {
    "c3_64": (lambda: syn.config3(n=64)[0], 0.6),                                          # lean
    "c3_300": (lambda: syn.config3(n=300)[0], 0.6),                                        # lean, the run's tail beyond FT_CULL_MAX
    "console_200": (lambda: syn.console_scene(n=200)[0], 0.6),                             # carved tori
    "like_spheres": (lambda: syn.console_like(n=120, factory=syn.random_sphere)[0], 0.6),  # carved spheres
    "like_capsules": (lambda: syn.console_like(n=120, factory=syn.random_capsule)[0], 0.6),
    "like_triangles": (lambda: syn.console_like(n=120, factory=syn.random_triangle)[0], 0.6),
    "c2_boxes": (lambda: syn.config2(boxes=True)[0], 0.6),                                 # mixed kinds
    "mixed_nested": (lambda: syn.mixed_nested()[0], 0.6),                                  # general, on-demand calls
    "combinator_zoo": (lambda: syn.combinator_zoo()[0], 0.6),
    "config5": (lambda: syn.config5()[0], 0.6),
}
SINGLE_MATERIAL = {"c3_64", "c3_300"}


@functools.lru_cache(maxsize=None)
def scene_of(name):
    return SCENES[name][0]()


def lattice_around(boundary, span, counts):
    """origin and step of a lattice of `counts` points over +-span boundary radii around the boundary's centre"""
    c, r = np.asarray(boundary[0:3], F), F(boundary[3])
    origin = c - F(span) * r
    step = (F(2.0 * span) * r / (np.asarray(counts, F) - F(1.0))).astype(F) if min(counts) > 1 else np.full(3, F(0.1))
    return tuple(float(v) for v in origin), tuple(float(v) for v in step)


def numpy_normal(dx, dy, dz, d):
    """SdfForm.normal from its four evaluations, as the header states it, in float32"""
    with np.errstate(all="ignore"):
        g = np.stack([dx - d, dy - d, dz - d], axis=-1).astype(F)
        return (g / np.sqrt((g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2])[..., None]).astype(F)


def oracle_field(oracle, os_, pts, eps=None, colors=False):
    """distance, normal (eps given) and colour per point of pts [n, 3] from the CPU oracle: one evaluation per call"""
    O = oracle.Oracle()
    form = O.object_form(os_.object)
    with np.errstate(all="ignore"):
        d = O.form_distance(form, pts)
        nrm = None
        if eps is not None:
            probes = []
            for a in range(3):
                q = pts.copy()
                q[:, a] = pts[:, a] + F(eps)
                probes.append(O.form_distance(form, q))
            nrm = numpy_normal(*probes, d)
    col = np.array([O.object_color(os_.object, p) for p in pts], F) if colors else None
    return d, nrm, col


@functools.lru_cache(maxsize=None)
def reference(oracle, name):
    """the family lattice of a scene and the oracle's values on it: computed once, shared, never written to"""
    scene, span = scene_of(name), SCENES[name][1]
    os_ = oracle.Oracle().scene(scene)
    O = oracle.Oracle()
    origin, step = lattice_around(O.form_boundary(O.object_form(os_.object)), span, COUNTS)
    pts = ft.lattice_points(origin, step, COUNTS).reshape(-1, 3)
    d, nrm, col = oracle_field(oracle, os_, pts, NORMAL_EPS, colors=True)
    for a in (pts, d, nrm, col):
        a.setflags(write=False)
    return origin, step, pts, d, nrm, col


def material_colors(samples):
    """the colour of descriptor(handle) per point, float32 [..., 3]"""
    handles = np.asarray(samples.material)
    out = np.empty(handles.shape + (3,), F)
    for h in np.unique(handles):
        out[handles == h] = np.asarray(samples.descriptor(h).args[0], F)
    return out


@pytest.mark.parametrize("name", list(SCENES))
def test_family_lattice_matches_the_oracle(gpu, oracle, name):
    origin, step, pts, d, nrm, col = reference(oracle, name)
    inside, outside = float((d < 0).mean()), float((d > 0).mean())
    print(f"{name}: {inside:.3f} of the points inside, {outside:.3f} outside")
    assert inside >= 0.03 and outside >= 0.5, (name, inside, outside)                      # a condition on the inputs, from the oracle alone
    ds = gpu.scene(scene_of(name))
    got = ds.sample_lattice(origin, step, COUNTS, normal_epsilon=NORMAL_EPS, material=True)
    assert got.distance.shape == COUNTS and got.normal.shape == COUNTS + (3,) and got.material.shape == COUNTS and got.material.dtype == np.int32
    assert_bit_equal(got.distance.reshape(-1), d, name + " distance")
    assert_bit_equal(got.normal.reshape(-1, 3), nrm, name + " normal")
    assert (got.material >= 0).all()
    assert_bit_equal(material_colors(got).reshape(-1, 3), col, name + " material colour")
    if name not in SINGLE_MATERIAL:
        assert len(np.unique(got.material)) >= 2, name


@pytest.mark.parametrize("counts", [(1, 1, 1), (1, 70, 1), (5, 1, 130), (3, 3, 3), (64, 4, 4)])
@pytest.mark.parametrize("name", ["c3_64", "console_200", "mixed_nested"])
def test_small_lattices(gpu, oracle, name, counts):
    os_ = oracle.Oracle().scene(scene_of(name))
    ds = gpu.scene(scene_of(name))
    origin, step = lattice_around(ds.boundary(), 0.5, counts)
    pts = ft.lattice_points(origin, step, counts).reshape(-1, 3)
    d, nrm, col = oracle_field(oracle, os_, pts, NORMAL_EPS, colors=True)
    got = ds.sample_lattice(origin, step, counts, normal_epsilon=NORMAL_EPS, material=True)
    assert got.distance.shape == counts
    assert_bit_equal(got.distance.reshape(-1), d, "distance")
    assert_bit_equal(got.normal.reshape(-1, 3), nrm, "normal")
    assert_bit_equal(material_colors(got).reshape(-1, 3), col, "material colour")


def test_grid_stride_every_workgroup_takes_a_second_brick(gpu, oracle):
    """48 x 40 x 44 = 84 480 points are 1 320 bricks of 4 x 4 x 4 and 1 440 of either other shape: with one workgroup of four waves per CU
    (256 CUs: 1 024 waves) every workgroup comes back for more"""
    counts = (48, 40, 44)
    os_ = oracle.Oracle().scene(scene_of("c3_64"))
    ds = gpu.scene(scene_of("c3_64"))
    origin, step = lattice_around(ds.boundary(), 0.6, counts)
    pts = ft.lattice_points(origin, step, counts).reshape(-1, 3)
    d, _, _ = oracle_field(oracle, os_, pts)
    with options(gpu, max_blocks_per_cu=1):
        got = ds.sample_lattice(origin, step, counts)
    assert got.normal is None and got.material is None
    assert_bit_equal(got.distance.reshape(-1), d, "grid-stride distance")


@pytest.mark.parametrize("name", ["c3_64", "console_200", "mixed_nested"])
def test_points_form_and_agreement_between_the_entries(gpu, oracle, name):
    origin, step, pts, d, nrm, col = reference(oracle, name)
    ds = gpu.scene(scene_of(name))
    lat = ds.sample_lattice(origin, step, COUNTS, normal_epsilon=NORMAL_EPS, material=True)
    for n in (1, 63, 64, 65, len(pts)):
        got = ds.sample_points(pts[:n], normal_epsilon=NORMAL_EPS, material=True)
        assert got.distance.shape == (n,) and got.normal.shape == (n, 3) and got.material.shape == (n,)
        assert_bit_equal(got.distance, d[:n], f"{n} points: distance")
        assert_bit_equal(got.normal, nrm[:n], f"{n} points: normal")
        assert np.array_equal(got.material, lat.material.reshape(-1)[:n])
    # sample_points on lattice_points(...) = sample_lattice, and both = eval_distance in the distance
    assert_bit_equal(got.distance, lat.distance.reshape(-1), "points against lattice")
    assert_bit_equal(got.normal, lat.normal.reshape(-1, 3), "points against lattice: normal")
    assert_bit_equal(ds.eval_distance(pts)[0], lat.distance.reshape(-1), "ft_eval_distance against lattice")
    # each subset of the outputs gives the bits of all three together
    for dist, eps, mat in ((True, None, False), (False, NORMAL_EPS, False), (False, None, True), (True, NORMAL_EPS, False), (True, None, True), (False, NORMAL_EPS, True)):
        for sub, whole in ((ds.sample_lattice(origin, step, COUNTS, normal_epsilon=eps, material=mat, distance=dist), lat),
                           (ds.sample_points(pts, normal_epsilon=eps, material=mat, distance=dist), got)):
            assert (sub.distance is not None, sub.normal is not None, sub.material is not None) == (dist, eps is not None, mat)
            if dist:
                assert_bit_equal(sub.distance, whole.distance, "subset: distance")
            if eps is not None:
                assert_bit_equal(sub.normal, whole.normal, "subset: normal")
            if mat:
                assert np.array_equal(sub.material, whole.material)
    # a leading shape is kept
    boxed = ds.sample_points(pts[:60].reshape(4, 15, 3), normal_epsilon=NORMAL_EPS)
    assert boxed.distance.shape == (4, 15) and boxed.normal.shape == (4, 15, 3)
    assert_bit_equal(boxed.distance.reshape(-1), d[:60], "leading shape")


GUARD = 0x5EEDFACE


class GuardedBuffer:
    """n_words 4-byte words of device memory between two rows of 64 guard words, from the HIP runtime the library is linked against"""

    def __init__(self, hip, n_words, fill=None):
        self.hip, self.n = hip, n_words
        self.base = C.c_void_p()
        assert hip.hipMalloc(C.byref(self.base), C.c_size_t(4 * (n_words + 128))) == 0
        self.ptr = self.base.value + 256
        self.reset(fill)

    def reset(self, fill=None):
        host = np.full(self.n + 128, GUARD, np.uint32)
        host[64:64 + self.n] = 0xFFFFFFFF if fill is None else np.ascontiguousarray(fill).view(np.uint32).reshape(-1)
        assert self.hip.hipMemcpy(self.base, host.ctypes.data_as(C.c_void_p), C.c_size_t(host.nbytes), 1) == 0      # host to device
        assert self.hip.hipDeviceSynchronize() == 0

    def read(self, dtype):
        """(the words in between as dtype, guards intact)"""
        host = np.empty(self.n + 128, np.uint32)
        assert self.hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), self.base, C.c_size_t(host.nbytes), 2) == 0      # device to host
        return host[64:64 + self.n].view(dtype), bool((host[:64] == GUARD).all() and (host[-64:] == GUARD).all())

    def free(self):
        assert self.hip.hipFree(self.base) == 0


@pytest.mark.parametrize("name", ["c3_64", "console_200", "mixed_nested"])
def test_device_forms_equal_host_forms_and_stay_inside_their_buffers(gpu, oracle, name):
    origin, step, pts, d, nrm, col = reference(oracle, name)
    ds = gpu.scene(scene_of(name))
    n = len(pts)
    host = ds.sample_lattice(origin, step, COUNTS, normal_epsilon=NORMAL_EPS, material=True)
    hip = C.CDLL("libamdhip64.so.7")           # the runtime the library is linked against (already loaded: same instance)
    hip.hipMalloc.argtypes, hip.hipMemcpy.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p]
    dpts = GuardedBuffer(hip, 3 * n, pts)
    bufs = [GuardedBuffer(hip, n), GuardedBuffer(hip, 3 * n), GuardedBuffer(hip, n)]
    try:
        for launch in ("lattice", "points", "points, distance only"):
            for b in bufs:
                b.reset()
            ptrs = [b.ptr for b in bufs] if launch != "points, distance only" else [bufs[0].ptr, None, None]
            if launch == "lattice":
                ds.sample_lattice_device(origin, step, COUNTS, *ptrs, normal_epsilon=NORMAL_EPS)
            else:
                ds.sample_points_device(dpts.ptr, n, *ptrs, normal_epsilon=NORMAL_EPS)
            ds.collect_stats()                                                             # synchronises the context's stream
            (gd, ok0), (gn, ok1), (gm, ok2) = bufs[0].read(np.float32), bufs[1].read(np.float32), bufs[2].read(np.int32)
            assert ok0 and ok1 and ok2 and dpts.read(np.float32)[1], launch
            assert_bit_equal(gd, host.distance.reshape(-1), launch + ": device distance")
            if ptrs[1] is None:                                                            # what was not asked for is not written
                assert (gn.view(np.uint32) == 0xFFFFFFFF).all() and (gm == -1).all()
                continue
            assert_bit_equal(gn.reshape(-1, 3), host.normal.reshape(-1, 3), launch + ": device normal")
            assert np.array_equal(gm, host.material.reshape(-1)), launch
    finally:
        for b in bufs + [dpts]:
            b.free()


def test_host_field_forms_leave_pending_statistics_alone():
    """ft_sample_lattice and ft_sample_points return no statistics and collect none: a frame launched before them and not yet collected is still
    there, whole, in the next collect_stats — every ray, hit, evaluation and flag counter of the same frame collected on its own (a field launch
    counts nothing: FtFieldArgs has no statistics block), and a kernel time (the field launches' event pairs are added to it)."""
    counters = ("rays_primary", "rays_shadow", "rays_ext", "hits_primary", "hits_shadow", "sdf_evals", "wave_evals", "flags")
    hip = C.CDLL("libamdhip64.so.7")           # the runtime the library is linked against (already loaded: same instance)
    hip.hipMalloc.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]

    def frame_stats(sample_between):
        """a 16 x 16 frame on a context and scene of its own (nothing pending, no tile order from an earlier frame), collected at the end"""
        dev = ft.Device(0)
        frame = C.c_void_p()
        assert hip.hipMalloc(C.byref(frame), C.c_size_t(16 * 16 * 12)) == 0
        try:
            ds = dev.scene(syn.config3(n=8)[0])
            ds.render_device(syn.EPSILON, syn.RAY_LENGTH, ft.ImageSize(16, 16), syn.default_camera(), frame.value)
            if sample_between:
                origin, step = lattice_around(ds.boundary(), 0.5, (2, 3, 4))
                lat = ds.sample_lattice(origin, step, (2, 3, 4), normal_epsilon=NORMAL_EPS, material=True)
                pts = ds.sample_points(ft.lattice_points(origin, step, (2, 3, 4)).reshape(-1, 3)[:5], normal_epsilon=NORMAL_EPS, material=True)
                assert_bit_equal(pts.distance, lat.distance.reshape(-1)[:5], "the two forms on the same points")
            return ds.collect_stats()
        finally:
            dev.close()
            assert hip.hipFree(frame) == 0

    alone, after = frame_stats(False), frame_stats(True)
    assert alone["rays_primary"] == 256 and alone["kernel_ms"] > 0.0
    assert {k: after[k] for k in counters} == {k: alone[k] for k in counters}
    assert after["kernel_ms"] > 0.0


TENSOR_PATH = r"""
import json, sys
import numpy as np
import torch                              # before the library: torch's HIP runtime is the one the process loads first
import fraytracer_amd as ft
sys.path.insert(0, "tests")
import test_gpu_field as T
bits = lambda t: np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t).view(np.uint32)
same = lambda t, a: bool(np.array_equal(bits(t), bits(a)))
dev = ft.Device(0)
res = []
for name in ("c3_64", "console_200", "mixed_nested"):
    ds = dev.scene(T.scene_of(name))
    origin, step = T.lattice_around(ds.boundary(), 0.6, T.COUNTS)
    pts = ft.lattice_points(origin, step, T.COUNTS)
    host = ds.sample_lattice(origin, step, T.COUNTS, normal_epsilon=T.NORMAL_EPS, material=True)
    dpts = torch.from_numpy(pts).cuda()
    r = {"scene": name}
    side = torch.cuda.Stream()            # on a side stream, behind the torch kernel that makes the points: the stream hand-over
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        moved = dpts * 1.0
        t = ds.sample_points(moved, normal_epsilon=T.NORMAL_EPS, material=True, bounded=True)
        u = ds.sample_points(moved, normal_epsilon=T.NORMAL_EPS, material=True)
    side.synchronize()
    r["tensor_types"] = t.distance.is_cuda and tuple(t.distance.shape) == T.COUNTS and tuple(t.normal.shape) == T.COUNTS + (3,) and t.material.dtype == torch.int32
    r["points: distance"], r["points: normal"], r["points: material"] = same(u.distance, host.distance), same(u.normal, host.normal), same(u.material, host.material)
    hb = ds.sample_lattice(origin, step, T.COUNTS, normal_epsilon=T.NORMAL_EPS, material=True, bounded=True)
    r["bounded"] = same(t.distance, hb.distance) and same(t.normal, hb.normal) and same(t.material, hb.material)
    tl = ds.sample_lattice(origin, step, T.COUNTS, like=dpts)               # torch's default stream: the side-stream path of on_current_stream
    torch.cuda.synchronize()
    r["lattice like"] = tl.distance.is_cuda and tl.normal is None and tl.material is None and same(tl.distance, host.distance)
    empty = ds.sample_points(dpts[:0, 0, 0], normal_epsilon=T.NORMAL_EPS)
    r["empty"] = tuple(empty.distance.shape) == (0,) and tuple(empty.normal.shape) == (0, 3)
    for bad, why in ((dpts.double(), "float32"), (dpts[..., :2].contiguous(), "[..., 3]"), (dpts[::2], "contiguous")):
        try:
            ds.sample_points(bad)
            r["refuses " + why] = False
        except ValueError as e:
            r["refuses " + why] = why in str(e)
    res.append(r)
dev.close()
print(json.dumps(res))
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
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert len(res) == 3
    for r in res:
        failed = [k for k, v in r.items() if k != "scene" and v is not True]
        assert not failed, (r["scene"], failed)


@pytest.mark.parametrize("name", ["c3_64", "console_200", "combinator_zoo"])
def test_options_change_no_bit(gpu, oracle, name):
    origin, step, pts, d, nrm, col = reference(oracle, name)
    ds = gpu.scene(scene_of(name))
    base = ds.sample_lattice(origin, step, COUNTS, normal_epsilon=NORMAL_EPS, material=True)
    for opt in ("cull", "carved", "lazy_union"):
        for v in (0, 1):
            with options(gpu, **{opt: v}):
                got = ds.sample_lattice(origin, step, COUNTS, normal_epsilon=NORMAL_EPS, material=True)
                pt = ds.sample_points(pts, normal_epsilon=NORMAL_EPS)
            assert_bit_equal(got.distance, base.distance, f"{opt} = {v}: distance")
            assert_bit_equal(got.normal, base.normal, f"{opt} = {v}: normal")
            assert np.array_equal(got.material, base.material), (opt, v)
            assert_bit_equal(pt.distance, base.distance.reshape(-1), f"{opt} = {v}: points")
    assert_bit_equal(base.distance.reshape(-1), d, "distance")
    brick = _lib.lib.ft_ctx_field_brick                                                    # internal: every brick shape gives the same bits
    brick.restype, brick.argtypes = C.c_int, [C.c_void_p, C.c_int32]
    try:
        for shape in (0, 1, 2):
            assert brick(gpu._ctx, shape) == 0
            got = ds.sample_lattice(origin, step, COUNTS, normal_epsilon=NORMAL_EPS, material=True)
            assert_bit_equal(got.distance, base.distance, f"brick {shape}: distance")
            assert_bit_equal(got.normal, base.normal, f"brick {shape}: normal")
            assert np.array_equal(got.material, base.material), shape
    finally:
        brick(gpu._ctx, -1)                                                                # the shipped rule


def first_sphere_centre(scene):
    node = scene.Object
    while node.kind != "sphere":
        node = [k for k in node.kids if not isinstance(k, ft.api.Material)][0]
    return np.asarray(node.args[0], F)


@pytest.mark.parametrize("name", ["c3_64", "mixed_nested"])
def test_edge_points(gpu, oracle, name):
    scene = scene_of(name)
    os_ = oracle.Oracle().scene(scene)
    ds = gpu.scene(scene)
    c = first_sphere_centre(scene)
    near = [c + F(s) * e for s in (1e-6, -1e-6) for e in np.eye(3, dtype=F)]
    odd = [[np.nan, 0, 0], [0, np.nan, 0], [np.nan] * 3, [np.inf, 0, 0], [0, -np.inf, 0], [np.inf, np.inf, -np.inf], [1e30, 0, 0], [1e30, -1e30, 1e30], [0, 0, 25.9]]
    pts = np.array([c] + near + odd + [c], F)
    for eps in (NORMAL_EPS, 0.0, 1e-30, 10.0):
        d, nrm, col = oracle_field(oracle, os_, pts, eps, colors=True)
        got = ds.sample_points(pts, normal_epsilon=eps, material=True)
        assert_bit_equal(got.distance, d, f"edge points, eps {eps}: distance")
        assert_bit_equal(got.normal, nrm, f"edge points, eps {eps}: normal")
        assert (got.material >= 0).all()
        ok = ~np.isnan(pts).any(axis=1)                                                    # a NaN point has no argmin worth comparing
        assert_bit_equal(material_colors(got)[ok], col[ok], f"edge points, eps {eps}: colour")
        one = ds.sample_points(pts[:1], normal_epsilon=eps)                                # the centre alone: 63 lanes on a copy of it
        assert_bit_equal(one.distance, d[:1], "one point")
        assert_bit_equal(one.normal, nrm[:1], "one point: normal")
    # lattices: far away (the smooth union is +inf there, the normal NaN), step 0 (64 equal points: rho = 0), a negative step
    for origin, step, counts in (((100.0, 100.0, 100.0), (0.05, 0.05, 0.05), (5, 6, 7)), (tuple(float(v) for v in c), (0.0, 0.0, 0.0), (4, 4, 4)),
                                 (tuple(float(v) for v in c + F(0.3)), (0.0, 0.0, 0.0), (3, 5, 9)), ((1.0, 1.5, 2.0), (-0.11, -0.07, -0.13), (9, 10, 11)),
                                 ((-1.0, 0.5, 0.0), (0.2, 0.0, -0.1), (6, 3, 17))):
        pts = ft.lattice_points(origin, step, counts).reshape(-1, 3)
        d, nrm, _ = oracle_field(oracle, os_, pts, NORMAL_EPS)
        got = ds.sample_lattice(origin, step, counts, normal_epsilon=NORMAL_EPS, material=True)
        assert_bit_equal(got.distance.reshape(-1), d, f"lattice at {origin} step {step}: distance")
        assert_bit_equal(got.normal.reshape(-1, 3), nrm, f"lattice at {origin} step {step}: normal")
        if name == "c3_64" and origin[0] == 100.0:
            assert np.isinf(d).all() and (d > 0).all() and np.isnan(nrm).all()


@pytest.mark.parametrize("name", ["c3_64", "console_200", "mixed_nested"])
def test_bounded_is_try_distance(gpu, oracle, name):
    scene = scene_of(name)
    os_ = oracle.Oracle().scene(scene)
    ds = gpu.scene(scene)
    b = ds.boundary()
    origin, step = lattice_around(b, 1.1, COUNTS)
    pts = ft.lattice_points(origin, step, COUNTS).reshape(-1, 3)
    diff = pts - np.asarray(b[0:3], F)
    inside = ((diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]) < F(b[3]) * F(b[3])
    share = float(inside.mean())
    print(f"{name}: {share:.3f} of the points inside the boundary sphere")
    assert 0.2 <= share <= 0.8                                                             # pi / 6 / 1.1^3 = 0.39 by geometry
    d, nrm, col = oracle_field(oracle, os_, pts[inside], NORMAL_EPS, colors=True)
    for got in (ds.sample_lattice(origin, step, COUNTS, normal_epsilon=NORMAL_EPS, material=True, bounded=True),
                ds.sample_points(pts, normal_epsilon=NORMAL_EPS, material=True, bounded=True)):
        gd, gn, gm = got.distance.reshape(-1), got.normal.reshape(-1, 3), got.material.reshape(-1)
        assert_bit_equal(gd[inside], d, "bounded: distance inside")
        assert_bit_equal(gn[inside], nrm, "bounded: normal inside")
        assert (gm[inside] >= 0).all()
        sub = ft.FieldSamples(None, None, gm[inside], ds.materials)
        assert_bit_equal(material_colors(sub), col, "bounded: colour inside")
        assert np.isnan(gd[~inside]).all() and np.isnan(gn[~inside]).all() and (gm[~inside] == -1).all()
    # a lattice wholly outside: nothing is evaluated at all
    far = ds.sample_lattice((1000.0, 1000.0, 1000.0), (0.1, 0.1, 0.1), (5, 5, 5), normal_epsilon=NORMAL_EPS, material=True, bounded=True)
    assert np.isnan(far.distance).all() and np.isnan(far.normal).all() and (far.material == -1).all()
    # SdfForm.tryDistance of the Python mirror agrees (its own inside test, ft_eval_distance)
    if name == "c3_64":
        form = scene.Object.kids[1]
        assert_bit_equal(ft.SdfForm.sample(form, origin, step, COUNTS, bounded=True, device=gpu).distance.reshape(-1), ft.SdfForm.tryDistance(form, pts, device=gpu), "tryDistance")
        assert_bit_equal(ft.SdfForm.normal(form, NORMAL_EPS, pts[inside], device=gpu), nrm, "SdfForm.normal")


@pytest.mark.parametrize("name", ["c3_64", "mixed_nested"])
def test_glibc_arithmetic(gpu, oracle, glibc_mode, name):
    origin, step, pts, _, _, _ = reference(oracle, name)                                   # the lattice only: the values are formed again under libm
    os_ = oracle.Oracle().scene(scene_of(name))
    d, nrm, _ = oracle_field(oracle, os_, pts, NORMAL_EPS)
    ds = gpu.scene(scene_of(name))
    got = ds.sample_lattice(origin, step, COUNTS, normal_epsilon=NORMAL_EPS, material=True)
    assert_bit_equal(got.distance.reshape(-1), d, name + " distance in glibc mode")
    assert_bit_equal(got.normal.reshape(-1, 3), nrm, name + " normal in glibc mode")
    assert_bit_equal(ds.sample_points(pts).distance, d, name + " points in glibc mode")
