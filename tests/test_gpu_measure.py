"""Measures on the GPU (ft_shells_measure, ft_mesh_measure): every record bit for bit against the restatement of the rule (tests/measure_restatement.py)
— the conversion kernel alone on crafted sums, the device's float64 sqrt and division, extreme coordinates, order independence at every grid, the
lattices and scenes of the shell tests, the selection, device memory, tensors, lifetimes."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import _lib
from helpers import options_left_at_defaults  # noqa: F401  (a fixture)

import measure_cases as cases
import measure_restatement as rule
import mesh_cases
import shells_cases
import shells_restatement as shells_rule

pytestmark = pytest.mark.gpu

L = _lib.lib
OK, INVALID = _lib.FT_OK, _lib.FT_ERR_INVALID
TRI = L.ft_ctx_measure_triangles                                                           # internal: not in the header
TRI.restype, TRI.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
FINISH = L.ft_ctx_measure_finish
FINISH.restype, FINISH.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
GRID = L.ft_ctx_measure_grid
GRID.restype, GRID.argtypes = C.c_int, [C.c_void_p, C.c_int32]
PROBE = L.ft_ctx_measure_probe
PROBE.restype, PROBE.argtypes = C.c_int, [C.c_void_p, C.c_int32, C.c_int32]


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def measure(gpu, v, t, vl, tl, n_shells):
    v, t = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(t, np.int32)
    vl, tl = (None if x is None else np.ascontiguousarray(x, np.int32) for x in (vl, tl))
    raw = np.full(n_shells * 9 + 8, 7.25)                                                  # 72 bytes per record, guard words behind them
    assert TRI(gpu._ctx, ptr(v), len(v), ptr(t), len(t), ptr(vl), ptr(tl), n_shells, ptr(raw)) == OK, _lib.last_error()
    assert (raw[n_shells * 9:] == 7.25).all()
    return raw[:n_shells * 9].view(rule.RECORD)


def assert_same_records(got, want, what):
    g = np.ascontiguousarray(got).view(rule.RECORD).reshape(-1) if not isinstance(got, np.ndarray) or got.dtype != rule.RECORD else got
    assert g.shape == want.shape, (what, g.shape, want.shape)
    for name in rule.RECORD.names:
        a, b = np.ascontiguousarray(g[name]), np.ascontiguousarray(want[name])
        kind = {8: np.uint64, 4: np.uint32}[a.dtype.itemsize]
        same = a.view(kind) == b.view(kind)
        assert same.all(), (what, name, int((~same).sum()), a[~same][:3], b[~same][:3])
    assert rule.same_bytes(g, want), what


# ---- the conversion alone ----------------------------------------------------------------------------------------------------------------------


def test_finish_kernel_converts_crafted_sums(gpu):
    qs = cases.finish_sums()
    words = np.array([[q & (2 ** 64 - 1), (q >> 64) & (2 ** 64 - 1)] for q in qs], np.uint64)
    assert (2 ** 64 - 1, 0) in map(tuple, words.tolist()) and (2 ** 64 - 1, 2 ** 64 - 1) in map(tuple, words.tolist())
    for s in (0, 37, -427, 677):                                                           # the scale's extremes: s_M at E = 128 and at E = -148
        out = np.full(len(qs) + 2, 7.25)
        assert FINISH(gpu._ctx, ptr(words), len(qs), s, ptr(out)) == OK and (out[-2:] == 7.25).all()
        want = np.array([rule.to_float(q, s) for q in qs])
        wrong = np.flatnonzero(out[:-2].view(np.uint64) != want.view(np.uint64))
        assert wrong.size == 0, (s, [(qs[i], out[i], want[i]) for i in wrong[:4]])
    # the rounding decisions themselves, spelled out
    spelled = {2 ** 53 + 1: 2.0 ** 53, 2 ** 53 + 3: 2.0 ** 53 + 4, 2 ** 54 + 3: 2.0 ** 54 + 4, 2 ** 54 + 1: 2.0 ** 54, -(2 ** 53 + 3): -(2.0 ** 53 + 4), 2 ** 64 - 1: 2.0 ** 64,
               -1: -1.0, (2 ** 53 + 1) * 2 ** 64 + 1: (2.0 ** 53 + 2) * 2.0 ** 64, (2 ** 53 + 1) * 2 ** 64 - 1: 2.0 ** 117}
    for q, x in spelled.items():
        assert float(q) == x and q in qs, q


# ---- sqrt and division ---------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("which", ["random", "near_squares"])
def test_float64_sqrt_and_division_are_the_cpu_ones(gpu, which):
    """every triangle a shell of its own and sizes within a few binades of the extent, so the quantum is finer than an area's last bit: the record's
    area is the device's 0.5 * sqrt(...) itself, its volume the device's S / 6.0, its moments S / 24.0"""
    v, t = cases.sqrt_random() if which == "random" else cases.sqrt_near_squares()
    tl = np.arange(len(t), dtype=np.int32)
    got = measure(gpu, v, t, np.repeat(tl, 3), tl, len(t))
    want = rule.measure(v, t, np.repeat(tl, 3), tl, len(t))
    direct = rule.terms(v, t)
    assert np.array_equal(want["area"].view(np.uint64), direct[:, 0].view(np.uint64))       # numpy's 0.5 * sqrt
    wrong = np.flatnonzero(got["area"].view(np.uint64) != direct[:, 0].view(np.uint64))
    print(which, "areas that differ from numpy's:", wrong.size, "of", len(t))
    assert wrong.size == 0, (got["area"][wrong[:4]], direct[wrong[:4], 0])
    assert_same_records(got, want, which)
    if which == "random":
        assert len(np.unique(got["volume"])) > 4000 and (got["moment"] != 0).all()


# ---- extremes ------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(cases.extremes()))
def test_extremes(gpu, name):
    v, t, vl, tl, n_shells = cases.extremes()[name]
    got = measure(gpu, v, t, vl, tl, n_shells)
    want = rule.measure(v, t, vl, tl, n_shells)
    assert_same_records(got, want, name)
    E = int(got["extent_exponent"][0])
    if name.startswith("denormal"):
        assert E == int(name.split("E")[1]) and (got["area"] > 0).all() and (np.abs(v) < 2.0 ** -126).all()
    elif name == "huge_E128":
        assert E == 128 and np.isfinite(got["area"]).all() and np.isfinite(got["moment"]).all() and (got["area"] > 1e70).all()
    elif name == "all_zero":
        assert E == 0 and got["area"][0] == 0 and got["n_unmeasured"][0] == 0 and got["bbox_min"][0].tolist() == [0, 0, 0]
    elif name == "non_finite":
        assert E == 2 and (got["n_unmeasured"] > 0).all() and got["n_unmeasured"].sum() < len(t) and np.isfinite(got["bbox_max"]).all()
    elif name == "signed_zero":
        assert np.signbit(got["bbox_min"][0, 0]) and not np.signbit(got["bbox_max"][0, 0])
        assert np.signbit(got["bbox_max"][1, 1]) and got["bbox_max"][1, 1] == 0 and not np.signbit(got["bbox_min"][2, 0]) and got["bbox_min"][2, 0] == 0
    elif name == "no_finite_value":
        assert got["bbox_min"][1].tolist() == [1.0, np.inf, 1.0] and got["bbox_max"][1].tolist() == [3.0, -np.inf, 5.0] and got["n_unmeasured"].tolist() == [0, 1, 0]
        assert got["bbox_min"][2].tolist() == [np.inf] * 3 and got["bbox_max"][2].tolist() == [-np.inf] * 3
    elif name == "out_of_range":
        assert got["n_unmeasured"].tolist() == [1, 1]
    elif name == "unused_vertex_sets_extent":
        assert E == 10


def test_no_labels_is_label_zero_and_zero_shells_write_nothing(gpu):
    v, t = cases.mixed(700)
    assert_same_records(measure(gpu, v, t, None, None, 1), rule.whole(v, t), "no labels")
    assert TRI(gpu._ctx, ptr(v), len(v), ptr(t), len(t), None, None, 0, None) == OK
    none = np.zeros((0, 3), np.int32)
    got = measure(gpu, v, none, None, None, 2)                                             # no triangle: the boxes and the extent only
    assert_same_records(got, rule.measure(v, none, None, None, 2), "no triangles")
    assert got["area"].tolist() == [0, 0] and np.isinf(got["bbox_min"][1]).all()


# ---- order independence --------------------------------------------------------------------------------------------------------------------------


def test_every_grid_and_both_flush_policies_give_the_same_bytes(gpu):
    """labels t % 7: neighbouring iterations of a lane differ in their label, so every lane flushes on every iteration and every wave holds all seven
    labels; one label throughout: no flush until the end.  Terms of both signs over 80 to 90 bits: low words wrap, high words are sign-extended."""
    v, t = cases.mixed()
    assert len(t) == 20000
    by7, vl7 = (np.arange(len(t)) % 7).astype(np.int32), (np.arange(len(v)) % 7).astype(np.int32)
    want7, want1 = rule.measure(v, t, vl7, by7, 7), rule.measure(v, t, None, None, 1)
    sums, _ = rule.integer_sums(v, t, by7, 7)
    assert any(q < 0 for row in sums for q in row) and any(q > 2 ** 64 for row in sums for q in row) and (want7["n_unmeasured"] > 0).any()
    try:
        for grid in (1, 2, 3, 0):                                                          # 0: as many workgroups as fill the device
            assert GRID(gpu._ctx, grid) == OK
            for eager in (0, 1):
                assert PROBE(gpu._ctx, 0, eager) == OK
                assert_same_records(measure(gpu, v, t, vl7, by7, 7), want7, f"labels t % 7, grid {grid}, eager {eager}")
                assert_same_records(measure(gpu, v, t, None, np.zeros(len(t), np.int32), 1), want1, f"one label, grid {grid}, eager {eager}")
    finally:
        assert GRID(gpu._ctx, 0) == OK and PROBE(gpu._ctx, 0, 0) == OK
    # sorted by label: a lane changes its label a few times at most
    order = np.argsort(by7, kind="stable")
    assert_same_records(measure(gpu, v, t[order], vl7, by7[order], 7), want7, "sorted by label")


# ---- the pipeline --------------------------------------------------------------------------------------------------------------------------------


def want_of(mesh, shells):
    v, t = ft.Mesh._host(mesh.vertices), ft.Mesh._host(mesh.triangles)
    S = len(shells.records)
    return rule.measure(v, t, shells.vertex_shell, shells.triangle_shell, S), rule.whole(v, t) if len(v) or len(t) else np.zeros(0, rule.RECORD)


@pytest.mark.parametrize("name", list(shells_cases.LATTICES))
def test_lattices(gpu, name):
    d, origin, step = shells_cases.lattice(name)
    mesh = shells_cases.mesh_of(name)
    sh = shells_rule.shells(mesh.triangles, len(mesh.vertices))
    got = gpu.mesh_values(d, origin, step, measures=True)
    assert np.array_equal(got.triangles, mesh.triangles) and np.array_equal(got.shells.records, sh.records)
    per_shell, whole = want_of(mesh, sh)
    assert_same_records(got.shells.measures.records, per_shell, name)
    assert_same_records(got.measure.records, whole, name + ": whole mesh")
    m = got.shells.measures
    assert np.array_equal(m.volume, per_shell["volume"]) and np.array_equal(m.area, per_shell["area"]) and m.extent_exponent == per_shell["extent_exponent"][0]
    with np.errstate(all="ignore"):
        assert np.array_equal(m.centroid, per_shell["moment"] / per_shell["volume"][:, None], equal_nan=True)
    if name in ("egg_crate", "egg_crate_shifted"):
        assert len(m) == {"egg_crate": 64, "egg_crate_shifted": 125}[name]
        whole_balls = got.shells.closed                                                    # the shifted crate's outer balls are cut open by the lattice's faces
        assert whole_balls.any() and (m.volume[whole_balls] > 0).all()
        assert np.allclose(m.volume[whole_balls], 4 / 3 * np.pi * 0.3 ** 3, rtol=0.1)          # balls of radius 0.3, as the lattice sees them
    if name == "two_spheres_nan":
        assert not got.shells.closed.all()
    plain = gpu.mesh_values(d, origin, step)                                               # the defaults: today's result
    assert plain.shells is None and plain.measure is None and np.array_equal(plain.triangles, got.triangles)
    assert gpu.mesh_values(d, origin, step, shells=True).shells.measures is None


def test_keep_bodies_on_the_hollow_ball(gpu):
    d, origin, step = shells_cases.lattice("hollow_ball")
    both = gpu.mesh_values(d, origin, step, measures=True)
    assert len(both.shells) == 2 and both.shells.closed.all() and sorted(np.sign(both.shells.measures.volume)) == [-1, 1]
    for keep in ("bodies", lambda s: s.closed & (s.measures.volume > 0)):
        kept = gpu.mesh_values(d, origin, step, keep=keep, measures=True)
        assert len(kept.shells) == 1 and kept.shells.measures.volume[0] > 0
        body = int(np.argmax(both.shells.measures.volume))
        assert kept.shells.measures.volume[0] == both.shells.measures.volume[body] and kept.shells.measures.area[0] == both.shells.measures.area[body]
        assert_same_records(kept.shells.measures.records, want_of(kept, kept.shells)[0], "selected mesh")
        assert_same_records(kept.measure.records, want_of(kept, kept.shells)[1], "selected mesh, whole")
    assert len(gpu.mesh_values(d, origin, step, keep="closed").shells) == 2                # connectivity alone keeps the cavity
    assert gpu.mesh_values(d, origin, step, keep="bodies").shells.measures is None


@pytest.mark.parametrize("name", list(mesh_cases.SCENES))
def test_scenes_refined_and_not_and_a_selected_mesh(gpu, oracle, name):
    origin, step, _ = mesh_cases.oracle_lattice(oracle, name)
    ds = gpu.scene(mesh_cases.scene_of(name))
    kw = dict(normal_epsilon=mesh_cases.NORMAL_EPS, material=True)
    plain = ds.mesh_lattice(origin, step, mesh_cases.COUNTS, **kw)
    for refine in (None, 8):
        got = ds.mesh_lattice(origin, step, mesh_cases.COUNTS, measures=True, refine=refine, **kw)
        assert np.array_equal(got.triangles, plain.triangles) and got.normal is not None and got.material is not None
        per_shell, whole = want_of(got, got.shells)
        assert_same_records(got.shells.measures.records, per_shell, f"{name}, refine {refine}")
        assert_same_records(got.measure.records, whole, f"{name}, refine {refine}: whole mesh")
        assert (got.shells.measures.n_unmeasured == 0).all() and (got.shells.measures.area > 0).all()
    kept = ds.mesh_lattice(origin, step, mesh_cases.COUNTS, keep=1, measures=True, **kw)
    assert len(kept.shells) == 1
    assert_same_records(kept.shells.measures.records, want_of(kept, kept.shells)[0], name + " largest")
    assert_same_records(kept.measure.records, want_of(kept, kept.shells)[1], name + " largest: whole mesh")
    assert np.array_equal(kept.shells.measures.records.view(np.uint8), kept.measure.records.view(np.uint8))      # one shell that is the whole mesh
    if name == "c3_64":
        via_form = ft.SdfForm.mesh(mesh_cases.scene_of(name).Object.kids[1], origin, step, mesh_cases.COUNTS, device=gpu, measures=True)
        assert_same_records(via_form.shells.measures.records, want_of(via_form, via_form.shells)[0], "SdfForm.mesh")


# ---- interfaces ----------------------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def hip():
    h = C.CDLL("libamdhip64.so.7")             # the runtime the library is linked against (already loaded: same instance)
    h.hipMalloc.argtypes, h.hipMemcpy.argtypes, h.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p]
    return h


def make_mesh(gpu, name):
    d, origin, step = shells_cases.lattice(name)
    lat, _ = ft.api._lattice(origin, step, d.shape)
    h = C.c_void_p()
    assert L.ft_mesh_values(gpu._ctx, C.byref(lat), d.ctypes.data_as(C.c_void_p), 0.0, C.byref(h)) == OK
    return h


@pytest.mark.parametrize("first", ["mesh", "shells"])
def test_device_records_alignment_and_lifetimes(gpu, hip, first):
    """records in device memory between guard words; a misaligned address is refused; the mesh and the shells are destroyed, in either order, before
    the records are read; shells of another mesh measure nothing"""
    name = "clipped_plus_whole"
    mesh = shells_cases.mesh_of(name)
    sh = shells_rule.shells(mesh.triangles, len(mesh.vertices))
    S = len(sh.records)
    want, whole = want_of(mesh, sh)
    a, b = make_mesh(gpu, name), make_mesh(gpu, name)
    sa = C.c_void_p()
    assert L.ft_mesh_shells(a, C.byref(sa)) == OK
    n_words = (S + 1) * 9
    host = np.full(n_words + 16, 7.25)
    base = C.c_void_p()
    assert hip.hipMalloc(C.byref(base), C.c_size_t(host.nbytes)) == 0
    try:
        assert hip.hipMemcpy(base, ptr(host), C.c_size_t(host.nbytes), 1) == 0
        out = base.value + 64
        for off in (1, 2, 4, 7):
            assert L.ft_shells_measure(a, sa, C.c_void_p(out + off)) == INVALID and "aligned" in _lib.last_error()
            assert L.ft_mesh_measure(a, C.c_void_p(out + off)) == INVALID
        assert L.ft_shells_measure(b, sa, C.c_void_p(out)) == INVALID and "not built from this mesh" in _lib.last_error()
        assert L.ft_shells_measure(a, sa, None) == INVALID and L.ft_mesh_measure(a, None) == INVALID
        assert L.ft_shells_measure(a, sa, C.c_void_p(out)) == OK
        assert L.ft_mesh_measure(a, C.c_void_p(out + 72 * S)) == OK                        # 72 S is a multiple of 8
        if first == "mesh":
            L.ft_mesh_destroy(a); L.ft_shells_destroy(sa)
        else:
            L.ft_shells_destroy(sa); L.ft_mesh_destroy(a)
        L.ft_mesh_destroy(b)
        back = np.empty_like(host)
        assert hip.hipMemcpy(ptr(back), base, C.c_size_t(back.nbytes), 2) == 0
        assert (back[:8] == 7.25).all() and (back[8 + n_words:] == 7.25).all()            # nothing outside the records
        assert_same_records(back[8:8 + 9 * S].view(rule.RECORD), want, "device records")
        assert_same_records(back[8 + 9 * S:8 + n_words].view(rule.RECORD), whole, "device record of the whole mesh")
    finally:
        assert hip.hipFree(base) == 0


def test_host_records_through_the_c_abi(gpu):
    name = "hollow_ball"
    mesh = shells_cases.mesh_of(name)
    sh = shells_rule.shells(mesh.triangles, len(mesh.vertices))
    want, whole = want_of(mesh, sh)
    a = make_mesh(gpu, name)
    sa, sel, ssel = C.c_void_p(), C.c_void_p(), C.c_void_p()
    try:
        assert L.ft_mesh_shells(a, C.byref(sa)) == OK
        rec = np.zeros(2, np.dtype(_lib.SHELL_MEASURE_DTYPE))
        assert L.ft_shells_measure(a, sa, ptr(rec)) == OK
        assert_same_records(rec, want, "host records")
        one = (_lib.ShellMeasure * 1)()
        assert L.ft_mesh_measure(a, one) == OK and one[0].area == whole["area"][0] and one[0].volume == whole["volume"][0] and one[0].extent_exponent == 1
        assert list(one[0].moment) == whole["moment"][0].tolist() and list(one[0].bbox_min) == whole["bbox_min"][0].tolist()
        # a selected mesh is a mesh like any other; the source's shells do not fit it
        keep = np.array([0, 1], np.uint8)
        assert L.ft_mesh_select(a, sa, ptr(keep), 2, C.byref(sel)) == OK and L.ft_mesh_shells(sel, C.byref(ssel)) == OK
        assert L.ft_shells_measure(sel, sa, ptr(rec)) == INVALID
        assert L.ft_shells_measure(sel, ssel, ptr(rec[:1])) == OK
        v, t, _, _, _ = shells_rule.select(mesh.vertices, mesh.triangles, sh, keep.astype(bool))
        assert_same_records(rec[:1], rule.whole(v, t), "the selected mesh")               # its own extent: the inner shell alone is smaller
        assert rec[0]["extent_exponent"] == 0 and want[1]["extent_exponent"] == 1 and abs(rec[0]["volume"] - want[1]["volume"]) < 1e-12
    finally:
        for h in (sa, ssel):
            L.ft_shells_destroy(h)
        for h in (a, sel):
            L.ft_mesh_destroy(h)


TENSOR_PATH = r"""
import json, sys
import numpy as np
import torch                              # before the library: torch's HIP runtime is the one the process loads first
import fraytracer_amd as ft
sys.path.insert(0, "tests")
import shells_cases
import shells_restatement as shells_rule
import measure_restatement as rule
host = lambda t: np.ascontiguousarray(t.detach().cpu().numpy())
dev = ft.Device(0)
r = {}
mesh = shells_cases.mesh_of("egg_crate")
sh = shells_rule.shells(mesh.triangles, len(mesh.vertices))
want = rule.measure(mesh.vertices, mesh.triangles, sh.vertex_shell, sh.triangle_shell, len(sh.records))
whole = rule.whole(mesh.vertices, mesh.triangles)
d, origin, step = shells_cases.lattice("egg_crate")
side = torch.cuda.Stream()                # on a side stream, behind the torch kernel that makes the values: the stream hand-over
side.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(side):
    vals = torch.from_numpy(np.array(d)).cuda() + 0
    m = dev.mesh_values(vals, origin, step, measures=True)
side.synchronize()
rec = m.shells.measures.records
r["tensors"] = bool(rec.is_cuda and tuple(rec.shape) == (len(want), 18) and rec.dtype == torch.float32 and m.measure.records.is_cuda and m.vertices.is_cuda)
r["aligned"] = rec.data_ptr() % 8 == 0
r["records on a side stream"] = rule.same_bytes(m.shells.measures.host(), want)
r["whole mesh"] = rule.same_bytes(m.measure.host(), whole)
m2 = dev.mesh_values(vals, origin, step, keep="bodies", measures=True)          # torch's default stream: the side-stream path
torch.cuda.synchronize()
r["keep bodies, tensors"] = bool(m2.shells.measures.records.is_cuda and rule.same_bytes(m2.shells.measures.host(), want))
r["properties"] = bool(np.array_equal(m.shells.measures.volume, want["volume"]) and m.shells.measures.bbox_min.dtype == np.float32)
ds = dev.scene(__import__("mesh_cases").scene_of("c3_64"))
like = torch.empty(1, device="cuda")
import mesh_cases, oracle.binding as ob
o, s, _ = mesh_cases.oracle_lattice(ob, "c3_64")
got = ds.mesh_lattice(o, s, mesh_cases.COUNTS, like=like, measures=True)
torch.cuda.synchronize()
v, t = host(got.vertices), host(got.triangles)
r["like"] = bool(got.shells.measures.records.is_cuda and rule.same_bytes(got.shells.measures.host(), rule.measure(v, t, host(got.shells.vertex_shell), host(got.shells.triangle_shell), len(got.shells)))
                 and rule.same_bytes(got.measure.host(), rule.whole(v, t)))
dev.close()
print(json.dumps(r))
"""


def test_tensor_path_in_a_process_that_loads_torch_first():
    """device tensors in, device records out, on the caller's stream: in a child process that loads torch before the library"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", TENSOR_PATH], cwd=root, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    failed = [k for k, v in r.items() if v is not True]
    assert not failed, failed
