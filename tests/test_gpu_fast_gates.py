"""The fast sphere arithmetic at the edges of its flatten-time gates (tests/gate_scenes.py), on the GPU: every scene at a gate and its twin one
float32 step outside, at points on sphere centres, on the shell of the near radius, at the |p|inf guard and where the terms are subnormal or
flushed, through the general interpreter (eval_distance), the lean lane evaluator with and without the culling pass (sample_points), the packed
latency evaluator (packs of 1, 8 and 32 rays born at every family, among them packs in which exactly one ray fails a guard) and whole frames; the union walks' and the carved tails' fast square roots at the same bounds;
smooth-union runs that fill the stage exactly, exceed it, or lie behind a stage another run has filled.  Everything bit for bit against the CPU
oracle, counters included; in the glibc arithmetic as well where ft_glibc_expf_main is called without its special cases."""
import functools

import numpy as np
import pytest

import fraytracer_amd as ft
import gate_scenes as G
from helpers import assert_bit_equal, check_counts, glibc_mode, options, options_left_at_defaults  # noqa: F401  (glibc_mode, options_left_at_defaults: fixtures)
from test_gpu_field import NORMAL_EPS, oracle_field

pytestmark = pytest.mark.gpu

F = np.float32
ALL_ON = dict(cert=1, occl=1, cull=1, reuse=1)
ALL_OFF = dict(cert=0, occl=0, cull=0, reuse=0)


@functools.lru_cache(maxsize=None)
def lean_case(oracle, name, side):
    """(blob, scene with the lights of its view, camera, point families, (lane evaluator's ray buffer, packs of 1, 8 and 32 rays)): chosen once with
    the oracle alone, shared, never written to"""
    blob = G.lean_blob(name, side)
    scene, cam, _, (_, cnt) = G.view_of(oracle, blob.object(), blob.focus, blob.eps, convex=blob.convex)
    fam = G.lean_families(oracle, blob)
    rays = G.ray_buffer(oracle, fam, blob.focus, blob.eps, cam)
    packs = G.ray_packs(oracle, fam, blob.focus, blob.eps, cam)
    for a in list(fam.values()) + [rays] + [r for _, r in packs]:
        a.setflags(write=False)
    return blob, scene, cam, fam, (rays, packs)


def check_points(ds, oracle, os_, fam, what, culls=(1, 0)):
    """eval_distance, and sample_points with a normal with the culling pass and without it, on every family"""
    gpu = ds.device
    for key, pts in fam.items():
        d, nrm, _ = oracle_field(oracle, os_, pts, NORMAL_EPS)
        assert_bit_equal(ds.eval_distance(pts)[0], d, f"{what}, {key}: eval_distance")
        for cull in culls:
            with options(gpu, cull=cull):
                got = ds.sample_points(pts, normal_epsilon=NORMAL_EPS)
            assert_bit_equal(got.distance, d, f"{what}, {key}, cull {cull}: distance")
            assert_bit_equal(got.normal, nrm, f"{what}, {key}, cull {cull}: normal")


EVALUATE_ALL = dict(escape=0, cert=0, occl=0)        # no shortcut ends a ray before its first evaluation: every born point is evaluated


def check_buffer(ds, os_, rays, what):
    """form_try_trace, object_try_trace and trace_rays of one buffer, taken whole, against the oracle's"""
    with np.errstate(all="ignore"):
        want_rgb, cnt = os_.trace_rays(rays)
        want_form, want_obj = os_.form_try_trace(rays)[0], os_.object_try_trace(rays)[0]
    assert_bit_equal(ds.form_try_trace(rays)[0], want_form, what + ": form_try_trace")
    assert_bit_equal(ds.object_try_trace(rays)[0], want_obj, what + ": object_try_trace")
    rgb, st = ds.trace_rays(rays)
    assert_bit_equal(rgb, want_rgb, what + ": trace_rays")
    check_counts(st, cnt)


def check_rays(ds, os_, buffers, what, tail_ks=(0, -1), convex=False):
    """the lane evaluator's buffer and every pack of 1, 8 and 32 rays (tail_k = -1, the default threshold of 32: the packed latency evaluator;
    tail_k = 0: one ray per lane), with the shortcuts on and with none that could end a ray before its first evaluation"""
    gpu = ds.device
    rays, packs = buffers
    assert len(rays) >= 256 and sorted({len(r) for _, r in packs}) == [1, 8, 32]
    with np.errstate(all="ignore"):                                                        # from the oracle alone, before any GPU value
        assert G.frame_is_telling(os_.trace_rays(rays)[1], len(rays), convex), what
        together = np.concatenate([r for _, r in packs])
        assert G.frame_is_telling(os_.trace_rays(together)[1], len(together), convex), what
    for k in tail_ks:
        for mode in ({}, EVALUATE_ALL):
            with options(gpu, tail_k=k, **mode):
                for label, r in [(f"{len(rays)} rays", rays)] + packs:
                    check_buffer(ds, os_, r, f"{what}, tail_k {k}, {mode}, {label}")


def check_frame(ds, os_, cam, eps, what, modes=(ALL_ON, ALL_OFF), size=(G.W, G.H), convex=False, telling=True):
    gpu = ds.device
    with np.errstate(all="ignore"):
        frame, cnt = os_.render(eps, G.LEN, size[0], size[1], cam.as_array())
    if telling:
        assert G.frame_is_telling(cnt, size[0] * size[1], convex), (what, cnt)
    else:
        assert cnt["flags"] == 0
    for mode in modes:
        with options(gpu, **mode):
            got, st = ds.render(eps, G.LEN, ft.ImageSize(*size), cam)
        assert_bit_equal(got, frame, f"{what}, {mode}")
        check_counts(st, cnt)


# ---- lean gate scenes ---------------------------------------------------------------------------------------------------------------------------------
LEAN = [pytest.param(n, s, id=f"{n}, {s}") for n, s in G.lean_cases()]


@pytest.mark.parametrize("name,side", LEAN)
def test_lean_gate_points(gpu, oracle, name, side):
    blob, scene, cam, fam, rays = lean_case(oracle, name, side)
    G.assert_families_tell(oracle, blob, fam)
    ds, os_ = gpu.scene(scene), oracle.Oracle().scene(scene)
    try:
        assert ds.info()["fast_path"] == (1 if side == "inside" else 0)
        check_points(ds, oracle, os_, fam, f"{name}, {side}")
    finally:
        ds.close()


@pytest.mark.parametrize("name,side", LEAN)
def test_lean_gate_rays(gpu, oracle, name, side):
    blob, scene, cam, fam, rays = lean_case(oracle, name, side)
    ds, os_ = gpu.scene(scene), oracle.Oracle().scene(scene)
    try:
        check_rays(ds, os_, rays, f"{name}, {side}", convex=blob.convex)
    finally:
        ds.close()


@pytest.mark.parametrize("name,side", LEAN)
def test_lean_gate_frame(gpu, oracle, name, side):
    blob, scene, cam, fam, rays = lean_case(oracle, name, side)
    ds, os_ = gpu.scene(scene), oracle.Oracle().scene(scene)
    try:
        check_frame(ds, os_, cam, blob.eps, f"{name}, {side}", convex=blob.convex)
    finally:
        ds.close()


@pytest.mark.parametrize("name", G.GLIBC_SCENES)
def test_lean_gates_in_the_glibc_arithmetic(gpu, oracle, glibc_mode, name):
    """the _libm kernels: under near_point_ok they call ft_glibc_expf_main, the main path without expf's special cases, on the promise t in [-87, 80]"""
    blob, scene, cam, fam, rays = lean_case(oracle, name, "inside")
    ds, os_ = gpu.scene(scene), oracle.Oracle().scene(scene)
    try:
        assert ds.info()["fast_path"] == 1
        check_points(ds, oracle, os_, fam, f"{name}, glibc mode")
        check_rays(ds, os_, rays, f"{name}, glibc mode", convex=blob.convex)
        check_frame(ds, os_, cam, blob.eps, f"{name}, glibc mode", convex=blob.convex)
    finally:
        ds.close()


# ---- union and carved gate scenes ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def union_case(oracle, name, variant):
    g = G.union_gates()[name]
    obj = G.union_object(name, variant)
    scene, cam, _, _ = G.view_of(oracle, obj, g["focus"], g["eps"])
    O = oracle.Oracle()
    boundary = O.form_boundary(O.object_form(O.scene(scene).object))
    ordinary = G.ordinary_family(None, boundary)
    fam = {"centres": G.centre_family(G.union_centres(name, variant)), "ordinary": ordinary, "guard": G.guard_family(ordinary)}
    for a in fam.values():
        a.setflags(write=False)
    return scene, cam, fam, g["eps"]


@pytest.mark.parametrize("variant", G.UNION_VARIANTS)
@pytest.mark.parametrize("name", G.UNION_NAMES)
def test_union_and_carved_gates(gpu, oracle, name, variant):
    """the union walk's fastQ and the carved tail's FT_CARVE_FAST_SPHERE at their bounds and one step outside, in the carved kernels and (carved = 0)
    in the general walk"""
    scene, cam, fam, eps = union_case(oracle, name, variant)
    ds, os_ = gpu.scene(scene), oracle.Oracle().scene(scene)
    try:
        info = ds.info()
        assert info["n_grids"] == 1 and info["fast_path"] == 3, info              # plain: the carved shape with an empty tail
        for carved in (1, 0):
            with options(gpu, carved=carved):
                check_points(ds, oracle, os_, fam, f"{name}, {variant}, carved {carved}", culls=(1,))
                check_frame(ds, os_, cam, eps, f"{name}, {variant}, carved {carved}", modes=(ALL_ON,))
    finally:
        ds.close()


# ---- stage scenes ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stage_case(oracle, name):
    scene = G.stage_scene(name)
    pts = G.blocks(np.random.default_rng(8).uniform(-8.0, 8.0, (512, 3)))
    rays = G.stage_rays(oracle, oracle.Oracle().scene(scene))
    for a in (pts, rays):
        a.setflags(write=False)
    return scene, pts, rays


@pytest.mark.parametrize("name", G.STAGE_NAMES)
def test_stage_scenes(gpu, oracle, name):
    """3072 spheres fill the stage exactly (the lean kernel); one more, or a second run behind a full stage, is a FT_FLAG_FAST run read from global memory"""
    scene, pts, rays = stage_case(oracle, name)
    ds, os_ = gpu.scene(scene), oracle.Oracle().scene(scene)
    try:
        info = ds.info()
        fast_path, cull_pc, n_consts, n_slots = G.STAGE_INFO[name]
        assert (info["fast_path"], info["cull_pc"]) == (fast_path, cull_pc), info
        assert n_consts is None or info["n_consts"] == n_consts, info
        check_frame(ds, os_, G.stage_camera(), 0.01, name, modes=(ALL_ON,), size=(24, 16))
        check_points(ds, oracle, os_, {"cube": pts}, name)
        assert G.frame_is_telling(os_.trace_rays(rays)[1], len(rays)), name                # from the oracle alone
        for k in (-1, 64):
            with options(gpu, tail_k=k):
                check_buffer(ds, os_, rays, f"{name}, tail_k {k}")
    finally:
        ds.close()


def test_stage_scene_in_the_glibc_arithmetic(gpu, oracle, glibc_mode):
    """2000 + 1100: the libm tables lie behind a stage that is full"""
    scene, pts, rays = stage_case(oracle, "2000 + 1100")
    ds, os_ = gpu.scene(scene), oracle.Oracle().scene(scene)
    try:
        origin, step, counts = (-3.0, -2.5, -3.5), (0.9, 0.8, 1.1), (7, 6, 7)
        lat = ft.lattice_points(origin, step, counts).reshape(-1, 3)
        d, nrm, _ = oracle_field(oracle, os_, lat, NORMAL_EPS)
        assert np.isfinite(d).all() and (d < 0).any() and (d > 0).any()
        got = ds.sample_lattice(origin, step, counts, normal_epsilon=NORMAL_EPS)
        assert_bit_equal(got.distance.reshape(-1), d, "2000 + 1100 in glibc mode: distance")
        assert_bit_equal(got.normal.reshape(-1, 3), nrm, "2000 + 1100 in glibc mode: normal")
    finally:
        ds.close()
