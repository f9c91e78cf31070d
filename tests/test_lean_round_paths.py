"""The lean kernel's round outside the sphere loop (kernels.hip ft_trace_body with VARIANT == 1): the per-wave sums that live in the LDS header, the
arguments that are read where they are used (a job's start, a pixel's colour, a light's record, the hand-out, the certificates' constants, the
statistics block) and the switches that are compared where they are tested.  None of it may move a float or a counter: every frame here is the CPU
oracle's bit for bit, on frames small enough that one wave holds lanes in every phase at once.

The scene is C3 with 64 spheres relit with three lights — a directional one, a directional one that most of the visible surface faces away from
(lightCos <= 0: no shadow ray) and a point light (a shadow ray of |dir| = 1 / distance) — so a lane meets every exit of settle()."""
import itertools

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import distributed
from fraytracer_amd import synthetic as syn
import edge_scenes as edge
from helpers import COUNTERS, assert_bit_equal, options, options_left_at_defaults  # noqa: F401  (options_left_at_defaults: a fixture)

pytestmark = pytest.mark.gpu

EPS, LEN = syn.EPSILON, syn.RAY_LENGTH
SWITCHES = ("cert", "occl", "cull", "reuse")
LIGHTS = [ft.SdfLight.directional((-0.5, -1.0, 1.0), (0.5, 0.5, 0.5)),
          ft.SdfLight.directional((0.3, -0.2, -1.0), (0.2, 0.3, 0.4)),           # from behind the cloud as the default camera sees it
          ft.SdfLight.point((3.0, 9.0, -4.0), (40.0, 30.0, 20.0))]

_SHARED = {}


def relit():
    if "scene" not in _SHARED:
        _SHARED["scene"] = ft.SdfScene(syn.config3(n=64, size=64)[0].Object, syn.BACKGROUND, LIGHTS)
    return _SHARED["scene"]


def want(oracle, w, h, cam=None, length=LEN, eps=EPS):
    """the oracle's (frame, counters) of the relit scene: computed once per frame, shared, never written to"""
    cam = cam or syn.default_camera()
    key = (w, h, cam.as_array().tobytes(), float(length).hex(), float(eps).hex())
    if key not in _SHARED:
        with np.errstate(all="ignore"):
            frame, cnt = oracle.Oracle().scene(relit()).render(eps, length, w, h, cam.as_array(), nthreads=16)
        frame.setflags(write=False)
        _SHARED[key] = (frame, cnt)
    return _SHARED[key]


@pytest.fixture(scope="module")
def ds(gpu):
    d = gpu.scene(relit())
    assert d.info()["fast_path"] == 1                                  # the lean kernel
    yield d
    d.close()


def check(got, gst, wanted, what):
    assert_bit_equal(got, wanted[0], what)
    for k in COUNTERS:
        assert gst[k] == wanted[1][k], (what, k, gst[k], wanted[1][k])


def test_every_exit_of_settle(ds, oracle):
    """72 x 56, ragged in both axes: primary misses (Length, escape), hits, a light the surface faces away from, shadow rays that miss and that
    hit, of a directional and of a point light, the last light's colour"""
    w, h = 72, 56
    wanted = want(oracle, w, h)
    cnt = wanted[1]
    assert 0 < cnt["hits_primary"] < cnt["rays_primary"] == w * h
    assert cnt["hits_primary"] < cnt["rays_shadow"] < 3 * cnt["hits_primary"]      # some cosines are <= 0, some are not
    assert 0 < cnt["hits_shadow"] < cnt["rays_shadow"]
    got, st = ds.render(EPS, LEN, ft.ImageSize(w, h), syn.default_camera())
    check(got, st, wanted, "72 x 56")


def test_option_combinations(gpu, ds, oracle):
    """cert, occl, cull, reuse in all 16 combinations at 96 x 96: the frame and the ray / hit counters never move; what is evaluated does not depend on
    the culling pass"""
    size = 96
    wanted = want(oracle, size, size)
    evals = {}
    with options(gpu) as set_:
        for combo in itertools.product((0, 1), repeat=4):
            set_(**dict(zip(SWITCHES, combo)))
            got, st = ds.render(EPS, LEN, ft.ImageSize(size, size), syn.default_camera())
            check(got, st, wanted, str(dict(zip(SWITCHES, combo))))
            evals[combo] = st["sdf_evals"]
    for (cert, occl, cull, reuse), n in evals.items():
        assert n == evals[(cert, occl, 1 - cull, reuse)], (cert, occl, reuse, evals)
    assert evals[(1, 1, 1, 1)] < evals[(0, 0, 1, 1)] < evals[(0, 0, 1, 0)], evals      # each shortcut is on when its switch says so


def test_arguments_read_at_use(ds):
    """160 x 96 in one launch, as two ranks' interleaved 16-column stripes and as two column ranges with a non-zero x0: the same frame, and the
    parts' counters add up to the launch's"""
    w, h, stripe = 160, 96, 16
    size, cam = ft.ImageSize(w, h), syn.default_camera()
    full, fst = ds.render(EPS, LEN, size, cam)
    inter = np.empty((w // (2 * stripe), 2, stripe, h, 3), np.float32)
    sts = []
    for rank in range(2):
        slab, st = ds.render(EPS, LEN, size, cam, **distributed.tiling(w, 2, rank, stripe))
        inter[:, rank] = slab.reshape(w // (2 * stripe), stripe, h, 3)
        sts.append(st)
    assert_bit_equal(inter.reshape(w, h, 3), full, "two ranks' stripes")
    for k in COUNTERS[:4]:
        assert sts[0][k] + sts[1][k] == fst[k], (k, sts[0][k], sts[1][k], fst[k])
    assert fst["flags"] == sts[0]["flags"] == sts[1]["flags"] == 0
    parts = [ds.render(EPS, LEN, size, cam, x0=0, n_columns=56), ds.render(EPS, LEN, size, cam, x0=56, n_columns=104)]
    assert_bit_equal(np.concatenate([p[0] for p in parts]), full, "column ranges")
    for k in COUNTERS[:4]:
        assert parts[0][1][k] + parts[1][1][k] == fst[k], k


def test_sibling_forms(ds, oracle):
    """the *_views, *_shade and *_vis builds of the same template"""
    w, h = 72, 56
    size = ft.ImageSize(w, h)
    cams = [syn.default_camera(), ft.Camera.lookAt(Position=(7.0, 3.0, -7.0), LookAt=(0.0, 0.0, 0.0), Up=(0.0, 1.0, 0.0), Lens=ft.Lens.create(60.0))]
    singles = [ds.render(EPS, LEN, size, c) for c in cams]
    for c, single in zip(cams, singles):
        check(single[0], single[1], want(oracle, w, h, cam=c), "render")
    views, vst = ds.render_views(EPS, LEN, size, cams)
    for v in range(2):
        assert_bit_equal(views[v], singles[v][0], f"view {v}")
    for k in COUNTERS:
        assert vst[k] == singles[0][1][k] + singles[1][1][k], k
    hits, _, _ = ds.render_hits(EPS, LEN, size, cams[0])
    frame, st = singles[0]
    rgb, sst = ds.shade_hits(hits.records)
    assert_bit_equal(rgb, frame, "shade_hits of render_hits")
    vis, lst = ds.light_visibility(hits.records)
    for s in (sst, lst):
        assert (s["rays_shadow"], s["hits_shadow"], s["flags"]) == (st["rays_shadow"], st["hits_shadow"], 0), s
    lit = sum(int(((vis >> k) & 1).sum()) for k in range(len(LIGHTS)))
    assert lit == st["rays_shadow"] - st["hits_shadow"] and int(vis.max()) < 1 << len(LIGHTS)


def test_edges_of_the_first_step(gpu, ds, oracle):
    """a camera inside the blob (a hit at the camera itself) and rays of Length <= 0 — in latency mode and out of it"""
    w, h = 48, 40
    cam = edge.camera_at(edge.interior_points(oracle, relit(), 1, 0.15)[0])
    inside = want(oracle, w, h, cam=cam)
    assert inside[1]["hits_primary"] == w * h
    g = np.random.default_rng(2)
    n = 96
    o = g.normal(size=(n, 3)); o *= 8.0 / np.linalg.norm(o, axis=1, keepdims=True)
    d = -o / 8.0
    rays = np.concatenate([o, d, np.full((n, 1), LEN), np.full((n, 1), EPS)], axis=1).astype(np.float32)
    rays[0:24:3, 6] = (0.0, -0.0, -1.0, 1e-40, -np.inf, 0.0, -2.5, 1.17549435e-38)      # Length <= 0, or so short that the first step uses it up
    os_ = oracle.Oracle().scene(relit())
    with np.errstate(all="ignore"):
        want_rgb, cnt = os_.trace_rays(rays)
    assert cnt["flags"] == 0 and 0 < cnt["hits_primary"] < n
    with options(gpu) as set_:
        for tail_k in (0, -1):                                            # never, and the default
            set_(tail_k=tail_k)
            got, st = ds.render(EPS, LEN, ft.ImageSize(w, h), cam)
            check(got, st, inside, f"camera inside, tail_k {tail_k}")
            got, st = ds.trace_rays(rays)
            assert_bit_equal(got, want_rgb, f"ray buffer, tail_k {tail_k}")
            for k in COUNTERS[1:]:
                assert st[k] == cnt[k], (tail_k, k, st[k], cnt[k])


def test_a_ray_that_ends_on_the_step_cap(ds, oracle):
    """epsilon 0: a ray into the blob never evaluates below it, its steps shrink to nothing and it ends on the step cap — flag 4, a miss.  One ray
    (2^20 rounds) beside seven ordinary ones"""
    g = np.random.default_rng(3)
    o = g.normal(size=(8, 3)); o *= 8.0 / np.linalg.norm(o, axis=1, keepdims=True)
    rays = np.concatenate([o, -o / 8.0, np.full((8, 1), LEN), np.full((8, 1), EPS)], axis=1).astype(np.float32)
    capped = np.float32((4.7729607, -6.201552, 1.6612042))           # chosen with the oracle: from here the march towards the origin stalls at the surface
    rays[5, 0:3], rays[5, 3:6], rays[5, 7] = capped, -capped / np.float32(8.0), 0.0
    with np.errstate(all="ignore"):
        want_rgb, cnt = oracle.Oracle().scene(relit()).trace_rays(rays)
    assert cnt["flags"] == 4
    got, st = ds.trace_rays(rays)
    assert_bit_equal(got, want_rgb, "ray buffer with a capped ray")
    for k in COUNTERS[1:]:
        assert st[k] == cnt[k], (k, st[k], cnt[k])
