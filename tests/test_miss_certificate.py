"""The lean kernel's miss certificate (FT_OPT_CERT; kernels.hip ft_miss_certificate, scene.cpp "Miss certificate").

A ray of a scene that is one smooth union of spheres ends as a miss once  -s ln sum_i exp(si (dist(segment, c_i) - r_i)) >= epsilon + certM
over the rest of its line.  The CPU test pins the bound and the margin formula against the oracle's float32 evaluation; the GPU tests
compare colours, ray / hit counters and flags with the oracle (which has no certificate at all) with the certificate on, with an
aggressive trigger policy (every lane, every step), with it off and with the escape shortcut off."""
import math

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import synthetic as syn
from helpers import COUNTERS, assert_bit_equal, glibc_math, host, options, options_left_at_defaults, seg_dist  # noqa: F401  (host, options_left_at_defaults: fixtures)

EPS, LEN = 0.01, 30.0
# FT_OPT_CERT_POLICY: primary rays from step 0, shadow rays from step 1, whenever one lane is due, again after every further step
EVERY_STEP = 0 | (1 << 8) | (1 << 16) | (1 << 24)


def margin(escR, cinf, strength, n):
    """scene.cpp "Miss certificate", restated: (certM, delta) for a support sphere of radius escR at |c|inf = cinf, n children"""
    u = 2.0 ** -24
    Rb = 2.5 * escR * 1.001
    e3 = 3.0 * 2.0 ** -23 * (cinf + 3.0 * Rb)
    delta = 1.01 * ((2.9 * e3) + math.sqrt((2.9 * e3) ** 2 + 7.2 * e3 * Rb)) / 1.8
    eGeo = 8.0 * u * 5.0 * escR + 16.0 * u * (cinf + 10.0 * escR)
    eSum = strength * ((2.0 * n + 4096.0) * 2.0 ** -23 + 2e-4)
    return (2.0 * delta + 2.0 * eGeo + eSum) * 1.01 + 1e-6, delta


@pytest.mark.parametrize("strength", [0.05, 0.25, 1.0])
def test_bound_and_margin_against_the_oracle(host, oracle, strength):
    """The library's certificate constants are the documented formula, and with them the bound holds against the oracle: at points within delta
    (the drift tube) of a random segment, the oracle's float32 f is never below F_lo(segment) - delta - (certM - 2 delta), where F_lo is the float64
    bound and certM - 2 delta the margin's share for float32 errors — so F_lo >= epsilon + certM leaves every such value >= epsilon + delta."""
    scene, _ = syn.config3(n=256, size=64, strength=strength)
    ds = host.scene(scene)
    try:
        cx, cy, cz, escR = ds.support_sphere()
        cert = ds.miss_certificate()
    finally:
        ds.close()
    assert escR > 0
    cinf = max(abs(cx), abs(cy), abs(cz))
    M, delta = margin(escR, cinf, strength, 256)
    assert cert["margin"] == pytest.approx(M, rel=1e-5), (cert, M)
    assert cert["clip"] == pytest.approx(2.0 * delta, rel=1e-5)
    assert cert["rho2"] == pytest.approx((2.5 * escR) ** 2, rel=1e-5)
    assert 2.0 * delta < cert["margin"] < 0.1
    if strength == 0.25:
        assert 0.045 < cert["margin"] < 0.05, cert           # 0.0476 for C3
    rng = syn.Rng(3)
    C = np.array([rng.pointInBall(4.0) for _ in range(256)], np.float64)
    R = np.array([rng.range(0.1, 0.5) for _ in range(256)], np.float64)
    O = oracle.Oracle()
    h = O.form_union_smooth(strength, [O.sphere(tuple(map(float, c)), float(r)) for c, r in zip(C.astype(np.float32), R.astype(np.float32))])
    err = cert["margin"] - 2.0 * delta
    assert err > 0
    k = 1.0 / strength
    g = np.random.default_rng(11)
    for _ in range(200):
        a = g.normal(size=3) * 3.0
        b = a + g.normal(size=3) * g.choice([0.3, 3.0, 10.0])
        dmin = seg_dist(C, a, b) - R
        m = dmin.min()
        flo = m - math.log(np.exp(-k * (dmin - m)).sum()) / k
        t = g.uniform(0.0, 1.0, (64, 1))
        off = g.normal(size=(64, 3)); off *= (delta * g.uniform(0.0, 1.0, (64, 1))) / np.linalg.norm(off, axis=1, keepdims=True)
        pts = (a + t * (b - a) + off).astype(np.float32)
        f = np.asarray(O.form_distance(h, pts), np.float64)
        assert (f >= flo - delta - err).all(), (flo, f.min(), err)


def test_no_certificate_without_the_shape(host):
    """only a program that is one smooth union of staged spheres gets constants; other scenes report margin < 0"""
    for scene in (syn.config2()[0], syn.mixed_nested()[0], syn.console_like(n=50)[0]):
        ds = host.scene(scene)
        try:
            assert ds.miss_certificate()["margin"] < 0.0
        finally:
            ds.close()
    ds = host.scene(syn.config3(n=64, size=16)[0])
    try:
        assert ds.miss_certificate()["margin"] > 0.0
    finally:
        ds.close()


def _render(gpu, oracle, scene, size, opts, eps=EPS, length=LEN, cam=None, **ext):
    cam = cam or syn.default_camera()
    ds = gpu.scene(scene)
    want, ocnt = oracle.Oracle().scene(scene).render(eps, length, size.X, size.Y, cam.as_array(), nthreads=16, **ext)
    out = {}
    try:
        with options(gpu) as set_:
            for name, o in opts.items():
                set_(**o)
                got, st = ds.render(eps, length, size, cam, **ext)
                assert_bit_equal(got, want, name)
                for k in COUNTERS:
                    assert st[k] == ocnt[k], (name, k, st[k], ocnt[k])
                out[name] = st
    finally:
        ds.close()
    return out


OPTS = {"on": {"cert": 1, "cert_policy": 0}, "every_step": {"cert": 1, "cert_policy": EVERY_STEP}, "off": {"cert": 0, "cert_policy": 0},
        "escape_off": {"cert": 1, "cert_policy": EVERY_STEP, "escape": 0}}


@pytest.mark.gpu
@pytest.mark.parametrize("strength", [0.05, 0.25, 0.5, 1.0])
def test_c3_small_frames(gpu, oracle, strength):
    scene, _ = syn.config3(n=256, size=96, strength=strength)
    st = _render(gpu, oracle, scene, ft.ImageSize(96, 96), OPTS)
    assert st["on"]["sdf_evals"] <= st["off"]["sdf_evals"]
    assert st["every_step"]["sdf_evals"] <= st["off"]["sdf_evals"]


@pytest.mark.gpu
def test_certificate_fires(gpu, oracle):
    """sdf_evals falls with the certificate on (C3 at 160^2)"""
    scene, _ = syn.config3(n=256, size=160)
    st = _render(gpu, oracle, scene, ft.ImageSize(160, 160), {"off": {"cert": 0}, "on": {"cert": 1}})
    assert st["on"]["sdf_evals"] < 0.97 * st["off"]["sdf_evals"], (st["on"]["sdf_evals"], st["off"]["sdf_evals"])


@pytest.mark.gpu
@pytest.mark.parametrize("eps", [0.0, 1e-5, 0.3, 5.0, 6.2, 7.0, -0.01])
def test_epsilon_range(gpu, oracle, eps):
    """epsilon at 0, tiny, large, near and beyond the gate (escR of C3 ~ 6.07), negative"""
    scene, _ = syn.config3(n=64, size=48)
    _render(gpu, oracle, scene, ft.ImageSize(48, 48), OPTS, eps=eps)


@pytest.mark.gpu
def test_glibc_arithmetic(gpu, oracle):
    scene, _ = syn.config3(n=128, size=64)
    with glibc_math(gpu, oracle):
        _render(gpu, oracle, scene, ft.ImageSize(64, 64), OPTS)


@pytest.mark.gpu
def test_latency_mode_forced(gpu, oracle):
    scene, _ = syn.config3(n=256, size=64)
    opts = {k: dict(v, tail_k=64) for k, v in OPTS.items()}
    _render(gpu, oracle, scene, ft.ImageSize(64, 64), opts)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1])
def test_grazing_rays_and_cameras_inside(gpu, oracle, seed):
    """Rays tangent to single children within +-2 margins, starts inside the cloud, epsilon from 1e-5 to 0.05, Length 30 and 1000, unit and
    slightly non-unit directions (the gate's 0.9 .. 1.2), explicit rays (SdfScene.trace: primary, normal, shadow ray)."""
    scene, _ = syn.config3(n=256, size=16, strength=0.25)
    rng = np.random.default_rng(seed)
    src = syn.Rng(3)
    C = np.array([src.pointInBall(4.0) for _ in range(256)], np.float64)
    R = np.array([src.range(0.1, 0.5) for _ in range(256)], np.float64)
    n = 768
    i = rng.integers(0, 256, n)
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(u, rng.normal(size=(n, 3))); v /= np.linalg.norm(v, axis=1, keepdims=True)
    eps = rng.choice([1e-5, 0.01, 0.05], (n, 1))
    M = 0.048
    closest = C[i] + u * (R[i][:, None] + eps + rng.uniform(-2.0, 2.0, (n, 1)) * M)
    start = closest - v * rng.choice([0.5, 3.0, 12.0], (n, 1))
    start[:192] = rng.normal(size=(192, 3)) * 2.0                                # cameras inside the cloud, random directions
    d = v.copy()
    d[:192] = rng.normal(size=(192, 3)); d[:192] /= np.linalg.norm(d[:192], axis=1, keepdims=True)
    d[576:] *= rng.choice([0.91, 1.19, 0.5], (192, 1))
    length = rng.choice([30.0, 1000.0], (n, 1))
    rays = np.concatenate([start, d, length, eps], axis=1).astype(np.float32)
    ds = gpu.scene(scene)
    os_ = oracle.Oracle().scene(scene)
    with np.errstate(all="ignore"):
        want, ocnt = os_.trace_rays(rays)
    evals = {}
    try:
        with options(gpu) as set_:
            for name, o in OPTS.items():
                set_(**o)
                with np.errstate(all="ignore"):
                    got, st = ds.trace_rays(rays)
                assert_bit_equal(got, want, name)
                for k in COUNTERS[1:]:
                    assert st[k] == ocnt[k], (name, k, st[k], ocnt[k])
                evals[name] = st["sdf_evals"]
    finally:
        ds.close()
    assert evals["every_step"] < evals["off"], evals


@pytest.mark.gpu
@pytest.mark.parametrize("ext", [dict(spp=4), dict(ao_samples=4, ao_radius=0.5)], ids=["spp4", "ao4"])
def test_extension_builds(gpu, oracle, ext):
    """the lean kernel's EXTENSION build certifies too (a render and its ft_render_hits twin count the same evaluations)"""
    scene, _ = syn.config3(n=128, size=48)
    st = _render(gpu, oracle, scene, ft.ImageSize(48, 48), OPTS, **ext)
    assert st["every_step"]["sdf_evals"] < st["off"]["sdf_evals"]
