"""Cluster bound of the miss certificate (scene.cpp certClusters, kernels.hip ft_miss_certificate with certK != 0).

A run of >= 32 spheres is grouped into at most 32 clusters; the certificate sums n_c exp(si (dist(segment, C) - R)) per cluster and replaces a
cluster by its members' exact terms only where a lane needs it.  The CPU tests check the grouping (every child in exactly one cluster, inside its
ball, in double on the float32 values) and that the cluster bound is never below the flat float64 bound.  The GPU tests compare colours and
counters with the oracle on the same layouts under the default policy, an every-step policy and with the certificate off."""
import contextlib
import math

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import synthetic as syn
from helpers import COUNTERS, assert_bit_equal, host, options, options_left_at_defaults, seg_dist  # noqa: F401  (host, options_left_at_defaults: fixtures)

EPS, LEN = 0.01, 30.0
EVERY_STEP = 0 | (1 << 8) | (1 << 16) | (1 << 24)
OLD_DEFAULT = 1 | (6 << 8) | (16 << 16)                   # the policy before cluster bounds: one try, primaries at step 1, shadow rays at step 6


def c3_children(n=256, seed=3):
    rng = syn.Rng(seed)
    C, R = [], []
    for _ in range(n):
        C.append(rng.pointInBall(4.0)); R.append(rng.range(0.1, 0.5))
    return np.array(C, np.float32), np.array(R, np.float32)


def layout(name):
    if name.startswith("c3_"):
        return c3_children(int(name[3:]))
    if name == "two_groups":
        C, R = c3_children(256)
        C = C * np.float32(0.5)
        C[::2, 0] += np.float32(-12.0); C[1::2, 0] += np.float32(12.0)
        return C, R
    if name == "coincident":
        C, R = c3_children(64)
        C[:40] = C[0]                                          # 40 spheres on one centre, radii as drawn
        C[40:] = C[40]
        return C, R
    if name == "one_far":
        C, R = c3_children(96)
        C[17] = np.array([0.0, 9.0, 2.0], np.float32)
        return C, R
    raise ValueError(name)


LAYOUTS = ["c3_31", "c3_32", "c3_33", "c3_255", "c3_256", "c3_257", "two_groups", "coincident", "one_far"]


def scene_of(C, R, strength):
    forms = [syn.SdfForm.Primitive.sphere(Center=tuple(float(v) for v in c), Radius=float(r)) for c, r in zip(C, R)]
    obj = syn.SdfObject.create(syn.SdfMaterial.createSolid((0.9, 0.6, 0.3)), syn.SdfForm.unionSmooth(strength, forms))
    return syn.SdfScene(obj, syn.BACKGROUND, [syn.SdfLight.directional((-0.5, -1.0, 1.0), (0.5, 0.5, 0.5))])


@pytest.mark.parametrize("strength", [0.05, 0.25, 1.0])
@pytest.mark.parametrize("name", LAYOUTS)
def test_clusters_partition_and_bound(host, name, strength):
    C, R = layout(name)
    n = len(C)
    ds = host.scene(scene_of(C, R, strength))
    try:
        cert = ds.miss_certificate()
        balls, members = ds.miss_certificate_clusters()
    finally:
        ds.close()
    assert cert["margin"] > 0.0, cert
    if n < 32:
        assert len(balls) == 0 and members == []
        return
    assert 2 <= len(balls) <= 32
    leaf = max(16, math.ceil(n / 32))
    assert all(1 <= len(m) <= leaf for m in members)
    # every child in exactly one cluster: the members, stacked, are the children as a multiset (float32 values, bit for bit)
    got = np.concatenate(members).view(np.uint32)
    want = np.concatenate([C, R[:, None]], axis=1).view(np.uint32)
    assert got.shape == want.shape
    assert np.array_equal(got[np.lexsort(got.T[::-1])], want[np.lexsort(want.T[::-1])])
    # inside the ball, in double on the float32 values
    for (cx, cy, cz, rad), m in zip(balls.astype(np.float64), members):
        m = m.astype(np.float64)
        assert (np.linalg.norm(m[:, :3] - [cx, cy, cz], axis=1) + m[:, 3] <= rad).all()
        assert rad <= (np.linalg.norm(m[:, :3] - [cx, cy, cz], axis=1) + m[:, 3]).max() * (1 + 1e-5) + 1e-30
    # the cluster bound is never below the flat bound (nor, cluster by cluster, below its members' terms) on random segments
    k = 1.0 / strength
    rs = np.random.default_rng(5)
    Cd, Rd, Bd = C.astype(np.float64), R.astype(np.float64), balls.astype(np.float64)
    counts = np.array([len(m) for m in members], np.float64)
    for _ in range(300):
        a = rs.normal(size=3) * 6.0
        b = a + rs.normal(size=3) * rs.choice([0.1, 2.0, 20.0])
        flat = np.exp(-k * (seg_dist(Cd, a, b) - Rd))
        clus = counts * np.exp(-k * (seg_dist(Bd[:, :3], a, b) - Bd[:, 3]))
        assert clus.sum() >= flat.sum() * (1 - 1e-12)
        for j, m in enumerate(members):
            m = m.astype(np.float64)
            assert clus[j] >= np.exp(-k * (seg_dist(m[:, :3], a, b) - m[:, 3])).sum() * (1 - 1e-12)


def test_constants_do_not_depend_on_the_clusters(host):
    """the certificate's constants are those of the flat certificate (the cluster bound adds roundings the sum's budget already covers)"""
    ds = host.scene(syn.config3(n=256, size=16)[0])
    try:
        balls, _ = ds.miss_certificate_clusters()
        c = ds.miss_certificate()
    finally:
        ds.close()
    assert len(balls) == 16
    assert 0.045 < c["margin"] < 0.05


def _render(gpu, oracle, scene, size, opts):
    cam = syn.default_camera()
    ds = gpu.scene(scene)
    want, ocnt = oracle.Oracle().scene(scene).render(EPS, LEN, size.X, size.Y, cam.as_array(), nthreads=16)
    out = {}
    with contextlib.closing(ds), options(gpu) as set_:
        for name, o in opts.items():
            set_(**o)
            got, st = ds.render(EPS, LEN, size, cam)
            assert_bit_equal(got, want, name)
            for k in COUNTERS:
                assert st[k] == ocnt[k], (name, k, st[k], ocnt[k])
            out[name] = st
    return out


OPTS = {"default": {"cert": 1, "cert_policy": 0}, "every_step": {"cert": 1, "cert_policy": EVERY_STEP}, "off": {"cert": 0, "cert_policy": 0}}


@pytest.mark.gpu
@pytest.mark.parametrize("strength", [0.05, 0.25, 1.0])
@pytest.mark.parametrize("name", LAYOUTS)
def test_layouts_bit_exact(gpu, oracle, name, strength):
    C, R = layout(name)
    st = _render(gpu, oracle, scene_of(C, R, strength), ft.ImageSize(40, 40), OPTS)
    assert st["default"]["sdf_evals"] <= st["off"]["sdf_evals"]
    assert st["every_step"]["sdf_evals"] <= st["off"]["sdf_evals"]


@pytest.mark.gpu
def test_new_default_takes_fewer_evaluations(gpu, oracle):
    """C3 at 160^2: the retuned schedule proves more rays than the one-try schedule it replaced"""
    scene, _ = syn.config3(n=256, size=160)
    st = _render(gpu, oracle, scene, ft.ImageSize(160, 160), {"old": {"cert": 1, "cert_policy": OLD_DEFAULT}, "new": {"cert": 1, "cert_policy": 0}})
    assert st["new"]["sdf_evals"] < 0.95 * st["old"]["sdf_evals"], (st["new"]["sdf_evals"], st["old"]["sdf_evals"])
