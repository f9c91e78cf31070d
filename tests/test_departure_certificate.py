"""The departure certificate (FT_OPT_DEPART; kernels.hip ft_miss_certificate with a tilted margin, scene.cpp "Departure certificate").

A ray of a scene that is one smooth union of spheres ends as a miss once, along the rest of its line o + t dir inside the clip ball,
f(x(t)) - m(t) >= epsilon with m(t) = depE (t / epsilon + 2) + depB + kappa.  The kernel shows it child by child: a term is taken at the clamped closest
approach t_c, lifted by slope t_c.  These CPU tests pin the constants to their formula and hold a float64 restatement of the kernel's condition
against the oracle's own float32 marches: it may hold on NO line whose march ends in a hit."""
import math

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import synthetic as syn
from helpers import host  # noqa: F401  (fixture)

EPS = 0.01
N_CAP = 131072.0


def constants(escR, cinf, strength, n):
    """scene.cpp "Departure certificate", restated"""
    u = 2.0 ** -24
    Rb = 2.5 * escR * 1.001
    e3 = 3.0 * 2.0 ** -23 * (cinf + 3.0 * Rb)
    eGeo = 8.0 * u * 5.0 * escR + 16.0 * u * (cinf + 10.0 * escR)
    eSum = strength * ((2.0 * n + 4096.0) * 2.0 ** -23 + 2e-4)
    tMax = 2.0 * Rb / 0.9
    step = 1.01 * e3
    cap = 0.05 * escR
    return {"step": step, "base": (3.0 * eGeo + eSum + 1e-6 * tMax) * 1.01 + 1e-6, "kappa": 1.01 * 0.505 * 4.2 * escR / 0.81,
            "eps_min": 1.01 * max(tMax * step / (cap - 2.0 * step), tMax / (N_CAP - 4.0)), "clip": cap}


def spheres(n=256):
    src = syn.Rng(3)
    C, R = [], []
    for _ in range(n):
        C.append(src.pointInBall(4.0)); R.append(src.range(0.1, 0.5))
    return np.array(C, np.float64), np.array(R, np.float64)


class Model:
    """the kernel's condition in float64, from the library's own constants"""

    def __init__(self, host, strength, n=256, scene=None, C=None, R=None):
        self.scene = scene if scene is not None else syn.config3(n=n, size=64, strength=strength)[0]
        ds = host.scene(self.scene)
        try:
            self.sup = ds.support_sphere()
            self.k = ds.departure_certificate()
            self.flat = ds.miss_certificate()
            self.occ = ds.occlusion_certificate()
        finally:
            ds.close()
        self.C, self.R = (np.array(C, np.float64), np.array(R, np.float64)) if C is not None else spheres(n)
        self.strength = strength

    def margin(self, eps):
        """(slope, base) as capi.cpp departSchedule forms them"""
        slope = self.k["step"] / eps * (1.0 + 1e-6)
        return slope, (2.0 * self.k["step"] + self.k["base"] + self.k["kappa"] * slope * slope) * (1.0 + 1e-6)

    def segment(self, rays):
        r = np.asarray(rays, np.float32).astype(np.float64)
        o, d, L, eps = r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7]
        k = self.k
        dd = (d * d).sum(1)
        w = o - np.array(self.sup[:3])
        ww, b = (w * w).sum(1), (w * d).sum(1)
        with np.errstate(all="ignore"):
            gate = (k["base"] >= 0) & (eps >= k["eps_min"]) & (eps <= self.sup[3]) & (L > 0) & (L < 1e9) & (dd >= np.float32(0.81)) & (dd <= np.float32(1.44)) & (ww <= self.flat["rho2"])
            Rc = (self.sup[3] + eps + k["clip"]) * 1.001
            disc = b * b - dd * (ww - Rc * Rc)
            sq = np.sqrt(np.maximum(disc, 0.0))
            t0 = np.maximum((-b - sq) / dd, 0.0); t1 = np.minimum((sq - b) / dd, L * k["len_factor"])
        return o, d, eps, gate & (disc > 0) & (t1 > t0), t0, t1

    def holds(self, rays):
        """rays [m, 8] float32 -> bool [m]: sum_i exp(-(d_i(t_c) - slope t_c) / s) < 0.9999 exp(-(epsilon + base) / s), t_c the closest approach of child i clamped to the clipped segment"""
        o, d, eps, ok, t0, t1 = self.segment(rays)
        with np.errstate(all="ignore"):
            slope, base = self.margin(eps)
            dd = (d * d).sum(1)
            rel = self.C[None] - o[:, None]
            tc = np.clip((rel * d[:, None]).sum(-1) / dd[:, None], t0[:, None], t1[:, None])
            dist = np.linalg.norm(rel - tc[..., None] * d[:, None], axis=-1) - self.R[None]
            lifted = dist - slope[:, None] * tc
            lhs = -(eps + base) / self.strength
            normal = lhs * 1.44269504 >= -100.0 + slope * t0 * 1.44269504 / self.strength
            with np.errstate(over="ignore"):
                s = np.exp(-lifted / self.strength - lhs[:, None]).sum(1)
        return ok & normal & (s < 0.9999)


START = {0.05: 4.7, 0.25: 6.0, 1.0: 10.0}


def shadow_lines(oracle, scene, n, eps, seed, start=6.0):
    """two shadow lines from every hit record of n random rays into the cloud: towards the scene's light, and a random direction about the normal"""
    g = np.random.default_rng(seed)
    o = g.normal(size=(n, 3)); o *= start / np.linalg.norm(o, axis=1, keepdims=True)
    aim = g.normal(size=(n, 3)); aim *= (3.5 * g.uniform(0.0, 1.0, (n, 1)) ** (1.0 / 3.0)) / np.linalg.norm(aim, axis=1, keepdims=True)
    d = aim - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d, np.full((n, 1), 30.0), np.full((n, 1), eps)], axis=1).astype(np.float32)
    with np.errstate(all="ignore"):
        rec, _ = oracle.Oracle().scene(scene).object_try_trace(rays)
    rec = rec[rec[:, 14].view(np.int32) != 0]
    light = -np.array([-0.5, -1.0, 1.0]); light /= np.linalg.norm(light)
    rnd = g.normal(size=(len(rec), 3)); rnd /= np.linalg.norm(rnd, axis=1, keepdims=True)
    rnd = rec[:, 8:11] + 0.9 * rnd; rnd /= np.linalg.norm(rnd, axis=1, keepdims=True)
    out = []
    for d in (np.repeat(light[None], len(rec), 0), rnd):
        d32 = d.astype(np.float32)
        out.append(np.concatenate([rec[:, 0:3], d32, np.full((len(rec), 1), 1000.0, np.float32), np.full((len(rec), 1), eps, np.float32)], axis=1))
    return np.concatenate(out).astype(np.float32)


def march_hits(oracle, scene, rays):
    """does the oracle's float32 march of each ray end in a hit (SdfForm.tryTrace)"""
    with np.errstate(all="ignore"):
        out, _ = oracle.Oracle().scene(scene).form_try_trace(rays)
    return out[:, 9].view(np.int32) != 0


@pytest.mark.parametrize("n", [64, 256])
@pytest.mark.parametrize("strength", [0.05, 0.25, 1.0])
def test_constants_are_the_stated_formula(host, strength, n):
    m = Model(host, strength, n=n)
    cinf = max(abs(v) for v in m.sup[:3])
    want = constants(m.sup[3], cinf, strength, n)
    for name, v in want.items():
        assert m.k[name] == pytest.approx(v, rel=2e-5), (name, m.k[name], v)
    assert m.k["step"] == m.occ["step"]                                # depE is occE itself
    assert m.k["len_factor"] == pytest.approx(max(m.flat["len_factor"], 1.0 + (N_CAP + 2002.0) * 2.0 ** -22), rel=1e-6)
    assert m.k["steps"] >= max(m.flat["steps"], N_CAP + 2000.0)
    assert m.k["eps_min"] < EPS and m.k["clip"] < 0.06 * m.sup[3]
    # the margin at a ray's start at epsilon 0.01 is far below the flat certificate's, and it reaches it only after many units
    slope, base = m.margin(EPS)
    assert base < 0.05 * m.flat["margin"] and slope * 10.0 + base < m.flat["margin"]
    # the largest slope the gate admits stays inside kappa's range: slope^2 / |dir|^2 <= 0.039
    assert (m.k["step"] / m.k["eps_min"]) ** 2 / 0.81 < 0.039


def test_no_constants_without_the_shape(host):
    for scene in (syn.config2()[0], syn.mixed_nested()[0], syn.console_like(n=50)[0], syn.config3(n=64, size=16, strength=0.005)[0]):
        ds = host.scene(scene)
        try:
            assert ds.departure_certificate()["base"] < 0.0
        finally:
            ds.close()


@pytest.mark.parametrize("n", [64, 256])
@pytest.mark.parametrize("strength", [0.05, 0.25, 1.0])
def test_condition_against_the_oracles_marches(host, oracle, strength, n):
    """it holds on NO line whose march ends in a hit; the share of the lit lines it holds on is printed, not asserted"""
    m = Model(host, strength, n=n)
    rays = shadow_lines(oracle, m.scene, 2500, EPS, 5, START[strength])
    assert len(rays) >= 500
    cond = m.holds(rays)
    hit = march_hits(oracle, m.scene, rays)
    lit = ~hit
    print(f"strength {strength} n {n}: lines {len(rays)} lit {int(lit.sum())} condition holds at birth on {int(cond.sum())} = {cond.sum() / max(lit.sum(), 1):.3f} of the lit")
    assert not (cond & hit).any(), rays[cond & hit][:4]


def test_lines_grazing_one_sphere(host, oracle):
    """lines that pass one sphere at a clearance of epsilon + m(t) -2 .. +2 margins, the closest approach at t = 0.05, 0.5 and 5"""
    g = np.random.default_rng(7)
    m = Model(host, 0.25, n=2)
    n = 900
    i = g.integers(0, 2, n)
    u = g.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(u, g.normal(size=(n, 3))); v /= np.linalg.norm(v, axis=1, keepdims=True)
    back = g.choice([0.05, 0.5, 5.0], (n, 1))
    slope, base = m.margin(EPS)
    marg = base + slope * back
    closest = m.C[i] + u * (m.R[i][:, None] + EPS + marg * (1.0 + g.integers(-2, 3, (n, 1)) * 0.5) + g.integers(-2, 3, (n, 1)) * m.k["base"])
    graze = np.concatenate([closest - v * back, v, np.full((n, 1), 1000.0), np.full((n, 1), EPS)], axis=1).astype(np.float32)
    cond = m.holds(graze); hit = march_hits(oracle, m.scene, graze)
    print(f"grazing: holds {int(cond.sum())} hits {int(hit.sum())} of {n}")
    assert cond.any() and (~cond).any()
    assert not (cond & hit).any()


def test_gate_edges(host, oracle):
    m = Model(host, 0.25)
    k = m.k
    base = shadow_lines(oracle, m.scene, 400, EPS, 9)[:240]
    assert m.holds(base).any()
    # epsilon at the floor, one float below it, 0 and negative
    floor = np.float32(k["eps_min"])
    at = base.copy(); at[:, 7] = floor
    c_at = m.holds(at)
    assert not (c_at & march_hits(oracle, m.scene, at)).any()
    for e in (np.nextafter(floor, np.float32(0.0)), np.float32(0.0), np.float32(-0.01)):
        r = base.copy(); r[:, 7] = e
        assert not m.holds(r).any(), e
    # |dir|^2 at both gate edges and one float outside
    for scale, may in ((0.9001, True), (1.0, True), (1.1999, True)):
        r = base.copy(); r[:, 3:6] *= np.float32(scale)
        c = m.holds(r)
        assert c.any() == may, scale
        assert not (c & march_hits(oracle, m.scene, r)).any(), scale
    for scale in (0.8999, 1.2001):
        r = base.copy(); r[:, 3:6] *= np.float32(scale)
        assert not m.holds(r).any(), scale
    # ... one float: an axis-parallel direction whose square is the first inside the gate, and its neighbour outside
    lit = base[c_lit := m.holds(base)][:1]
    axis = lit[0, 3:6] / np.linalg.norm(lit[0, 3:6])
    for edge, outwards in ((0.81, 0.0), (1.44, 2.0)):
        x = np.float32(math.sqrt(edge))
        while not (np.float32(0.81) <= np.float64(x) ** 2 <= np.float32(1.44)):
            x = np.nextafter(x, np.float32(1.0))
        while np.float32(0.81) <= np.float64(np.nextafter(x, np.float32(outwards))) ** 2 <= np.float32(1.44):
            x = np.nextafter(x, np.float32(outwards))
        inside = lit.copy(); inside[0, 0:3] = (0.0, 0.0, 0.0); inside[0, 3:6] = (x, 0.0, 0.0)
        outside = inside.copy(); outside[0, 3] = np.nextafter(x, np.float32(outwards))
        assert m.segment(inside)[3][0] and not m.segment(outside)[3][0], edge
    del axis, c_lit
    # Length ending inside the clip ball: the segment ends there, and a hit beyond it does not count
    c = m.holds(base)
    _, _, _, _, t0, t1 = m.segment(base)
    r = base.copy(); r[:, 6] = (0.5 * (t0 + t1)).astype(np.float32) + np.float32(1e-3)
    cs = m.holds(r)
    assert cs.sum() >= c.sum() and not (cs & march_hits(oracle, m.scene, r)).any()
    # a start beyond certRho2
    far = base.copy(); far[:, 0:3] = (np.array(m.sup[:3]) + np.array([0.0, 0.0, 1.0]) * math.sqrt(m.flat["rho2"]) * 1.001).astype(np.float32)
    assert not m.holds(far).any()


def two_clusters(strength=0.05, light=(-1.0, 0.0, 0.0)):
    """two spheres of radius 0.5 at x = -6 and x = +6 under a weak union: half way between them every term of the reference's float32 sum has flushed to 0"""
    C, R = [(-6.0, 0.0, 0.0), (6.0, 0.0, 0.0)], [0.5, 0.5]
    forms = [ft.SdfForm.Primitive.sphere(Center=c, Radius=r) for c, r in zip(C, R)]
    obj = ft.SdfObject.create(ft.SdfMaterial.createSolid((0.9, 0.6, 0.3)), ft.SdfForm.unionSmooth(strength, forms))
    return ft.SdfScene(obj, syn.BACKGROUND, [ft.SdfLight.directional(light, (0.5, 0.5, 0.5))]), C, R


def test_gap_where_every_term_underflows(host, oracle):
    """lines across the gap towards the far sphere: some marches step over the dead zone and hit, and on none of those may the condition hold; lines that
    leave the near sphere outwards are lit and certified"""
    scene, C, R = two_clusters()
    m = Model(host, 0.05, scene=scene, C=C, R=R)
    assert m.k["base"] > 0.0
    g = np.random.default_rng(3)
    n = 256
    off = g.uniform(-0.3, 0.3, (n, 2)); off[0] = 0.0
    far = np.concatenate([np.full((n, 1), -5.489), off, np.tile([1.0, 0.0, 0.0], (n, 1)), np.full((n, 1), 1000.0), np.full((n, 1), EPS)], axis=1).astype(np.float32)
    hit = march_hits(oracle, scene, far)
    c = m.holds(far)
    assert 0 < hit.sum() < n and not (c & hit).any()
    away = far.copy(); away[:, 3] = -1.0; away[:, 0] = -6.52
    ca = m.holds(away)
    assert ca.all() and not march_hits(oracle, scene, away).any()


def test_per_child_inequality_with_kappa(host):
    """min over the segment of |x(t) - c| - slope t  >=  |x(t_c) - c| - slope t_c - kappa on 10^5 random (segment, child) pairs, the slope at the gate's largest"""
    m = Model(host, 0.25)
    escR = m.sup[3]
    slope = m.k["step"] / m.k["eps_min"]
    kappa = m.k["kappa"] * slope * slope
    assert 0.0 < kappa < 1e-3 * escR
    g = np.random.default_rng(11)
    n = 100000
    Rc = 2.06 * escR
    o = g.normal(size=(n, 3)); o *= (Rc * g.uniform(0.0, 1.0, (n, 1)) ** (1.0 / 3.0)) / np.linalg.norm(o, axis=1, keepdims=True)
    d = g.normal(size=(n, 3)); d *= g.uniform(0.9, 1.2, (n, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
    c = g.normal(size=(n, 3)); c *= (escR * g.uniform(0.0, 1.0, (n, 1)) ** (1.0 / 3.0)) / np.linalg.norm(c, axis=1, keepdims=True)
    dd = (d * d).sum(1); b = (o * d).sum(1)
    t1 = (-b + np.sqrt(b * b - dd * ((o * o).sum(1) - Rc * Rc))) / dd * g.uniform(0.05, 1.0, n)
    tc = np.clip(((c - o) * d).sum(1) / dd, 0.0, t1)
    bound = np.linalg.norm(o + tc[:, None] * d - c, axis=1) - slope * tc - kappa
    t = np.linspace(0.0, 1.0, 2001)[None] * t1[:, None]
    for lo in range(0, n, 5000):
        s = slice(lo, lo + 5000)
        val = np.linalg.norm(o[s, None] + t[s, :, None] * d[s, None] - c[s, None], axis=-1) - slope * t[s]
        assert (val.min(1) >= bound[s]).all()
    # and kappa is not idle: without it the bound fails somewhere
    val0 = np.linalg.norm(o + tc[:, None] * d - c, axis=1) - slope * tc
    tau = slope * np.linalg.norm(o + tc[:, None] * d - c, axis=1) / (dd * np.sqrt(1.0 - slope * slope / dd))
    inner = (tc > 0) & (tc + tau < t1)
    true_min = np.linalg.norm(o + (tc + tau)[:, None] * d - c, axis=1) - slope * (tc + tau)
    assert inner.any() and (true_min[inner] < val0[inner]).all() and (true_min[inner] >= bound[inner]).all()


def test_cluster_form_bounds_the_flat_form(host):
    """a cluster's term n_c exp(-(dist(S, C) - R - slope t_C - slope R / 0.9) / s) is at least the sum of its members' lifted terms, on random segments"""
    m = Model(host, 0.25)
    ds = host.scene(m.scene)
    try:
        clusters, members = ds.miss_certificate_clusters()
    finally:
        ds.close()
    assert len(clusters) >= 2
    slope, _ = m.margin(EPS)
    g = np.random.default_rng(13)
    n = 400
    o = g.normal(size=(n, 3)); o *= 5.0 / np.linalg.norm(o, axis=1, keepdims=True)
    aim = g.normal(size=(n, 3))
    d = aim - o; d *= g.uniform(0.9, 1.2, (n, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
    t1 = g.uniform(0.5, 12.0, n)
    dd = (d * d).sum(1)

    def lifted(c, r):
        tc = np.clip(((c[None] - o) * d).sum(1) / dd, 0.0, t1)
        return np.linalg.norm(o + tc[:, None] * d - c[None], axis=1) - r - slope * tc

    for cl, kids in zip(np.asarray(clusters, np.float64), members):
        kids = np.asarray(kids, np.float64)
        bound = len(kids) * np.exp(-(lifted(cl[:3], cl[3]) - slope * cl[3] / 0.9) / m.strength)
        exact = sum(np.exp(-lifted(k[:3], k[3]) / m.strength) for k in kids)
        assert (bound >= exact * (1.0 - 1e-12)).all()
