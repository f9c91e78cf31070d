"""Inputs shared by the mesher's tests (tests/test_mesh_host.py, tests/test_gpu_mesh.py): analytic fields, the scenes and their lattice, the
CPU oracle's distances on it — computed once, shared, never written to."""
import functools

import numpy as np

import fraytracer_amd as ft
from fraytracer_amd import synthetic as syn

F = np.float32
COUNTS = (21, 18, 23)                      # 8 694 points; no count is a multiple of a wave's 64 lanes or of a tile
SPAN = 1.25                                # half-width of the scene lattices in boundary radii: the whole surface lies inside
NORMAL_EPS = 0.00125

SCENES = {
    "c3_64": lambda: syn.config3(n=64)[0],                                                 # lean
    "console_200": lambda: syn.console_scene(n=200)[0],                                    # carved tori
    "mixed_nested": lambda: syn.mixed_nested()[0],                                         # general, on-demand calls
}


@functools.lru_cache(maxsize=None)
def scene_of(name):
    return SCENES[name]()


def lattice_around(boundary, span, counts):
    """origin and step of a lattice of `counts` points over +-span boundary radii around the boundary's centre"""
    c, r = np.asarray(boundary[0:3], F), F(boundary[3])
    origin = c - F(span) * r
    step = (F(2.0 * span) * r / (np.asarray(counts, F) - F(1.0))).astype(F)
    return tuple(float(v) for v in origin), tuple(float(v) for v in step)


@functools.lru_cache(maxsize=None)
def oracle_lattice(oracle, name, libm=False):
    """(origin, step, the oracle's distances float32 COUNTS) of a scene's lattice.  libm: the caller holds the oracle's libm switch (helpers.glibc_math)
    — part of the key only, so that the two arithmetics never share an entry"""
    os_ = oracle.Oracle().scene(scene_of(name))
    O = oracle.Oracle()
    form = O.object_form(os_.object)
    origin, step = lattice_around(O.form_boundary(form), SPAN, COUNTS)
    pts = ft.lattice_points(origin, step, COUNTS).reshape(-1, 3)
    with np.errstate(all="ignore"):
        d = np.ascontiguousarray(O.form_distance(form, pts), dtype=F).reshape(COUNTS)
    d.setflags(write=False)
    return origin, step, d


def outer_layer(shape):
    m = np.zeros(shape, bool)
    m[0], m[-1], m[:, 0], m[:, -1], m[:, :, 0], m[:, :, -1] = True, True, True, True, True, True
    return m


def analytic(n=17, half=1.5):
    """name -> (values float32 [n, n, n], origin, step, Euler characteristic) over +-half: a sphere, a torus, two disjoint spheres"""
    origin, step = (-half,) * 3, (2.0 * half / (n - 1),) * 3
    p = ft.lattice_points(origin, step, (n, n, n))
    X, Y, Z = p[..., 0], p[..., 1], p[..., 2]
    ball = lambda cx, r: (np.sqrt((X - F(cx)) ** 2 + Y * Y + Z * Z) - F(r)).astype(F)
    ring = np.sqrt(X * X + Y * Y) - F(0.9)
    return {"sphere": (ball(0.0, 1.0), origin, step, 2),
            "torus": ((np.sqrt(ring * ring + Z * Z) - F(0.35)).astype(F), origin, step, 0),
            "two_spheres": (np.minimum(ball(0.7, 0.45), ball(-0.7, 0.45)), origin, step, 4)}
