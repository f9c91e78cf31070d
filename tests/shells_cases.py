"""Inputs shared by the shell tests (tests/test_shells_host.py, tests/test_gpu_shells.py): lattices whose meshes fall into several pieces, open and
closed, and plain triangle lists — each computed once, shared, never written to.

    LATTICES: name -> (values float32 [nx, ny, nz], origin, step);  mesh_of(name) -> the restated mesh (tests/mesh_restatement.py)
    LISTS:    name -> (triangles int32 [nT, 3], n_vertices)"""
import functools
import itertools

import numpy as np

import fraytracer_amd as ft

import mesh_cases
import mesh_restatement as mesh_rule

F = np.float32
NOISE_SEED = 0                             # picked so that the restatement gives the conditions test_shells_host.py asserts of "noise"


def one_cell_patterns():
    """the mesher test's generator: every sign pattern of one cell -> (values [2, 2, 2], origin, step) x 256"""
    rng = np.random.default_rng(7)
    for pattern in itertools.product((False, True), repeat=8):
        mag = rng.uniform(0.05, 2.0, (2, 2, 2)).astype(F)
        yield np.where(np.array(pattern).reshape(2, 2, 2), -mag, mag).astype(F), (0.25, -1.5, 3.0), (0.5, 0.75, 1.25)


def _grid17():
    half, n = 1.5, 17
    origin, step = (-half,) * 3, (2.0 * half / (n - 1),) * 3
    p = ft.lattice_points(origin, step, (n, n, n))
    return origin, step, p[..., 0], p[..., 1], p[..., 2]


def _ball(X, Y, Z, cx, r):
    return (np.sqrt((X - F(cx)) ** 2 + Y * Y + Z * Z) - F(r)).astype(F)


def _hollow_ball():
    origin, step, X, Y, Z = _grid17()
    return (np.abs(_ball(X, Y, Z, 0.0, 0.9)) - F(0.25)).astype(F), origin, step


def _clipped_plus_whole():
    origin, step, X, Y, Z = _grid17()
    return np.minimum(_ball(X, Y, Z, 1.2, 0.8), _ball(X, Y, Z, -0.8, 0.4)), origin, step


def _two_spheres_nan():
    d, origin, step, _ = mesh_cases.analytic()["two_spheres"]
    _, _, X, _, _ = _grid17()
    d = d.copy()
    near = np.where(X > 0, np.abs(d), np.inf).reshape(-1)             # the three lattice points nearest the surface of the sphere at x > 0
    d.reshape(-1)[np.argsort(near, kind="stable")[:3]] = np.nan
    return d, origin, step


def _egg_crate(origin, n=33):
    step = (4.0 / (n - 1),) * 3
    p = ft.lattice_points((origin,) * 3, step, (n, n, n))
    frac = (p - np.floor(p) - F(0.5)).astype(F)
    return (np.sqrt((frac * frac).sum(axis=-1, dtype=F)) - F(0.3)).astype(F), (origin,) * 3, step


def _noise():
    rng = np.random.default_rng(NOISE_SEED)
    shape = (9, 8, 10)
    d = rng.standard_normal(shape).astype(F)
    d[rng.random(shape) < 0.1] = np.nan
    d[rng.random(shape) < 0.1] = F(0.0)                                # exactly iso
    return d, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)


def _capped_rod():
    shape = (6, 6, 200)
    origin, step = (-1.0, -1.0, 0.0), (0.4, 0.4, 0.1)
    p = ft.lattice_points(origin, step, shape)
    radial = np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - F(0.7)
    return np.maximum(radial, np.abs(p[..., 2] - F(9.95)) - F(9.6)).astype(F), origin, step


def _analytic(name):
    d, origin, step, _ = mesh_cases.analytic()[name]
    return d, origin, step


LATTICES = {
    "sphere": lambda: _analytic("sphere"), "torus": lambda: _analytic("torus"), "two_spheres": lambda: _analytic("two_spheres"),
    "hollow_ball": _hollow_ball, "clipped_plus_whole": _clipped_plus_whole, "two_spheres_nan": _two_spheres_nan,
    "egg_crate": lambda: _egg_crate(0.0), "egg_crate_shifted": lambda: _egg_crate(0.5), "noise": _noise, "capped_rod": _capped_rod,
    "egg_crate_41": lambda: _egg_crate(0.5, 41),                                           # the tile tests': more than 256 tiles of 128 vertices
}


@functools.lru_cache(maxsize=None)
def lattice(name):
    d, origin, step = LATTICES[name]()
    d = np.ascontiguousarray(d, dtype=F)
    d.setflags(write=False)
    return d, origin, step


@functools.lru_cache(maxsize=None)
def mesh_of(name):
    m = mesh_rule.extract(*lattice(name))
    m.vertices.setflags(write=False)
    m.triangles.setflags(write=False)
    return m


def _strip(n, seed):
    """n triangles in a row, consistently oriented, their n + 2 vertex numbers a random permutation"""
    i = np.arange(n, dtype=np.int64)
    tri = np.where((i % 2 == 0)[:, None], np.stack([i, i + 1, i + 2], axis=1), np.stack([i, i + 2, i + 1], axis=1))
    return np.random.default_rng(seed).permutation(n + 2)[tri].astype(np.int32), n + 2


def _fan(n, closed):
    i = np.arange(1, n + 1, dtype=np.int64)
    nxt = i % n + 1 if closed else i + 1
    return np.stack([np.zeros(n, np.int64), i, nxt], axis=1).astype(np.int32), n + 1 if closed else n + 2


def _sparse_strips():
    """a strip cut into pieces (two triangles in a row left out every 997), on 20 002 of 270 001 vertex numbers: most vertices unused, 2 110 tiles of 128 vertices"""
    tri, _ = _strip(20000, 2)
    tri = tri[(np.arange(len(tri)) % 997 != 500) & (np.arange(len(tri)) % 997 != 501)]      # two in a row: the neighbours share no vertex any more
    ids = np.sort(np.random.default_rng(3).permutation(270001)[:20002])
    return ids[tri].astype(np.int32), 270001


LISTS = {
    "permuted_strip": lambda: _strip(20000, 1),
    "open_fan": lambda: _fan(3000, False),
    "closed_fan": lambda: _fan(3000, True),
    "double_cover": lambda: (np.array([[0, 1, 2], [0, 2, 1]], np.int32), 3),
    "side_twice": lambda: (np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4]], np.int32), 5),
    "shared_vertex": lambda: (np.array([[0, 1, 2], [2, 3, 4]], np.int32), 5),
    "isolated_between": lambda: (np.array([[0, 1, 2], [4, 5, 6], [6, 5, 8]], np.int32), 10),     # 3, 7 and 9 are named by no triangle
    "sparse_strips": _sparse_strips,
    "no_triangles": lambda: (np.zeros((0, 3), np.int32), 7),
}


@functools.lru_cache(maxsize=None)
def triangle_list(name):
    tri, nv = LISTS[name]()
    tri = np.ascontiguousarray(tri, dtype=np.int32)
    tri.setflags(write=False)
    return tri, int(nv)
