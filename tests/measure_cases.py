"""Crafted inputs of the measure tests (tests/test_measure_host.py, tests/test_gpu_measure.py): each computed once, shared, never written to.

    solids()            name -> (vertices float32 [nV, 3], triangles int32 [nT, 3], exact volume, exact area or None, exact moment or None)
    finish_sums()       Python ints: the crafted 128-bit sums of the conversion test
    sqrt_random()       (vertices, triangles): a few thousand triangles of one binade of sizes, |n|^2 all over float64
    sqrt_near_squares() (vertices, triangles): 256 triangles whose |n|^2 is a perfect square +- 1 ulp (128 each)
    extremes()          name -> (vertices, triangles, vertex_label, triangle_label, n_shells)
    mixed(n)            n triangles with positive and negative terms over more than 64 bits, for the order tests"""
import functools
import math
from fractions import Fraction

import numpy as np

F = np.float32


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


CUBE_CORNERS = np.array([[x, y, z] for x in (0, 2) for y in (0, 2) for z in (0, 2)], F)      # index = 4 x + 2 y + z (bits)
# two triangles per face, counter-clockwise seen from the outside
CUBE_TRIANGLES = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
OCTA_CORNERS = np.array([[3, 0, 0], [-3, 0, 0], [0, 4, 0], [0, -4, 0], [0, 0, 5], [0, 0, -5]], F)
OCTA_TRIANGLES = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)


@functools.lru_cache(maxsize=None)
def solids():
    shift = np.array([100, -37, 5], F)
    out = {
        "cube": (CUBE_CORNERS.copy(), CUBE_TRIANGLES.copy(), 8.0, 24.0, (8.0, 8.0, 8.0)),
        "cube_translated": (CUBE_CORNERS + shift, CUBE_TRIANGLES.copy(), 8.0, 24.0, (8.0 * 101, 8.0 * -36, 8.0 * 6)),
        "cube_reversed": (CUBE_CORNERS.copy(), CUBE_TRIANGLES[:, ::-1].copy(), -8.0, 24.0, (-8.0, -8.0, -8.0)),
        # |x| / 3 + |y| / 4 + |z| / 5 <= 1: volume 4/3 * 3 * 4 * 5 = 80; the areas are no integers
        "octahedron": (OCTA_CORNERS.copy(), OCTA_TRIANGLES.copy(), 80.0, None, (0.0, 0.0, 0.0)),
        "triangle": (np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0]], F), np.array([[0, 1, 2]], np.int32), 0.0, 6.0, (0.0, 0.0, 0.0)),
    }
    for v, t, *_ in out.values():
        _frozen(v, t)
    return out


def finish_sums():
    """the patterns of the conversion test: small values, ties and near-ties at bit 53, the same with guard and sticky bits round the word
    boundary (bits 64 .. 121), a low word of all ones under a high word of 0 and of -1, and every negative"""
    base = [0, 1, 2 ** 53 + 1, 2 ** 53 + 3, 2 ** 54 + 2 + 1, 2 ** 54 + 2 - 1, 2 ** 54 + 2, 2 ** 53 - 1, 2 ** 64 - 1, 2 ** 64, 2 ** 64 + 1]
    out = list(base)
    for shift in range(1, 68):                                         # 2^53 + 1 << 67 has its top bit at 120; 2^54 + 3 << 67 at 121
        out += [p << shift for p in base[2:7]]
    out += [(2 ** 53 + 1) * 2 ** 64 + 1, (2 ** 53 + 1) * 2 ** 64 - 1, (2 ** 53 + 3) * 2 ** 64 - 1, (2 ** 53 + 1) * 2 ** 11 * (2 ** 53) + 1,
            2 ** 121 + 2 ** 68, 2 ** 121 + 2 ** 68 + 1, 2 ** 121 + 2 ** 68 - 1, 2 ** 121 + 3 * 2 ** 68, 2 ** 122 - 1, 2 ** 122]
    out += [-q for q in out if q]
    out += [2 ** 64 - 1, -1, -(2 ** 64), -(2 ** 64) - 1, -(2 ** 64) + 1]   # as words: (ones, 0), (ones, -1), (0, -1), (ones, -2), (1, -1)
    return out


@functools.lru_cache(maxsize=None)
def sqrt_random(n=4096, seed=11):
    """n triangles of their own three vertices each: coordinates uniform in (-1, 1) times a power of two that differs from triangle to triangle by
    at most 2^3 (so no area falls below the call's quantum: the record's area is the term itself)"""
    rng = np.random.default_rng(seed)
    scale = np.ldexp(1.0, rng.integers(-3, 1, n))[:, None, None]
    v = (rng.uniform(-1.0, 1.0, (n, 3, 3)) * scale).astype(F).reshape(-1, 3)
    t = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    return _frozen(v, t)


def _f32_below(x):
    """the largest float32 whose square is at most the Fraction x (x >= 0)"""
    f = F(math.sqrt(x))
    while Fraction(float(f)) ** 2 > x:
        f = np.nextafter(f, F(0))
    return f


@functools.lru_cache(maxsize=None)
def sqrt_near_squares(n_each=128, seed=12):
    """triangles (0, (big, p, 0), (0, q, 1)): n = (p, -big, big q), so |n|^2 = (p^2 + big^2) + (big q)^2 with three free float32 values.  For an
    integer K below 2^24 the target K^2 + ulp is reached with big = K, the target K^2 - ulp with big = K - 1; candidates whose float64 sum is not
    exactly the target are dropped (test_measure_host.py checks the property of the ones kept)"""
    rng = np.random.default_rng(seed)
    tris = {+1: [], -1: []}
    while min(len(x) for x in tris.values()) < n_each:
        K = int(rng.integers(2 ** 20, 2 ** 24))
        ulp = Fraction(2) ** (math.frexp(float(K * K))[1] - 1 - 52)
        for sign in (+1, -1):
            if len(tris[sign]) >= n_each:
                continue
            target = Fraction(K * K) + sign * ulp
            big = K if sign > 0 else K - 1
            p = _f32_below(target - big * big)
            rest = target - big * big - Fraction(float(p)) ** 2
            q = F(math.sqrt(rest) / big)
            nz = np.float64(big) * np.float64(q)
            got = (np.float64(p) * np.float64(p) + np.float64(big) * np.float64(big)) + nz * nz
            if Fraction(float(got)) == target:
                tris[sign].append([[0, 0, 0], [big, p, 0], [0, q, 1]])
    v = np.array(tris[+1] + tris[-1], F).reshape(-1, 3)
    t = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    return _frozen(v, t)


def _random_triangles(rng, n_vertices, n_triangles, magnitude):
    v = (rng.uniform(-1.0, 1.0, (n_vertices, 3)) * magnitude).astype(F)
    t = rng.integers(0, n_vertices, (n_triangles, 3)).astype(np.int32)
    return v, t


def of_extent(E, n=64, seed=5):
    """n random triangles whose largest |coordinate| lies in [2^(E-1), 2^E): E >= -148"""
    rng = np.random.default_rng(seed + 1000 + E)
    with np.errstate(all="ignore"):
        limit = np.nextafter(F(np.ldexp(1.0, E)), F(0))                # the largest float32 below 2^E (2^128 is float32's infinity; below 2^-148 lies 2^-149 only)
        v = np.clip(np.ldexp(rng.uniform(-1.0, 1.0, (3 * n, 3)), E).astype(F), -limit, limit)
    v[0, 0] = limit
    return _frozen(v, np.arange(3 * n, dtype=np.int32).reshape(n, 3))


@functools.lru_cache(maxsize=None)
def extremes():
    rng = np.random.default_rng(21)
    out = {}
    for E in (-148, -140, -126):                                        # every coordinate a float32 denormal
        v, t = of_extent(E)
        out[f"denormal_E{E}"] = (v, t, np.arange(len(v), dtype=np.int32) // 3 % 3, np.arange(len(t), dtype=np.int32) % 3, 3)
    v, t = _random_triangles(rng, 40, 90, 3e38)
    v[0] = [3e38, -3e38, 3e38]
    out["huge_E128"] = (v, t, (np.arange(40) % 2).astype(np.int32), (np.arange(90) % 2).astype(np.int32), 2)
    out["all_zero"] = (np.zeros((5, 3), F), np.array([[0, 1, 2], [2, 3, 4]], np.int32), np.zeros(5, np.int32), np.zeros(2, np.int32), 1)
    # one NaN, one +inf, one -inf coordinate in different triangles and shells; the non-finite values count for neither extent nor box
    v, t = _random_triangles(rng, 30, 60, 4.0)
    t = np.sort(rng.permuted(np.tile(np.arange(30), (60, 1)), axis=1)[:, :3], axis=1).astype(np.int32)
    vl, tl = (np.arange(30) % 3).astype(np.int32), (np.arange(60) % 3).astype(np.int32)
    v[3, 1], v[10, 0], v[20, 2] = np.nan, np.inf, -np.inf
    out["non_finite"] = (v, t, vl, tl, 3)
    # -0 against +0: a shell whose x values are -0 and +0 only, one whose largest is -0, one whose smallest is +0
    v = np.array([[-0.0, 0.0, 1.0], [0.0, -0.0, 2.0], [-0.0, 0.0, 3.0], [-1.0, -0.0, 0.0], [-0.0, -2.0, -0.0], [-3.0, -0.0, 0.0], [0.0, 1.0, 0.0], [2.0, 0.0, 0.0],
                  [0.0, 0.0, 5.0]], F)
    out["signed_zero"] = (v, np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], np.int32), np.repeat(np.arange(3), 3).astype(np.int32), np.arange(3, dtype=np.int32), 3)
    # shell 1 has no finite y at all (and its only triangle is unmeasured); shell 2 has no vertex: +inf / -inf boxes
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, np.nan, 1], [2, np.inf, 2], [3, -np.inf, 5]], F)
    out["no_finite_value"] = (v, np.array([[0, 1, 2], [3, 4, 5]], np.int32), np.array([0, 0, 0, 1, 1, 1], np.int32), np.array([0, 1], np.int32), 3)
    # indices and labels out of range: triangle 1 names vertex 7 of 6 (unmeasured in shell 0), triangle 2 a negative one, triangle 3 has label 5 of 2
    # (left out), triangle 4 label -1 (left out); vertex 4 has label 9 (in no box), vertex 5 label -1
    v, _ = _random_triangles(rng, 6, 1, 10.0)
    out["out_of_range"] = (v, np.array([[0, 1, 2], [0, 1, 7], [-1, 2, 3], [1, 2, 3], [2, 3, 4], [3, 2, 1]], np.int32), np.array([0, 0, 1, 1, 9, -1], np.int32),
                           np.array([0, 0, 1, 5, -1, 1], np.int32), 2)
    # unused vertices count for the extent: the largest coordinate belongs to a vertex no triangle names and no shell holds
    v, t = _random_triangles(rng, 12, 20, 1.0)
    v[11] = [1000.0, 0.0, 0.0]
    vl = np.zeros(12, np.int32)
    vl[11] = -1
    out["unused_vertex_sets_extent"] = (v, np.minimum(t, 10).astype(np.int32), vl, np.zeros(20, np.int32), 1)
    for parts in out.values():
        _frozen(*parts)
    return out


@functools.lru_cache(maxsize=None)
def mixed(n=20000, seed=31):
    """n triangles over 6 000 vertices, coordinates uniform in (-1, 1) * 100 with a few far smaller: volumes and moments of both signs whose
    quantised terms fill 80 to 90 bits, so the low words wrap and the high words are sign-extended; a handful of non-finite vertices"""
    rng = np.random.default_rng(seed)
    v, t = _random_triangles(rng, 6000, n, 100.0)
    v[::97] *= F(2.0 ** -20)
    v[5, 0], v[77, 2] = np.nan, np.inf
    return _frozen(v, t)
