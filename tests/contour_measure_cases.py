"""Inputs shared by the contour measures' tests (tests/test_contour_measure_host.py, tests/test_gpu_contour_measure.py): contours no slicer would
write, given as (points float32 [nP, 3], polylines int32 [nL, 4] with the columns of ft_polyline, axis, n_slices), and the torus of the public path."""
import functools

import numpy as np

F = np.float32
BLOCK, WAVE = 256, 64                      # the kernels' workgroup and a wave: what the shapes below straddle


def records(rows):
    return np.asarray(rows, np.int32).reshape(-1, 4)


def in_plane(uv, axis, along=0.0):
    """float32 [n, 3]: in-plane coordinates (u, v) placed at (axis + 1) % 3 and (axis + 2) % 3, `along` along the axis"""
    uv = np.asarray(uv, F).reshape(-1, 2)
    p = np.empty((len(uv), 3), F)
    p[:, axis] = along
    p[:, (axis + 1) % 3], p[:, (axis + 2) % 3] = uv[:, 0], uv[:, 1]
    return p


def wobbly_loop(n, seed, radius=1.0, centre=(0.0, 0.0)):
    """n points counter-clockwise around `centre`, radii and angles jittered: float32 [n, 2] with all 24 bits in use"""
    rng = np.random.default_rng(seed)
    t = (np.arange(n) + rng.uniform(-0.3, 0.3, n)) * (2.0 * np.pi / max(n, 1))
    r = radius * rng.uniform(0.7, 1.3, n)
    return np.stack([centre[0] + r * np.cos(t), centre[1] + r * np.sin(t)], axis=1).astype(F)


SINGLE_COUNTS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000)


def single(n, closed, axis=2):
    """one polyline of n points: 1000 points span several workgroups"""
    return in_plane(wobbly_loop(n, 100 + n), axis, 0.5), records([[0, n, 0, int(closed)]]), axis, 1


def straddling():
    """a closed polyline of 300 points behind one of 250: its first point lies in wave 3 of workgroup 0, its last in wave 0 of workgroup 2, so the
    closing segment's two ends sit in different waves and in different workgroups"""
    uv = np.concatenate([wobbly_loop(250, 1), wobbly_loop(300, 2, 2.0, (0.25, -0.5))])
    assert 250 // BLOCK != 549 // BLOCK and (250 % BLOCK) // WAVE != (549 % BLOCK) // WAVE
    return in_plane(uv, 2), records([[0, 250, 0, 1], [250, 300, 0, 1]]), 2, 1


def triangles64():
    """64 three-point loops back to back, alternately counter-clockwise and clockwise: 21 or 22 runs in every wave, runs that straddle waves"""
    uv = []
    for l in range(64):
        tri = wobbly_loop(3, 300 + l, 0.5 + 0.01 * l, (0.1 * (l % 8), 0.1 * (l // 8)))
        uv.append(tri if l % 2 == 0 else tri[::-1])
    return in_plane(np.concatenate(uv), 0), records([[3 * l, 3, l % 3, 1] for l in range(64)]), 0, 3


def lane_starts():
    """runs that start on lane 0 (points 0, 128) and on lane 63 (points 63, 191), one of them a single lane long"""
    rows = [[0, 63, 0, 1], [63, 65, 0, 0], [128, 63, 1, 1], [191, 1, 1, 0], [192, 40, 0, 1]]
    uv = np.concatenate([wobbly_loop(c, 400 + i) for i, (_, c, _, _) in enumerate(rows)])
    return in_plane(uv, 1), records(rows), 1, 2


def tiny_counts():
    """polylines of 0 and 1 points, closed and open, between ordinary ones; point 7 belongs to no polyline and still counts for the extent"""
    uv = np.concatenate([wobbly_loop(7, 5), [[900.0, -900.0]]]).astype(F)
    rows = [[0, 0, 0, 1], [0, 1, 0, 1], [1, 1, 1, 0], [2, 0, 1, 0], [2, 5, 0, 1], [7, 0, 1, 1]]
    return in_plane(uv, 2), records(rows), 2, 2


def permuted(axis):
    """the same polygon (an L with a square hole, integer coordinates) in the plane of each axis"""
    outer = [[0, 0], [6, 0], [6, 2], [2, 2], [2, 5], [0, 5]]
    hole = [[1, 1], [1, 2], [2, 2], [2, 1]]                           # clockwise: (1,1) -> (1,2) -> (2,2) -> (2,1)
    uv = np.asarray(outer + hole, F)
    return in_plane(uv, axis, 3.0), records([[0, 6, 0, 1], [6, 4, 0, 1]]), axis, 1


def scattered_slices():
    """polylines of slices 0, 1, 0, 2, 1 (a slice's polylines are not contiguous) and a slice 3 without any"""
    rows, uv, first = [], [], 0
    for i, (w, n, closed, flip) in enumerate([(0, 40, 1, False), (1, 70, 1, False), (0, 9, 1, True), (2, 130, 0, False), (1, 33, 1, True)]):
        loop = wobbly_loop(n, 600 + i, 1.0 + i)
        uv.append(loop[::-1] if flip else loop)
        rows.append([first, n, w, closed])
        first += n
    return in_plane(np.concatenate(uv), 2), records(rows), 2, 4


def non_finite():
    """non-finite u or v: unmeasured segments, boxes over the finite values only; a polyline without a finite v; and, in the last polyline, a
    non-finite coordinate along the axis only, which nothing reads"""
    p = in_plane(np.concatenate([wobbly_loop(70, 7), wobbly_loop(5, 8), wobbly_loop(66, 9)]), 2, 1.0)
    p[3, 0] = np.nan; p[10, 1] = np.inf; p[11, 1] = -np.inf; p[69, 0] = np.inf           # u = x, v = y for axis 2
    p[70:75, 1] = np.nan
    p[80, 2] = np.nan; p[100, 2] = np.inf; p[140, 2] = -np.inf
    return p, records([[0, 70, 0, 1], [70, 5, 0, 0], [75, 66, 1, 1]]), 2, 2


def huge():
    """E = 128: coordinates up to float32's largest"""
    uv = (wobbly_loop(200, 12).astype(np.float64) * 2.55e38).astype(F)
    uv[0] = [np.finfo(F).max, -np.finfo(F).max]
    uv[1] = [-np.finfo(F).max, np.finfo(F).max]
    assert np.isfinite(uv).all()
    return in_plane(uv, 2, 1e38), records([[0, 120, 0, 1], [120, 80, 0, 0]]), 2, 1


def denormal(E):
    """E = -148: every coordinate is 0 or +-2^-149; E = -140: denormals of up to nine bits"""
    rng = np.random.default_rng(13 - E)
    top = 2 ** (E + 149)
    k = rng.integers(-top + 1, top, size=(150, 2)) if top > 1 else rng.integers(-1, 2, size=(150, 2))
    k[0] = [top - 1 if top > 1 else 1, -(top - 1) if top > 1 else -1]
    uv = (k.astype(np.float64) * 2.0 ** -149).astype(F)
    return in_plane(uv, 0, 0.0), records([[0, 100, 0, 1], [100, 50, 1, 0]]), 0, 2


def wrapping():
    """terms chosen so the low 64-bit word wraps, in both directions: 125 laps counter-clockwise round a rectangle (500 equal positive C_t of about 53
    significant bits at 2^87, so every few additions carry into the high word), then 175 laps clockwise (the sum crosses zero and ends negative), as
    one open polyline; then each direction as a polyline of its own"""
    a, b = F(1.2345678), F(1.7654321)
    ccw = np.array([[a, b], [-a, b], [-a, -b], [a, -b]], F)
    uv = np.concatenate([np.tile(ccw, (125, 1)), np.tile(ccw[::-1], (175, 1)), np.tile(ccw, (125, 1)), np.tile(ccw[::-1], (175, 1))])
    return in_plane(uv, 2), records([[0, 1200, 0, 0], [1200, 500, 0, 1], [1700, 700, 0, 1]]), 2, 1


def ties():
    """E = 0 (the largest coordinate is 0.75): the length's quantum is 2^-88, and the first three polylines are single segments of 1, 3 and 5 times
    2^-89, half-way between two multiples: they round to 0, 2 and 2 quanta"""
    h = 2.0 ** -89
    uv = np.array([[0, 0], [h, 0], [0, 0], [0, 3 * h], [0, 0], [-5 * h, 0], [0.75, 0.5], [0.25, 0.5], [0.25, -0.125]], F)
    return in_plane(uv, 2), records([[0, 2, 0, 0], [2, 2, 0, 0], [4, 2, 0, 0], [6, 3, 0, 1]]), 2, 1


def mixed():
    """a few thousand points in loops of 3 to 300 points over five slices, both orientations, open and closed: for the grids and the eager variant"""
    rng = np.random.default_rng(21)
    rows, uv, first = [], [], 0
    while first < 6000:
        n = int(rng.choice([3, 4, 5, 17, 64, 131, 300]))
        loop = wobbly_loop(n, 1000 + first, float(rng.uniform(0.5, 40.0)), tuple(rng.uniform(-30, 30, 2)))
        uv.append(loop[::-1] if rng.random() < 0.4 else loop)
        rows.append([first, n, int(rng.integers(0, 5)), int(rng.random() < 0.8)])
        first += n
    p = in_plane(np.concatenate(uv), 1, 2.0)
    p[rng.integers(0, len(p), 25), 2] = np.nan                        # u of axis 1 is z
    return p, records(rows), 1, 5


CASES = {"straddling": straddling, "triangles64": triangles64, "lane_starts": lane_starts, "tiny_counts": tiny_counts, "scattered_slices": scattered_slices,
         "non_finite": non_finite, "huge_E128": huge, "denormal_E-148": lambda: denormal(-148), "denormal_E-140": lambda: denormal(-140), "wrapping": wrapping,
         "ties": ties, "mixed": mixed, "permuted_0": lambda: permuted(0), "permuted_1": lambda: permuted(1), "permuted_2": lambda: permuted(2)}


@functools.lru_cache(maxsize=None)
def case(name):
    p, rec, axis, n_slices = CASES[name]()
    p, rec = np.ascontiguousarray(p, F), np.ascontiguousarray(rec, np.int32)
    p.setflags(write=False); rec.setflags(write=False)
    return p, rec, axis, n_slices


# ---- the torus of the public path ----------------------------------------------------------------------------------------------------------------
TORUS_MAJOR, TORUS_MINOR = 0.9, 0.35


def torus_lattice(axis):
    """(origin, step, counts): 48 x 48 points over +-1.5 in the plane and 5 planes 0.25 apart along `axis`, the middle one through the torus' centre
    (-0.5 + 2 * 0.25 is exactly 0 in float32)"""
    origin, step, counts = [-1.5] * 3, [3.0 / 47.0] * 3, [48] * 3
    origin[axis], step[axis], counts[axis] = -0.5, 0.25, 5
    return tuple(origin), tuple(step), tuple(counts)


def torus_normal(axis):
    n = [0.0, 0.0, 0.0]
    n[axis] = 1.0
    return tuple(n)


def torus_distances(axis):
    """the torus' distance on its lattice, restated in float64 numpy (the field's topology, not its bits): float32 [counts]"""
    import fraytracer_amd as ft
    origin, step, counts = torus_lattice(axis)
    p = ft.lattice_points(origin, step, counts).astype(np.float64)
    u, v, a = p[..., (axis + 1) % 3], p[..., (axis + 2) % 3], p[..., axis]
    ring = np.sqrt(u * u + v * v) - TORUS_MAJOR
    return (np.sqrt(ring * ring + a * a) - TORUS_MINOR).astype(F)
