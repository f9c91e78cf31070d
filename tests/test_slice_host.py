"""The slicing rule by itself (tests/slice_restatement.py, numpy and plain Python) held to what the header's "Slicing" says it means: a slice is the
section of the mesher's surface by a lattice plane — every contour point is bit for bit the mesher's vertex of the same edge, every segment an edge of
one of its triangles — with closed, consistently oriented loops.  No GPU and nothing of the library's: the GPU tests then hold the library to this
restatement bit for bit."""
import itertools

import numpy as np
import pytest

import mesh_cases as cases
import mesh_restatement as mesh_rule
import slice_restatement as rule

F = np.float32
AXES = (0, 1, 2)
UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def lines_of(c):
    return [(c.points[f:f + n], w, bool(closed)) for f, n, w, closed in c.polylines.tolist()]


def assert_is_a_section_of_the_mesh(d, origin, step, iso, axis, what):
    """the contours of `axis` against mesh_restatement.extract of the same lattice"""
    with np.errstate(all="ignore"):
        s = (np.asarray(d, F) - F(iso)).astype(F)
    mesh = mesh_rule.extract(d, origin, step, iso)
    # the mesher's numbering of every edge (q, e), as mesh_restatement.extract forms it
    carries = np.zeros(s.shape + (7,), bool)
    inside, finite = s < 0, np.isfinite(s)
    nx, ny, nz = s.shape
    for e, (di, dj, dk) in enumerate(mesh_rule.DIRS):
        a, b = (slice(0, nx - di), slice(0, ny - dj), slice(0, nz - dk)), (slice(di, nx), slice(dj, ny), slice(dk, nz))
        carries[a + (e,)] = finite[a] & finite[b] & (inside[a] != inside[b])
    mesh_index = np.where(carries.reshape(-1), np.cumsum(carries.reshape(-1)) - 1, -1)
    assert mesh_index.max() + 1 == len(mesh.vertices)
    index = rule.vertex_table(s, axis)
    pos, q, e = rule.positions(s, index, origin, step)
    assert set(np.unique(e)) <= set(rule.plane_edges(axis)), what
    same = mesh_index[q * 7 + e]
    assert (same >= 0).all(), what                                                         # the same existence rule
    assert np.array_equal(pos.view(np.uint32), mesh.vertices[same].view(np.uint32)), what + ": a contour point is not the mesher's vertex"
    starts, ends, _ = rule.segments(s, index, axis)
    assert len(np.unique(starts)) == len(starts) and len(np.unique(ends)) == len(ends), what          # at most one segment leaves and one enters a vertex
    t = mesh.triangles.astype(np.int64)
    und = set(map(tuple, np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1).tolist()))
    for a, b in zip(same[starts].tolist(), same[ends].tolist()):
        assert (min(a, b), max(a, b)) in und, what + ": a segment that is no edge of a mesh triangle"
    return len(starts)


def touches_border(points, origin, step, counts, axis):
    u, v = rule.in_plane_axes(axis)
    o, st = np.asarray(origin, F), np.asarray(step, F)
    for ax in (u, v):
        lo, hi = o[ax], (o[ax] + F(counts[ax] - 1) * st[ax]).astype(F)
        if (points[:, ax] == lo).any() or (points[:, ax] == hi).any():
            return True
    return False


@pytest.mark.parametrize("axis", AXES)
@pytest.mark.parametrize("name", ["sphere", "torus", "two_spheres"])
def test_analytic_fields(name, axis):
    d, origin, step, _ = cases.analytic()[name]
    assert assert_is_a_section_of_the_mesh(d, origin, step, 0.0, axis, name) > 50
    c = rule.extract(d, origin, step, axis)
    assert c.skipped == 0 and c.points.dtype == np.float32 and c.polylines.dtype == np.int32
    assert c.closed == len(c.polylines) > 0                                                # the surface lies inside the lattice: every polyline is a loop
    assert (np.diff(c.polylines[:, 0]) == c.polylines[:-1, 1]).all() and c.polylines[-1, :2].sum() == len(c.points)
    holes = 0
    for pts, w, closed in lines_of(c):
        assert closed and len(pts) >= 3
        holes += rule.signed_area(pts, axis) < 0.0                                         # clockwise seen from +axis
        plane = F(origin[axis]) + F(w) * F(step[axis])
        assert (pts[:, axis] == plane).all()
    # only the torus cut across its axis has holes: one per plane through the tube, inside a counter-clockwise rim
    assert (holes > 0) == (name == "torus" and axis == 2) and 2 * holes <= len(c.polylines)


@pytest.mark.parametrize("axis", AXES)
@pytest.mark.parametrize("name", list(cases.SCENES))
def test_oracle_distances_of_the_scenes(oracle, name, axis):
    origin, step, d = cases.oracle_lattice(oracle, name)
    assert assert_is_a_section_of_the_mesh(d, origin, step, 0.0, axis, name) >= 100        # segments: the input does reach the rule
    c = rule.extract(d, origin, step, axis)
    assert np.isfinite(d).all() and c.skipped == 0
    for pts, w, closed in lines_of(c):
        assert closed or touches_border(pts[[0, -1]], origin, step, cases.COUNTS, axis), (name, axis, w)
    assert c.closed >= 5


def planar_field(axis, fn, n=33, half=1.6):
    """fn(U, V) on an n x n plane of a lattice with one slice along `axis` -> (values, origin, step)"""
    u, v = rule.in_plane_axes(axis)
    t = np.linspace(-half, half, n).astype(F)
    U, V = np.meshgrid(t, t, indexing="ij")
    shape = [1, 1, 1]
    shape[u], shape[v] = n, n
    vals = fn(U, V).astype(F)
    vals = vals if u < v else vals.T                                                       # the array's axes are in (i, j, k) order
    step = [1.0, 1.0, 1.0]
    step[u] = step[v] = 2.0 * half / (n - 1)
    origin = [0.5, 0.5, 0.5]
    origin[u] = origin[v] = -half
    return vals.reshape(shape), tuple(origin), tuple(step)


@pytest.mark.parametrize("axis", AXES)
def test_a_disc_runs_counter_clockwise_and_a_hole_clockwise(axis):
    d, origin, step = planar_field(axis, lambda U, V: np.sqrt(U * U + V * V) - F(1.0))
    c = rule.extract(d, origin, step, axis)
    assert len(c.polylines) == 1 and c.closed == 1 and c.polylines[0].tolist()[2:] == [0, 1]
    area = rule.signed_area(c.points, axis)
    assert 0.9 * np.pi < area < np.pi                                                      # inscribed in the unit circle, positive
    d, origin, step = planar_field(axis, lambda U, V: np.abs(np.sqrt(U * U + V * V) - F(1.0)) - F(0.4))
    c = rule.extract(d, origin, step, axis)
    assert len(c.polylines) == 2 and c.closed == 2
    areas = sorted(rule.signed_area(pts, axis) for pts, _, _ in lines_of(c))
    assert -np.pi * 0.36 < areas[0] < -0.9 * np.pi * 0.36 and 0.9 * np.pi * 1.96 < areas[1] < np.pi * 1.96      # the hole (r = 0.6) and the rim (r = 1.4)
    # a negative step mirrors the drawing, not the rule: the direction is combinatorial
    flipped = rule.extract(d, origin, tuple(-x for x in step), axis)
    assert np.array_equal(flipped.polylines, c.polylines)


@pytest.mark.parametrize("axis", AXES)
def test_every_sign_pattern_of_one_cell(axis):
    rng = np.random.default_rng(30 + axis)
    u, v = rule.in_plane_axes(axis)
    shape = [1, 1, 1]
    shape[u] = shape[v] = 2
    segments = 0
    for pattern in itertools.product((False, True), repeat=4):
        inside = np.array(pattern).reshape(shape)
        mag = rng.uniform(0.1, 1.0, shape).astype(F)
        d = np.where(inside, -mag, mag).astype(F)
        c = rule.extract(d, *UNIT, axis)
        at = lambda du, dv: bool(inside[tuple(du * rule.unit(u) + dv * rule.unit(v))])
        want = sum(0 < sum(at(*corner) for corner in tri) < 3 for tri in rule.TRIANGLES)
        got = int((c.polylines[:, 1] - 1 + c.polylines[:, 3]).sum())                       # an open polyline of m + 1 points, a closed one of m
        assert got == want and c.closed == 0 and c.skipped == 0, pattern
        segments += got
        assert_is_a_section_of_the_mesh(np.concatenate([d, d], axis=axis), *UNIT, 0.0, axis, str(pattern))
        # the inside lies to the left of every segment: a step to the left of its midpoint lands where the cell's piecewise linear interpolant (the
        # two triangles') is negative
        f = lambda du, dv: float(d[tuple(du * rule.unit(u) + dv * rule.unit(v))])
        def interpolant(x, y):
            if x >= y:
                return f(0, 0) + x * (f(1, 0) - f(0, 0)) + y * (f(1, 1) - f(1, 0))
            return f(0, 0) + y * (f(0, 1) - f(0, 0)) + x * (f(1, 1) - f(0, 1))
        for pts, _, _ in lines_of(c):
            for a, b in zip(pts[:-1].astype(np.float64), pts[1:].astype(np.float64)):
                mid, way = 0.5 * (a + b), b - a
                left = np.array([-way[v], way[u]]) / np.hypot(way[u], way[v])
                assert abs(interpolant(mid[u], mid[v])) < 1e-6, pattern
                assert interpolant(mid[u] + 1e-3 * left[0], mid[v] + 1e-3 * left[1]) < 0.0, pattern
                assert interpolant(mid[u] - 1e-3 * left[0], mid[v] - 1e-3 * left[1]) > 0.0, pattern
    assert segments == 2 * 6 * 2                                                           # per triangle 6 of its 8 patterns, 2 for the fourth corner


@pytest.mark.parametrize("axis", AXES)
def test_values_of_exactly_iso_keep_loops_closed(axis):
    d, origin, step, _ = cases.analytic()["sphere"]
    d = d.copy()
    flat = np.abs(d) < 0.08
    assert flat.sum() >= 100
    d[flat] = 0.0
    for values, iso in ((d, 0.0), (d + F(0.25), 0.25)):
        c = rule.extract(values, origin, step, axis, iso)
        assert c.closed == len(c.polylines) > 0 and c.skipped == 0
        assert_is_a_section_of_the_mesh(values, origin, step, iso, axis, f"iso {iso}")
    zero = [np.array_equal(a, b) for pts, _, _ in lines_of(c) for a, b in zip(pts, np.roll(pts, -1, axis=0))]
    assert any(zero)                                                                       # zero-length segments are there


@pytest.mark.parametrize("axis", AXES)
def test_non_finite_corners_skip_their_triangles_and_open_the_chains(axis):
    d, origin, step, _ = cases.analytic()["sphere"]
    whole = rule.extract(d, origin, step, axis)
    d = d.copy()
    d[8, 8, 14], d[3, 9, 9], d[9, 3, 8], d[14, 8, 8], d[8, 14, 8] = np.nan, np.inf, -np.inf, np.nan, np.inf
    c = rule.extract(d, origin, step, axis)
    assert c.skipped == 5 * 6                                                              # an interior point is a corner of 6 triangles of its plane
    assert c.closed < len(c.polylines) and len(c.points) < len(whole.points) + len(c.polylines)
    assert_is_a_section_of_the_mesh(d, origin, step, 0.0, axis, "holes")
    # an open chain starts at a vertex no segment ends in: no two polylines share a point index, and the first points are in key order
    assert (np.diff(c.polylines[:, 0]) == c.polylines[:-1, 1]).all()
    u, v = rule.in_plane_axes(axis)
    one = [1, 1, 1]
    one[axis] = 3
    assert rule.extract(np.zeros(one, F), *UNIT, axis).polylines.shape == (0, 4)           # a count of 1 in the plane: no cells, an empty result
    everything = np.full((3, 3, 3), np.nan, F)
    assert rule.extract(everything, *UNIT, axis).skipped == 3 * 4 * 2 and len(rule.extract(everything, *UNIT, axis).points) == 0
