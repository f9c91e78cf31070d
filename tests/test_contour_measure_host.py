"""Contour measures, the parts that need no GPU: the restatement of the rule (tests/contour_measure_restatement.py) against an independent statement
— exact shoelace values in fractions for polygons with small integer coordinates (the signs, the divisors 2 and 6, the (u, v) of every axis), exact
lengths, the three bounds at the extremes of the extent, quantisation ties, the slices' integer sums — and the shapes of the GPU test's inputs."""
from fractions import Fraction

import numpy as np
import pytest

import contour_measure_cases as cases
import contour_measure_restatement as rule
import slice_restatement


def shoelace(uv, closed=True):
    """(area, moment u, moment v) of a polygon with integer coordinates as exact fractions, from the textbook formulas"""
    pts = [(Fraction(int(x)), Fraction(int(y))) for x, y in uv]
    pairs = list(zip(pts, pts[1:] + pts[:1])) if closed else list(zip(pts, pts[1:]))
    cross = [px * qy - qx * py for (px, py), (qx, qy) in pairs]
    area = sum(cross) / 2
    mu = sum(c * (p[0] + q[0]) for c, (p, q) in zip(cross, pairs)) / 6
    mv = sum(c * (p[1] + q[1]) for c, (p, q) in zip(cross, pairs)) / 6
    return area, mu, mv


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_integer_polygons_give_the_exact_shoelace_values_on_every_axis(axis):
    p, rec, _, n_slices = cases.case(f"permuted_{axis}")
    got, per = rule.measure(p, rec, axis, n_slices)
    u, v = (axis + 1) % 3, (axis + 2) % 3
    total = [Fraction(0)] * 3
    for l, (first, count, _, closed) in enumerate(rec.tolist()):
        want = shoelace(p[first:first + count][:, [u, v]])
        assert Fraction(float(got["area"][l])) == want[0] and Fraction(float(got["moment"][l, 0])) == want[1] and Fraction(float(got["moment"][l, 1])) == want[2], (axis, l)
        total = [a + b for a, b in zip(total, want)]
    # the L is 6 x 2 + 2 x 3 = 18, counter-clockwise; the hole a unit square, clockwise; the section encloses 17
    assert got["area"].tolist() == [18.0, -1.0] and per["area"].tolist() == [17.0]
    assert [Fraction(float(per["moment"][0, 0])), Fraction(float(per["moment"][0, 1]))] == total[1:]
    assert got["length"].tolist() == [22.0, 4.0] and per["length"].tolist() == [26.0]       # axis-parallel edges: exact
    assert (per["n_polylines"][0], per["n_closed"][0], per["n_outer"][0], per["n_holes"][0], per["n_unmeasured"][0]) == (2, 2, 1, 1, 0)
    assert got["bbox_min"].tolist() == [[0, 0], [1, 1]] and got["bbox_max"].tolist() == [[6, 5], [2, 2]] and per["bbox_max"].tolist() == [[6, 5]]
    assert got["extent_exponent"].tolist() == [3, 3]                                       # the largest coordinate is 6 < 2^3
    # the centroid of the L with its hole: moment / area
    cx, cy = total[1] / 17, total[2] / 17
    assert abs(float(per["moment"][0, 0] / per["area"][0]) - float(cx)) < 1e-15 and abs(float(per["moment"][0, 1] / per["area"][0]) - float(cy)) < 1e-15


def test_a_coordinate_on_the_wrong_axis_would_show():
    """u and v are not interchangeable: the L's moments differ, and the three axes read three different pairs of columns"""
    p, rec, _, _ = cases.case("permuted_0")
    assert not np.array_equal(p[:, 1], p[:, 2])
    wrong, _ = rule.measure(p[:, [0, 2, 1]], rec, 0, 1)                                    # u and v swapped: the mirror image
    right, _ = rule.measure(p, rec, 0, 1)
    assert wrong["area"].tolist() == [-18.0, 1.0] and right["area"].tolist() == [18.0, -1.0]
    assert wrong["moment"][0].tolist() == (-right["moment"][0][::-1]).tolist() and right["moment"][0, 0] != right["moment"][0, 1]


def test_lengths_of_3_4_5_edges_and_open_polylines():
    uv = np.array([[0, 0], [3, 0], [3, 4], [0, 0], [-4, 3], [-4, 0]], np.float32)
    p = cases.in_plane(uv, 2, 7.0)
    got, per = rule.measure(p, cases.records([[0, 3, 0, 1], [3, 3, 0, 0]]), 2, 1)
    assert got["length"].tolist() == [12.0, 8.0] and per["length"].tolist() == [20.0]       # 3 + 4 + 5 closed; 5 + 3 open: no closing segment
    assert got["area"][0] == 6.0 and shoelace(uv[:3])[0] == 6
    open_area = shoelace(uv[3:], closed=False)
    assert Fraction(float(got["area"][1])) == open_area[0]                                 # the rule's number over its m - 1 segments
    assert per["area"][0] == 6.0 and per["n_closed"][0] == 1 and per["n_polylines"][0] == 2  # open polylines add length only
    # the coordinate along the axis is not read, except by the extent: 7 < 2^3
    assert got["extent_exponent"][0] == 3 and rule.measure(cases.in_plane(uv, 2, 70.0), cases.records([[0, 3, 0, 1]]), 2, 1)[0]["extent_exponent"][0] == 7


def test_single_points_and_empty_polylines():
    p, rec, axis, n_slices = cases.case("tiny_counts")
    got, per = rule.measure(p, rec, axis, n_slices)
    assert got["length"][[0, 1, 2, 3, 5]].tolist() == [0, 0, 0, 0, 0] and got["area"][[0, 1, 2, 3, 5]].tolist() == [0, 0, 0, 0, 0]
    assert np.isinf(got["bbox_min"][[0, 3, 5]]).all() and np.isfinite(got["bbox_min"][[1, 2, 4]]).all()
    assert got["extent_exponent"][0] == 10 and (np.abs(p[:7]) < 2).all()                   # point 7 (900) is in no polyline and sets the extent
    assert per["n_polylines"].tolist() == [3, 3] and per["n_closed"].tolist() == [3, 1] and per["n_outer"].tolist() == [1, 0]
    assert rule.segments(4, 1, True) == [(4, 4)] and rule.segments(4, 1, False) == [] and rule.segments(4, 0, True) == []


@pytest.mark.parametrize("E", [-148, 0, 128])
def test_the_three_bounds_hold_at_the_extremes(E):
    """|coordinate| < 2^E: random coordinates and the adversarial ones, all +-(2^E - ulp)"""
    top = np.finfo(np.float32).max if E == 128 else np.nextafter(np.float32(2.0 ** E), np.float32(0))      # 2^E - ulp; at E = 128 float32's largest, at E = -148 2^-149
    assert np.isfinite(top) and top > 0 and rule.extent_exponent([top]) == E
    rng = np.random.default_rng(E + 200)
    signs = np.array([[a, b, c, d] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1) for d in (-1, 1)], np.float64)
    adversarial = signs * np.float64(top)
    random = (rng.uniform(-1, 1, (4000, 4)) * np.float64(top)).astype(np.float32).astype(np.float64)
    for quad in (adversarial, random):
        x = rule.terms(quad[:, 0:2], quad[:, 2:4])
        assert np.isfinite(x).all()
        B = rule.bounds(E)
        for k, b in ((0, B[0]), (1, B[1]), (2, B[2]), (3, B[2])):
            assert (np.abs(x[:, k]) < np.ldexp(1.0, b)).all(), (E, k)
            q = [abs(rule.quantise(t, rule.SHIFT - b)) for t in x[:, k]]
            assert max(q) <= 2 ** 90, (E, k)
    worst = rule.terms(adversarial[:, 0:2], adversarial[:, 2:4])
    assert np.abs(worst[:, 1]).max() == 2.0 * float(top) * float(top)                      # the area's bound is reached up to the coordinates' last ulp


def test_quantisation_rounds_half_to_even_once():
    assert [rule.quantise(x, 0) for x in (0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999999999999994, 2.5000000000000004)] == [0, 2, 2, 0, -2, -2, 0, 3]
    assert rule.quantise(3 * 2.0 ** -3, 2) == 2 and rule.quantise(5 * 2.0 ** -3, 2) == 2 and rule.quantise(7 * 2.0 ** -3, 2) == 4
    assert rule.quantise(2.0 ** -700, 90) == 0 and rule.quantise(-(2.0 ** -1070), 531) == 0   # underflow towards a value below 1/2
    assert rule.to_float(2 ** 53 + 1, 0) == 2.0 ** 53 and rule.to_float(2 ** 53 + 3, 0) == 2.0 ** 53 + 4 and rule.to_float(-(2 ** 54 + 2), 1) == -(2.0 ** 53)
    # ties inside records: at E = 0 the length's quantum is 2^-88, and segments of 1, 3 and 5 times 2^-89 lie half-way between two multiples
    p, rec, axis, n_slices = cases.case("ties")
    got, per = rule.measure(p, rec, axis, n_slices)
    assert got["extent_exponent"][0] == 0 and got["length"][:3].tolist() == [0.0, 2.0 ** -87, 2.0 ** -87] and per["length"][0] == 2.0 ** -86 + got["length"][3]


@pytest.mark.parametrize("name", ["scattered_slices", "mixed", "non_finite", "wrapping"])
def test_slice_sums_are_the_sums_of_the_polylines_integers(name):
    p, rec, axis, n_slices = cases.case(name)
    got, per = rule.measure(p, rec, axis, n_slices)
    E = int(got["extent_exponent"][0]) if len(got) else 0
    sums, bad = rule.integer_sums(p, rec, axis)
    for w in range(n_slices):
        mine = [l for l in range(len(rec)) if rec[l, 2] == w]
        Q = [sum(sums[l][0] for l in mine)] + [sum(sums[l][k] for l in mine if rec[l, 3]) for k in (1, 2, 3)]
        want = rule.results(Q, E)
        assert (per["length"][w], per["area"][w], per["moment"][w, 0], per["moment"][w, 1]) == want, (name, w)
        assert per["n_unmeasured"][w] == sum(bad[l] for l in mine) and per["n_polylines"][w] == len(mine)
        assert per["n_outer"][w] == sum(1 for l in mine if rec[l, 3] and sums[l][1] > 0) and per["n_holes"][w] == sum(1 for l in mine if rec[l, 3] and sums[l][1] < 0)
    if name == "scattered_slices":
        assert rec[:, 2].tolist() == [0, 1, 0, 2, 1] and per["n_polylines"].tolist() == [2, 2, 1, 0]
        assert per["area"][3] == 0 and np.isinf(per["bbox_min"][3]).all() and per["n_holes"].tolist() == [1, 1, 0, 0] and per["area"][2] == 0   # slice 2: an open polyline
    if name == "non_finite":
        assert got["n_unmeasured"].tolist() == [7, 4, 0] and np.isfinite(got["bbox_max"][0]).all() and got["bbox_min"][1, 1] == np.inf and np.isfinite(got["bbox_min"][1, 0])
    if name == "wrapping":
        low = [sum(q & (2 ** 64 - 1) for q in [sums[1][1] // 500] * 500)]
        assert low[0] >= 2 ** 64 and sums[0][1] < 0 and sums[1][1] > 2 ** 64 and sums[2][1] < -(2 ** 64)


def test_shapes_of_the_gpu_cases():
    p, rec, _, _ = cases.case("triangles64")
    assert len(rec) == 64 and (rec[:, 1] == 3).all() and len(p) == 192
    got, _ = rule.measure(p, rec, 0, 3)
    assert (np.sign(got["area"]) == np.where(np.arange(64) % 2 == 0, 1, -1)).all()
    assert [int(r[0]) % 64 for r in cases.case("lane_starts")[1]][:4] == [0, 63, 0, 63]
    for name in ("huge_E128", "denormal_E-148", "denormal_E-140"):
        p, rec, axis, n = cases.case(name)
        got, per = rule.measure(p, rec, axis, n)
        assert got["extent_exponent"][0] == int(name.split("E")[1]) and np.isfinite(got["moment"]).all() and (got["length"] > 0).all(), name
        assert (got["area"] != 0).all() and (got["moment"] != 0).any(), name
    assert (np.abs(cases.case("denormal_E-140")[0]) < 2.0 ** -126).all()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_the_torus_lattice_has_one_outer_loop_and_one_hole_on_its_middle_plane(axis):
    origin, step, counts = cases.torus_lattice(axis)
    c = slice_restatement.extract(cases.torus_distances(axis), origin, step, axis)
    middle = [r for r in c.polylines.tolist() if r[2] == 2]
    assert len(middle) == 2 and all(r[3] == 1 for r in middle)
    assert (c.points[middle[0][0]:middle[0][0] + middle[0][1], axis] == 0).all()           # the plane through the centre
    got, per = rule.measure(c.points, c.polylines, axis, counts[axis])
    areas = sorted(got["area"][[l for l, r in enumerate(c.polylines.tolist()) if r[2] == 2]])
    assert areas[0] < 0 < areas[1] and per["n_outer"][2] == 1 and per["n_holes"][2] == 1
    R, r = cases.TORUS_MAJOR, cases.TORUS_MINOR
    assert abs(per["area"][2] - np.pi * ((R + r) ** 2 - (R - r) ** 2)) < 0.05                # the annulus, as the lattice sees it
    assert per["n_polylines"][0] == 0 and per["n_polylines"][4] == 0 and per["n_holes"][1] == 1
