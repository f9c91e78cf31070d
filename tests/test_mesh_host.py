"""The extraction rule of the mesher by itself (tests/mesh_restatement.py, numpy): what the header's "Meshing" promises of its output — a closed,
consistently oriented surface — on analytic fields, on values of exactly iso, on every sign pattern of one cell and on the CPU oracle's distances
of three scenes.  No GPU and nothing of the library's: the GPU tests then hold the library to this restatement bit for bit."""
import itertools

import numpy as np
import pytest

import mesh_cases as cases
import mesh_restatement as rule

F = np.float32


def assert_closed_surface(mesh, what):
    cnt = rule.directed_edge_counts(mesh.triangles)
    assert cnt, what
    assert all(n == 1 for n in cnt.values()), f"{what}: a directed edge occurs more than once"
    assert all((b, a) in cnt for a, b in cnt), f"{what}: a directed edge without its reverse"
    assert len(np.unique(mesh.triangles)) == len(mesh.vertices), f"{what}: a vertex no triangle refers to"


@pytest.mark.parametrize("name", ["sphere", "torus", "two_spheres"])
def test_analytic_fields_give_closed_oriented_surfaces(name):
    d, origin, step, chi = cases.analytic()[name]
    assert np.isfinite(d).all() and not (d[cases.outer_layer(d.shape)] < 0).any()          # conditions on the input
    mesh = rule.extract(d, origin, step)
    lo, hi = np.asarray(origin, F), np.asarray(origin, F) + F(16) * np.asarray(step, F)
    assert (mesh.vertices > lo).all() and (mesh.vertices < hi).all()                        # strictly inside the outer layer
    assert mesh.skipped == 0 and mesh.vertices.dtype == np.float32 and mesh.triangles.dtype == np.int32
    assert_closed_surface(mesh, name)
    assert rule.euler_characteristic(mesh) == chi
    assert rule.signed_volume(mesh) > 0.0                                                  # counter-clockwise seen from the outside


def test_values_of_exactly_iso_keep_the_surface_closed():
    d, origin, step, chi = cases.analytic()["sphere"]
    d = d.copy()
    flat = np.abs(d) < 0.08
    assert flat.sum() >= 100
    d[flat] = 0.0                                                                          # +0: not inside
    for values, iso in ((d, 0.0), (d + F(0.25), 0.25)):                                    # the zeros become exactly iso; every other value keeps its sign (|d| >= 0.08)
        mesh = rule.extract(values, origin, step, iso)
        assert_closed_surface(mesh, f"iso {iso}")
        assert rule.euler_characteristic(mesh) == chi and rule.signed_volume(mesh) > 0.0
    v = mesh.vertices[mesh.triangles.astype(np.int64)]
    assert (np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1) == 0).any()      # zero-area triangles are there


def test_every_sign_pattern_of_one_cell():
    rng = np.random.default_rng(20)
    per_inside = {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}
    for pattern in itertools.product((False, True), repeat=8):
        inside = np.array(pattern).reshape(2, 2, 2)
        mag = rng.uniform(0.1, 1.0, (2, 2, 2)).astype(F)
        mesh = rule.extract(np.where(inside, -mag, mag), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
        want = 0
        for perm in rule.PERMS:
            want += per_inside[sum(bool(inside[tuple(c)]) for c in rule.tetrahedron_corners(perm))]
        assert len(mesh.triangles) == want, pattern
        edges = sum(bool(inside[0, 0, 0]) != bool(inside[d]) for d in rule.DIRS)           # the cell's origin owns the seven edges that leave it
        assert len(mesh.vertices) >= edges and mesh.skipped == 0
        if len(mesh.triangles):
            assert mesh.triangles.min() >= 0 and mesh.triangles.max() < len(mesh.vertices)
            assert (mesh.triangles[:, 0] < mesh.triangles[:, 1]).all() and (mesh.triangles[:, 0] < mesh.triangles[:, 2]).all()   # smallest index first


def test_non_finite_values_skip_their_tetrahedra():
    d, origin, step, _ = cases.analytic()["sphere"]
    d = d.copy()
    d[8, 8, 14], d[3, 9, 9], d[9, 3, 8] = np.nan, np.inf, -np.inf
    mesh = rule.extract(d, origin, step)
    assert mesh.skipped == 3 * 24                                                          # an interior point is a corner of 24 tetrahedra
    whole = rule.extract(cases.analytic()["sphere"][0], origin, step)
    assert len(mesh.triangles) < len(whole.triangles)
    cnt = rule.directed_edge_counts(mesh.triangles)
    assert all(n == 1 for n in cnt.values())                                               # still consistently oriented; open around the holes
    assert rule.extract(d[:1], origin, step).triangles.shape == (0, 3)                     # a count of 1: no cells, an empty mesh


@pytest.mark.parametrize("name", list(cases.SCENES))
def test_oracle_distances_give_closed_oriented_surfaces(oracle, name):
    origin, step, d = cases.oracle_lattice(oracle, name)
    # conditions on the input, from the oracle alone
    assert np.isfinite(d).all() and not (d[cases.outer_layer(d.shape)] < 0).any()
    mesh = rule.extract(d, origin, step)
    print(f"{name}: {len(mesh.vertices)} vertices, {len(mesh.triangles)} triangles")
    assert len(mesh.vertices) >= 400
    assert mesh.skipped == 0
    assert_closed_surface(mesh, name)
    assert rule.signed_volume(mesh) > 0.0
