"""The refinement rule (include/fraytracer_hip.h "Refinement") on the CPU: the numpy restatement (tests/refine_restatement.py) on the oracle's
distances, over the three scenes of mesh_cases at two levels — with no round it is the mesher's and the slicer's vertex, every round keeps a bracket,
the vertices close in on the surface as the rule promises, and a refined contour point is a refined mesh vertex."""
import numpy as np
import pytest

import mesh_cases as cases
import mesh_restatement
import refine_cases as rc
import refine_restatement as rule
import slice_restatement

F = np.float32
NAMES = list(cases.SCENES)
same_bits = lambda a, b: a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("iso", rc.ISOS)
@pytest.mark.parametrize("name", NAMES)
def test_no_round_is_the_unrefined_vertex(oracle, name, iso):
    origin, step, d = cases.oracle_lattice(oracle, name)
    mesh = mesh_restatement.extract(d, origin, step, iso)
    assert len(mesh.vertices) >= 400
    assert same_bits(rc.refined(oracle, name, iso, 0), mesh.vertices)
    for axis in range(3):
        want = slice_restatement.extract(d, origin, step, axis, iso)
        assert len(want.points) >= 100
        assert same_bits(rc.refined(oracle, name, iso, 0, axis)[rc.slice_order(oracle, name, iso, axis)], want.points), axis


@pytest.mark.parametrize("iso", rc.ISOS)
@pytest.mark.parametrize("name", NAMES)
def test_every_round_keeps_a_bracket(oracle, name, iso):
    br, _ = rc.brackets(oracle, name, iso)
    rounds = []

    def each(old, M, new):
        assert np.isfinite(new.sA).all() and np.isfinite(new.sB).all()
        assert ((new.sA < 0) != (new.sB < 0)).all()                                        # exactly one end inside
        keptA = (new.A.view(np.uint32) == old.A.view(np.uint32)).all(axis=1) & (new.sA.view(np.uint32) == old.sA.view(np.uint32))
        keptB = (new.B.view(np.uint32) == old.B.view(np.uint32)).all(axis=1) & (new.sB.view(np.uint32) == old.sB.view(np.uint32))
        isM_A, isM_B = (new.A.view(np.uint32) == M.view(np.uint32)).all(axis=1), (new.B.view(np.uint32) == M.view(np.uint32)).all(axis=1)
        assert ((keptA & isM_B) | (keptB & isM_A) | (keptA & keptB)).all()                  # one end of the old one plus M (or, for a non-finite sM, the old one)
        assert (keptA | keptB).all()
        assert ((new.sA < 0) == (old.sA < 0)).all()                                        # A stays on its side
        rounds.append(int((~(keptA & keptB)).sum()))
    rule.bisect(*br, rc.distance_of(oracle, name), iso, 12, each)
    assert len(rounds) == 12 and rounds[0] == len(br.sA)                                   # no midpoint value was non-finite in the first round


@pytest.mark.parametrize("R", [0, 4, 8, 12])
@pytest.mark.parametrize("iso", rc.ISOS)
@pytest.mark.parametrize("name", NAMES)
def test_the_vertices_close_in_on_the_surface(oracle, name, iso, R):
    """|D(v) - iso| <= L * 2^-R for every vertex, L the Euclidean length of its lattice edge in float64, D the oracle's: the field is 1-Lipschitz and a
    zero lies inside a bracket of length L * 2^-R.  No chosen tolerance; beyond R = 12 the evaluation's float32 noise takes over, so not tested there."""
    _, length = rc.brackets(oracle, name, iso)
    v = rc.refined(oracle, name, iso, R)
    residual = np.abs(rc.distance_of(oracle, name)(v).astype(np.float64) - np.float64(F(iso)))
    bound = length * 2.0 ** -R
    print(f"{name} iso {iso} R {R}: max |D(v) - iso| {residual.max():.3g}, median {np.median(residual):.3g}, max over the bound {np.max(residual / bound):.3f}")
    assert (residual <= bound).all(), (float(np.max(residual / bound)), int((residual > bound).sum()))


@pytest.mark.parametrize("name", NAMES)
def test_a_refined_contour_point_is_a_refined_mesh_vertex(oracle, name):
    iso, R = 0.03, 8
    mesh_br, _ = rc.brackets(oracle, name, iso)
    key = lambda br, r: br.A[r].tobytes() + br.B[r].tobytes()
    by_edge = {key(mesh_br, r): r for r in range(len(mesh_br.sA))}
    mesh = rc.refined(oracle, name, iso, R)
    for axis in range(3):
        br, _ = rc.brackets(oracle, name, iso, axis)
        rows = np.array([by_edge[key(br, r)] for r in range(len(br.sA))], np.int64)        # every slice edge is a mesh edge
        assert same_bits(rc.refined(oracle, name, iso, R, axis), mesh[rows]), axis
        assert len(rows) >= 100 and len(np.unique(rows)) == len(rows)
