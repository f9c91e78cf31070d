"""The restatement of the shell rule (tests/shells_restatement.py) against independent facts, on the inputs the GPU tests use (tests/shells_cases.py):
Euler characteristics, closedness against mesh_restatement.is_closed, shell counts against a flood fill of the inside mask (scipy, where present), the
invariants of the selection, and the conditions each input is there for — so that a changed input cannot quietly stop exercising its case."""
import numpy as np
import pytest

import mesh_restatement as mesh_rule
import shells_cases as cases
import shells_restatement as rule


def shells_of(name):
    m = cases.mesh_of(name)
    return m, rule.shells(m.triangles, len(m.vertices))


def per_shell(m, sh, s):
    """the triangles of shell s as a mesh of their own, through the restated selection"""
    v, t, _, _, _ = rule.select(m.vertices, m.triangles, sh, np.arange(len(sh.records)) == s)
    return mesh_rule.Mesh(v, t, 0)


def test_analytic_surfaces():
    for name, n_shells, chi in (("sphere", 1, [2]), ("torus", 1, [0]), ("two_spheres", 2, [2, 2]), ("hollow_ball", 2, [2, 2]), ("capped_rod", 1, [2])):
        m, sh = shells_of(name)
        assert sh.info["n_shells"] == n_shells == sh.info["n_closed"] and sh.info["n_unused_vertices"] == 0 and sh.info["n_border_edges"] == 0, name
        assert rule.euler(sh.records).tolist() == chi, name
        for s in range(n_shells):
            part = per_shell(m, sh, s)
            assert mesh_rule.is_closed(part.triangles) and mesh_rule.euler_characteristic(part) == chi[s], (name, s)
        assert mesh_rule.is_closed(m.triangles)
    _, sh = shells_of("two_spheres")
    assert sh.records[:, 2].tolist() == [676, 676]
    _, sh = shells_of("hollow_ball")
    assert sorted(sh.records[:, 2].tolist()) == [1344, 4224]                              # the cavity wall is the smaller one
    m, sh = shells_of("capped_rod")
    assert len(m.vertices) > 16 * 512                                                      # one shell across many tiles along k


def test_open_shells():
    m, sh = shells_of("clipped_plus_whole")
    assert sh.info["n_shells"] == 2 and sh.info["n_closed"] == 1 and sorted(sh.records[:, 3].tolist()) == [0, 50]
    m, sh = shells_of("two_spheres_nan")
    assert m.skipped > 0 and sh.info["n_shells"] == 2 and sh.info["n_closed"] == 1 and sh.info["n_border_edges"] > 0
    for name in ("clipped_plus_whole", "two_spheres_nan"):
        m, sh = shells_of(name)
        for s in range(2):
            part = per_shell(m, sh, s)
            assert mesh_rule.is_closed(part.triangles) == (sh.records[s, 3] == 0), (name, s)
            assert mesh_rule.euler_characteristic(part) == rule.euler(sh.records)[s], (name, s)      # no directed side occurs twice in a mesher output


def test_egg_crates():
    m, sh = shells_of("egg_crate")
    assert sh.info["n_shells"] == 64 == sh.info["n_closed"] and (sh.records[:, 2] == 648).all() and (rule.euler(sh.records) == 2).all()
    assert (np.diff(sh.vertex_shell) != 0).sum() > 10 * 64                                 # interleaved in vertex order, not shell after shell
    m, sh = shells_of("egg_crate_shifted")
    assert sh.info["n_shells"] == 125 and sh.info["n_closed"] == 27
    assert len(m.vertices) > 2 * 4 * 512 and len(m.vertices) % 1024 and len(m.triangles) % 1024      # tiles: several per scan thread, a part-filled last one


def test_noise_has_what_it_is_there_for():
    m, sh = shells_of("noise")
    d, _, _ = cases.lattice("noise")
    assert np.isnan(d).sum() > 40 and (d == 0).sum() > 40
    assert sh.info["n_shells"] >= 5 and (sh.records[:, 2] == 1).sum() >= 1 and sh.info["n_unused_vertices"] >= 10
    assert (sh.vertex_shell == -1).sum() == sh.info["n_unused_vertices"] == len(m.vertices) - len(np.unique(m.triangles))


def test_every_sign_pattern_of_one_cell():
    several = 0
    for d, origin, step in cases.one_cell_patterns():
        m = mesh_rule.extract(d, origin, step)
        sh = rule.shells(m.triangles, len(m.vertices))
        assert sh.info["n_unused_vertices"] == 0 and sh.records[:, 1].sum() == len(m.vertices) and sh.records[:, 2].sum() == len(m.triangles)
        several += sh.info["n_shells"] > 1
    assert several >= 10                                                                   # several shells inside one cell


def test_shell_counts_agree_with_a_flood_fill_of_the_inside_mask():
    ndimage = pytest.importorskip("scipy.ndimage")
    # 26-connected inside regions that do not touch the lattice's border each have one outer shell; the hollow ball adds its cavity wall
    for name, cavities in (("sphere", 0), ("two_spheres", 0), ("egg_crate", 0), ("hollow_ball", 1)):
        d, _, _ = cases.lattice(name)
        _, regions = ndimage.label(d < 0, structure=np.ones((3, 3, 3)))
        _, sh = shells_of(name)
        assert sh.info["n_shells"] == regions + cavities, name


def test_triangle_lists():
    want = {"permuted_strip": (1, 0, [20002]), "open_fan": (1, 0, [3002]), "closed_fan": (1, 0, [3000]), "double_cover": (1, 1, [0]), "side_twice": (1, 0, [6]),
            "shared_vertex": (1, 0, [6]), "isolated_between": (2, 0, [3, 4]), "no_triangles": (0, 0, [])}
    for name, (n_shells, n_closed, border) in want.items():
        tri, nv = cases.triangle_list(name)
        sh = rule.shells(tri, nv)
        assert (sh.info["n_shells"], sh.info["n_closed"], sh.records[:, 3].tolist()) == (n_shells, n_closed, border), name
    tri, nv = cases.triangle_list("permuted_strip")
    assert nv == 20002 and len(tri) == 20000 and not (np.diff(tri[:, 0]) == 1).all()
    assert rule.euler(rule.shells(*cases.triangle_list("double_cover")).records).tolist() == [2]
    sh = rule.shells(*cases.triangle_list("side_twice"))                                  # 0 -> 1 occurs twice and 1 -> 0 once: neither is a border edge
    assert sh.records[0].tolist() == [0, 5, 3, 6]
    sh = rule.shells(*cases.triangle_list("isolated_between"))
    assert sh.vertex_shell.tolist() == [0, 0, 0, -1, 1, 1, 1, -1, 1, -1] and sh.triangle_shell.tolist() == [0, 1, 1] and sh.info["n_unused_vertices"] == 3
    sh = rule.shells(*cases.triangle_list("no_triangles"))
    assert sh.vertex_shell.tolist() == [-1] * 7 and sh.records.shape == (0, 4) and sh.info["n_unused_vertices"] == 7


def test_selection_invariants():
    for name in ("egg_crate_shifted", "noise", "clipped_plus_whole"):
        m, sh = shells_of(name)
        S = len(sh.records)
        nrm = np.arange(3 * len(m.vertices), dtype=np.float32).reshape(-1, 3)
        mat = np.arange(len(m.vertices), dtype=np.int32)
        for keep in (np.zeros(S, bool), np.ones(S, bool), np.arange(S) % 2 == 0, rule.largest(sh.records, 1), sh.records[:, 3] == 0):
            v, t, n, mt, new = rule.select(m.vertices, m.triangles, sh, keep, nrm, mat)
            assert len(v) == sh.records[keep, 1].sum() and len(t) == sh.records[keep, 2].sum() and len(n) == len(v) == len(mt)
            assert (np.diff(mt) > 0).all()                                                 # old relative order
            assert np.array_equal(n, nrm[mt]) and np.array_equal(v, m.vertices[mt])
            assert (t[:, 0] < t[:, 1]).all() and (t[:, 0] < t[:, 2]).all()                 # every triangle still starts with its smallest index
            again = rule.shells(t, len(v))
            kept = sh.records[keep].copy()
            kept[:, 0] = new[kept[:, 0]]
            assert np.array_equal(again.records, kept) and again.info["n_unused_vertices"] == 0, name
    assert rule.largest(np.array([[0, 3, 5, 0], [3, 3, 9, 0], [6, 3, 9, 0], [9, 3, 1, 0]]), 2).tolist() == [False, True, True, False]
    assert rule.largest(np.array([[0, 3, 5, 0], [3, 3, 5, 0]]), 1).tolist() == [True, False]       # a tie goes to the lower number
