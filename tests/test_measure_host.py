"""The rule of the header's "Measures" on the CPU, by its restatement alone (tests/measure_restatement.py): exact cases, the hollow ball's body and
cavity, the scenes' shells against the whole mesh within the derived quantisation bound, and the bounds of the quantised terms."""
import numpy as np
import pytest

import measure_cases as cases
import measure_restatement as rule
import mesh_cases
import mesh_restatement as mesh_rule
import shells_cases
import shells_restatement as shells_rule


@pytest.mark.parametrize("name", list(cases.solids()))
def test_exact_solids(name):
    """small-integer coordinates: every term is an exact integer, far above the quantum, so the results are the exact numbers"""
    v, t, volume, area, moment = cases.solids()[name]
    r = rule.whole(v, t)[0]
    assert r["volume"] == volume, (name, r["volume"])
    if area is not None:
        assert r["area"] == area, (name, r["area"])
    assert tuple(r["moment"]) == moment, (name, r["moment"])
    assert r["n_unmeasured"] == 0 and r["extent_exponent"] == rule.extent_exponent(v)
    assert np.array_equal(r["bbox_min"], v.min(axis=0)) and np.array_equal(r["bbox_max"], v.max(axis=0))
    if name == "cube_translated":
        assert np.array_equal(r["moment"] / r["volume"], [101.0, -36.0, 6.0]) and r["extent_exponent"] == 7      # 102 < 2^7
    if name == "octahedron":
        assert abs(r["area"] - 4 * np.sqrt(12.0 ** 2 + 15.0 ** 2 + 20.0 ** 2)) < 1e-12                            # 8 faces of |(20, 15, 12)| / 2 each
    if name == "triangle":
        assert r["extent_exponent"] == 3


def test_extent_exponent():
    f = np.float32
    for m, E in ((0.0, 0), (1.0, 1), (0.75, 0), (1.999, 1), (2.0, 2), (2.0 ** -149, -148), (2.0 ** -127, -126), (2.0 ** -126, -125), (3e38, 128), (3.4028235e38, 128)):
        assert rule.extent_exponent(np.array([[f(m), 0, -f(m)]], f)) == E, m
        assert E == 0 and m == 0 or 2.0 ** (E - 1) <= float(f(m)) < 2.0 ** E
    assert rule.extent_exponent(np.array([[np.nan, np.inf, -np.inf]], f)) == 0 and rule.extent_exponent(np.zeros((0, 3), f)) == 0
    assert rule.extent_exponent(np.array([[np.inf, -3.0, 1.0]], f)) == 2


def test_box_orders_signed_zeros_and_skips_non_finite_values():
    f = np.float32
    lo, hi = rule.box(np.array([0.0, -0.0, 0.0], f))
    assert np.signbit(lo) and not np.signbit(hi)
    lo, hi = rule.box(np.array([np.nan, -2.0, np.inf, 5.0, -np.inf], f))
    assert (lo, hi) == (-2.0, 5.0)
    assert rule.box(np.array([np.nan, np.inf], f)) == (np.inf, -np.inf) and rule.box(np.zeros(0, f)) == (np.inf, -np.inf)
    vals = np.random.default_rng(0).standard_normal(1000).astype(f)
    assert rule.box(vals) == (vals.min(), vals.max())
    assert [rule.key(np.array(x, f).view(np.uint32)) for x in (-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf)] == sorted(
        rule.key(np.array(x, f).view(np.uint32)) for x in (-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf))


def test_hollow_ball_is_a_body_and_a_cavity():
    m = shells_cases.mesh_of("hollow_ball")
    sh = shells_rule.shells(m.triangles, len(m.vertices))
    assert sh.info["n_shells"] == 2 and sh.info["n_closed"] == 2
    r = rule.measure(m.vertices, m.triangles, sh.vertex_shell, sh.triangle_shell, 2)
    outer, inner = (0, 1) if r["volume"][0] > 0 else (1, 0)
    assert r["volume"][outer] > 0 > r["volume"][inner] and r["volume"].sum() > 0
    assert (r["bbox_min"][outer] < r["bbox_min"][inner]).all() and (r["bbox_max"][inner] < r["bbox_max"][outer]).all()
    # a ball of radius 1.15 without one of radius 0.65, as the 17^3 lattice sees them
    assert abs(r["volume"][outer] - 4 / 3 * np.pi * 1.15 ** 3) < 0.25 and abs(-r["volume"][inner] - 4 / 3 * np.pi * 0.65 ** 3) < 0.12
    assert (r["n_unmeasured"] == 0).all() and np.abs(r["moment"] / r["volume"][:, None]).max() < 0.02


@pytest.mark.parametrize("name", list(mesh_cases.SCENES))
def test_scene_shells_add_up_to_the_whole_mesh(oracle, name):
    """The sums of the shells' areas and volumes equal the whole mesh's to within the quantisation bound nT * 2^(B_K - 90).  Derived: every triangle
    is in exactly one shell and its quantised terms are the same integers in both calls, so in exact arithmetic the shells' sums Q add up to the
    whole mesh's with no difference at all — asserted as integers, which is the bound and more.  The float64 records round once more each (the
    conversion, and the division by 6), and numpy's sum of S records rounds S - 1 times: on the records the bound holds with (2 S + 2) * 2^-53 *
    sum |record| added, which is derived the same way and is all that is allowed on top."""
    origin, step, d = mesh_cases.oracle_lattice(oracle, name)
    m = mesh_rule.extract(d, origin, step)
    sh = shells_rule.shells(m.triangles, len(m.vertices))
    S = sh.info["n_shells"]
    parts = rule.measure(m.vertices, m.triangles, sh.vertex_shell, sh.triangle_shell, S)
    whole = rule.whole(m.vertices, m.triangles)[0]
    E = int(whole["extent_exponent"])
    BA, BW, _ = rule.bounds(E)
    nT = len(m.triangles)
    assert (parts["extent_exponent"] == E).all() and parts["n_unmeasured"].sum() == whole["n_unmeasured"] == 0
    q_parts, _ = rule.integer_sums(m.vertices, m.triangles, sh.triangle_shell, S)
    q_whole, _ = rule.integer_sums(m.vertices, m.triangles, None, 1)
    assert [sum(q[k] for q in q_parts) for k in range(5)] == q_whole[0]
    rounding = (2 * S + 2) * 2.0 ** -53
    print(name, "area", abs(parts["area"].sum() - whole["area"]), "volume", abs(parts["volume"].sum() - whole["volume"]), "quantisation bounds",
          nT * 2.0 ** (BA - 90), nT * 2.0 ** (BW - 90))
    assert abs(parts["area"].sum() - whole["area"]) <= nT * 2.0 ** (BA - 90) + rounding * np.abs(parts["area"]).sum()
    assert abs(parts["volume"].sum() - whole["volume"]) <= nT * 2.0 ** (BW - 90) + rounding * np.abs(parts["volume"]).sum()
    # the quantised area is the plain float64 sum to within the same bound
    assert abs(whole["area"] - rule.terms(m.vertices, m.triangles)[:, 0].sum()) <= nT * 2.0 ** (BA - 90) + nT * 2.0 ** -52 * whole["area"]
    closed = sh.records[:, 3] == 0
    assert closed.any()
    # an outer shell: no other closed shell's box contains its box
    for s in np.flatnonzero(closed):
        inside_another = any(o != s and (parts["bbox_min"][o] <= parts["bbox_min"][s]).all() and (parts["bbox_max"][s] <= parts["bbox_max"][o]).all()
                             for o in np.flatnonzero(closed))
        if not inside_another:
            assert parts["volume"][s] > 0, (name, s)
    if sh.info["n_unused_vertices"] == 0:                                                  # the whole mesh's box holds every vertex, the shells' the used ones
        assert np.array_equal(parts["bbox_min"].min(axis=0), whole["bbox_min"]) and np.array_equal(parts["bbox_max"].max(axis=0), whole["bbox_max"])


@pytest.mark.parametrize("E", [-149, -148, -126, 0, 127, 128])
def test_quantised_terms_stay_inside_their_bound(E):
    """|q| <= 2^91 for random triangles with coordinates up to m < 2^E.  E = -149 cannot come from a vertex (the smallest positive float32 is 2^-149,
    whose E is -148): it is forced on all-zero coordinates, the only ones below 2^-149"""
    if E == -149:
        v, t = np.zeros((6, 3), np.float32), np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    else:
        v, t = cases.of_extent(E, n=200)
        assert rule.extent_exponent(v) == E and np.isfinite(v).all()
    q = rule.quantised(v, t, E)
    assert len(q) == len(t)
    assert max(abs(x) for row in q for x in row) <= 2 ** 91
    if E != -149:
        assert max(abs(x) for row in q for x in row) >= 2 ** 60                              # and they use the accumulator's width
        x = rule.terms(v, t)
        BA, BW, BM = rule.bounds(E)
        assert np.isfinite(x).all() and (np.abs(x[:, 0]) < 2.0 ** BA).all() and (np.abs(x[:, 1]) < 2.0 ** BW).all() and (np.abs(x[:, 2:]) < 2.0 ** BM).all()
        r = rule.measure(v, t, None, None, 1)[0]
        assert np.isfinite(r["area"]) and np.isfinite(r["volume"]) and np.isfinite(r["moment"]).all() and r["area"] > 0


def test_near_square_triangles_are_what_they_claim():
    v, t = cases.sqrt_near_squares()
    assert len(t) == 256
    a, b, c = (v[t[:, i]].astype(np.float64) for i in range(3))
    u, w = b - a, c - a
    n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)
    nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    for x, sign in zip(nn, [+1] * 128 + [-1] * 128):
        square = np.nextafter(x, -np.inf if sign > 0 else np.inf)
        root = int(round(float(np.sqrt(square))))
        assert float(root) ** 2 == square and root * root < 2 ** 53, (x, sign)
    # the quantum is finer than the areas' last bit: the record's area is the term itself
    tl = np.arange(len(t), dtype=np.int32)
    r = rule.measure(v, t, np.repeat(tl, 3), tl, len(t))
    assert np.array_equal(r["area"], 0.5 * np.sqrt(nn))
    v, t = cases.sqrt_random()
    tl = np.arange(len(t), dtype=np.int32)
    r = rule.measure(v, t, np.repeat(tl, 3), tl, len(t))
    assert np.array_equal(r["area"], rule.terms(v, t)[:, 0]) and (r["area"] > 0).all()


def test_labels_and_indices_out_of_range():
    v, t, vl, tl, nS = cases.extremes()["out_of_range"]
    r = rule.measure(v, t, vl, tl, nS)
    assert r["n_unmeasured"].tolist() == [1, 1]
    only = rule.measure(v, t[[0]], vl, tl[[0]], nS)
    assert r["area"][0] == only["area"][0] and r["volume"][0] == only["volume"][0]
    assert np.array_equal(r["bbox_max"][0], v[:2].max(axis=0)) and np.array_equal(r["bbox_min"][1], v[2:4].min(axis=0))
    v, t, vl, tl, nS = cases.extremes()["no_finite_value"]
    r = rule.measure(v, t, vl, tl, nS)
    assert r["n_unmeasured"].tolist() == [0, 1, 0] and r["bbox_min"][1].tolist() == [1.0, np.inf, 1.0] and r["bbox_max"][1].tolist() == [3.0, -np.inf, 5.0]
    assert r["bbox_min"][2].tolist() == [np.inf] * 3 and r["bbox_max"][2].tolist() == [-np.inf] * 3 and r["area"][1] == 0 and r["area"][0] == 0.5
    v, t, vl, tl, nS = cases.extremes()["unused_vertex_sets_extent"]
    assert rule.measure(v, t, vl, tl, nS)["extent_exponent"][0] == 10 and rule.measure(v[:11], t, vl[:11], tl, nS)["extent_exponent"][0] <= 1


def test_the_sums_do_not_depend_on_the_order():
    v, t = cases.mixed(2000)
    tl = (np.arange(len(t)) % 7).astype(np.int32)
    vl = (np.arange(len(v)) % 7).astype(np.int32)
    want = rule.measure(v, t, vl, tl, 7)
    p = np.random.default_rng(1).permutation(len(t))
    assert rule.same_bytes(rule.measure(v, t[p], vl, tl[p], 7), want)
    assert (want["n_unmeasured"] > 0).any() and (want["volume"] != 0).all()
