"""The flatten-time gates of the fast sphere arithmetic (scene.cpp fastSphereRun, noteUnionChild, carvedShape), on the CPU: each gate flips the
classification between two adjacent floats, the stage limit between 3072 and 3073 spheres; and the oracle's float32 distance of every lean gate
scene agrees with the float64 formula -s ln sum exp(-(|c - p| - r) / s) at every point family, so that the oracle and the kernels cannot be wrong
together at t = 80 or at coordinates of 1e4.

Measured deviation |f32 - f64| / (s (n 2^-23 + |t|max 2^-22) + (|p|inf + |c|inf + r) 2^-21), maximum over all lean gate scenes and families:
0.189 (MEASURED below, rounded up), at the guard points of the a = 2^-20 twin; no scene is below 0.0004 or above 0.19, the ones at |c| about 1e4
being the lowest because c - p is exact there.  The oracle's exp is the project's fixed algorithm; its log is the C library's logf, so the test
allows 4 x the measured value for other builds of it."""
import numpy as np
import pytest

import fraytracer_amd as ft
import gate_scenes as G
from helpers import host  # noqa: F401  (a fixture)

MEASURED = 0.19
F = np.float32


def classify(host, scene):
    ds = host.scene(scene)
    try:
        return ds.info(), ds.miss_certificate()["margin"]
    finally:
        ds.close()


def one_step_apart(inside, outside):
    """the two blobs differ in exactly one float32 value, and there by exactly one step"""
    a = np.concatenate([[F(inside.strength)], inside.spheres.reshape(-1)]).astype(F)
    b = np.concatenate([[F(outside.strength)], outside.spheres.reshape(-1)]).astype(F)
    at = np.nonzero(a != b)[0]
    return len(at) == 1 and (np.nextafter(a[at[0]], b[at[0]]) == b[at[0]])


@pytest.mark.parametrize("name", G.LEAN_NAMES)
def test_each_gate_flips_between_adjacent_floats(host, name):
    inside, outside = G.lean_gates()[name]
    assert 8 <= len(inside.spheres) <= 40
    info, margin = classify(host, inside.scene())
    assert info["fast_path"] == 1 and margin >= 0.0, (info, margin)                        # the certificate's constants exist on the inside only
    if outside is None:
        return
    assert one_step_apart(inside, outside)
    info, margin = classify(host, outside.scene())
    assert info["fast_path"] == 0 and margin < 0.0, (info, margin)


def test_gate_values_are_the_stated_ones():
    """the scenes sit where the table of DESIGN.md section 4 says: a = 32 and 2^-20 exactly, r a = 80 exactly, r = 2^-20, |c|inf = 1e4"""
    g = G.lean_gates()
    assert g["a = 32"][0].a == 32.0 and g["a = 32"][1].a == G.above(32.0)
    assert g["a = 2^-20"][0].a == 2.0 ** -20 and g["a = 2^-20"][1].a < 2.0 ** -20
    for name in ("r a = 80 at a = 32", "r a = 80 at r = 1e4"):
        for side, blob in zip(("inside", "outside"), g[name]):
            ra = float((blob.spheres[:, 3] * F(blob.a)).max())                             # float32 product, as scene.cpp forms it
            assert (ra == 80.0) if side == "inside" else (ra > 80.0), (name, side, ra)
    assert g["r = 2^-20"][0].spheres[:, 3].min() == F(2.0 ** -20) and g["r = 2^-20"][1].spheres[:, 3].min() == F(G.below(2.0 ** -20))
    assert np.abs(g["|c| = 1e4"][0].spheres[:, :3]).max() == F(1.0e4) and np.abs(g["|c| = 1e4"][1].spheres[:, :3]).max() == F(G.above(1.0e4))
    far = g["cluster at 1e4"][0]
    assert (np.abs(far.spheres[:, :3]).min(axis=1) > 9980.0).all() and (far.spheres[-2, :3] == np.array(G.CORNER, F)).all() and far.spheres[-1, 3] == F(2.0 ** -20)
    for name in G.NEAR_SCENES:
        assert (np.linalg.norm(g[name][0].spheres[:, :3].astype(np.float64), axis=1) <= 1.0).all() and g[name][0].near_radius() > 1.0, name


@pytest.mark.parametrize("name", G.STAGE_NAMES)
def test_stage_limit(host, name):
    info, margin = classify(host, G.stage_scene(name))
    fast_path, cull_pc, n_consts, n_slots = G.STAGE_INFO[name]
    assert (info["fast_path"], info["cull_pc"]) == (fast_path, cull_pc), info
    assert n_consts is None or info["n_consts"] == n_consts, info
    assert n_slots is None or info["n_slots"] == n_slots, info
    assert (margin >= 0.0) == (fast_path == 1)


@pytest.mark.parametrize("variant", G.UNION_VARIANTS)
@pytest.mark.parametrize("name", G.UNION_NAMES)
def test_union_and_carved_classification(host, name, variant):
    info, margin = classify(host, ft.SdfScene(G.union_object(name, variant), (0.1, 0.1, 0.1), []))
    assert info["n_grids"] == 1 and info["n_children"] == (60 if "corner" in name else 16) and margin < 0.0, info
    assert info["fast_path"] == 3, info                        # a plain union of primitives is the carved shape with an empty tail (scene.cpp carvedShape)


def test_union_twins_are_one_step_apart():
    for name, g in G.union_gates().items():
        at = np.argwhere(g["rows"] != g["twin"])
        assert len(at) == 1, name
        i, j = at[0]
        assert np.nextafter(g["rows"][i, j], F(np.inf)) == g["twin"][i, j] and g["rows"][i, j] == F(1.0e4), name
        rows = g["rows"]
        assert (np.abs(rows[:, :3]) <= F(1.0e4)).all() and rows[:, 3].min() >= F(2.0 ** -20) and rows[:, 3].max() <= F(1.0e4)
        assert (rows[:, 3] == F(2.0 ** -20)).any() or (rows[:, 3] == F(1.0e4)).any(), name


@pytest.mark.parametrize("name,side", G.lean_cases(), ids=lambda v: str(v))
def test_oracle_against_float64(oracle, name, side):
    blob = G.lean_blob(name, side)
    fam = G.lean_families(oracle, blob)
    G.assert_families_tell(oracle, blob, fam)
    O = oracle.Oracle()
    form = O.object_form(O.scene(blob.scene()).object)
    s, n = blob.strength, len(blob.spheres)
    c_inf, r_max = float(np.abs(blob.spheres[:, :3]).max()), float(blob.spheres[:, 3].max())
    worst = 0.0
    for key, pts in fam.items():
        with np.errstate(all="ignore"):
            d32 = O.form_distance(form, pts).astype(np.float64)
        d64, total, t_abs, _ = blob.exact(pts)
        ok = np.isfinite(d64) & (total >= 2.0 ** -125) & (total <= 1.0e38) & np.isfinite(pts).all(axis=1)      # the float32 sum is a normal number
        if key not in ("guard", "far ring"):                                               # the far ring's sums are mostly subnormal or zero
            assert ok.mean() >= 0.9, (key, float(ok.mean()))
        assert np.isfinite(d32[ok]).all(), key
        scale = s * (n * 2.0 ** -23 + t_abs * 2.0 ** -22) + (np.abs(pts).max(axis=1) + c_inf + r_max) * 2.0 ** -21
        dev = np.abs(d32[ok] - d64[ok]) / scale[ok]
        if len(dev):
            print(f"{name}, {side}, {key}: {ok.sum()} points compared, deviation {dev.max():.4f}")
            worst = max(worst, float(dev.max()))
    assert worst <= 4.0 * MEASURED, (name, side, worst)


def test_views_and_ray_buffers_tell(oracle):
    """the conditions on every frame and ray buffer that the GPU tests trace, from the oracle alone: no flag, hits and misses, lit and shadowed hits"""
    for name, side in G.lean_cases():
        blob = G.lean_blob(name, side)
        scene, cam, os_, (frame, cnt) = G.view_of(oracle, blob.object(), blob.focus, blob.eps, convex=blob.convex)
        fam = G.lean_families(oracle, blob)
        rays = G.ray_buffer(oracle, fam, blob.focus, blob.eps, cam)
        packs = G.ray_packs(oracle, fam, blob.focus, blob.eps, cam)
        assert len(rays) >= 256 and sorted({len(r) for _, r in packs}) == [1, 8, 32]
        together = np.concatenate([r for _, r in packs])
        with np.errstate(all="ignore"):
            for buf in (rays, together):
                rc = os_.trace_rays(buf)[1]
                assert G.frame_is_telling(rc, len(buf), blob.convex), (name, side, rc)
            assert all(os_.trace_rays(r)[1]["flags"] == 0 for _, r in packs), (name, side)
    for name in G.UNION_NAMES:
        g = G.union_gates()[name]
        for variant in G.UNION_VARIANTS:
            G.view_of(oracle, G.union_object(name, variant), g["focus"], g["eps"])
