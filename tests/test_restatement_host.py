"""The second restatement (tests/restatement.py: numpy float32, from the F# text) against the CPU oracle and against the product's host flattener,
bit for bit, on the scenes and point families of tests/form_scenes.py: capsules, tori and triangles with their construction-time constants and
boundaries, the union and intersection rules for boundaries, SdfForm.intersect with its pruning test, subtract, the grid union over children
whose boundaries are not their surfaces, unionSmooth over other children than spheres, SdfObject.union's choice of material, and the tryTrace
records and whole frames on such forms.  Two restatements by different routes agreeing is the strongest pin the project has: the reference
ships no fixtures.

Triangles are not compared where a Dot that goes into MathF.Sign is NaN: .NET throws there, the project flags and takes the sign as 0.
The flattened primitive constants (dirInv, the normalised normal, planeD, the triangle's edge normals) have no export in the C ABI; they are
reached through every distance the device computes (tests/test_gpu_restatement.py) and through tests/golden/flatten_constants.json."""
import numpy as np
import pytest

import fraytracer_amd as ft
import form_scenes as S
import restatement as R
from helpers import assert_bit_equal, host  # noqa: F401  (host: a fixture)

F = np.float32


def oracle_scene(oracle, b):
    O = oracle.Oracle()
    memo = {}
    os_ = O.scene(b.scene)
    ft.realise(b.scene.Object, O, memo)
    return O, os_, memo


def same_boundary(got, want, what):
    assert_bit_equal(np.array(got, F), np.concatenate([want[0], [want[1]]]).astype(F), what)


@pytest.mark.parametrize("name", S.NAMES)
def test_scene_tells(oracle, name):
    S.assert_tells(S.built(name, oracle))


@pytest.mark.parametrize("name", S.NAMES)
def test_distance_and_colour_match_oracle(oracle, name):
    b = S.built(name, oracle)
    O, os_, _ = oracle_scene(oracle, b)
    d, rec = b.distance
    keep = ~rec.threw
    with np.errstate(all="ignore"):
        want = O.form_distance(O.object_form(os_.object), b.pts)
    bad = np.flatnonzero(keep & ~((d.view(np.uint32) == want.view(np.uint32)) | (np.isnan(d) & np.isnan(want))))
    assert bad.size == 0, (name, b.family_at(bad[0]), b.pts[bad[0]], d[bad[0]], want[bad[0]], bad.size)
    some = np.flatnonzero(b.keep)[::3]
    col = np.array([O.object_color(os_.object, p) for p in b.pts[some]], F)
    assert_bit_equal(b.colour[0][some], col, f"{name}: object colour")
    inside = b.inside                                       # tryDistance is Distance where isInside, by the same boundary the oracle must report
    assert inside[b.keep].any() and not inside[b.keep].all()
    assert_bit_equal(b.try_distance[inside & keep], want[inside & keep], f"{name}: tryDistance")
    assert np.isnan(b.try_distance[~inside]).all()


@pytest.mark.parametrize("name", S.NAMES)
def test_boundaries_and_lookups_match_oracle_and_flattener(oracle, host, name):
    b = S.built(name, oracle)
    O, os_, mo = oracle_scene(oracle, b)
    mh = {}
    ft.realise(b.scene.Object, host, mh)
    forms = R.all_forms(b.scene.Object)
    for f in forms:
        want = b.R.forms[id(f)].boundary
        same_boundary(O.form_boundary(mo[id(f)]), want, f"{name}: oracle's boundary of {f}")
        same_boundary(host.form_boundary(mh[id(f)]), want, f"{name}: flattener's boundary of {f}")
    for i, o in b.R.objects.items():                        # the forms SdfObject.union / subtract / intersect build themselves
        same_boundary(O.form_boundary(O.object_form(mo[i])), o.form.boundary, f"{name}: oracle's boundary of an object's form")
        same_boundary(host.form_boundary(host.object_form(mh[i])), o.form.boundary, f"{name}: flattener's boundary of an object's form")
    ds = host.scene(b.scene)
    same_boundary(ds.boundary(), b.boundary, f"{name}: scene.boundary()")
    assert ds.info()["fast_path"] == b.case.family
    unions = [(mo[id(f)], b.R.forms[id(f)]) for f in forms if f.kind == "union"]
    unions += [(O.object_form(mo[i]), o.form) for i, o in b.R.objects.items() if isinstance(o, R.ObjectUnion)]
    assert len(unions) == len(b.R.unions)
    for handle, union in unions:
        g, want = O.grid(handle), union.lookup.dump()
        assert g["counts"] == want["counts"]
        for k in ("aabbMin", "cellSize", "cellSizeInv", "centers", "lower"):
            assert_bit_equal(g[k], want[k], f"{name}: lookup {k}")
        assert np.array_equal(g["cell_start"], want["cell_start"]) and np.array_equal(g["child"], want["child"])
    if ds.info()["n_grids"] == 1 and len(unions) == 1:
        g, want = ds.grid(0), unions[0][1].lookup.dump()
        assert g["counts"] == want["counts"]
        for k in ("aabbMin", "cellSizeInv", "centers", "lower"):
            assert_bit_equal(g[k], want[k], f"{name}: flattened grid {k}")
        assert np.array_equal(g["cell_start"], want["cell_start"]) and np.array_equal(g["child"], want["child"])
    else:
        assert not name.startswith(("union of", "carved")), name
    ds.close()


@pytest.mark.parametrize("name", S.NAMES)
def test_records_and_frame_match_oracle(oracle, name):
    b = S.built(name, oracle)
    _, os_, _ = oracle_scene(oracle, b)
    with np.errstate(all="ignore"):
        form, fc = os_.form_try_trace(b.rays)
        obj, oc = os_.object_try_trace(b.rays)
        frame, cnt = os_.render(b.case.eps, b.case.length, S.W, S.H, b.cam.as_array())
    assert fc["flags"] == oc["flags"] == 0
    assert_bit_equal(b.form_records, form, f"{name}: SdfForm.tryTrace")
    assert_bit_equal(b.object_records[0], obj, f"{name}: SdfObject.tryTrace")
    assert_bit_equal(b.frame[0], frame, f"{name}: frame")
    assert {k: cnt[k] for k in b.frame[1]} == b.frame[1]
    hits = int((b.form_records[:, 9].view(np.int32) != 0).sum())
    assert (b.case.empty and hits == 0) or 0 < hits < len(b.rays)
