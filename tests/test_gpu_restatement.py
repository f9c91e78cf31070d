"""The device against the second restatement (tests/restatement.py), bit for bit, with the CPU oracle left out: every kernel value here is held to
numpy float32 written from the F# text, not to anything that descends from oracle/ft_oracle.cpp.  (The oracle module is touched for one thing
only, the project's fixed expf / logf that unionSmooth needs, as in tests/test_oracle_numpy_crosscheck.py.)  Scenes and point families:
tests/form_scenes.py — capsules, tori and triangles alone, in unions of 9 and 12 with a twin whose one radius lies below 2^-20 (the IEEE root
instead of the fast one), under subtract(intersect(union, [X]), Y), an intersect that prunes, a union of combinator objects and smooth unions.

Every scene runs under each arrangement that changes which code evaluates it: the carved kernels on and off (off: the interpreter walks the
family-3 scenes), the lazy union on and off, tail_k at -1 and at 64 (the latency-mode evaluators take the ray buffers whole).  The kernel family
itself is asserted from info()["fast_path"]: 0 for single primitives, the pruning and the smooth scenes and for the carved shape built from
forms under one material, 3 for the unions and what is carved from them object by object, 2 for the union of combinator objects."""
import contextlib
import itertools

import numpy as np
import pytest

import fraytracer_amd as ft
import form_scenes as S
from helpers import assert_bit_equal, options, options_left_at_defaults  # noqa: F401  (options_left_at_defaults: a fixture)

pytestmark = pytest.mark.gpu

ARRANGEMENTS = [dict(carved=c, lazy_union=l, tail_k=t) for c, l, t in itertools.product((1, 0), (1, 0), (-1, 64))]


@contextlib.contextmanager
def device_scene(gpu, b):
    ds = gpu.scene(b.scene)
    try:
        assert ds.info()["fast_path"] == b.case.family, (b.name, ds.info())
        yield ds
    finally:
        ds.close()


def material_index(b, samples):
    """the restatement's index of the material behind each handle of a FieldSamples; -1 stays -1"""
    index = {id(m): k for k, m in enumerate(b.R.materials)}
    handles = np.asarray(samples.material)
    out = np.full(handles.shape, -1, np.int64)
    for h in np.unique(handles[handles >= 0]):
        out[handles == h] = index[id(samples.descriptor(h))]
    return out


@pytest.mark.parametrize("name", S.NAMES)
def test_points(gpu, oracle, name):
    """eval_distance; sample_points with distance, normal and material; bounded sample_points against tryDistance"""
    b = S.built(name, oracle)
    S.assert_tells(b)
    keep, valued = b.keep, ~b.distance[1].threw             # a distance is compared wherever the reference computes one, points at infinity included
    d, nrm, (_, material), bounded = b.distance[0], b.normal, b.colour, b.try_distance
    with device_scene(gpu, b) as ds:
        for arr in ARRANGEMENTS:
            what = f"{name}, {arr}"
            with options(gpu, **arr):
                assert_bit_equal(ds.eval_distance(b.pts)[0][valued], d[valued], what + ": eval_distance")
                got = ds.sample_points(b.pts, normal_epsilon=S.NORMAL_EPS, material=True)
                assert_bit_equal(got.distance[valued], d[valued], what + ": distance")
                assert_bit_equal(got.normal[keep], nrm[keep], what + ": normal")
                assert np.array_equal(material_index(b, got)[keep], material[keep]), what + ": material"
                got = ds.sample_points(b.pts, material=True, bounded=True)
                assert_bit_equal(got.distance[keep], bounded[keep], what + ": tryDistance")
                assert np.array_equal(got.material[keep] >= 0, b.inside[keep]), what + ": material of a point outside the boundary"


@pytest.mark.parametrize("name", S.NAMES)
def test_rays(gpu, oracle, name):
    """SdfForm.tryTrace and SdfObject.tryTrace records of the pixel rays and of rays born at family points"""
    b = S.built(name, oracle)
    form, (obj, _) = b.form_records, b.object_records
    hits = int((form[:, 9].view(np.int32) != 0).sum())
    assert (b.case.empty and hits == 0) or 0 < hits < len(b.rays)
    with device_scene(gpu, b) as ds:
        for arr in ARRANGEMENTS:
            with options(gpu, **arr):
                assert_bit_equal(ds.form_try_trace(b.rays)[0], form, f"{name}, {arr}: form_try_trace")
                assert_bit_equal(ds.object_try_trace(b.rays)[0], obj, f"{name}, {arr}: object_try_trace")


@pytest.mark.parametrize("name", S.NAMES)
def test_frame(gpu, oracle, name):
    b = S.built(name, oracle)
    frame, cnt = b.frame
    assert S.frame_is_telling(b.case, cnt, S.W * S.H), (name, cnt)
    with device_scene(gpu, b) as ds:
        for arr in ARRANGEMENTS:
            with options(gpu, **arr):
                got, st = ds.render(b.case.eps, b.case.length, ft.ImageSize(S.W, S.H), b.cam)
            assert_bit_equal(got, frame, f"{name}, {arr}: frame")
            assert {k: st[k] for k in cnt} == cnt, (name, arr, st, cnt)
