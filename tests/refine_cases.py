"""Inputs shared by the refinement's tests (tests/test_refine_host.py, tests/test_gpu_refine.py): the scenes and lattices of mesh_cases, the oracle's
distance as a callable, and the restatement's refined vertices on the oracle's distances — computed once, shared, never written to."""
import functools

import numpy as np

import mesh_cases as cases
import refine_restatement as rule
import slice_restatement as slices

F = np.float32
ISOS = (0.0, 0.03)


@functools.lru_cache(maxsize=None)
def form_of(oracle, name):
    """(an Oracle, the scene in it, the scene object's form)"""
    os_ = oracle.Oracle().scene(cases.scene_of(name))
    O = oracle.Oracle()
    return O, os_, O.object_form(os_.object)


def distance_of(oracle, name):
    """points float32 [n, 3] -> the oracle's sdf.Distance float32 [n]"""
    O, _, form = form_of(oracle, name)

    def distance(pts):
        pts = np.ascontiguousarray(pts, dtype=F).reshape(-1, 3)
        if not len(pts):
            return np.zeros(0, F)
        with np.errstate(all="ignore"):
            return np.ascontiguousarray(O.form_distance(form, pts), dtype=F)
    return distance


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def brackets(oracle, name, iso, axis=None, libm=False):
    """(Brackets, edge lengths) of a scene's lattice: the mesher's (axis None) or a slice axis'.  libm: as in mesh_cases.oracle_lattice"""
    origin, step, d = cases.oracle_lattice(oracle, name, libm)
    br, length = rule.lattice_brackets(d, origin, step, iso, rule.MESH_DIRS if axis is None else rule.slice_dirs(axis))
    return rule.Brackets(*map(frozen, br)), frozen(length)


@functools.lru_cache(maxsize=None)
def refined(oracle, name, iso, R, axis=None, libm=False):
    """the restatement's vertices after R rounds on the oracle's distances, in key order"""
    br, _ = brackets(oracle, name, iso, axis, libm)
    return frozen(rule.bisect(*br, distance_of(oracle, name), iso, R))


@functools.lru_cache(maxsize=None)
def slice_order(oracle, name, iso, axis):
    """the vertex (in the slice's key order) behind every point of the unrefined contours, from slice_restatement's pieces"""
    _, _, d = cases.oracle_lattice(oracle, name)
    with np.errstate(all="ignore"):
        s = (d - F(iso)).astype(F)
    starts, ends, _ = slices.segments(s, slices.vertex_table(s, axis), axis)
    order = [v for walk, _ in slices.chain(starts, ends) for v in walk]
    return frozen(np.asarray(order, np.int64))
