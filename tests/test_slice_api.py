"""Slicing (ft_slice_lattice, ft_slice_values, ft_slice_values_device and what reads the contours): the parts that need no GPU — the ABI, the
header's statement of the rule, every refusal that comes before the device is asked for, the empty result of a lattice without cells, the direction
table against the integer geometry, Contours.layer and the SVG writer, the build's bookkeeping, the C++ and F# mirrors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import _lib
from fraytracer_amd import synthetic as syn
from helpers import HEADER, ROOT, assert_cpp_compiles, assert_declared_exported_bound, dev_ptr as _p, host_ptr as ptr

import slice_restatement as rule

NAMES = ("ft_slice_lattice", "ft_slice_values", "ft_slice_values_device", "ft_slices_get_info", "ft_slices_device_buffers", "ft_slices_read", "ft_slices_destroy")
INVALID, UNSUPPORTED, NO_DEVICE, OK = _lib.FT_ERR_INVALID, _lib.FT_ERR_UNSUPPORTED, _lib.FT_ERR_NO_DEVICE, _lib.FT_OK
L = _lib.lib


def test_symbols_are_declared_exported_and_bound():
    assert_declared_exported_bound(NAMES)
    assert C.sizeof(_lib.Polyline) == 16 and C.sizeof(_lib.SlicesInfo) == 48 and (_lib.FT_SLICE_NORMAL, _lib.FT_SLICE_MATERIAL) == (1, 2)
    assert [n for n, _ in _lib.Polyline._fields_] == ["first", "count", "slice", "closed"]
    assert L.ft_abi_version() == 5                                                         # additive: the ABI version stays
    assert ft.Contours is ft.api.Contours and "Contours" in ft.__all__
    assert callable(ft.SdfForm.slice) and callable(ft.DeviceScene.slice_lattice) and callable(ft.Device.slice_values)


def test_header_is_still_plain_c99(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER])
    src = tmp_path / "use.c"
    src.write_text('#include "fraytracer_hip.h"\n'
                   "typedef char polyline_is_16_bytes[sizeof(ft_polyline) == 16 ? 1 : -1];\n"
                   "typedef char info_is_48_bytes[sizeof(ft_slices_info) == 48 ? 1 : -1];\n"
                   "int f(ft_ctx* c, const ft_scene* s, const float* v, void* d, ft_vec3* p, ft_polyline* l, int32_t* m) {\n"
                   "    ft_lattice lat = {{0.0f, 0.0f, 0.0f}, {1.0f, 1.0f, 1.0f}, 2, 3, 4};\n"
                   "    ft_slices* r = 0; ft_slices_info i; void* b[4];\n"
                   "    int rc = ft_slice_lattice(c, s, &lat, 2, 0.0f, 0.001f, FT_SLICE_NORMAL | FT_SLICE_MATERIAL, &r) + ft_slice_values(c, &lat, v, 0, 0.5f, &r)\n"
                   "           + ft_slice_values_device(c, &lat, d, 1, 0.0f, &r) + ft_slices_get_info(r, &i) + ft_slices_device_buffers(r, &b[0], &b[1], &b[2], &b[3])\n"
                   "           + ft_slices_read(r, p, l, p, m);\n"
                   "    ft_slices_destroy(r);\n"
                   "    return rc + l[0].first + l[0].count + l[0].slice + l[0].closed + (int)i.n_closed + i.axis + i.n_slices;\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_header_states_the_rule_once():
    text = open(HEADER).read()
    m = re.search(r"/\* Slicing:(?:(?!\*/).)*?\*/\s*#define FT_SLICE_NORMAL", text, flags=re.S)
    assert m and text.count("/* Slicing:") == 1 and text.index("/* Meshing:") < m.start()
    doc = " ".join(re.sub(r"\n \*", "\n", m.group(0)).split())
    for phrase in ("exactly the section of the mesher's surface by a lattice plane", "(0,0)-(1,1) diagonal", "u = (a + 1) % 3", "v = (a + 2) % 3",
                   "(u, v, a) is right-handed", "A count of 1 along a is one slice", "A count of 1 along u or v leaves no cells", "no device needed",
                   "s[q] = d[q] - iso, inside iff s[q] < 0", "+v, +u and +u+v", "e 0, 1, 2 for axis 0; 0, 3, 4 for axis 1; 1, 3, 5 for axis 2",
                   "operation for operation", "bit for bit the vertex the mesher puts on the same edge", "keys order by q, then e",
                   "T0 = {c0, c0 + u, c0 + u + v}", "T1 = {c0, c0 + v, c0 + u + v}", "counted in n_skipped", "one segment", "never from floats or the sign of a step",
                   "the inside corners lie to the segment's left", "(det(M2 - M1, L - M1) > 0) == (L is inside)", "counter-clockwise seen from +a",
                   "holes run clockwise", "start of at most one segment and the end of at most one", "maximal chain of segments", "starting at the vertex of smallest key",
                   "whose first vertex no segment ends in", "its m + 1 points", "A vertex that no segment uses is not written",
                   "ordered by the key of their first point", "ft_polyline.slice tells them apart", "closed unless it ends on the lattice's border",
                   "zero-length segments but keeps loops closed", "2^31 or more points or polylines is FT_ERR_UNSUPPORTED", "never FT_FIELD_BOUNDED",
                   "ft_sample_points_device", "synchronises the context's stream TWICE", "2^R at least the vertex total", "without a synchronisation between them",
                   "nothing is written at or beyond the counted totals", "after the counts and before the flag bits", "On any failure *out is NULL",
                   "outlive their scene but not their context", "accepts NULL for any part"):
        assert phrase in doc, phrase
    # what is shared with the mesher is stated there, not again
    for phrase in ("one true division", "never a fused multiply-add", "t = s[q] / (s[q] - s[q'])"):
        assert phrase not in doc, phrase


@pytest.fixture(scope="module")
def host_scene():
    """a scene on a host-only context: what a call on it returns other than FT_ERR_NO_DEVICE comes from a check made before any device work"""
    dev = ft.Device(-1)
    ds = dev.scene(syn.config3(n=8)[0])
    yield dev._ctx, ds._scene
    dev.close()


def lattice(nx=2, ny=3, nz=4):
    return _lib.Lattice(_lib.Vec3(0, 0, 0), _lib.Vec3(1, 1, 1), nx, ny, nz)


def test_every_refusal_comes_before_the_device_is_asked_for(host_scene):
    ctx, sc = host_scene
    vals = np.zeros(24, np.float32)
    lat = lattice()
    out = C.c_void_p(0xDEAD)
    o = C.byref(out)

    def refused(rc, want):
        assert rc == want and out.value is None, (rc, want, out.value)                     # *out is NULL on any failure
        out.value = 0xDEAD

    # the arguments pass: only then is the device missed
    for axis in (0, 1, 2):
        refused(L.ft_slice_lattice(ctx, sc, C.byref(lat), axis, 0.0, 0.0, 0, o), NO_DEVICE)
        refused(L.ft_slice_lattice(ctx, sc, C.byref(lat), axis, 0.25, 0.001, 3, o), NO_DEVICE)
        refused(L.ft_slice_values(ctx, C.byref(lat), ptr(vals), axis, 0.0, o), NO_DEVICE)
        refused(L.ft_slice_values_device(ctx, C.byref(lat), _p(4096), axis, 0.0, o), NO_DEVICE)
    refused(L.ft_slice_values_device(ctx, C.byref(lattice(16777216, 2, 2)), _p(4096), 1, 0.0, o), NO_DEVICE)      # the largest count
    # NULL where none is allowed
    refused(L.ft_slice_lattice(None, sc, C.byref(lat), 2, 0.0, 0.0, 0, o), INVALID)
    refused(L.ft_slice_lattice(ctx, None, C.byref(lat), 2, 0.0, 0.0, 0, o), INVALID)
    refused(L.ft_slice_lattice(ctx, sc, None, 2, 0.0, 0.0, 0, o), INVALID)
    assert L.ft_slice_lattice(ctx, sc, C.byref(lat), 2, 0.0, 0.0, 0, None) == INVALID
    refused(L.ft_slice_values(None, C.byref(lat), ptr(vals), 2, 0.0, o), INVALID)
    refused(L.ft_slice_values(ctx, None, ptr(vals), 2, 0.0, o), INVALID)
    refused(L.ft_slice_values(ctx, C.byref(lat), None, 2, 0.0, o), INVALID)
    assert L.ft_slice_values(ctx, C.byref(lat), ptr(vals), 2, 0.0, None) == INVALID
    refused(L.ft_slice_values_device(None, C.byref(lat), _p(4096), 2, 0.0, o), INVALID)
    refused(L.ft_slice_values_device(ctx, None, _p(4096), 2, 0.0, o), INVALID)
    refused(L.ft_slice_values_device(ctx, C.byref(lat), None, 2, 0.0, o), INVALID)
    assert L.ft_slice_values_device(ctx, C.byref(lat), _p(4096), 2, 0.0, None) == INVALID
    # a count < 1 or > 2^24
    for bad in (lattice(0, 3, 4), lattice(2, -1, 4), lattice(2, 3, 0), lattice(16777217, 2, 2), lattice(2, 16777217, 2), lattice(2, 2, 16777217)):
        refused(L.ft_slice_lattice(ctx, sc, C.byref(bad), 2, 0.0, 0.0, 0, o), INVALID)
        refused(L.ft_slice_values(ctx, C.byref(bad), ptr(vals), 2, 0.0, o), INVALID)
        refused(L.ft_slice_values_device(ctx, C.byref(bad), _p(4096), 2, 0.0, o), INVALID)
    # an axis outside 0 .. 2
    for axis in (-1, 3, 7, -2 ** 31, 2 ** 31 - 1):
        refused(L.ft_slice_lattice(ctx, sc, C.byref(lat), axis, 0.0, 0.0, 0, o), INVALID)
        assert b"axis" in L.ft_last_error()
        refused(L.ft_slice_values(ctx, C.byref(lat), ptr(vals), axis, 0.0, o), INVALID)
        refused(L.ft_slice_values_device(ctx, C.byref(lat), _p(4096), axis, 0.0, o), INVALID)
    # unknown flag bits
    for flags in (4, 7, 0x80000000):
        refused(L.ft_slice_lattice(ctx, sc, C.byref(lat), 2, 0.0, 0.0, flags, o), INVALID)
    # a misaligned device pointer
    for addr in (4097, 4098, 4099):
        refused(L.ft_slice_values_device(ctx, C.byref(lat), _p(addr), 2, 0.0, o), INVALID)
    # too many points for one call; the last two are exactly 0xFFFF0000
    for huge in (lattice(65536, 65536, 2), lattice(16777216, 256, 2), lattice(16777216, 16777216, 16777216), lattice(2, 65536, 65536), lattice(65536, 32768, 2),
                 lattice(65535, 32768, 2), lattice(65536, 65535, 1)):
        refused(L.ft_slice_lattice(ctx, sc, C.byref(huge), 0, 0.0, 0.0, 0, o), UNSUPPORTED)
        refused(L.ft_slice_values(ctx, C.byref(huge), ptr(vals), 0, 0.0, o), UNSUPPORTED)
        refused(L.ft_slice_values_device(ctx, C.byref(huge), _p(4096), 0, 0.0, o), UNSUPPORTED)
    refused(L.ft_slice_values_device(ctx, C.byref(lattice(65535, 32767, 2)), _p(4096), 0, 0.0, o), NO_DEVICE)      # below it
    # the order: the counts before the axis, the axis before the flag bits, the flag bits before the alignment, invalid before unsupported
    refused(L.ft_slice_lattice(ctx, sc, C.byref(lattice(0, 3, 4)), 5, 0.0, 0.0, 4, o), INVALID)
    assert b"count" in L.ft_last_error()
    refused(L.ft_slice_lattice(ctx, sc, C.byref(lat), 5, 0.0, 0.0, 4, o), INVALID)
    assert b"axis" in L.ft_last_error()
    refused(L.ft_slice_lattice(ctx, sc, C.byref(lat), 2, 0.0, 0.0, 4, o), INVALID)
    assert b"flag" in L.ft_last_error()
    refused(L.ft_slice_values_device(ctx, C.byref(lat), _p(4097), 3, 0.0, o), INVALID)
    assert b"axis" in L.ft_last_error()
    refused(L.ft_slice_values_device(ctx, C.byref(lattice(65536, 65536, 2)), _p(4097), 2, 0.0, o), INVALID)
    refused(L.ft_slice_values_device(ctx, C.byref(lattice(65536, 65536, 2)), _p(4096), 3, 0.0, o), INVALID)
    # a scene of another context
    other = ft.Device(-1)
    try:
        foreign = other.scene(syn.config3(n=8)[0])._scene
        refused(L.ft_slice_lattice(ctx, foreign, C.byref(lat), 2, 0.0, 0.0, 0, o), INVALID)
    finally:
        other.close()
    # readers of the contours: NULL
    info = _lib.SlicesInfo()
    assert L.ft_slices_get_info(None, C.byref(info)) == INVALID and L.ft_slices_read(None, None, None, None, None) == INVALID
    assert L.ft_slices_device_buffers(None, None, None, None, None) == INVALID
    L.ft_slices_destroy(None)                                                              # a no-op


def test_a_lattice_without_cells_is_an_empty_result_without_a_device(host_scene):
    ctx, sc = host_scene
    vals = np.full(70, -1.0, np.float32)
    # (lattice, axis, form): a count of 1 along u or v; a count of 1 along the axis alone is one slice and needs the device
    for lat, axis, make in ((lattice(1, 1, 1), 0, "values"), (lattice(1, 70, 1), 0, "values"), (lattice(7, 1, 10), 2, "device"), (lattice(5, 14, 1), 1, "scene"),
                            (lattice(5, 1, 14), 0, "values")):
        out = C.c_void_p()
        if make == "values":
            rc = L.ft_slice_values(ctx, C.byref(lat), ptr(vals), axis, 0.0, C.byref(out))
        elif make == "device":
            rc = L.ft_slice_values_device(ctx, C.byref(lat), _p(4096), axis, 0.0, C.byref(out))
        else:
            rc = L.ft_slice_lattice(ctx, sc, C.byref(lat), axis, 0.0, 0.001, _lib.FT_SLICE_NORMAL, C.byref(out))
        assert rc == OK and out.value
        info = _lib.SlicesInfo()
        assert L.ft_slices_get_info(out, C.byref(info)) == OK and L.ft_slices_get_info(out, None) == INVALID
        assert (info.n_points, info.n_polylines, info.n_closed, info.n_skipped) == (0, 0, 0, 0)
        assert (info.axis, info.n_slices) == (axis, (lat.nx, lat.ny, lat.nz)[axis])
        assert (info.has_normal, info.has_material) == ((1, 0) if make == "scene" else (0, 0))
        bufs = [C.c_void_p(1) for _ in range(4)]
        assert L.ft_slices_device_buffers(out, *map(C.byref, bufs)) == OK and [b.value for b in bufs] == [None] * 4
        assert L.ft_slices_device_buffers(out, None, None, None, None) == OK
        assert L.ft_slices_read(out, None, None, None, None) == OK
        if make != "scene":
            assert L.ft_slices_read(out, None, None, ptr(vals), None) == INVALID               # normals of contours built without them
        L.ft_slices_destroy(out)
    out = C.c_void_p(0xDEAD)
    assert L.ft_slice_values(ctx, C.byref(lattice(1, 5, 14)), ptr(vals), 0, 0.0, C.byref(out)) == NO_DEVICE and out.value is None      # one slice of 5 x 14
    dev = ft.Device(-1)
    try:
        c = dev.slice_values(np.zeros((4, 1, 4), np.float32), (0, 0, 0), (1, 1, 1), axis=0)
        assert c.points.shape == (0, 3) and c.polylines.shape == (0, 4) and c.polylines.dtype == np.int32 and (c.skipped, c.closed, c.axis, c.slices) == (0, 0, 0, 4)
        assert c.normal is None and c.material is None and c.layer(0) == []
        with pytest.raises(ValueError, match=r"\[nx, ny, nz\]"):
            dev.slice_values(np.zeros((4, 4), np.float32), (0, 0, 0), (1, 1, 1))
        with pytest.raises(ft.FrayTracerError) as e:
            dev.slice_values(np.zeros((2, 2, 2), np.float32), (0, 0, 0), (1, 1, 1))
        assert e.value.code == NO_DEVICE
        with pytest.raises(ft.FrayTracerError) as e:
            dev.slice_values(np.zeros((2, 2, 2), np.float32), (0, 0, 0), (1, 1, 1), axis=3)
        assert e.value.code == INVALID
        ds = dev.scene(syn.config3(n=8)[0])
        with pytest.raises(ValueError, match="like"):
            ds.slice_lattice((0, 0, 0), (1, 1, 1), (2, 2, 2), like=np.zeros(3))
        with pytest.raises(ValueError, match="counts"):
            ds.slice_lattice((0, 0, 0), (1, 1, 1), (2, 0, 2))
        with pytest.raises(ft.FrayTracerError) as e:
            ds.slice_lattice((0, 0, 0), (1, 1, 1), (2, 2, 2), axis=1, normal_epsilon=0.01, material=True)
        assert e.value.code == NO_DEVICE
    finally:
        dev.close()


def test_internal_tile_switch_is_per_context(host_scene):
    ctx, _ = host_scene
    fn = L.ft_ctx_slice_tile                                                               # internal: not in the header
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int32]
    assert [fn(ctx, t) for t in (128, 256, 1024, 512)] == [OK] * 4
    assert [fn(ctx, t) for t in (0, 64, 192, 2048, -256)] == [INVALID] * 5 and fn(None, 256) == INVALID
    assert "ft_ctx_slice_tile" not in open(HEADER).read()
    probe = L.ft_ctx_slice_probe                                                           # internal (tools/slice_probe.py): where this context's extractions end
    probe.restype, probe.argtypes = C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]
    last = (C.c_int64 * 2)(7, 7)
    assert [probe(ctx, s, None) for s in (1, 2, 0)] == [OK] * 3 and probe(ctx, 0, last) == OK and list(last) == [0, 0]
    assert [probe(ctx, s, None) for s in (-1, 3)] == [INVALID] * 2 and probe(None, 0, None) == INVALID
    assert "ft_ctx_slice_probe" not in open(HEADER).read()


def test_direction_table_is_the_integer_geometry():
    """the table the link kernel reads (built at compile time, slice.hip) against the restatement's direction, word by word: entry [triangle][inside
    mask] = 1 | start slot << 1 | end slot << 5, slot = (owner corner 2 du + dv) << 2 | (direction 2 du + dv)"""
    fn = L.ft_slice_table                                                                  # internal: not in the header
    fn.restype = C.POINTER(C.c_uint32)
    table = fn()

    def slot(tri, x, y):
        lo, hi = sorted((tri[x], tri[y]), key=sum)
        return ((2 * lo[0] + lo[1]) << 2) | (2 * (hi[0] - lo[0]) + (hi[1] - lo[1]))

    words = 0
    for t, tri in enumerate(rule.TRIANGLES):
        for mask in range(8):
            seg = rule.directed_segment(tri, [bool(mask >> x & 1) for x in range(3)])
            word = int(table[t * 8 + mask])
            if seg is None:
                assert word == 0 and mask in (0, 7), (t, mask)
                continue
            assert word == 1 | (slot(tri, *seg[0]) << 1) | (slot(tri, *seg[1]) << 5), (t, mask)
            words += 1
    assert words == 12


def sample_contours():
    """two loops in slice 0 (a rim and its hole), an open chain in slice 1"""
    n = 12
    t = np.arange(n, dtype=np.float32) - np.float32(5.4)
    r = np.sqrt(t[:, None] ** 2 + t[None, :] ** 2)
    d = np.stack([np.abs(r - np.float32(3.5)) - np.float32(1.3), np.broadcast_to(t[:, None] - np.float32(0.2), (n, n))], axis=2).astype(np.float32)
    c = rule.extract(d, (0.0, 0.0, 0.0), (0.5, 0.25, 1.0), 2)
    assert c.polylines[:, 2].tolist().count(0) == 2 and c.polylines[:, 2].tolist().count(1) == 1 and c.closed == 2
    return c


def test_layer_and_svg_round_trip(tmp_path):
    c = sample_contours()
    got = ft.Contours(c.points, c.polylines, skipped=c.skipped, closed=c.closed, axis=2, slices=2)
    for w in (0, 1):
        rows = [r for r in c.polylines.tolist() if r[2] == w]
        layer = got.layer(w)
        assert [(len(p), closed) for p, closed in layer] == [(n, bool(cl)) for _, n, _, cl in rows]
        assert all(np.array_equal(p, c.points[f:f + n]) for (p, _), (f, n, _, _) in zip(layer, rows))     # the rule's order
        path = tmp_path / f"layer{w}.svg"
        got.write_svg(str(path), w)
        text = path.read_text()
        assert text.startswith("<svg ") and text.rstrip().endswith("</svg>") and 'scale(1,-1)' in text and "evenodd" in text
        paths = re.findall(r'<path d="M ([^"]*?)( Z)?"', text)
        assert len(paths) == len(rows)
        for (body, z), (f, n, _, cl) in zip(paths, rows):
            xy = np.array([[float(x) for x in pair.split()] for pair in body.split(" L ")], np.float32)
            assert np.array_equal(xy.view(np.uint32), c.points[f:f + n, :2].view(np.uint32))       # float32 round-trips through 9 digits; u right, v up
            assert bool(z) == bool(cl)
    assert got.layer(5) == [] and got.descriptor(-1) is None
    assert ft.Contours(c.points, c.polylines, material=np.zeros(len(c.points), np.int32), materials={0: "x"}).descriptor(0) == "x"
    # another axis: u = z, v = x
    side = ft.Contours(c.points[:, [1, 2, 0]], c.polylines, axis=1, slices=2)
    side.write_svg(str(tmp_path / "side.svg"), 0)
    body = re.findall(r'<path d="M ([^"]*?)( Z)?"', (tmp_path / "side.svg").read_text())[0][0]
    first = [float(x) for x in body.split(" L ")[0].split()]
    f0 = [r for r in c.polylines.tolist() if r[2] == 0][0][0]
    assert np.array_equal(np.array(first, np.float32), c.points[f0, :2])


def test_the_build_knows_the_new_translation_unit():
    csrc = os.path.join(ROOT, "fraytracer_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    rule_ = re.search(r"^slice\.o:(.*)$", mk, flags=re.M).group(1).split()
    inc = set(re.findall(r'^\s*#include\s+"([^"]+)"', open(os.path.join(csrc, "slice.hip")).read(), flags=re.M))
    assert inc == {"ft_slice.h"} and set(rule_) == {"slice.hip", "ft_slice.h"}             # every header it includes is listed
    assert not re.findall(r'^\s*#include\s+"([^"]+)"', open(os.path.join(csrc, "ft_slice.h")).read(), flags=re.M)
    assert "ft_slice.h" in re.search(r"^capi\.o:(.*)$", mk, flags=re.M).group(1).split()
    assert re.search(r"^\$\(OUT\):.*\bslice\.o\b", mk, flags=re.M)
    for target in ("profile", "experiment"):
        assert "slice.hip" in re.search(r"^%s:.*\n\t(.*)$" % target, mk, flags=re.M).group(1), target
    files = re.search(r"^FILES = \[(.*?)\]", open(os.path.join(csrc, "source_hash.py")).read(), flags=re.M | re.S).group(1)
    assert {"fraytracer_amd/csrc/slice.hip", "fraytracer_amd/csrc/ft_slice.h"} <= set(re.findall(r'"([^"]+)"', files))
    # kernels.hip and what it includes, and the mesher's unit, do not know the slicer
    for f in ("kernels.hip", "ft_kernels.h", "ft_device.h", "ft_math.h", "ft_libm.h", "mesh.hip", "ft_mesh.h"):
        assert "slice" not in open(os.path.join(csrc, f)).read().lower(), f
    # no atomics in the slicer: the order is the rule's
    assert "atomic" not in open(os.path.join(csrc, "slice.hip")).read().replace("No atomics", "")
    assert os.path.exists(os.path.join(ROOT, "profiles", "slice_kernel_resources.txt"))


def test_cpp_slice_mirror_compiles(tmp_path):
    assert_cpp_compiles(tmp_path, "slice.cpp",
                        "FrayTracer::Slice::Contours f(ft_ctx* ctx, const FrayTracer::SdfScene& s, const std::vector<float>& values) {\n"
                        "    FrayTracer::Slice::Request r; r.axis = 1; r.iso = 0.125f; r.normal = true; r.normalEpsilon = 0.00125f; r.material = true;\n"
                        "    ft_lattice l{{0.0f, 0.0f, 0.0f}, {0.1f, 0.1f, 0.1f}, 4, 5, 6};\n"
                        "    FrayTracer::Slice::Contours a = FrayTracer::Slice::ofLattice(s, l, r);\n"
                        "    FrayTracer::Slice::Contours b = FrayTracer::Slice::ofValues(ctx, l, values, 0, 0.5f);\n"
                        "    a.polylines.insert(a.polylines.end(), b.polylines.begin(), b.polylines.end());\n"
                        "    a.skipped += b.skipped; a.closed += b.closed; a.slices += b.polylines.empty() ? 0 : b.polylines[0].slice;\n"
                        "    return a;\n"
                        "}\n")


def test_fsharp_binding_imports_the_slice_forms():
    fs = open(os.path.join(ROOT, "host", "fsharp", "FrayTracer.Hip.fs")).read()
    for name in NAMES:
        assert re.search(r"\[<DllImport\(Lib\)>\] extern (int|void) " + name + r"\(", fs), name
    for name in ("ft_slice_lattice", "ft_slice_values_device", "ft_slice_values"):         # the ft_slices** out-parameter is a plain nativeint
        assert re.search(r"extern int " + name + r"\([^)]*int axis, float32 iso[^)]*, nativeint slices\)", fs), name
    fields = lambda name: [(n, t) for n, t in re.findall(r"(\w+)\s*:\s*([\w.]+)", re.search(r"type\s+" + name + r"\s*=\s*\{(.*?)\}", fs, flags=re.S).group(1))]
    assert fields("FtPolyline") == [("First", "int"), ("Count", "int"), ("Slice", "int"), ("Closed", "int")]
    assert fields("FtSlicesInfo") == [("NPoints", "int64"), ("NPolylines", "int64"), ("NClosed", "int64"), ("NSkipped", "int64"), ("Axis", "int"), ("NSlices", "int"),
                                      ("HasNormal", "int"), ("HasMaterial", "int")]


def test_example_exists_and_parses():
    path = os.path.join(ROOT, "examples", "slice.py")
    compile(open(path).read(), path, "exec")
