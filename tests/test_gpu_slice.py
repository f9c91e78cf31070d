"""Slicing on the GPU (ft_slice_lattice, ft_slice_values, ft_slice_values_device): points, ft_polyline records and the four totals bit for bit against
the restatement of the rule (tests/slice_restatement.py) — every sign pattern of one cell, special values, the lattice shapes that leave tiles and
waves part-filled, further rounds of the scan, every tile, chains one vertex longer than a power of two, loops longer than a tile, hundreds of
polylines, the scene form on the CPU oracle's distances with normals and materials, the glibc arithmetic, the device buffers and the lifetimes."""
import ctypes as C
import itertools

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import _lib
from fraytracer_amd import synthetic as syn
from helpers import assert_bit_equal, glibc_mode, options_left_at_defaults  # noqa: F401  (fixtures)

import mesh_cases as cases
import slice_restatement as rule
from test_gpu_mesh import GuardedBuffer, from_device, guarded_host, hip  # noqa: F401  (hip: fixture)

pytestmark = pytest.mark.gpu

F = np.float32
L = _lib.lib
AXES = (0, 1, 2)
TILE = 512                                 # items per workgroup of the tiled kernels (ft_slice.h FT_SLICE_TILE_DEFAULT)
SCAN_ROUND = 512 * 4                       # tiles per round of the scan kernels (FT_SLICE_SCAN_BLOCK * FT_SLICE_SCAN_ITEMS)
UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def assert_same_contours(got, want, what):
    points, lines = host(got.points), host(got.polylines)
    assert points.dtype == np.float32 and lines.dtype == np.int32, what
    assert points.shape == want.points.shape and lines.shape == want.polylines.shape, (what, points.shape, want.points.shape, lines.shape, want.polylines.shape)
    assert np.array_equal(lines, want.polylines), what + ": polylines"
    assert np.array_equal(points.view(np.uint32), want.points.view(np.uint32)), what + ": points"
    assert (got.closed, got.skipped) == (want.closed, want.skipped), (what, got.closed, want.closed, got.skipped, want.skipped)
    assert got.closed == int(lines[:, 3].sum()) and len(points) == int(lines[:, 1].sum())


def check_values(gpu, values, axis, origin=UNIT[0], step=UNIT[1], iso=0.0, what=""):
    got = gpu.slice_values(values, origin, step, axis, iso)
    want = rule.extract(values, origin, step, axis, iso)
    assert_same_contours(got, want, f"{what} axis {axis}")
    assert got.normal is None and got.material is None and got.axis == axis and got.slices == np.shape(values)[axis]
    return want


def plane_shape(axis, n_axis, n_u, n_v):
    shape = [0, 0, 0]
    shape[axis], shape[(axis + 1) % 3], shape[(axis + 2) % 3] = n_axis, n_u, n_v
    return tuple(shape)


def planar(axis, fn, n_u, n_v, n_axis=1):
    """fn(U, V) of the in-plane indices, the same in each of n_axis planes -> float32 values in (i, j, k) order"""
    U, V = np.meshgrid(np.arange(n_u, dtype=F), np.arange(n_v, dtype=F), indexing="ij")
    u, v = rule.in_plane_axes(axis)
    plane = np.asarray(fn(U, V), F)
    out = np.empty(plane_shape(axis, n_axis, n_u, n_v), F)
    src = plane if u < v else plane.T
    out[...] = np.expand_dims(src, axis)
    return out


@pytest.mark.parametrize("axis", AXES)
def test_every_sign_pattern_of_one_cell(gpu, axis):
    """16 slices of 2 x 2 points: slice w has the sign pattern w"""
    rng = np.random.default_rng(70 + axis)
    u, v = rule.in_plane_axes(axis)
    d = rng.uniform(0.05, 2.0, plane_shape(axis, 16, 2, 2)).astype(F)
    for w, pattern in enumerate(itertools.product((False, True), repeat=4)):
        for c, inside in enumerate(pattern):
            idx = [0, 0, 0]
            idx[axis], idx[u], idx[v] = w, c >> 1, c & 1
            if inside:
                d[tuple(idx)] *= F(-1.0)
    want = check_values(gpu, d, axis, (0.25, -1.5, 3.0), (0.5, 0.75, 1.25), what="patterns")
    assert int((want.polylines[:, 1] - 1).sum()) == 2 * 6 * 2 and sorted(set(want.polylines[:, 2].tolist())) == list(range(1, 15))


SPECIALS = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, np.inf, -np.inf, np.nan, 3.0e38, -3.0e38, 1.0, -1.0, 0.5, -0.5], F)


@pytest.mark.parametrize("iso", [0.0, 0.5, -1e-40])                                       # -1e-40: d - iso of a denormal d is a denormal, or rounds to 0
def test_special_values(gpu, iso):
    rng = np.random.default_rng(13)
    skipped = points = opened = 0
    for axis in AXES:
        for shape in ((2, 2, 2), (3, 3, 3), (4, 3, 5), (6, 7, 5)):
            for _ in range(6):
                d = rng.standard_normal(shape).astype(F)
                where = rng.random(shape) < 0.4
                d[where] = rng.choice(SPECIALS, int(where.sum()))
                d[rng.random(shape) < 0.1] = F(iso)                                        # values of exactly iso
                want = check_values(gpu, d, axis, (-1.0, 0.5, 2.0), (0.3, -0.2, 0.0), iso, f"iso {iso} {shape}")      # a negative and a zero step as well
                skipped, points, opened = skipped + want.skipped, points + len(want.points), opened + len(want.polylines) - want.closed
        whole = np.full((3, 3, 3), np.nan, F)
        assert check_values(gpu, whole, axis, iso=iso).skipped == 3 * 4 * 2                # nothing but NaN: every triangle skipped, no point
    assert skipped > 100 and points > 100 and opened > 50                                  # the inputs did reach the rules


@pytest.mark.parametrize("axis", AXES)
@pytest.mark.parametrize("shape", ["counts", "one slice", "no cells u", "no cells v", "2 x 2", "3 x 65", "65 x 2", "65 x 65"])
def test_lattice_shapes(gpu, axis, shape):
    dims = {"counts": cases.COUNTS, "one slice": plane_shape(axis, 1, 9, 11), "no cells u": plane_shape(axis, 5, 1, 7), "no cells v": plane_shape(axis, 4, 6, 1),
            "2 x 2": plane_shape(axis, 3, 2, 2), "3 x 65": plane_shape(axis, 2, 3, 65), "65 x 2": plane_shape(axis, 2, 65, 2), "65 x 65": plane_shape(axis, 2, 65, 65)}[shape]
    d = np.random.default_rng(sum(dims) + axis).standard_normal(dims).astype(F)
    want = check_values(gpu, d, axis, (0.1, 0.2, 0.3), (0.01, 0.02, 0.03), what=shape)
    assert (len(want.polylines) > 0) == (not shape.startswith("no cells"))
    check_values(gpu, d, axis, (0.1, 0.2, 0.3), (0.01, 0.02, 0.03), 0.75, shape + " iso 0.75")


def set_tile(gpu, tile):
    fn = L.ft_ctx_slice_tile                                                               # internal: not in the header
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int32]
    assert fn(gpu._ctx, tile) == 0


def test_tiles_cross_the_rounds_of_the_scan(gpu):
    """2 x 513 x 513 = 526 338 points are 4 113 tiles of 128: the scan's single workgroup takes 512 x 4 = 2 048 tile sums per round, so the sums cross a
    thread's four items, a wave's 64 threads, the workgroup's 8 waves and the carries into a second and a third round.  Two bands with wavy rims around j = 8.5 and j = 510.5 with
    nothing in between: empty tiles between busy ones, busy ones in both rounds, and open chains that run from border to border across hundreds of
    tiles."""
    shape = (2, 513, 513)
    j = np.arange(shape[1], dtype=F)[None, :, None]
    rng = np.random.default_rng(3)
    d = (np.minimum(np.abs(j - F(8.5)), np.abs(j - F(510.5))) - F(1.2) + rng.uniform(-0.2, 0.2, shape).astype(F)).astype(F)
    assert -(-d.size // 128) > 2 * SCAN_ROUND and ((513 + 510) * 513) // 128 >= 2 * SCAN_ROUND      # the second band of slice 1 lies in the third round
    try:
        set_tile(gpu, 128)
        want = check_values(gpu, d, 0, what="scan rounds")
    finally:
        set_tile(gpu, TILE)
    assert len(want.points) > 4000 and want.closed == 0 and len(want.polylines) == 8 and (want.polylines[:, 1] > 513).all()
    starts = want.polylines[:, 0]
    assert (np.diff(starts) > 0).all()


@pytest.mark.parametrize("axis", AXES)
def test_every_tile_gives_the_same_contours(gpu, axis):
    d = np.random.default_rng(5).standard_normal((21, 18, 23)).astype(F)
    d[4, 5, 6], d[10, 10, 10] = np.nan, np.inf
    want = rule.extract(d, *UNIT, axis)
    try:
        for t in (128, 256, 1024, 512):
            set_tile(gpu, t)
            assert_same_contours(gpu.slice_values(d, *UNIT, axis), want, f"tile {t}")
    finally:
        set_tile(gpu, TILE)


def test_empty_results(gpu):
    d = np.full((9, 10, 11), 0.5, F)
    for axis in AXES:
        for values in (d, -d):                                                             # all outside, all inside: nothing crosses
            got = gpu.slice_values(values, *UNIT, axis)
            assert got.points.shape == (0, 3) and got.polylines.shape == (0, 4) and got.polylines.dtype == np.int32 and (got.closed, got.skipped) == (0, 0)
    # vertices but no segment: one finite inside point among NaN
    lone = np.full((1, 3, 3), np.nan, F)
    lone[0, 1, 1], lone[0, 1, 2] = -1.0, 1.0
    want = check_values(gpu, lone, 0, what="a vertex no segment uses")
    assert len(want.points) == 0 and want.skipped == 8
    ds = gpu.scene(cases.scene_of("c3_64"))
    far = ds.slice_lattice((100.0, 100.0, 100.0), (0.1, 0.1, 0.1), (5, 6, 7), axis=2, normal_epsilon=cases.NORMAL_EPS, material=True)
    assert far.points.shape == (0, 3) and far.normal.shape == (0, 3) and far.material.shape == (0,) and far.skipped == 2 * 4 * 5 * 7      # +inf there


# ---- the jump rounds ---------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [33, 513, 2049])
def test_one_open_chain_of_a_power_of_two_plus_one_vertices(gpu, n):
    """d = u - 0.5 on 1 x 2 x n (axis 0): every cell's +u edges and its diagonal are crossed, one chain of 2 n - 1 = 2^m + 1 vertices from border to
    border, one vertex more than the rounds before the last can cover, across tiles"""
    d = np.empty((1, 2, n), F)
    d[0, 0], d[0, 1] = -0.5, 0.5
    want = check_values(gpu, d, 0, (1.0, 2.0, 3.0), (1.0, 0.5, 0.25), what=f"chain {n}")
    assert want.polylines.tolist() == [[0, 2 * n - 1, 0, 0]] and ((2 * n - 2) & (2 * n - 3)) == 0
    # the same chain in the other direction, and as the last slice of two
    check_values(gpu, -d, 0, what=f"chain {n} reversed")
    check_values(gpu, np.concatenate([np.ones_like(d), d]), 0, what=f"chain {n} in slice 1")


@pytest.mark.parametrize("axis", AXES)
def test_one_loop_longer_than_a_tile(gpu, axis):
    d = planar(axis, lambda U, V: np.sqrt((U - F(79.3)) ** 2 + (V - F(80.1)) ** 2) - F(70.4), 160, 160)
    want = check_values(gpu, d, axis, what="disc")
    assert want.polylines.shape == (1, 4) and want.closed == 1 and want.polylines[0, 1] > TILE
    assert rule.signed_area(want.points, axis) > 0.0


# ---- many polylines ----------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("axis", AXES)
def test_concentric_rings(gpu, axis):
    rings = lambda U, V: np.cos(F(2.0 * np.pi / 9.0) * np.sqrt((U - F(47.6)) ** 2 + (V - F(48.2)) ** 2))
    want = check_values(gpu, planar(axis, rings, 97, 97, n_axis=2), axis, what="rings")
    loops = [(rule.signed_area(want.points[f:f + n], axis), w) for f, n, w, closed in want.polylines.tolist() if closed]
    in_first = sorted(a for a, w in loops if w == 0)
    assert len(in_first) >= 8 and sum(a < 0 for a in in_first) >= 4 and sum(a > 0 for a in in_first) >= 4      # nested loops of alternating direction
    assert len(want.polylines) > want.closed > 0                                           # and arcs cut by the border


@pytest.mark.parametrize("axis", AXES)
def test_hundreds_of_six_point_loops(gpu, axis):
    dots = lambda U, V: np.where((U % 3 == 1) & (V % 3 == 1), F(-0.3), F(0.6))
    want = check_values(gpu, planar(axis, dots, 100, 100, n_axis=3), axis, (0.5, 0.25, 0.125), (0.1, 0.2, 0.3), what="dots")
    assert want.polylines.shape == (3 * 33 * 33, 4) and (want.polylines[:, 1] == 6).all() and want.closed == len(want.polylines)
    assert len(want.points) > 8 * 1024                                                     # the polylines' first points lie in many tiles of vertices


@pytest.mark.parametrize("axis", AXES)
def test_stripes_end_on_the_border(gpu, axis):
    stripes = lambda U, V: np.sin(F(0.7) * U + F(0.002) * V + F(0.3))
    want = check_values(gpu, planar(axis, stripes, 90, 70, n_axis=2), axis, what="stripes")
    assert want.closed == 0 and len(want.polylines) >= 2 * 15 and (want.polylines[:, 1] >= 70).all()


# ---- the scene form ----------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("axis", AXES)
@pytest.mark.parametrize("name", list(cases.SCENES))
def test_scene_form_matches_the_restatement_on_the_oracle_distances(gpu, oracle, name, axis):
    origin, step, d = cases.oracle_lattice(oracle, name)
    want = rule.extract(d, origin, step, axis)
    assert len(want.points) >= 100 and want.closed >= 5
    ds = gpu.scene(cases.scene_of(name))
    got = ds.slice_lattice(origin, step, cases.COUNTS, axis=axis, normal_epsilon=cases.NORMAL_EPS, material=True)
    assert_same_contours(got, want, name)
    assert got.normal.shape == want.points.shape and got.material.shape == (len(want.points),) and got.material.dtype == np.int32
    # exactly what sample_points gives for those points
    pts = ds.sample_points(got.points, normal_epsilon=cases.NORMAL_EPS, material=True)
    assert_bit_equal(got.normal, pts.normal, name + ": normal against sample_points")
    assert np.array_equal(got.material, pts.material) and (got.material >= 0).all()
    assert got.descriptor(got.material[0]) is not None
    # without the flags: the same contours, nothing else; another level; the values form on the lattice's distances
    plain = ds.slice_lattice(origin, step, cases.COUNTS, axis=axis)
    assert_same_contours(plain, want, name + " without flags")
    assert plain.normal is None and plain.material is None
    only_material = ds.slice_lattice(origin, step, cases.COUNTS, axis=axis, material=True)
    assert only_material.normal is None and np.array_equal(only_material.material, got.material)
    assert_same_contours(ds.slice_lattice(origin, step, cases.COUNTS, axis=axis, iso=0.03), rule.extract(d, origin, step, axis, 0.03), name + " iso 0.03")
    assert_same_contours(gpu.slice_values(ds.sample_lattice(origin, step, cases.COUNTS).distance, origin, step, axis), want, name + " values form")
    # layer(w): the records of slice w, in order
    w = int(want.polylines[len(want.polylines) // 2, 2])
    layer = got.layer(w)
    rows = [r for r in want.polylines.tolist() if r[2] == w]
    assert len(layer) == len(rows) and all(np.array_equal(p, want.points[f:f + n]) and c == bool(cl) for (p, c), (f, n, _, cl) in zip(layer, rows))


def test_scene_form_under_the_glibc_arithmetic(gpu, oracle, glibc_mode):
    origin, step, d = cases.oracle_lattice(oracle, "c3_64", libm=True)                     # formed under the oracle's libm switch (glibc_mode holds it)
    ds = gpu.scene(cases.scene_of("c3_64"))
    for axis in AXES:
        got = ds.slice_lattice(origin, step, cases.COUNTS, axis=axis, normal_epsilon=cases.NORMAL_EPS)
        assert_same_contours(got, rule.extract(d, origin, step, axis), "glibc")
        assert_bit_equal(got.normal, ds.sample_points(got.points, normal_epsilon=cases.NORMAL_EPS).normal, "glibc: normal")


def test_sdf_form_slice(gpu, oracle):
    origin, step, d = cases.oracle_lattice(oracle, "c3_64")
    form = cases.scene_of("c3_64").Object.kids[1]
    got = ft.SdfForm.slice(form, origin, step, cases.COUNTS, axis=1, device=gpu)
    assert_same_contours(got, rule.extract(d, origin, step, 1), "SdfForm.slice")


# ---- device buffers and lifetimes --------------------------------------------------------------------------------------------------------------


def read_slices(handle, normals=False, materials=False):
    info = _lib.SlicesInfo()
    assert L.ft_slices_get_info(handle, C.byref(info)) == 0
    n, m = info.n_points, info.n_polylines
    parts = [guarded_host((n, 3), np.float32), guarded_host((m, 4), np.int32), guarded_host((n, 3), np.float32) if normals else None,
             guarded_host((n,), np.int32) if materials else None]
    ptrs = [None if p is None else p[0].ctypes.data_as(C.c_void_p) for p in parts]
    assert L.ft_slices_read(handle, *ptrs) == 0
    assert all(p is None or p[1]() for p in parts)                                         # the guard words around the caller's buffers
    return info, [None if p is None else p[0] for p in parts]


def same_parts(parts, want):
    return np.array_equal(parts[0].view(np.uint32), want.points.view(np.uint32)) and np.array_equal(parts[1], want.polylines)


@pytest.mark.parametrize("name,axis", [("c3_64", 2), ("console_200", 1)])
def test_device_buffers_and_the_values_device_form(gpu, oracle, hip, name, axis):
    origin, step, d = cases.oracle_lattice(oracle, name)
    want = rule.extract(d, origin, step, axis)
    ds = gpu.scene(cases.scene_of(name))
    lat, _ = ft.api._lattice(origin, step, cases.COUNTS)
    kept = GuardedBuffer(hip, int(np.prod(cases.COUNTS)))
    a, b = C.c_void_p(), C.c_void_p()
    try:
        ds.sample_lattice_device(origin, step, cases.COUNTS, kept.ptr)                     # a lattice kept on the device, sliced where it lies
        assert L.ft_slice_values_device(gpu._ctx, C.byref(lat), C.c_void_p(kept.ptr), axis, 0.0, C.byref(a)) == 0
        assert L.ft_slice_lattice(gpu._ctx, ds._scene, C.byref(lat), axis, 0.0, cases.NORMAL_EPS, 3, C.byref(b)) == 0
        values, intact = kept.read(np.float32)
        assert intact and np.array_equal(values.view(np.uint32), d.reshape(-1).view(np.uint32))        # the input lattice is unchanged, its guards too
        (ia, pa), (ib, pb) = read_slices(a), read_slices(b, True, True)
        totals = (len(want.points), len(want.polylines), want.closed, want.skipped, axis, cases.COUNTS[axis])
        assert (ia.n_points, ia.n_polylines, ia.n_closed, ia.n_skipped, ia.axis, ia.n_slices, ia.has_normal, ia.has_material) == totals + (0, 0)
        assert (ib.n_points, ib.n_polylines, ib.n_closed, ib.n_skipped, ib.axis, ib.n_slices, ib.has_normal, ib.has_material) == totals + (1, 1)
        assert same_parts(pa, want) and same_parts(pb, want)
        assert L.ft_slices_read(a, None, None, pb[2].ctypes.data_as(C.c_void_p), None) == _lib.FT_ERR_INVALID         # built without normals
        # ft_slices_device_buffers = ft_slices_read
        bufs = [C.c_void_p() for _ in range(4)]
        assert L.ft_slices_device_buffers(b, *map(C.byref, bufs)) == 0 and all(p.value and p.value % 4 == 0 for p in bufs)
        n, m = ib.n_points, ib.n_polylines
        for p, shape, dtype, got in zip(bufs, ((n, 3), (m, 4), (n, 3), (n,)), (np.float32, np.int32, np.float32, np.int32), pb):
            assert np.array_equal(from_device(hip, p.value, shape, dtype).view(np.uint32), got.view(np.uint32))
        bufs_a = [C.c_void_p(1) for _ in range(4)]
        assert L.ft_slices_device_buffers(a, *map(C.byref, bufs_a)) == 0 and bufs_a[0].value and bufs_a[1].value and not bufs_a[2].value and not bufs_a[3].value
        _, only_lines = read_slices(b)                                                     # parts of a read: any may be NULL
        assert np.array_equal(only_lines[1], want.polylines)
        assert L.ft_slices_read(b, None, None, None, None) == 0
    finally:
        L.ft_slices_destroy(a)
        L.ft_slices_destroy(b)
        kept.free()


def test_two_results_alive_at_once_destroyed_in_either_order(gpu):
    rng = np.random.default_rng(9)
    fields = [rng.standard_normal(shape).astype(F) for shape in ((6, 7, 8), (9, 5, 4))]
    wants = [rule.extract(d, *UNIT, 2) for d in fields]
    for order in ((0, 1), (1, 0)):
        handles = []
        for d in fields:
            lat, _ = ft.api._lattice(*UNIT, d.shape)
            h = C.c_void_p()
            assert L.ft_slice_values(gpu._ctx, C.byref(lat), d.ctypes.data_as(C.c_void_p), 2, 0.0, C.byref(h)) == 0
            handles.append(h)
        assert handles[0].value != handles[1].value
        first, second = order
        assert same_parts(read_slices(handles[first])[1], wants[first]) and same_parts(read_slices(handles[second])[1], wants[second])      # each is whole while the other lives ...
        L.ft_slices_destroy(handles[first])
        assert same_parts(read_slices(handles[second])[1], wants[second])                  # ... and after it is gone
        L.ft_slices_destroy(handles[second])
    # a result outlives its scene
    dev = ft.Device(0)
    try:
        ds = dev.scene(cases.scene_of("c3_64"))
        origin, step = cases.lattice_around(ds.boundary(), cases.SPAN, cases.COUNTS)
        lat, _ = ft.api._lattice(origin, step, cases.COUNTS)
        whole = ds.slice_lattice(origin, step, cases.COUNTS, axis=0)
        h = C.c_void_p()
        assert L.ft_slice_lattice(dev._ctx, ds._scene, C.byref(lat), 0, 0.0, 0.0, 0, C.byref(h)) == 0
        ds.close()
        _, parts = read_slices(h)
        assert len(parts[0]) > 0 and np.array_equal(parts[0].view(np.uint32), whole.points.view(np.uint32)) and np.array_equal(parts[1], whole.polylines)
        L.ft_slices_destroy(h)
    finally:
        dev.close()


def test_the_launches_event_pairs_are_collected_by_the_next_stats_call(hip):
    """a slice returns no statistics and collects none: a frame launched before it and not yet collected is still there, whole, in the next
    collect_stats — every counter of the same frame collected on its own, and a kernel time to which the slicer's launches have added theirs"""
    counters = ("rays_primary", "rays_shadow", "rays_ext", "hits_primary", "hits_shadow", "sdf_evals", "wave_evals", "flags")

    def frame_stats(slice_between):
        dev = ft.Device(0)
        frame = C.c_void_p()
        assert hip.hipMalloc(C.byref(frame), C.c_size_t(16 * 16 * 12)) == 0
        try:
            ds = dev.scene(syn.config3(n=8)[0])
            ds.render_device(syn.EPSILON, syn.RAY_LENGTH, ft.ImageSize(16, 16), syn.default_camera(), frame.value)
            if slice_between:
                origin, step = cases.lattice_around(ds.boundary(), 1.0, (20, 21, 22))
                got = ds.slice_lattice(origin, step, (20, 21, 22), axis=2, normal_epsilon=cases.NORMAL_EPS)
                assert len(got.polylines) > 0 and got.normal.shape == got.points.shape         # every kernel of the slicer and both field launches ran
            return ds.collect_stats()
        finally:
            dev.close()
            assert hip.hipFree(frame) == 0

    alone, after = frame_stats(False), frame_stats(True)
    assert alone["rays_primary"] == 256 and alone["kernel_ms"] > 0.0
    assert {k: after[k] for k in counters} == {k: alone[k] for k in counters}
    assert after["kernel_ms"] > 0.0


TENSOR_PATH = r"""
import json, sys
import numpy as np
import torch                              # before the library: torch's HIP runtime is the one the process loads first
import fraytracer_amd as ft
sys.path.insert(0, "tests")
import mesh_cases as cases
import slice_restatement as rule
same = lambda t, a: bool(np.array_equal(np.ascontiguousarray(t.detach().cpu().numpy()).view(np.uint32), np.ascontiguousarray(a).view(np.uint32)))
dev = ft.Device(0)
d = np.random.default_rng(2).standard_normal((21, 18, 23)).astype(np.float32)
want = rule.extract(d, (0, 0, 0), (1, 1, 1), 1, 0.25)
r = {}
side = torch.cuda.Stream()                # on a side stream, behind the torch kernel that makes the values: the stream hand-over
side.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(side):
    t = torch.from_numpy(d).cuda() * 1.0
    m = dev.slice_values(t, (0, 0, 0), (1, 1, 1), 1, 0.25)
side.synchronize()
r["tensors"] = m.points.is_cuda and m.polylines.is_cuda and m.polylines.dtype == torch.int32 and m.normal is None
r["values: points"], r["values: polylines"] = same(m.points, want.points), same(m.polylines, want.polylines)
r["values: totals"] = (m.closed, m.skipped) == (want.closed, want.skipped)
r["input unchanged"] = same(t, d)
ds = dev.scene(cases.scene_of("c3_64"))
origin, step = cases.lattice_around(ds.boundary(), cases.SPAN, cases.COUNTS)
host = ds.slice_lattice(origin, step, cases.COUNTS, axis=0, normal_epsilon=cases.NORMAL_EPS, material=True)
like = ds.slice_lattice(origin, step, cases.COUNTS, axis=0, normal_epsilon=cases.NORMAL_EPS, material=True, like=t)      # torch's default stream: the side-stream path
torch.cuda.synchronize()
r["like"] = like.points.is_cuda and same(like.points, host.points) and same(like.polylines, host.polylines) and same(like.normal, host.normal) and same(like.material, host.material)
r["like: layer"] = len(like.layer(10)) == len(host.layer(10)) > 0
for bad, why in ((t.double(), "float32"), (t[::2], "contiguous")):
    try:
        dev.slice_values(bad, (0, 0, 0), (1, 1, 1))
        r["refuses " + why] = False
    except ValueError as e:
        r["refuses " + why] = why in str(e)
dev.close()
print(json.dumps(r))
"""


def test_tensor_path_in_a_process_that_loads_torch_first():
    """device tensors in, device tensors out, on the caller's stream: in a child process that loads torch before the library"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", TENSOR_PATH], cwd=root, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    failed = [k for k, v in r.items() if v is not True]
    assert not failed, failed
