"""The rule of ft_slice_lattice / ft_slice_values (include/fraytracer_hip.h "Slicing"), restated in numpy float32 and plain Python: per lattice plane
the two triangles of every cell, one directed segment per crossed triangle, and the segments chained into polylines by walking dictionaries.  It shares
no code and no table with the library: the direction of every segment is worked out here from the integer corner offsets.

    extract(values, origin, step, axis, iso) -> Contours(points float32 [n, 3], polylines int32 [m, 4] (first, count, slice, closed), closed, skipped)

and, for the tests that hold it to the mesher's rule, the pieces: vertex_table, segments."""
import collections
import itertools

import numpy as np

F = np.float32
Contours = collections.namedtuple("Contours", "points polylines closed skipped")


def in_plane_axes(axis):
    return (axis + 1) % 3, (axis + 2) % 3


def unit(axis):
    d = np.zeros(3, np.int64)
    d[axis] = 1
    return d


def edge_number(d):
    """the mesher's e of a direction (di, dj, dk)"""
    return int(4 * d[0] + 2 * d[1] + d[2] - 1)


def plane_edges(axis):
    """the three directions without a component along `axis`: +v, +u, +u+v -> their e"""
    u, v = in_plane_axes(axis)
    return sorted(edge_number(d) for d in (unit(v), unit(u), unit(u) + unit(v)))


# the two triangles of a cell as (du, dv) corner offsets, in the rule's order
TRIANGLES = (((0, 0), (1, 0), (1, 1)), ((0, 0), (0, 1), (1, 1)))


def det2(a, b):
    return a[0] * b[1] - a[1] * b[0]


def directed_segment(corners, inside):
    """one triangle: corners three (du, dv) offsets, inside three booleans -> ((L, M_start), (L, M_end)) as corner positions in `corners`, or None.
    L is the corner that differs from the other two; with u to the right and v up the inside lies to the left."""
    n = sum(inside)
    if n in (0, 3):
        return None
    l = [x for x in range(3) if inside[x] == (n == 1)][0]
    m1, m2 = [x for x in range(3) if x != l]
    L, M1, M2 = (np.asarray(corners[x], np.int64) for x in (l, m1, m2))
    forward = (det2(M2 - M1, L - M1) > 0) == bool(inside[l])
    return ((l, m1), (l, m2)) if forward else ((l, m2), (l, m1))


def vertex_table(s, axis):
    """signed values s [nx, ny, nz] -> index int64 [nx, ny, nz, 7] (the number of the vertex on edge (q, e) in key order, -1 where there is none; only
    the plane's three e can carry one)"""
    nx, ny, nz = s.shape
    inside, finite = s < 0, np.isfinite(s)
    carries = np.zeros((nx, ny, nz, 7), bool)
    u, v = in_plane_axes(axis)
    for d in (unit(v), unit(u), unit(u) + unit(v)):
        di, dj, dk = (int(x) for x in d)
        a = (slice(0, nx - di), slice(0, ny - dj), slice(0, nz - dk))
        b = (slice(di, nx), slice(dj, ny), slice(dk, nz))
        carries[a + (edge_number(d),)] = finite[a] & finite[b] & (inside[a] != inside[b])
    flat = carries.reshape(-1)
    return np.where(flat, np.cumsum(flat, dtype=np.int64) - 1, -1).reshape(nx, ny, nz, 7)


def positions(s, index, origin, step):
    """the mesher's position rule for every vertex of `index`, in key order -> (float32 [nv, 3], owner q, e)"""
    nx, ny, nz = s.shape
    o, st = np.asarray(origin, F).reshape(3), np.asarray(step, F).reshape(3)
    qe = np.flatnonzero(index.reshape(-1) >= 0)
    q, e = qe // 7, qe % 7
    ijk = np.stack(np.unravel_index(q, (nx, ny, nz)), axis=1)
    dirs = np.array([((k + 1) >> 2 & 1, (k + 1) >> 1 & 1, (k + 1) & 1) for k in range(7)], np.int64)
    far = ijk + dirs[e]
    sq, sn = s[tuple(ijk.T)], s[tuple(far.T)]
    out = np.empty((len(qe), 3), F)
    with np.errstate(all="ignore"):
        t = (sq / (sq - sn).astype(F)).astype(F)
        for a in range(3):
            pa = (o[a] + (ijk[:, a].astype(F) * st[a]).astype(F)).astype(F)
            pb = (o[a] + (far[:, a].astype(F) * st[a]).astype(F)).astype(F)
            out[:, a] = (pa + (t * (pb - pa).astype(F)).astype(F)).astype(F)
    return out, q, e


def segments(s, index, axis):
    """-> (start vertex, end vertex) int64 arrays over every segment of every slice, and the number of skipped triangles"""
    nx, ny, nz = s.shape
    inside, finite = s < 0, np.isfinite(s)
    u, v = in_plane_axes(axis)
    cells = [nx, ny, nz]
    cells[u] -= 1
    cells[v] -= 1
    def corner(arr, c):                                                # arr at the cells' corner c = (du, dv)
        lo = c[0] * unit(u) + c[1] * unit(v)
        return arr[tuple(slice(int(lo[x]), int(lo[x]) + cells[x]) for x in range(3))]
    starts, ends, skipped = [], [], 0
    for tri in TRIANGLES:
        ok = np.logical_and.reduce([corner(finite, c) for c in tri])
        skipped += int((~ok).sum())
        ins = [corner(inside, c) for c in tri]
        for pattern in itertools.product((False, True), repeat=3):
            seg = directed_segment(tri, pattern)
            if seg is None:
                continue
            sel = ok & np.logical_and.reduce([ins[x] == pattern[x] for x in range(3)])
            if not sel.any():
                continue
            ids = []
            for x, y in seg:                                           # the edge between corners x and y: owned by the one nearer c0
                lo, hi = sorted((tri[x], tri[y]), key=sum)
                d = (hi[0] - lo[0]) * unit(u) + (hi[1] - lo[1]) * unit(v)
                ids.append(corner(index[..., edge_number(d)], lo)[sel])
            assert (ids[0] >= 0).all() and (ids[1] >= 0).all()
            starts.append(ids[0])
            ends.append(ids[1])
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.int64)
    return cat(starts), cat(ends), skipped


def chain(starts, ends):
    """directed segments -> [(vertex list, closed)] in the rule's order.  Every vertex starts at most one segment and ends at most one."""
    nxt, prv = {}, {}
    for a, b in zip(starts.tolist(), ends.tolist()):
        assert a not in nxt and b not in prv and a != b, (a, b)
        nxt[a] = b
        prv[b] = a
    lines, seen = [], set()
    for head in sorted(v for v in nxt if v not in prv):                # open: from the vertex no segment ends in
        walk = [head]
        while walk[-1] in nxt:
            walk.append(nxt[walk[-1]])
        seen.update(walk)
        lines.append((walk, False))
    for v in sorted(nxt):                                              # closed: from the smallest vertex of the cycle
        if v in seen:
            continue
        walk = [v]
        while nxt[walk[-1]] != v:
            walk.append(nxt[walk[-1]])
        seen.update(walk)
        lines.append((walk, True))
    lines.sort(key=lambda line: line[0][0])
    return lines


def extract(values, origin, step, axis, iso=0.0):
    d = np.ascontiguousarray(values, dtype=F)
    assert d.ndim == 3 and axis in (0, 1, 2)
    u, v = in_plane_axes(axis)
    if d.shape[u] == 1 or d.shape[v] == 1:                             # no cells
        return Contours(np.zeros((0, 3), F), np.zeros((0, 4), np.int32), 0, 0)
    with np.errstate(all="ignore"):
        s = (d - F(iso)).astype(F)
    index = vertex_table(s, axis)
    pos, q, _ = positions(s, index, origin, step)
    starts, ends, skipped = segments(s, index, axis)
    plane = np.stack(np.unravel_index(q, d.shape), axis=1)[:, axis] if len(q) else np.zeros(0, np.int64)
    order, records, first = [], [], 0
    for walk, closed in chain(starts, ends):
        records.append((first, len(walk), int(plane[walk[0]]), int(closed)))
        order.extend(walk)
        first += len(walk)
    assert first < 2 ** 31
    points = pos[np.asarray(order, np.int64)] if order else np.zeros((0, 3), F)
    polylines = np.asarray(records, np.int32).reshape(-1, 4)
    return Contours(np.ascontiguousarray(points, dtype=F), polylines, int(polylines[:, 3].sum()), skipped)


def signed_area(points, axis):
    """twice-halved shoelace area of a closed polyline in its (u, v) plane: positive when counter-clockwise seen from +axis"""
    u, v = in_plane_axes(axis)
    p = np.asarray(points, np.float64)
    x, y = p[:, u], p[:, v]
    return 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))
