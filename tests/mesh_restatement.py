"""The extraction rule of ft_mesh_lattice / ft_mesh_values (include/fraytracer_hip.h "Meshing"), restated in numpy float32: marching tetrahedra
on the Kuhn subdivision of every lattice cell.  It shares no code and no table with the library: the orientation of every triangle is worked
out here from the integer corner offsets, and a triangle is rotated by the vertex indices it actually got.

    extract(values, origin, step, iso) -> Mesh(vertices float32 [nv, 3], triangles int32 [nt, 3], skipped)

and what the tests ask of a mesh: directed_edge_counts, is_closed, euler_characteristic, signed_volume."""
import collections
import itertools

import numpy as np

F = np.float32
# edge direction e = 4 di + 2 dj + dk - 1
DIRS = tuple(((e + 1) >> 2 & 1, (e + 1) >> 1 & 1, (e + 1) & 1) for e in range(7))
# one tetrahedron per permutation of the axes, in lexicographic order: c0 = (0, 0, 0), c1 = c0 + unit(p[0]), c2 = c1 + unit(p[1]), c3 = (1, 1, 1)
PERMS = tuple(itertools.permutations(range(3)))

Mesh = collections.namedtuple("Mesh", "vertices triangles skipped")


def tetrahedron_corners(perm):
    c = [np.zeros(3, np.int64)]
    for axis in perm:
        nxt = c[-1].copy()
        nxt[axis] += 1
        c.append(nxt)
    return c


def det3(a, b, c):
    return int(np.dot(a, np.cross(b, c)))


def oriented_cycle(corners, inside):
    """the crossing edges of one tetrahedron as a cycle of corner pairs (x, y), x before y in corner order, counter-clockwise seen from the
    outside; decided on the integer corner offsets alone.  inside: four booleans.  Three pairs, four for a quad, none where nothing crosses."""
    A = [x for x in range(4) if inside[x]]
    B = [x for x in range(4) if not inside[x]]
    pair = lambda x, y: (min(x, y), max(x, y))
    if len(A) in (0, 4):
        return []
    if len(A) == 1:
        a = corners[A[0]]
        # a vertex on edge (a, b) is a + t (b - a) with t > 0: the triangle's normal n satisfies n . (v1 - a) = t1 t2 t3 det[b1 - a, b2 - a, b3 - a],
        # and it must point away from the inside corner
        cyc = [pair(A[0], b) for b in B]
        if det3(*(corners[b] - a for b in B)) < 0:
            cyc = [cyc[0], cyc[2], cyc[1]]
        return cyc
    if len(A) == 3:
        b = corners[B[0]]
        cyc = [pair(a, B[0]) for a in A]
        if det3(*(corners[a] - b for a in A)) > 0:                     # towards the outside corner: n . (v1 - b) < 0
            cyc = [cyc[0], cyc[2], cyc[1]]
        return cyc
    a1, a2, b1, b2 = A[0], A[1], B[0], B[1]
    cyc = [pair(a1, b1), pair(a1, b2), pair(a2, b2), pair(a2, b1)]
    # with every vertex at its edge's midpoint the quad is a parallelogram with normal (b2 - b1) x (a2 - a1) (for the cycle as written); it must
    # point from the inside corners to the outside ones
    out = (corners[b1] + corners[b2]) - (corners[a1] + corners[a2])
    if det3(corners[b2] - corners[b1], corners[a2] - corners[a1], out) < 0:
        cyc = cyc[::-1]
    return cyc


def rotate_smallest_first(rows):
    """every row of an integer array rotated so that its smallest entry comes first"""
    n, w = rows.shape
    r = np.argmin(rows, axis=1)
    return rows[np.arange(n)[:, None], (r[:, None] + np.arange(w)[None, :]) % w]


def extract(values, origin, step, iso=0.0):
    d = np.ascontiguousarray(values, dtype=F)
    assert d.ndim == 3
    nx, ny, nz = d.shape
    o, st = np.asarray(origin, F).reshape(3), np.asarray(step, F).reshape(3)
    if min(nx, ny, nz) == 1:                                           # no cells: an empty mesh
        return Mesh(np.zeros((0, 3), F), np.zeros((0, 3), np.int32), 0)
    with np.errstate(all="ignore"):
        s = (d - F(iso)).astype(F)
    inside, finite = s < 0, np.isfinite(s)                            # +0, -0 and NaN are not inside
    # ---- vertices: edge (q, e) carries one iff both ends are finite and exactly one is inside; numbered by (q, e)
    carries = np.zeros((nx, ny, nz, 7), bool)
    for e, (di, dj, dk) in enumerate(DIRS):
        a = (slice(0, nx - di), slice(0, ny - dj), slice(0, nz - dk))
        b = (slice(di, nx), slice(dj, ny), slice(dk, nz))
        carries[a + (e,)] = finite[a] & finite[b] & (inside[a] != inside[b])
    flat = carries.reshape(-1)
    index = np.where(flat, np.cumsum(flat, dtype=np.int64) - 1, -1).reshape(nx, ny, nz, 7)
    qe = np.flatnonzero(flat)
    q, e = qe // 7, qe % 7
    ijk = np.stack(np.unravel_index(q, (nx, ny, nz)), axis=1)
    far = ijk + np.asarray(DIRS, np.int64)[e]
    sq, sn = s[tuple(ijk.T)], s[tuple(far.T)]
    vertices = np.empty((len(qe), 3), F)
    with np.errstate(all="ignore"):
        t = (sq / (sq - sn).astype(F)).astype(F)                       # one true division; always from the owner towards the far end
        for a in range(3):
            pa = (o[a] + (ijk[:, a].astype(F) * st[a]).astype(F)).astype(F)
            pb = (o[a] + (far[:, a].astype(F) * st[a]).astype(F)).astype(F)
            vertices[:, a] = (pa + (t * (pb - pa).astype(F)).astype(F)).astype(F)
    # ---- triangles: per cell, per tetrahedron
    cx, cy, cz = nx - 1, ny - 1, nz - 1
    cell = (np.arange(cx)[:, None, None] * ny + np.arange(cy)[None, :, None]) * nz + np.arange(cz)[None, None, :]     # in the points' indexing
    corner = lambda arr, c: arr[c[0]:c[0] + cx, c[1]:c[1] + cy, c[2]:c[2] + cz]
    rows, skipped = [], 0
    for tet, perm in enumerate(PERMS):
        C = tetrahedron_corners(perm)
        ok = np.logical_and.reduce([corner(finite, c) for c in C])
        skipped += int((~ok).sum())
        ins = [corner(inside, c) for c in C]
        for pattern in itertools.product((False, True), repeat=4):
            cyc = oriented_cycle(C, pattern)
            if not cyc:
                continue
            sel = ok & np.logical_and.reduce([ins[x] == pattern[x] for x in range(4)])
            if not sel.any():
                continue
            ids = []
            for x, y in cyc:                                           # edge (C[x], C[y]): owned by C[x], direction C[y] - C[x]
                dv = C[y] - C[x]
                edge = 4 * dv[0] + 2 * dv[1] + dv[2] - 1
                ids.append(corner(index[..., edge], C[x])[sel])
            poly = rotate_smallest_first(np.stack(ids, axis=1))
            assert (poly >= 0).all()
            cells = cell[sel]
            if len(cyc) == 3:
                rows.append(np.column_stack([cells, np.full(len(cells), tet), np.zeros(len(cells), np.int64), poly]))
            else:
                for sub, tri in enumerate((poly[:, [0, 1, 2]], poly[:, [0, 2, 3]])):
                    rows.append(np.column_stack([cells, np.full(len(cells), tet), np.full(len(cells), sub), tri]))
    if rows:
        allrows = np.concatenate(rows)
        allrows = allrows[np.lexsort((allrows[:, 2], allrows[:, 1], allrows[:, 0]))]
        triangles = allrows[:, 3:6]
    else:
        triangles = np.zeros((0, 3), np.int64)
    assert len(vertices) < 2 ** 31 and len(triangles) < 2 ** 31
    return Mesh(vertices, np.ascontiguousarray(triangles, dtype=np.int32), skipped)


# ---- what a closed, consistently oriented surface is ------------------------------------------------------------------------------------------


def directed_edge_counts(triangles):
    t = np.asarray(triangles, np.int64)
    return collections.Counter(map(tuple, np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]).tolist()))


def is_closed(triangles):
    """every directed edge occurs once, and its reverse once"""
    cnt = directed_edge_counts(triangles)
    return all(n == 1 and cnt.get((b, a), 0) == 1 for (a, b), n in cnt.items())


def euler_characteristic(mesh):
    t = np.asarray(mesh.triangles, np.int64)
    used = np.unique(t)
    und = np.unique(np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1), axis=0)
    return len(used) - len(und) + len(t)


def signed_volume(mesh):
    v = np.asarray(mesh.vertices, np.float64)[np.asarray(mesh.triangles, np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)
