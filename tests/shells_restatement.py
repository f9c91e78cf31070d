"""The rule of ft_mesh_shells / ft_shells_triangles / ft_mesh_select (include/fraytracer_hip.h "Shells"), restated from its text in plain Python: a
union-find over the triangles' sides, border edges through a set of directed sides, the selection by boolean masks and cumsum.  It shares no code
with the library and is no round-based propagation.

    shells(triangles, n_vertices) -> Shells(vertex_shell int32 [nV], triangle_shell int32 [nT], records int32 [S, 4], info dict)
    select(vertices, triangles, sh, keep, normal=None, material=None) -> (vertices, triangles, normal, material, new index per old vertex)"""
import collections

import numpy as np

Shells = collections.namedtuple("Shells", "vertex_shell triangle_shell records info")


def shells(triangles, n_vertices):
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    nV, nT = int(n_vertices), len(tri)
    assert nT == 0 or (tri.min() >= 0 and tri.max() < nV)
    assert ((tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])).all()
    rows = tri.tolist()
    parent = list(range(nV))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    used = [False] * nV
    for a, b, c in rows:
        used[a] = used[b] = used[c] = True
        for x, y in ((a, b), (b, c), (c, a)):                         # the triangles' sides are the graph's edges
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
    # numbering: ascending order of the smallest vertex index; vertices are visited in ascending order, so a shell is met first at its smallest
    number, vertex_shell, first = {}, np.full(nV, -1, np.int32), []
    for v in range(nV):
        if not used[v]:
            continue
        r = find(v)
        if r not in number:
            number[r] = len(number)
            first.append(v)
        vertex_shell[v] = number[r]
    S = len(number)
    triangle_shell = vertex_shell[tri[:, 0]].astype(np.int32) if nT else np.zeros(0, np.int32)
    sides = set()
    for a, b, c in rows:
        sides.update(((a, b), (b, c), (c, a)))
    records = np.zeros((S, 4), np.int32)
    records[:, 0] = first
    records[:, 1] = np.bincount(vertex_shell[vertex_shell >= 0], minlength=S)
    records[:, 2] = np.bincount(triangle_shell, minlength=S)
    for (a, b, c), s in zip(rows, triangle_shell.tolist()):
        for x, y in ((a, b), (b, c), (c, a)):                         # each side judged on its own: a border edge iff no triangle has y -> x
            if (y, x) not in sides:
                records[s, 3] += 1
    info = {"n_vertices": nV, "n_triangles": nT, "n_shells": S, "n_closed": int((records[:, 3] == 0).sum()), "n_unused_vertices": int(nV - sum(used)),
            "n_border_edges": int(records[:, 3].sum())}
    return Shells(vertex_shell, triangle_shell, records, info)


def euler(records):
    """V - (3F + B) // 2 + F per shell: valid where no directed side occurs twice"""
    r = np.asarray(records, np.int64).reshape(-1, 4)
    return r[:, 1] - (3 * r[:, 2] + r[:, 3]) // 2 + r[:, 2]


def largest(records, k):
    """bool [S]: the k shells with the most triangles, ties going to the lower number"""
    r = np.asarray(records, np.int64).reshape(-1, 4)
    order = sorted(range(len(r)), key=lambda s: (-int(r[s, 2]), s))
    keep = np.zeros(len(r), bool)
    keep[order[:max(int(k), 0)]] = True
    return keep


def select(vertices, triangles, sh, keep, normal=None, material=None):
    keep = np.asarray(keep).astype(bool)
    assert keep.shape == (len(sh.records),)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    vmask = np.zeros(len(sh.vertex_shell), bool)
    vmask[sh.vertex_shell >= 0] = keep[sh.vertex_shell[sh.vertex_shell >= 0]]
    tmask = keep[sh.triangle_shell] if len(tri) else np.zeros(0, bool)
    new_index = np.where(vmask, np.cumsum(vmask) - 1, -1)            # the rank among the kept
    out_t = new_index[tri[tmask]].astype(np.int32).reshape(-1, 3)
    pick = lambda a: None if a is None else np.asarray(a)[vmask]
    return np.asarray(vertices)[vmask], out_t, pick(normal), pick(material), new_index
