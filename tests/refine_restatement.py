"""The rule of ft_mesh_lattice_refined / ft_slice_lattice_refined / ft_refine_segments (include/fraytracer_hip.h "Refinement"), restated in numpy
float32 from the header's text.  It shares nothing with the library.

    lattice_brackets(values, origin, step, iso, dirs) -> Brackets(A [n, 3], B [n, 3], sA [n], sB [n]) in key order, and the edges' lengths
    midpoint, round_, finish                          -> one step of the rule each
    bisect(A, B, sA, sB, distance, iso, R)            -> the vertices after R rounds; distance is a callable on float32 [n, 3] points
    segments(a, b, dA, dB, distance, iso, R)          -> (points, status)"""
import collections

import numpy as np

F = np.float32
Brackets = collections.namedtuple("Brackets", "A B sA sB")
# edge direction e = 4 di + 2 dj + dk - 1: the mesher's seven
MESH_DIRS = tuple(((e + 1) >> 2 & 1, (e + 1) >> 1 & 1, (e + 1) & 1) for e in range(7))


def slice_dirs(axis):
    """the three directions with no component along `axis`, ascending e"""
    return tuple(d for d in MESH_DIRS if d[axis] == 0)


def lattice_brackets(values, origin, step, iso, dirs=MESH_DIRS):
    """edge (q, e) carries a vertex iff s[q] and s[q'] are both finite and exactly one end is inside; A = p(q), the owner, B = p(q'); keys order by q,
    then e -> (Brackets, float64 [n] Euclidean length of each edge)"""
    d = np.ascontiguousarray(values, dtype=F)
    nx, ny, nz = d.shape
    o, st = np.asarray(origin, F).reshape(3), np.asarray(step, F).reshape(3)
    with np.errstate(all="ignore"):
        s = (d - F(iso)).astype(F)
    inside, finite = s < 0, np.isfinite(s)
    carries = np.zeros((nx, ny, nz, len(dirs)), bool)
    for x, (di, dj, dk) in enumerate(dirs):
        if nx - di < 1 or ny - dj < 1 or nz - dk < 1:
            continue
        a = (slice(0, nx - di), slice(0, ny - dj), slice(0, nz - dk))
        b = (slice(di, nx), slice(dj, ny), slice(dk, nz))
        carries[a + (x,)] = finite[a] & finite[b] & (inside[a] != inside[b])
    qe = np.flatnonzero(carries.reshape(-1))                           # q major, e minor: key order
    q, x = qe // len(dirs), qe % len(dirs)
    ijk = np.stack(np.unravel_index(q, (nx, ny, nz)), axis=1)
    far = ijk + np.asarray(dirs, np.int64)[x]
    A, B = np.empty((len(qe), 3), F), np.empty((len(qe), 3), F)
    for ax in range(3):                                                # the lattice's point rule: one product, rounded, then one sum, rounded
        A[:, ax] = (o[ax] + (ijk[:, ax].astype(F) * st[ax]).astype(F)).astype(F)
        B[:, ax] = (o[ax] + (far[:, ax].astype(F) * st[ax]).astype(F)).astype(F)
    length = np.linalg.norm(B.astype(np.float64) - A.astype(np.float64), axis=1)
    return Brackets(A, B, s[tuple(ijk.T)].copy(), s[tuple(far.T)].copy()), length


def midpoint(A, B):
    with np.errstate(all="ignore"):
        return ((A + B).astype(F) * F(0.5)).astype(F)                  # one sum, rounded, then one product, rounded


def round_(br, M, dM, iso):
    """one round: M the midpoints, dM = D(M) -> the next Brackets"""
    with np.errstate(all="ignore"):
        sM = (np.asarray(dM, F) - F(iso)).astype(F)
    ok = np.isfinite(sM)                                               # not finite: the bracket stays as it is
    toA = ok & ((sM < 0) == (br.sA < 0))
    toB = ok & ~toA
    A, B, sA, sB = br.A.copy(), br.B.copy(), br.sA.copy(), br.sB.copy()
    A[toA], sA[toA] = M[toA], sM[toA]
    B[toB], sB[toB] = M[toB], sM[toB]
    return Brackets(A, B, sA, sB)


def finish(br):
    with np.errstate(all="ignore"):
        t = (br.sA / (br.sA - br.sB).astype(F)).astype(F)
        return (br.A + (t[:, None] * (br.B - br.A).astype(F)).astype(F)).astype(F)


def bisect(A, B, sA, sB, distance, iso, R, each=None):
    """R rounds and the finish.  each: called with (old Brackets, M, new Brackets) after every round"""
    br = Brackets(np.array(A, F), np.array(B, F), np.array(sA, F), np.array(sB, F))
    for _ in range(R):
        M = midpoint(br.A, br.B)
        with np.errstate(all="ignore"):
            dM = np.asarray(distance(M), F) if len(M) else np.zeros(0, F)
        new = round_(br, M, dM, iso)
        if each is not None:
            each(br, M, new)
        br = new
    return finish(br)


def segments(a, b, dA, dB, distance, iso, R):
    """status 1 where sA = D(a) - iso and sB = D(b) - iso are both finite and exactly one is inside; the point is then the finish after R rounds, else
    three NaN"""
    a, b = np.ascontiguousarray(a, F).reshape(-1, 3), np.ascontiguousarray(b, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        sA, sB = (np.asarray(dA, F) - F(iso)).astype(F), (np.asarray(dB, F) - F(iso)).astype(F)
    status = np.isfinite(sA) & np.isfinite(sB) & ((sA < 0) != (sB < 0))
    points = np.full(a.shape, np.nan, F)
    if status.any():
        points[status] = bisect(a[status], b[status], sA[status], sB[status], distance, iso, R)
    return points, status.astype(np.int32)
