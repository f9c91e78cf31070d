"""The rule of include/fraytracer_hip.h "Measures", restated from that text alone in numpy float64 and Python integers: float64 terms by individually
rounded operations, one quantisation per term, exact integer sums, one conversion.  Nothing here knows how the device does it.

    measure(vertices, triangles, vertex_label, triangle_label, n_shells) -> record array [n_shells] of RECORD
    whole(vertices, triangles)                                            -> record array [1]: every label 0"""
import numpy as np

RECORD = np.dtype([("area", "<f8"), ("volume", "<f8"), ("moment", "<f8", (3,)), ("bbox_min", "<f4", (3,)), ("bbox_max", "<f4", (3,)),
                   ("n_unmeasured", "<i4"), ("extent_exponent", "<i4")])
assert RECORD.itemsize == 72
SHIFT = 90


def extent_exponent(vertices):
    """E: 0 if the largest finite |coordinate| m is 0 (or there is none), else ilogb(m) + 1 — denormals by their true exponent"""
    v = np.asarray(vertices, np.float32).reshape(-1)
    v = np.abs(v[np.isfinite(v)])
    if v.size == 0 or v.max() == 0:
        return 0
    _, e = np.frexp(np.float64(v.max()))                               # m = f * 2^e, 0.5 <= f < 1: ilogb(m) = e - 1; float64 holds a float32 denormal as a normal
    return int(e)


def bounds(E):
    """B_A, B_W, B_M"""
    return 2 * E + 3, 3 * E + 3, 4 * E + 5


def measured(vertices, triangles):
    """bool [nT]: the three indices are in range and the nine coordinates finite"""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    ok = ((t >= 0) & (t < len(v))).all(axis=1)
    fine = np.zeros(len(t), bool)
    fine[ok] = np.isfinite(v[t[ok]]).all(axis=(1, 2))
    return fine


def terms(vertices, triangles):
    """float64 [n, 5] for triangles that are all measured: A_t, W_t, M_t,x, M_t,y, M_t,z — one numpy operation per operation of the rule"""
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    with np.errstate(all="ignore"):
        u, w = b - a, c - a
        nx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
        ny = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
        nz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
        area = 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)
        six = ((a[:, 0] * (b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]) + a[:, 1] * (b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2]))
               + a[:, 2] * (b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]))
        m = [six * ((a[:, i] + b[:, i]) + c[:, i]) for i in range(3)]
    return np.stack([area, six] + m, axis=1)


def quantise(term, s):
    """round-half-to-even(term * 2^s) as a Python int: the scaling is exact (or underflows below 1/2), rint rounds once and gives a float64 that
    is an integer, which int() takes over exactly"""
    with np.errstate(all="ignore"):
        return int(np.rint(np.ldexp(np.float64(term), int(s))))


def quantised(vertices, triangles, E):
    """list of 5-tuples of Python ints, one per (measured) triangle: quantise() applied to every term, whole columns at a time"""
    B = bounds(E)
    x = terms(vertices, triangles)
    with np.errstate(all="ignore"):
        cols = [np.rint(np.ldexp(x[:, k], SHIFT - B[min(k, 2)])).tolist() for k in range(5)]      # float64 values that are integers: int() is exact
    return [tuple(int(c[i]) for c in cols) for i in range(len(x))]


def to_float(Q, s):
    """fl64(Q) * 2^-s: float(int) rounds half to even, the scaling is exact"""
    return np.ldexp(np.float64(float(Q)), -int(s))


def key(bits):
    bits = int(bits)
    return (~bits & 0xFFFFFFFF) if bits & 0x80000000 else bits ^ 0x80000000


def box(values):
    """(min, max) as float32 over the finite values, by the ordered key of their bits; +inf / -inf without one"""
    vals = np.asarray(values, np.float32)
    vals = vals[np.isfinite(vals)]
    if vals.size == 0:
        return np.float32(np.inf), np.float32(-np.inf)
    keys = [key(b) for b in vals.view(np.uint32)]
    return vals[int(np.argmin(keys))], vals[int(np.argmax(keys))]


def integer_sums(vertices, triangles, triangle_label, n_shells, E=None):
    """Q: per shell the five exact sums of the quantised terms of its measured triangles, as Python ints [n_shells][5]; and the unmeasured counts"""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
    tl = np.zeros(len(t), np.int64) if triangle_label is None else np.asarray(triangle_label, np.int64)
    E = extent_exponent(v) if E is None else E
    fine = measured(v, t)
    inside = (tl >= 0) & (tl < n_shells)
    sums = [[0] * 5 for _ in range(n_shells)]
    pick = np.flatnonzero(fine & inside)
    for row, s in zip(quantised(v, t[pick], E), tl[pick]):
        for k in range(5):
            sums[s][k] += row[k]
    return sums, np.bincount(tl[inside & ~fine], minlength=n_shells).astype(np.int32)


def measure(vertices, triangles, vertex_label, triangle_label, n_shells, E=None):
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    vl = np.zeros(len(v), np.int64) if vertex_label is None else np.asarray(vertex_label, np.int64)
    E = extent_exponent(v) if E is None else E
    B = bounds(E)
    shift = [SHIFT - B[0], SHIFT - B[1], SHIFT - B[2], SHIFT - B[2], SHIFT - B[2]]
    sums, bad = integer_sums(v, triangles, triangle_label, n_shells, E)
    out = np.zeros(n_shells, RECORD)
    out["n_unmeasured"] = bad
    for s in range(n_shells):
        S = [to_float(sums[s][k], shift[k]) for k in range(5)]
        out["area"][s] = S[0]
        out["volume"][s] = S[1] / np.float64(6.0)
        for i in range(3):
            out["moment"][s, i] = S[2 + i] / np.float64(24.0)
            out["bbox_min"][s, i], out["bbox_max"][s, i] = box(v[vl == s, i])
    out["extent_exponent"] = E
    return out


def whole(vertices, triangles):
    return measure(vertices, triangles, None, None, 1)


def same_bytes(got, want):
    """two record arrays, bit for bit"""
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return g.shape == w.shape and g.dtype.itemsize == w.dtype.itemsize and g.tobytes() == w.tobytes()
