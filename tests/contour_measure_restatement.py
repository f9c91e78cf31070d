"""The rule of include/fraytracer_hip.h "Contour measures", restated from that text alone in numpy float64 and Python integers: float64 terms by
individually rounded operations, one quantisation per term, exact integer sums, one conversion.  Nothing here knows how the device does it.

    measure(points, polylines, axis, n_slices) -> (record array [nL] of RECORD, record array [n_slices] of SLICE_RECORD)"""
import numpy as np

RECORD = np.dtype([("length", "<f8"), ("area", "<f8"), ("moment", "<f8", (2,)), ("bbox_min", "<f4", (2,)), ("bbox_max", "<f4", (2,)),
                   ("n_unmeasured", "<i4"), ("extent_exponent", "<i4")])
SLICE_RECORD = np.dtype([("length", "<f8"), ("area", "<f8"), ("moment", "<f8", (2,)), ("bbox_min", "<f4", (2,)), ("bbox_max", "<f4", (2,)),
                         ("n_polylines", "<i4"), ("n_closed", "<i4"), ("n_outer", "<i4"), ("n_holes", "<i4"), ("n_unmeasured", "<i4"), ("extent_exponent", "<i4")])
assert RECORD.itemsize == 56 and SLICE_RECORD.itemsize == 72
SHIFT = 90


def extent_exponent(points):
    """E ("Measures"): 0 if the largest finite |coordinate| m is 0 (or there is none), else ilogb(m) + 1 — denormals by their true exponent"""
    v = np.asarray(points, np.float32).reshape(-1)
    v = np.abs(v[np.isfinite(v)])
    if v.size == 0 or v.max() == 0:
        return 0
    _, e = np.frexp(np.float64(v.max()))                               # m = f * 2^e, 0.5 <= f < 1: ilogb(m) = e - 1
    return int(e)


def bounds(E):
    """B_L, B_C, B_M"""
    return E + 2, 2 * E + 2, 3 * E + 3


def plane(axis):
    """(u, v) of an axis"""
    return (axis + 1) % 3, (axis + 2) % 3


def segments(first, count, closed):
    """the index pairs (i, j) of a polyline's segments, in order: consecutive points, then the closing segment of a closed polyline"""
    idx = [(first + i, first + i + 1) for i in range(count - 1)]
    if closed and count > 0:
        idx.append((first + count - 1, first))
    return idx


def terms(P, Q):
    """float64 [n, 4] for segments (P, Q) given as float64 [n, 2] (u, v) each: L_t, C_t, M_t,u, M_t,v — one numpy operation per operation of the rule"""
    Pu, Pv, Qu, Qv = P[:, 0], P[:, 1], Q[:, 0], Q[:, 1]
    with np.errstate(all="ignore"):
        du = Qu - Pu
        dv = Qv - Pv
        a = du * du
        b = dv * dv
        L = np.sqrt(a + b)
        c0 = Pu * Qv
        c1 = Qu * Pv
        C = c0 - c1
        su = Pu + Qu
        sv = Pv + Qv
        Mu = C * su
        Mv = C * sv
    return np.stack([L, C, Mu, Mv], axis=1)


def quantise(term, s):
    """round-half-to-even(term * 2^s) as a Python int: the scaling is exact (or underflows below 1/2), rint rounds once"""
    with np.errstate(all="ignore"):
        return int(np.rint(np.ldexp(np.float64(term), int(s))))


def to_float(Q, s):
    """fl64(Q) * 2^-s: float(int) rounds half to even, the scaling is exact"""
    return np.ldexp(np.float64(float(Q)), -int(s))


def key(bits):
    bits = int(bits)
    return (~bits & 0xFFFFFFFF) if bits & 0x80000000 else bits ^ 0x80000000


def box(values):
    """(min, max) as float32 over the finite values, by the ordered key of their bits; +inf / -inf without one"""
    vals = np.asarray(values, np.float32).reshape(-1)
    vals = vals[np.isfinite(vals)]
    if vals.size == 0:
        return np.float32(np.inf), np.float32(-np.inf)
    keys = [key(b) for b in vals.view(np.uint32)]
    return vals[int(np.argmin(keys))], vals[int(np.argmax(keys))]


def integer_sums(points, polylines, axis, E=None):
    """per polyline the four exact sums Q_L, Q_C, Q_M,u, Q_M,v of its measured segments' quantised terms as Python ints [nL][4], and the unmeasured
    segments int [nL]"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    rec = np.asarray(polylines, np.int64).reshape(-1, 4)
    E = extent_exponent(p) if E is None else E
    B = bounds(E)
    shift = [SHIFT - B[0], SHIFT - B[1], SHIFT - B[2], SHIFT - B[2]]
    u, v = plane(axis)
    uv = p[:, [u, v]]
    sums, bad = [], []
    for first, count, _, closed in rec.tolist():
        seg = np.array(segments(first, count, closed), np.int64).reshape(-1, 2)
        A, Bq = uv[seg[:, 0]], uv[seg[:, 1]]
        fine = np.isfinite(A).all(axis=1) & np.isfinite(Bq).all(axis=1)
        x = terms(A[fine].astype(np.float64), Bq[fine].astype(np.float64))
        with np.errstate(all="ignore"):
            cols = [np.rint(np.ldexp(x[:, k], shift[k])).tolist() for k in range(4)]      # float64 values that are integers: int() is exact
        sums.append([sum(int(q) for q in cols[k]) for k in range(4)])
        bad.append(int((~fine).sum()))
    return sums, bad


def results(Q, E):
    """length, area, moment u, moment v of four integer sums"""
    B = bounds(E)
    S = [to_float(Q[0], SHIFT - B[0]), to_float(Q[1], SHIFT - B[1]), to_float(Q[2], SHIFT - B[2]), to_float(Q[3], SHIFT - B[2])]
    return S[0], S[1] / np.float64(2.0), S[2] / np.float64(6.0), S[3] / np.float64(6.0)


def measure(points, polylines, axis, n_slices, E=None):
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    rec = np.asarray(polylines, np.int64).reshape(-1, 4)
    E = extent_exponent(p) if E is None else E
    u, v = plane(axis)
    sums, bad = integer_sums(p, rec, axis, E)
    out, per = np.zeros(len(rec), RECORD), np.zeros(n_slices, SLICE_RECORD)
    out["extent_exponent"], per["extent_exponent"] = E, E
    slice_sums = [[0, 0, 0, 0] for _ in range(n_slices)]
    slice_points = [[] for _ in range(n_slices)]
    for l, (first, count, w, closed) in enumerate(rec.tolist()):
        out["length"][l], out["area"][l], out["moment"][l, 0], out["moment"][l, 1] = results(sums[l], E)
        for x, c in enumerate((u, v)):
            out["bbox_min"][l, x], out["bbox_max"][l, x] = box(p[first:first + count, c])
        out["n_unmeasured"][l] = bad[l]
        slice_sums[w][0] += sums[l][0]
        per["n_polylines"][w] += 1
        per["n_unmeasured"][w] += bad[l]
        slice_points[w].append(p[first:first + count])
        if closed:
            for k in (1, 2, 3):
                slice_sums[w][k] += sums[l][k]
            per["n_closed"][w] += 1
            per["n_outer"][w] += 1 if sums[l][1] > 0 else 0
            per["n_holes"][w] += 1 if sums[l][1] < 0 else 0
    for w in range(n_slices):
        per["length"][w], per["area"][w], per["moment"][w, 0], per["moment"][w, 1] = results(slice_sums[w], E)
        pts = np.concatenate(slice_points[w]) if slice_points[w] else np.zeros((0, 3), np.float32)
        for x, c in enumerate((u, v)):
            per["bbox_min"][w, x], per["bbox_max"][w, x] = box(pts[:, c])
    return out, per


def same_bytes(got, want):
    """two record arrays, bit for bit"""
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return g.shape == w.shape and g.dtype.itemsize == w.dtype.itemsize and g.tobytes() == w.tobytes()
