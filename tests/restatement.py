"""A second restatement of the reference's form, object and scene arithmetic: plain numpy float32, written from the F# text (file:line cited per
function, paths under src/FrayTracer/), vectorised over points and scalar over children.  Shared by tests/test_restatement_host.py and
tests/test_gpu_restatement.py; there is no test in it.

It walks the scene descriptions of fraytracer_amd.api (kind, args, kids), imports nothing from oracle/ or fraytracer_amd/csrc and reads nothing the
oracle or the flattener computed.  The one exception is expf / logf for unionSmooth: MathF.Exp / MathF.Log are platform libm in .NET, the project
replaces them by fixed algorithms of its own, and the caller hands those in (tests/test_oracle_numpy_crosscheck.py does the same and checks exp
against an exact rational evaluation).

Assumed System.Numerics / MathF semantics, no others (HISTORY.md): Dot = (x x' + y y') + z z'; Length = sqrt(Dot); Normalize = v / Length
and Vector3 / float as true division; -v = Zero - v; Lerp = a (1 - t) + b t; Cross by components; MathF.Min / Max = IEEE 754:2019 minimum / maximum
(a NaN wins, -0 < +0); MathF.Sqrt correctly rounded; conv.i4 of a value out of range = INT_MIN; Array.sortInPlaceBy with ties in input order;
no contraction of a b + c anywhere (numpy never fuses).

Three things are the project's conventions, not the reference's, and are marked where they occur: MathF.Sign(NaN) throws in .NET (here: recorded
in Record.threw, so that a test leaves those points out); a NaN distance in a march would spin forever (here: the ray ends as a miss, flag 1);
a march has no step cap in the reference (here: MAX_STEPS, flag 4, and the tests assert that no ray reaches it)."""
import numpy as np

F = np.float32
MAX_STEPS = 1 << 14
FLAG_NAN, FLAG_SIGN, FLAG_CAP = 1, 2, 4


def v3(v):
    return np.asarray(v, F).reshape(3)


# ---- System.Numerics.Vector3 / Vector2 as assumed ---------------------------------------------------------------------------------------------------
def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def length2(a):
    return dot(a, a)


def length(a):
    return np.sqrt(dot(a, a))


def distance(a, b):
    return length(a - b)


def distance2(a, b):
    return length2(a - b)


def over(a, s):
    """Vector3 / float"""
    return a / np.asarray(s, F)[..., None]


def times(a, s):
    """Vector3 * float"""
    return a * np.asarray(s, F)[..., None]


def normalize(a):
    return over(a, length(a))


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def inverse_length(a):                                      # Math.fs:69
    return over(a, length2(a))


# ---- System.MathF as assumed (Math.fs:40-59) --------------------------------------------------------------------------------------------------------
def mathf_max(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F))
    r = np.where(a > b, a, b)                               # an unordered pair leaves b, which is the NaN unless a is
    r = np.where(np.isnan(a), a, r)
    zeros = (a == 0) & (b == 0)
    return np.where(zeros, np.where(np.signbit(a), b, a), r).astype(F)


def mathf_min(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F))
    r = np.where(a < b, a, b)
    r = np.where(np.isnan(a), a, r)
    zeros = (a == 0) & (b == 0)
    return np.where(zeros, np.where(np.signbit(a), a, b), r).astype(F)


def clamp01(x):                                             # Math.fs:51
    return mathf_max(F(0), mathf_min(F(1), x))


def conv_i4(x):
    """float32 -> int as conv.i4 after MathF.Floor / Ceiling (Math.fs:57,59): out of range and NaN give INT_MIN"""
    x = np.asarray(x, np.float64)
    ok = (x >= -2.0 ** 31) & (x < 2.0 ** 31)
    return np.where(ok, np.where(ok, x, 0.0), -2.0 ** 31).astype(np.int64)


class Record:
    """which branches the active points of one evaluation took: what keeps a test from passing vacuously"""

    def __init__(self, n):
        self.threw = np.zeros(n, bool)                      # MathF.Sign(NaN): .NET throws there
        self.capsule = [0, 0, 0]                            # t <= 0, t >= 1, between
        self.t_is_0 = self.t_is_1 = 0
        self.face = self.edge = self.edge_dot_zero = 0
        self.taken = self.pruned = 0                        # SdfForm.intersect's steps


# ---- SdfBoundary.fs:7-63 ----------------------------------------------------------------------------------------------------------------------------
def boundary_union(a, b):                                   # SdfBoundary.fs:7-22
    (ac, ar), (bc, br) = a, b
    diff = bc - ac
    d = length(diff)
    if d + br <= ar:
        return a
    if d + ar <= br:
        return b
    along = over(diff, d)
    pa = ac - times(along, ar)
    pb = bc + times(along, br)
    return times(pa + pb, F(0.5)), F(distance(pa, pb) * F(0.5))


def boundary_intersection(a, b):                            # SdfBoundary.fs:29-49
    (ac, ar), (bc, br) = a, b
    diff = bc - ac
    d = length(diff)
    if d + br <= ar:
        return b
    if d + ar <= br:
        return a
    along = over(diff, d)
    pa = ac + times(along, ar)
    pb = bc - times(along, br)
    d2, ar2, br2 = d * d, ar * ar, br * br
    # :48: the bracket is not squared in the text
    return times(pa + pb, F(0.5)), F(np.sqrt(F(4) * d2 * ar2 - (d2 - br2 + ar2)) / (F(2) * d))


def reduce(rule, boundaries):                               # Seq.reduce: unionMany :24-27, intersectionMany :51-54
    acc = boundaries[0]
    for b in boundaries[1:]:
        acc = rule(acc, b)
    return acc


def is_inside(b, p):                                        # SdfBoundary.fs:56
    return distance2(b[0], p) < b[1] * b[1]


def min_distance(b, p):                                     # SdfBoundary.fs:62
    return distance(b[0], p) - b[1]


def max_distance(b, p):                                     # SdfBoundary.fs:63
    return distance(b[0], p) + b[1]


class Lookup:
    """SdfBoundary.buildSpatialLookup over boundaries (SdfBoundary.fs:225-282), every cell at once"""

    def __init__(self, boundaries):
        n = len(boundaries)
        self.bc = np.stack([b[0] for b in boundaries]).astype(F)
        self.br = np.array([b[1] for b in boundaries], F)
        lo = self.bc - self.br[:, None]                     # AABB.getMin / getMax :66-67
        hi = self.bc + self.br[:, None]
        amin, amax, total = lo[0], hi[0], self.br[0]
        for i in range(1, n):                               # :229-232, in input order
            amin = np.where(amin < lo[i], amin, lo[i])      # Vector3.Min / Max by components
            amax = np.where(amax > hi[i], amax, hi[i])
            total = total + self.br[i]
        count_size = F(1.5) * (total / F(n))                # :233
        size = amax - amin                                  # :235
        c = max(int(conv_i4(np.ceil(size[0] / count_size))), 1)    # :237-239: X on all three axes
        self.counts = (c, c, c)
        self.amin = amin
        self.cell = size / np.array([c, c, c], F)           # :240
        self.cell_inv = F(1) / self.cell                    # :241
        idx = np.stack(np.meshgrid(np.arange(c), np.arange(c), np.arange(c), indexing="ij"), -1).reshape(-1, 3).astype(F)
        self.centers = (amin + self.cell * F(0.5)) + self.cell * idx                       # :246, cell (x, y, z) at (x c + y) c + z
        reach = np.stack([max_distance(b, self.centers) for b in boundaries])              # :251
        nearest = reach[0]
        for i in range(1, n):                               # Seq.min :252
            nearest = np.where(reach[i] < nearest, reach[i], nearest)
        upper = nearest + length(self.cell * F(0.5))        # :253
        lower = np.stack([min_distance(b, self.centers) for b in boundaries])              # :257
        keep = lower < upper[None, :]                       # :258
        self.n_items = keep.sum(axis=0)
        m = int(self.n_items.max())
        order = np.argsort(np.where(keep, lower, np.inf).T, axis=1, kind="stable")[:, :m]          # :267-268, ties in input order
        self.child = order
        self.lower = np.take_along_axis(lower.T, order, axis=1)

    def dump(self):
        """the lists laid out cell after cell, as the oracle and the flattener dump theirs"""
        start = np.concatenate([[0], np.cumsum(self.n_items)]).astype(np.uint32)
        valid = np.arange(self.child.shape[1])[None, :] < self.n_items[:, None]
        return {"counts": self.counts, "aabbMin": self.amin, "cellSize": self.cell, "cellSizeInv": self.cell_inv, "centers": self.centers,
                "cell_start": start, "lower": self.lower[valid], "child": self.child[valid].astype(np.int32)}

    def ties(self):
        """cells whose list holds two equal LowerBounds: there the order is the sort's, which the reference leaves open"""
        valid = np.arange(self.child.shape[1])[None, :] < self.n_items[:, None]
        same = (self.lower[:, 1:] == self.lower[:, :-1]) & valid[:, 1:]
        return int(same.any(axis=1).sum())

    def cell_of(self, p):                                   # :276-282
        c = (p - self.amin) * self.cell_inv
        i = [np.clip(conv_i4(np.floor(c[:, k])), 0, self.counts[k] - 1) for k in range(3)]
        return (i[0] * self.counts[1] + i[1]) * self.counts[2] + i[2]

    def walk(self, p, D, object_rule):
        """the loop of SdfForm.union (SdfForm.fs:23-34: from item 1, MathF.min) or of SdfObject.union's colour (SdfObject.fs:28-43: from item 0,
        strict <) over the list of each point's cell; D[k] = child k's distance at every point -> (min, item that gave it, [k, point] evaluated)"""
        n = p.shape[0]
        at = np.arange(n)
        cell = self.cell_of(p)
        to_centre = distance(self.centers[cell], p)
        first = self.child[cell, 0]
        low, who = D[first, at], first.copy()
        used = np.zeros(D.shape, bool)
        used[first, at] = True
        for j in range(0 if object_rule else 1, self.child.shape[1]):
            listed = j < self.n_items[cell]
            k = np.where(listed, self.child[cell, j], 0)
            go = listed & (low > self.lower[cell, j] - to_centre) & (low > min_distance((self.bc[k], self.br[k]), p))
            used[k[go], at[go]] = True
            dk = D[k, at]
            if object_rule:
                better = go & (dk < low)
                low, who = np.where(better, dk, low), np.where(better, k, who)
            else:
                low = np.where(go, mathf_min(low, dk), low)
        return low, who, used


# ---- SdfForm.fs ---------------------------------------------------------------------------------------------------------------------------------------
class Sphere:                                               # SdfForm.fs:125-135
    def __init__(self, centre, radius):
        self.c, self.r = v3(centre), F(radius)
        self.boundary = (self.c, self.r)

    def distance(self, p, rec=None, active=None):
        return distance(self.c, p) - self.r


class Capsule:                                              # SdfForm.fs:145-170
    def __init__(self, a, b, radius):
        self.a, self.r = v3(a), F(radius)
        self.dir = v3(b) - self.a
        self.dir_inv = inverse_length(self.dir)
        self.boundary = (self.a * (F(1) - F(0.5)) + v3(b) * F(0.5), F(self.r + distance(self.a, v3(b)) * F(0.5)))      # Vector3.Lerp

    def distance(self, p, rec=None, active=None):
        diff = p - self.a
        t = dot(diff, self.dir_inv)
        d = np.where(t <= 0, length(diff), np.where(t >= 1, distance(diff, self.dir), distance(diff, times(self.dir, t))))
        if rec is not None:
            rec.capsule[0] += int((active & (t <= 0)).sum())
            rec.capsule[1] += int((active & ~(t <= 0) & (t >= 1)).sum())
            rec.capsule[2] += int((active & ~(t <= 0) & ~(t >= 1)).sum())
            rec.t_is_0 += int((active & (t == 0)).sum())
            rec.t_is_1 += int((active & (t == 1)).sum())
        return d - self.r


class Torus:                                                # SdfForm.fs:181-203
    def __init__(self, centre, normal, major, minor):
        self.c, self.major, self.minor = v3(centre), F(major), F(minor)
        self.n = normalize(v3(normal))
        self.plane_d = -dot(self.c, self.n)
        self.boundary = (self.c, F(self.major + self.minor))

    def distance(self, p, rec=None, active=None):
        to_plane = dot(p, self.n) + self.plane_d
        to_centre = distance(self.c, p - times(self.n, to_plane))
        to_circle = to_centre - self.major
        return np.sqrt(to_plane * to_plane + to_circle * to_circle) - self.minor           # Vector2.Length


class Triangle:                                             # SdfForm.fs:214-268
    def __init__(self, ctx, v1, v2, v3_, radius):
        self.ctx = ctx
        self.v = (v3(v1), v3(v2), v3(v3_))
        a, b, c = self.v
        self.r = F(radius)
        self.e = (b - a, c - b, a - c)                      # v21, v32, v13
        self.e_inv = tuple(inverse_length(e) for e in self.e)
        self.nor = normalize(cross(self.e[0], self.e[2]))
        self.out = tuple(normalize(cross(e, self.nor)) for e in self.e)                    # n21, n32, n13
        area_inv = F(0.5) / length2(cross(a - b, b - c))    # :255
        w1 = length2(b - c) * dot(a - b, a - c) * area_inv
        w2 = length2(a - c) * dot(b - a, b - c) * area_inv
        w3 = F(1) - w1 - w2
        centre = times(a, w1) + times(b, w2) + times(c, w3)
        radius = length(self.e[0]) * length(self.e[1]) * length(self.e[2]) / F(2) / length(cross(self.e[0], self.e[1])) + self.r
        self.boundary = (centre.astype(F), F(radius))

    def distance(self, p, rec=None, active=None):
        rel = [p - v for v in self.v]                       # p1, p2, p3
        side = [dot(self.out[k], rel[k]) for k in range(3)]
        thrown = np.isnan(side[0]) | np.isnan(side[1]) | np.isnan(side[2])
        if thrown.any():                                    # convention: .NET throws; the value below takes Sign(NaN) as 0, like the project
            self.ctx.flags |= FLAG_SIGN
        signs = sum(np.sign(np.where(np.isnan(s), F(0), s)).astype(np.int32) for s in side)
        sq = [distance2(rel[k], times(self.e[k], clamp01(dot(self.e_inv[k], rel[k])))) for k in range(3)]      # :240-242
        edges = np.sqrt(mathf_min(sq[2], mathf_min(sq[1], sq[0])))                         # x |> MathF.min m = MathF.Min(m, x), :243
        face = np.abs(dot(self.nor, rel[0]))                # :247
        by_edges = signs < 2
        if rec is not None:
            rec.threw |= active & thrown
            rec.edge += int((active & by_edges).sum())
            rec.face += int((active & ~by_edges).sum())
            rec.edge_dot_zero += int((active & ((side[0] == 0) | (side[1] == 0) | (side[2] == 0))).sum())
        return np.where(by_edges, edges, face) - self.r


class Union:                                                # SdfForm.fs:14-40
    def __init__(self, kids):
        self.kids = kids
        self.lookup = Lookup([k.boundary for k in kids])
        self.boundary = reduce(boundary_union, [k.boundary for k in kids])

    def distance(self, p, rec=None, active=None):
        D = np.stack([k.distance(p) for k in self.kids])
        low, _, used = self.lookup.walk(p, D, False)
        if rec is not None:
            for k, kid in enumerate(self.kids):
                kid.distance(p, rec, active & used[k])
        return low


class Subtract:                                             # SdfForm.fs:42-49
    def __init__(self, a, b):
        self.a, self.b = a, b
        self.boundary = a.boundary

    def distance(self, p, rec=None, active=None):
        da = self.a.distance(p, rec, active)
        return mathf_max(-self.b.distance(p, rec, active), da)      # x |> MathF.max m = MathF.Max(m, x)


class Intersect:                                            # SdfForm.fs:51-67
    def __init__(self, kids):
        self.kids = kids
        self.boundary = reduce(boundary_intersection, [k.boundary for k in kids])

    def distance(self, p, rec=None, active=None):
        high = self.kids[0].distance(p, rec, active)
        for kid in self.kids[1:]:
            take = high < max_distance(kid.boundary, p)     # :62
            d = kid.distance(p, rec, None if rec is None else active & take)
            if rec is not None:
                rec.taken += int((active & take).sum())
                rec.pruned += int((active & ~take).sum())
            high = np.where(take, mathf_max(high, d), high)
        return high


class UnionSmooth:                                          # SdfForm.fs:69-91
    def __init__(self, ctx, strength, kids):
        self.ctx, self.k, self.kids = ctx, F(strength), kids
        self.k_inv = F(-1) / self.k
        self.boundary = reduce(boundary_union, [k.boundary for k in kids])

    def distance(self, p, rec=None, active=None):
        total = np.zeros(p.shape[0], F)
        for kid in self.kids:
            total = total + self.ctx.expf(self.k_inv * kid.distance(p, rec, active))
        return -self.ctx.logf(total) * self.k


# ---- SdfObject.fs -------------------------------------------------------------------------------------------------------------------------------------
class Created:                                              # SdfObject.fs:6-10
    def __init__(self, material, form):
        self.m, self.form = material, form

    def material(self, p):
        return np.full(p.shape[0], self.m, np.int64)


class ObjectUnion:                                          # SdfObject.fs:12-48
    def __init__(self, kids):
        self.kids = kids
        self.form = Union([k.form for k in kids])           # :26 builds the same lookup a second time; one is kept here

    def material(self, p):
        D = np.stack([k.form.distance(p) for k in self.kids])
        _, who, _ = self.form.lookup.walk(p, D, True)
        out = np.empty(p.shape[0], np.int64)
        for k in np.unique(who):
            out[who == k] = self.kids[k].material(p[who == k])
        return out


class Carved:                                               # SdfObject.fs:50-64: subtract and intersect keep the object's material
    def __init__(self, obj, form):
        self.obj, self.form = obj, form

    def material(self, p):
        return self.obj.material(p)


class Restatement:
    """the compiled twin of one scene description; expf / logf: float32 array -> float32 array, the project's fixed algorithms"""

    def __init__(self, expf=None, logf=None):
        self.expf, self.logf = expf, logf
        self.flags = 0
        self.materials, self.colours = [], []               # Material descriptions and their colours, by index
        self.forms = {}                                     # id(description) -> compiled form, every node met
        self.unions = []                                    # every compiled union, SdfObject.union's among them
        self.objects = {}                                   # id(description) -> compiled object
        self._keep = []                                     # the descriptions themselves, so that no id is used twice

    # ---- compiling ---------------------------------------------------------------------------------------------------------------------
    def form(self, node):
        if id(node) in self.forms:
            return self.forms[id(node)]
        kids = [self.form(k) for k in node.kids]
        k, a = node.kind, node.args
        if k == "sphere": f = Sphere(*a)
        elif k == "capsule": f = Capsule(*a)
        elif k == "torus": f = Torus(*a)
        elif k == "triangle": f = Triangle(self, *a)
        elif k == "union": f = kids[0] if len(kids) == 1 else Union(kids)                  # SdfForm.fs:17
        elif k == "subtract": f = Subtract(*kids)
        elif k == "intersect": f = kids[0] if len(kids) == 1 else Intersect(kids)          # SdfForm.fs:54
        elif k == "unionSmooth": f = kids[0] if len(kids) == 1 else UnionSmooth(self, a[0], kids)
        else: raise ValueError(k)
        if k == "union" and len(kids) > 1:
            self.unions.append(f)
        self.forms[id(node)] = f
        self._keep.append(node)
        return f

    def object(self, node):
        if id(node) not in self.objects:
            self.objects[id(node)] = self._object(node)
            self._keep.append(node)
        return self.objects[id(node)]

    def _object(self, node):
        k = node.kind
        if k == "create":
            self.materials.append(node.kids[0])
            self.colours.append(v3(node.kids[0].args[0]))
            return Created(len(self.materials) - 1, self.form(node.kids[1]))
        if k == "union":
            kids = [self.object(c) for c in node.kids]
            if len(kids) == 1:                              # SdfObject.fs:15
                return kids[0]
            union = ObjectUnion(kids)
            self.unions.append(union.form)
            return union
        obj = self.object(node.kids[0])
        if k == "subtract":
            return Carved(obj, Subtract(obj.form, self.form(node.kids[1])))
        if k == "intersect":
            forms = [obj.form] + [self.form(c) for c in node.kids[1:]]
            return Carved(obj, forms[0] if len(forms) == 1 else Intersect(forms))
        raise ValueError(k)

    # ---- points ------------------------------------------------------------------------------------------------------------------------
    def distance(self, form, pts, record=False):
        """form.Distance at pts [n, 3] -> float32 [n] (and the Record of the evaluation)"""
        p = np.ascontiguousarray(pts, F).reshape(-1, 3)
        with np.errstate(all="ignore"):
            if not record:
                return form.distance(p).astype(F)
            rec = Record(len(p))
            return form.distance(p, rec, np.ones(len(p), bool)).astype(F), rec

    def try_distance(self, form, pts):                      # SdfForm.fs:7-12, NaN standing for ValueNone
        p = np.ascontiguousarray(pts, F).reshape(-1, 3)
        with np.errstate(all="ignore"):
            return np.where(is_inside(form.boundary, p), form.distance(p), F(np.nan)).astype(F)

    def normal(self, form, eps, pts):                       # SdfForm.fs:106-112
        p = np.ascontiguousarray(pts, F).reshape(-1, 3)
        with np.errstate(all="ignore"):
            probes = []
            for axis in range(3):
                q = p.copy()
                q[:, axis] = p[:, axis] + eps
                probes.append(form.distance(q))
            return normalize(np.stack(probes, axis=1) - form.distance(p)[:, None]).astype(F)

    def colour(self, obj, pts):
        """object.Material.Color at pts -> (float32 [n, 3], index into self.materials per point)"""
        p = np.ascontiguousarray(pts, F).reshape(-1, 3)
        with np.errstate(all="ignore"):
            m = obj.material(p)
        return np.stack(self.colours)[m], m

    # ---- rays [n, 8] = Origin, Direction, Length, Epsilon (Types.fs:9-17) -------------------------------------------------------------------
    def march(self, form, rays):
        """SdfForm.tryTrace (SdfForm.fs:93-104) -> (hit mask, the rays as they ended, Distance at the hit)"""
        r = np.ascontiguousarray(rays, F).reshape(-1, 8).copy()
        alive = np.ones(len(r), bool)
        hit = np.zeros(len(r), bool)
        at_hit = np.zeros(len(r), F)
        with np.errstate(all="ignore"):
            for step in range(MAX_STEPS + 1):
                alive &= ~(r[:, 6] <= 0)                    # :94
                i = np.flatnonzero(alive)
                if i.size == 0:
                    return hit, r, at_hit
                if step == MAX_STEPS:
                    break
                d = form.distance(r[i, 0:3]).astype(F)
                nan = np.isnan(d)
                if nan.any():                               # convention: the reference would never return
                    self.flags |= FLAG_NAN
                    alive[i[nan]] = False
                near = d < r[i, 7]                          # :98
                hit[i[near]], at_hit[i[near]] = True, d[near]
                alive[i[near]] = False
                go, dg = i[~near & ~nan], d[~near & ~nan]
                r[go, 0:3] = r[go, 0:3] + times(r[go, 3:6], dg)     # Ray.move, Ray.fs:6-13
                r[go, 6] = r[go, 6] - dg
        self.flags |= FLAG_CAP
        return hit, r, at_hit

    def form_try_trace(self, form, rays):
        """[n, 10]: the ray at the hit, Distance, 1 as int32 bits; a miss is zeros"""
        hit, r, d = self.march(form, rays)
        out = np.zeros((len(r), 10), F)
        out[hit, 0:8], out[hit, 8] = r[hit], d[hit]
        out[hit, 9] = np.array([1], np.int32).view(F)[0]
        return out

    def object_try_trace(self, obj, rays):
        """SdfObject.tryTrace (SdfObject.fs:66-78) -> ([n, 16]: ray pulled back, Normal, Color, 1 as int32 bits, 0; a miss is zeros, material index
        per ray or -1)"""
        hit, r, _ = self.march(obj.form, rays)
        out = np.zeros((len(r), 16), F)
        material = np.full(len(r), -1, np.int64)
        h = r[hit]
        with np.errstate(all="ignore"):
            eps = h[:, 7]
            back = h[:, 0:3] + times(h[:, 3:6], -eps)       # Ray.get (-Epsilon), SdfForm.fs:115 and SdfObject.fs:73
            nrm = np.empty((len(h), 3), F)
            for e in np.unique(eps):                        # normalFromRay: epsilon = Epsilon * 0.125
                nrm[eps == e] = self.normal(obj.form, e * F(0.125), back[eps == e])
            col, material[hit] = self.colour(obj, h[:, 0:3])                               # :77: at the ray's origin before the pull
            out[hit, 0:3], out[hit, 3:6], out[hit, 6], out[hit, 7] = back, h[:, 3:6], h[:, 6] - (-eps), eps
        out[hit, 8:11], out[hit, 11:14] = nrm, col
        out[hit, 14] = np.array([1], np.int32).view(F)[0]
        return out, material

    def trace(self, obj, background, lights, rays):
        """SdfScene.trace (SdfScene.fs:7-28) with SdfLight.directional / point (SdfLight.fs:6-42); lights as descriptions -> (colours [n, 3],
        counters named like the project's)"""
        rec, _ = self.object_try_trace(obj, rays)
        bg = v3(background)
        hit = rec[:, 14].view(np.int32) != 0
        cnt = {"rays_primary": len(rec), "hits_primary": int(hit.sum()), "rays_shadow": 0, "hits_shadow": 0}
        out = np.tile(bg, (len(rec), 1))
        h = rec[hit]
        light = np.tile(bg, (len(h), 1))                    # :12
        with np.errstate(all="ignore"):
            for l in lights:
                where, colour = v3(l.args[0]), v3(l.args[1])
                shadow = h[:, 0:8].copy()
                if l.kind == "directional":                 # SdfLight.fs:6-21
                    towards = np.tile(normalize((F(0) - where)[None, :]), (len(h), 1))
                    shadow[:, 3:6], shadow[:, 6] = towards, F(1000)
                    gives = np.tile(colour, (len(h), 1))
                else:                                       # SdfLight.fs:23-42
                    diff = where - h[:, 0:3]
                    towards = normalize(diff)               # :25, at result.Position
                    d2 = length2(diff)
                    shadow[:, 3:6], shadow[:, 6] = over(diff, d2), np.sqrt(d2)
                    gives = colour[None, :] / d2[:, None]
                cos = dot(h[:, 8:11], towards)              # SdfScene.fs:15
                lit = np.flatnonzero(cos > 0)               # :17
                blocked = self.object_try_trace(obj, shadow[lit])[0][:, 14].view(np.int32) != 0
                cnt["rays_shadow"] += len(lit)
                cnt["hits_shadow"] += int(blocked.sum())
                free = lit[~blocked]
                light[free] = light[free] + times(gives[free], cos[free])                  # :23
            out[hit] = h[:, 11:14] * (light * (F(1) / F(np.pi)))                           # :28, MathF.piInv = 1f / MathF.PI
        cnt["flags"] = self.flags
        return out.astype(F), cnt

    def pixel_rays(self, cam12, W, H, eps, length_):
        """the rays of Image.render (Image.fs:17-34, Camera.fs:44-54), column by column; cam12 = Position, Forward, UpScaled, RightScaled"""
        c = np.asarray(cam12, F)
        pos, fw, up, rt = c[0:3], c[3:6], c[6:9], c[9:12]
        m = F(max(W, H))
        xs, ys = np.meshgrid(np.arange(W, dtype=F), np.arange(H, dtype=F), indexing="ij")
        px, py = (xs / m).reshape(-1), (ys / m).reshape(-1)
        with np.errstate(all="ignore"):
            d = normalize((fw + times(rt, px - F(0.5))) + times(up, py - F(0.5)))
        n = len(d)
        return np.concatenate([np.tile(pos, (n, 1)), d, np.full((n, 1), length_, F), np.full((n, 1), eps, F)], axis=1).astype(F)

    def render(self, obj, background, lights, cam12, W, H, eps, length_):
        rgb, cnt = self.trace(obj, background, lights, self.pixel_rays(cam12, W, H, eps, length_))
        return rgb.reshape(W, H, 3), cnt


def all_forms(node, out=None, seen=None):
    """every Form description under a node, children before parents"""
    out, seen = ([], set()) if out is None else (out, seen)
    if id(node) in seen:
        return out
    seen.add(id(node))
    for k in node.kids:
        all_forms(k, out, seen)
    if type(node).__name__ == "Form":
        out.append(node)
    return out
