"""Scenes, points and rays at the edges of the flatten-time gates of the fast sphere arithmetic: shared by the CPU classification and float64
tests (tests/test_fast_gates_host.py) and the GPU parity tests (tests/test_gpu_fast_gates.py).

The gates (scene.cpp fastSphereRun, noteUnionChild, carvedShape's fastSphere): strength > 0, 2^-20 <= a = |1 / strength| <= 32,
every parameter finite, |c|inf <= 1e4, 2^-20 <= r <= 1e4, r a <= 80, and the staged constants end within FT_MAX_STAGE_FLOATS (3072 spheres).  Each
lean scene here meets one gate exactly and every other gate with room to spare; its twin moves that one value one float32 step outside.  The
kernels guard per evaluation and per wave (fast_point_ok: |p|inf < 20000; near_point_ok: |p|^2 <= nearR2), so every point family is laid out in
blocks of 64 consecutive points: one wave of ft_sample_points and ft_eval_points.  Cameras, lights and seeds are chosen with the CPU oracle alone."""
import functools

import numpy as np

from fraytracer_amd import Camera, Lens, SdfForm, SdfLight, SdfMaterial, SdfObject, SdfScene
from fraytracer_amd import synthetic as syn

F = np.float32
P = SdfForm.Primitive
W, H = 32, 24
LEN = 30.0
CORNER = (1.0e4, -1.0e4, 1.0e4)                   # |c|inf at its gate on every axis
FAR = (9994.0, -9994.0, 9994.0)                   # the cluster that sits wholly at |c| about 1e4
R_MIN, R_MAX, C_MAX, P_MAX = 2.0 ** -20, 1.0e4, 1.0e4, 20000.0
STAGE_SPHERES = 3072                              # FT_MAX_STAGE_FLOATS / 4
MAT = (0.9, 0.6, 0.3)


def above(v):
    return float(np.nextafter(F(v), F(np.inf)))


def below(v):
    return float(np.nextafter(F(v), F(-np.inf)))


def cluster(seed, n, centre, spread, rlo, rhi):
    """n spheres (x, y, z, r), float32: centres uniform in the ball of radius `spread` around `centre`, radii uniform in [rlo, rhi]"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v *= (spread * rng.uniform(0.0, 1.0, (n, 1)) ** (1.0 / 3.0)) / np.linalg.norm(v, axis=1, keepdims=True)
    return np.concatenate([np.asarray(centre, np.float64) + v, rng.uniform(rlo, rhi, (n, 1))], axis=1).astype(F)


def with_sphere(spheres, c, r):
    return np.concatenate([spheres, np.array([[c[0], c[1], c[2], r]], F)]).astype(F)


class Blob:
    """one smooth union of spheres: `spheres` float32 [n, 4], `focus` the point cameras and rays aim at, `eps` the rays' Epsilon"""

    def __init__(self, strength, spheres, focus=(0.0, 0.0, 0.0), eps=0.01):
        self.strength, self.spheres, self.eps = float(F(strength)), np.ascontiguousarray(spheres, F), eps
        self.convex = self.strength >= 1.0e5
        self.focus = np.asarray(focus, np.float64)

    @property
    def a(self):
        """|strengthInverse| as scene.cpp forms it: -1.0f / strength in float32"""
        return float(abs(F(-1.0) / F(self.strength)))

    def form(self):
        return SdfForm.unionSmooth(self.strength, [P.sphere(tuple(float(v) for v in s[:3]), float(s[3])) for s in self.spheres])

    def object(self):
        return SdfObject.create(SdfMaterial.createSolid(MAT), self.form())

    def scene(self, lights=()):
        return SdfScene(self.object(), syn.BACKGROUND, list(lights))

    def near_radius(self):
        """scene.cpp's stated rule: nearR = 86 / a - max|c| - 1e-3 (1 + max|c|), in double; <= 0: no near region"""
        c = self.spheres[:, :3].astype(np.float64)
        max_c = float(np.sqrt((c * c).sum(axis=1)).max())
        return 86.0 / self.a - max_c - 1e-3 * (1.0 + max_c)

    def exact(self, pts):
        """float64: (-s ln sum exp(t_i), sum exp(t_i), max |t_i|) with t_i = -(|c_i - p| - r_i) / s, per point"""
        p = np.asarray(pts, np.float64).reshape(-1, 1, 3)
        c, r = self.spheres[None, :, :3].astype(np.float64), self.spheres[None, :, 3].astype(np.float64)
        s = float(self.strength)
        with np.errstate(all="ignore"):
            t = -(np.sqrt(((c - p) ** 2).sum(axis=2)) - r) / s
            total = np.exp(t).sum(axis=1)
            return -s * np.log(total), total, np.abs(t).max(axis=1), t.max(axis=1)


# ---- lean gate scenes: name -> (inside, outside or None) ---------------------------------------------------------------------------------------------
def _base():
    """13 spheres with centres within 0.95 of the origin: two lobes of six (r = 0.25) above and below it, so that the body has a waist and one
    lobe can shadow the other, and one sphere exactly at the origin"""
    lobes = np.concatenate([cluster(1, 6, (0.0, 0.62, 0.0), 0.3, 0.25, 0.25), cluster(2, 6, (0.1, -0.62, 0.0), 0.3, 0.25, 0.25)])
    return with_sphere(lobes, (0.0, 0.0, 0.0), 0.125)


def _off_centre():
    """12 small spheres in two lobes next to (0, 0.9, 0): every centre is about max|c| from the origin on the same side, so at the antipode of the
    near shell every child is as far as the rule behind nearR allows and every term of the sum is near exp(-86) at once"""
    return np.concatenate([cluster(3, 6, (0.12, 0.9, 0.0), 0.03, 0.04, 0.04), cluster(4, 6, (-0.12, 0.9, 0.0), 0.03, 0.04, 0.04)])


def _far_cluster(corner, tiny):
    s = cluster(7, 14, FAR, 4.0, 0.6, 1.6)
    return with_sphere(with_sphere(s, corner, 1.5), (9995.0, -9993.5, 9992.0), tiny)


@functools.lru_cache(maxsize=None)
def lean_gates():
    base = _base()
    ground = (0.0, -1.0e4, 0.0)                   # a sphere of r = 1e4 whose surface passes through the origin
    corner_out = (above(C_MAX), CORNER[1], CORNER[2])
    return {
        "a = 32": (Blob(2.0 ** -5, base), Blob(below(2.0 ** -5), base)),
        "a = 32, off centre": (Blob(2.0 ** -5, _off_centre(), (0.0, 0.9, 0.0)), Blob(below(2.0 ** -5), _off_centre(), (0.0, 0.9, 0.0))),
        "a = 2^-20": (Blob(2.0 ** 20, base), Blob(above(2.0 ** 20), base)),
        "r a = 80 at a = 32": (Blob(2.0 ** -5, with_sphere(base, (0.9, -0.2, 0.1), 2.5)), Blob(2.0 ** -5, with_sphere(base, (0.9, -0.2, 0.1), above(2.5)))),
        "r a = 80 at r = 1e4": (Blob(125.0, with_sphere(base, ground, R_MAX)), Blob(125.0, with_sphere(base, ground, above(R_MAX)))),
        "r = 2^-20": (Blob(0.25, with_sphere(base, (0.4, 0.9, -0.3), R_MIN)), Blob(0.25, with_sphere(base, (0.4, 0.9, -0.3), below(R_MIN)))),
        "|c| = 1e4": (Blob(0.25, with_sphere(base, CORNER, 0.5)), Blob(0.25, with_sphere(base, corner_out, 0.5))),
        "near control": (Blob(0.25, base), None),
        "cluster at 1e4": (Blob(0.5, _far_cluster(CORNER, R_MIN), FAR, 0.03), Blob(0.5, _far_cluster((CORNER[0], below(-C_MAX), CORNER[2]), R_MIN), FAR, 0.03)),
    }


LEAN_NAMES = ["a = 32", "a = 32, off centre", "a = 2^-20", "r a = 80 at a = 32", "r a = 80 at r = 1e4", "r = 2^-20", "|c| = 1e4", "near control", "cluster at 1e4"]
NEAR_SCENES = ["a = 32", "a = 32, off centre", "r a = 80 at a = 32", "near control"]          # all centres within 1.0 of the origin: a near region exists
GLIBC_SCENES = ["r a = 80 at a = 32", "a = 32, off centre", "cluster at 1e4"]


def lean_cases():
    """(name, side) of every lean gate scene"""
    return [(n, side) for n in LEAN_NAMES for side in ("inside", "outside") if side == "inside" or lean_gates()[n][1] is not None]


def lean_blob(name, side):
    return lean_gates()[name][0 if side == "inside" else 1]


# ---- stage scenes ------------------------------------------------------------------------------------------------------------------------------------
def _many(seed, n):
    """a cloud sparse enough to stay lumpy under strength 0.25: its bumps shadow each other"""
    return cluster(seed, n, (0.0, 0.0, 0.0), 7.0, 0.05, 0.3)


def stage_camera():
    """far enough for the cloud to leave the frame's corners empty, near enough for the distance to be finite (86 s = 21.5 off the surface)"""
    return Camera.lookAt(Position=(0.0, 0.0, -22.0), LookAt=(0.0, 0.0, 0.0), Up=(0.0, 1.0, 0.0), Lens=Lens.create(60.0))


def stage_rays(oracle, os_, n=8):
    """n pixel rays of the 24 x 16 frame of stage_camera, taken in pixel order by turns from the misses, the hits with a shadowed light and the
    other hits (the oracle's counters of each ray alone)"""
    c = stage_camera().as_array()
    rays = np.stack([oracle.pixel_ray(c, 24, 16, x, y, 0.01, LEN) for x in range(24) for y in range(16)])
    kinds = {0: [], 1: [], 2: []}
    for r in rays:
        cnt = os_.trace_rays(r[None])[1]
        kinds[0 if cnt["hits_primary"] == 0 else 1 if cnt["hits_shadow"] >= 1 else 2].append(r)
        if all(3 * len(v) >= n for v in kinds.values()):
            break
    picked = [kinds[k % 3][k // 3] for k in range(n)]
    return np.ascontiguousarray(np.stack(picked), F)


@functools.lru_cache(maxsize=None)
def stage_blobs():
    """name -> list of Blobs whose union (one Blob: the blob itself) is the scene's object"""
    return {"3072": [Blob(0.25, _many(11, STAGE_SPHERES))], "3073": [Blob(0.25, _many(11, STAGE_SPHERES + 1))],
            "2000 + 1100": [Blob(0.25, _many(12, 2000)), Blob(0.25, _many(13, 1100))],
            "40 + 3072": [Blob(0.25, _many(14, 40)), Blob(0.25, _many(11, STAGE_SPHERES))],
            "3072 + 40": [Blob(0.25, _many(11, STAGE_SPHERES)), Blob(0.25, _many(14, 40))]}


STAGE_NAMES = ["3072", "3073", "2000 + 1100", "40 + 3072", "3072 + 40"]
# info() of the stage scenes, as the flattener states them: (fast_path, cull_pc, n_consts or None, n_slots or None)
STAGE_INFO = {"3072": (1, 0, 12352, None), "3073": (0, -1, None, None), "2000 + 1100": (0, 0, 12464, 3), "40 + 3072": (0, 0, None, 3), "3072 + 40": (0, 0, None, 3)}


def stage_scene(name, lights=None):
    blobs = stage_blobs()[name]
    lights = default_lights() if lights is None else lights
    if len(blobs) == 1:
        return blobs[0].scene(lights)
    return SdfScene(SdfObject.union([b.object() for b in blobs]), syn.BACKGROUND, list(lights))


def default_lights():
    """around the origin the reference's own lights are close by (Program.fs:79-82)"""
    return syn.program_lights()


# ---- union and carved gate scenes ----------------------------------------------------------------------------------------------------------------------
def _solid(k, form):
    return SdfObject.create(SdfMaterial.createSolid((0.2 + 0.01 * (k % 60), 0.9 - 0.01 * (k % 50), 0.3 + 0.01 * (k % 40))), form)


def _prims(kind, spheres):
    """one primitive of `kind` per (c, r) row: the sphere itself, a capsule from c, a torus at c"""
    out = []
    for k, s in enumerate(spheres):
        c, r = tuple(float(v) for v in s[:3]), float(s[3])
        if kind == "sphere":
            out.append(P.sphere(c, r))
        elif kind == "capsule":                   # From = c: a gate value of c is a gate value of the capsule; To steps towards the origin
            to = tuple(float(F(v) - F(np.sign(v)) * F(0.5 + 0.01 * (k % 7))) if v != 0.0 else 0.25 for v in c)
            out.append(P.capsule(c, to, r))
        else:                                     # minor radius r (a gate value of r is one of the torus), major radius 2 r
            n = np.array([0.3 + 0.1 * (k % 5), 1.0, -0.2 * (k % 3)]); n /= np.linalg.norm(n)
            out.append(P.torus(c, tuple(float(v) for v in n), float(F(r) * F(2.0)), r))
    return out


def _union_rows(where):
    if where == "corner":                         # about 60 bodies around FAR, one centre exactly at the corner, one radius at 2^-20
        rows = with_sphere(with_sphere(cluster(21, 58, FAR, 4.0, 0.3, 1.0), CORNER, 1.0), (9993.0, -9995.0, 9996.5), R_MIN)
        return rows, len(rows) - 2, len(rows) - 1
    # around the origin, on a ground sphere of r = 1e4.  16 bodies, not 60: the reference's grid has ceil(width / (1.5 mean radius)) cells per axis,
    # and one radius of 1e4 among 60 makes that 80^3 cells with every child in each
    rows = cluster(22, 15, (0.0, 2.0, 0.0), 4.0, 0.3, 1.0)
    rows = with_sphere(rows, (0.0, -1.0e4, 0.0), R_MAX)
    return rows, None, len(rows) - 1


@functools.lru_cache(maxsize=None)
def union_gates():
    """name -> dict(scene pieces): the union's forms at the gate, its twin with one value one step outside, the carve's tail spheres at the gate
    and one step outside, focus and epsilon.  Kinds: sphere, capsule, torus; places: corner (|c| about 1e4) and origin (r = 1e4)."""
    out = {}
    for kind in ("sphere", "capsule", "torus"):
        for where in ("corner", "origin"):
            if where == "origin" and kind == "torus":
                continue                          # a torus of major radius 1e4 has a bounding radius beyond the gate: no inside scene exists
            rows, at_c, at_r = _union_rows(where)
            twin = rows.copy()
            if where == "corner":
                twin[at_c, 0] = above(C_MAX)      # one coordinate of one centre
                focus, eps = FAR, 0.03
                tail = ((CORNER, 12.0), ((9994.5, -9993.0, 9995.0), R_MIN))                # intersect with a sphere centred at the gate, subtract one of r at the gate
                tail_out = (((above(C_MAX), CORNER[1], CORNER[2]), 12.0), ((9994.5, -9993.0, 9995.0), below(R_MIN)))
            else:
                twin[at_r, 3] = above(R_MAX)
                focus, eps = (0.0, 2.0, 0.0), 0.01
                tail = (((0.0, 0.0, 0.0), R_MAX), ((0.5, 2.5, -1.0), 1.5))
                tail_out = (((0.0, 0.0, 0.0), above(R_MAX)), ((0.5, 2.5, -1.0), 1.5))
            out[f"{PLURAL[kind]} at the {where}"] = dict(kind=kind, rows=rows, twin=twin, tail=tail, tail_out=tail_out, focus=np.asarray(focus, np.float64), eps=eps)
    return out


PLURAL = {"sphere": "spheres", "capsule": "capsules", "torus": "tori"}
UNION_NAMES = ["spheres at the corner", "spheres at the origin", "capsules at the corner", "capsules at the origin", "tori at the corner"]
UNION_VARIANTS = ["plain", "plain twin", "carved", "carved twin", "carved, tail outside"]


def union_object(name, variant):
    g = union_gates()[name]
    rows = g["twin"] if "twin" in variant else g["rows"]
    union = SdfObject.union([_solid(k, f) for k, f in enumerate(_prims(g["kind"], rows))])
    if variant.startswith("plain"):
        return union
    (ic, ir), (sc, sr) = g["tail_out"] if variant.endswith("tail outside") else g["tail"]
    return SdfObject.subtract(SdfObject.intersect(union, [P.sphere(ic, ir)]), P.sphere(sc, sr))


def union_centres(name, variant):
    """the special points of the union's primitives: centres, end points (float32 [m, 3])"""
    g = union_gates()[name]
    rows = g["twin"] if "twin" in variant else g["rows"]
    pts = []
    for f in _prims(g["kind"], rows):
        pts += [f.args[0]] if f.kind != "capsule" else [f.args[0], f.args[1]]
    return np.array(pts, F)


# ---- cameras and lights, chosen with the oracle alone ------------------------------------------------------------------------------------------------------
def surface_point(O, form, focus):
    """where the form's distance changes sign on the line from `focus` towards -z (float64 bisection on the oracle's values); `focus` if it never does"""
    radii = np.concatenate([[0.0], np.geomspace(1e-2, 1e8, 81)])
    pts = focus + np.outer(radii, [0.0, 0.0, -1.0])
    with np.errstate(all="ignore"):
        d = O.form_distance(form, pts.astype(F))
    neg = np.nonzero(d < 0)[0]
    if len(neg) == 0 or neg[-1] + 1 >= len(radii):
        return focus.copy()
    lo, hi = radii[neg[-1]], radii[neg[-1] + 1]
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        with np.errstate(all="ignore"):
            inside = O.form_distance(form, (focus + mid * np.array([0.0, 0.0, -1.0])).astype(F)[None])[0] < 0
        lo, hi = (mid, hi) if inside else (lo, mid)
    return focus + hi * np.array([0.0, 0.0, -1.0])


LIGHT_OFFSETS = ((3.0, 4.0, -5.0), (0.2, 4.0, 0.7), (0.2, 2.0, 0.5), (2.0, 0.1, 0.2))


def lights_at(s, offset=LIGHT_OFFSETS[0]):
    """one directional light and a point light within 10 of the surface point `s`: never the reference's point light at the origin, whose shadow ray
    from 17 000 away has |dir| = 1 / distance and ends on the step cap"""
    return [SdfLight.directional((-0.5, -1.0, 1.0), (0.5, 0.5, 0.5)), SdfLight.point(tuple(float(F(v)) for v in s + np.array(offset)), (10.0, 0.0, 0.0))]


def frame_is_telling(cnt, rays, convex=False):
    """the condition on every frame and ray buffer, from the oracle's counters alone.  convex: the body is a ball (a = 2^-20 melts everything within
    1e4 into one ball of radius 2.6e6), on which no point that faces a light is shadowed: hits and misses are all that can be asked for"""
    if cnt["flags"] != 0 or not 0 < cnt["hits_primary"] < rays:
        return False
    return convex or (cnt["hits_shadow"] >= 1 and cnt["rays_shadow"] - cnt["hits_shadow"] >= 1)


def view_of(oracle, obj, focus, eps, w=W, h=H, convex=False):
    """(scene, camera, oracle scene, (frame, counters)): the first point light and camera of fixed lists, the camera at 1.5 to 20 off the surface point below `focus` and tilted
    by 0 to 80 degrees, whose oracle frame meets frame_is_telling; a 8 x 6 probe frame comes first, so a view that runs to the step cap costs little"""
    O = oracle.Oracle()
    bare = O.scene(SdfScene(obj, syn.BACKGROUND, []))
    s = surface_point(O, O.object_form(bare.object), np.asarray(focus, np.float64))
    for offset in LIGHT_OFFSETS:
        scene = SdfScene(obj, syn.BACKGROUND, lights_at(s, offset))
        os_ = O.scene(scene)
        for k in (10.0, 4.0, 2.5, 1.5, 20.0):
            for tilt in (0.0, 30.0, 45.0, 65.0, 80.0):
                pos = s + np.array([0.0, 0.0, -k])
                th = np.radians(tilt)
                look = pos + 10.0 * np.array([np.sin(th), 0.0, np.cos(th)])
                cam = Camera.lookAt(Position=tuple(float(F(v)) for v in pos), LookAt=tuple(float(F(v)) for v in look), Up=(0.0, 1.0, 0.0), Lens=Lens.create(60.0))
                with np.errstate(all="ignore"):
                    if os_.render(eps, LEN, 8, 6, cam.as_array())[1]["flags"] != 0:
                        continue
                    frame, cnt = os_.render(eps, LEN, w, h, cam.as_array())
                if frame_is_telling(cnt, w * h, convex):
                    frame.setflags(write=False)
                    return scene, cam, os_, (frame, cnt)
    raise AssertionError("no camera whose oracle frame has hits, misses, lit and shadowed points and no flag")


# ---- point families: float32 [64 k, 3] -----------------------------------------------------------------------------------------------------------------------
def blocks(pts, fill=None):
    """pad to whole blocks of 64 with `fill` (default: the first point)"""
    pts = np.asarray(pts, F).reshape(-1, 3)
    pad = (-len(pts)) % 64
    if pad:
        pts = np.concatenate([pts, np.tile(pts[:1] if fill is None else np.asarray(fill, F).reshape(1, 3), (pad, 1))])
    return np.ascontiguousarray(pts, F)


def centre_family(centres):
    """every centre; each with each coordinate one float32 step either way; each +- 1e-30 and +- 1e-12 where that changes the float"""
    c = np.asarray(centres, F).reshape(-1, 3)
    out = [c]
    for axis in range(3):
        for to in (np.inf, -np.inf):
            q = c.copy()
            q[:, axis] = np.nextafter(c[:, axis], F(to))
            out.append(q)
    for delta in (1e-30, -1e-30, 1e-12, -1e-12):
        q = (c + F(delta)).astype(F)
        out.append(q[(q != c).any(axis=1)])
    return blocks(np.concatenate(out)[:4032])


def _directions(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


SHELL = (0.9, 1.0 - 1e-4, 1.0 - 1e-6, 1.0, 1.0 + 1e-6, 1.0 + 1e-4, 1.03, 1.06, 1.1)
ANTIPODE = 64 * len(SHELL)                        # the last points of the shell family


def shell_family(near_r, centres, seed=3):
    """around the origin at radii near_r x SHELL: per factor two whole blocks; then blocks of 63 points at 0.9 near_r and one at a factor >= 1 in a
    lane that moves from block to block; then per factor one block within 0.05 rad of the antipode of the children's mean centre, where every
    child is farthest at once.  1.03 and 1.06 lie between the near radius and what a constant of 90 in place of 86 would make of it at a = 32."""
    rng = np.random.default_rng(seed)
    out = [near_r * f * _directions(rng, 128) for f in SHELL]
    lane = 0
    for f in SHELL[3:]:
        for _ in range(3):
            b = near_r * 0.9 * _directions(rng, 64)
            b[lane] = near_r * f * _directions(rng, 1)[0]
            lane = (lane + 23) % 64
            out.append(b)
    mean = np.asarray(centres, np.float64).mean(axis=0)
    anti = -mean / np.linalg.norm(mean) if np.linalg.norm(mean) > 0 else np.array([0.0, 0.0, 1.0])
    for f in SHELL:
        d = anti + 0.05 * rng.normal(size=(64, 3)) / np.sqrt(3.0)
        out.append(near_r * f * d / np.linalg.norm(d, axis=1, keepdims=True))
    return blocks(np.concatenate(out))


def ordinary_family(blob, boundary, n=1024, seed=4):
    """uniform in the form's boundary sphere; where that sphere is mostly empty space in which the distance is +inf (a far outlier among the
    children: fewer than 95 % of its points have a finite float64 value), uniform in the ball around the focus that holds the children near it"""
    rng = np.random.default_rng(seed)
    c, r = np.asarray(boundary[0:3], np.float64), float(boundary[3])
    u = _directions(rng, n) * rng.uniform(0.0, 1.0, (n, 1)) ** (1.0 / 3.0)
    pts = blocks(c + u * r)
    if blob is None or np.isfinite(blob.exact(pts)[0]).mean() >= 0.95:
        return pts
    d = np.linalg.norm(blob.spheres[:, :3].astype(np.float64) - blob.focus, axis=1)
    return blocks(blob.focus + u * (d + blob.spheres[:, 3])[d < 100.0].max())


def guard_family(ordinary, seed=5):
    """|p|inf at nextbelow(20000), 20000 and nextabove(20000) on each axis and sign: each alone in a block of otherwise ordinary points, in a lane
    that moves, and as a whole block (the other two coordinates ordinary)"""
    rng = np.random.default_rng(seed)
    out, lane = [], 0
    for v in (below(P_MAX), P_MAX, above(P_MAX)):
        for axis in range(3):
            for sign in (1.0, -1.0):
                alone = ordinary[rng.integers(0, len(ordinary), 64)].copy()
                alone[lane, axis] = sign * v
                lane = (lane + 29) % 64
                whole = ordinary[rng.integers(0, len(ordinary), 64)].copy()
                whole[:, axis] = sign * v
                out += [alone, whole]
    return blocks(np.concatenate(out))


FAR_T = (-122.0, -86.0)


def far_ring_family(blob, n=1024, seed=6):
    """points at which the nearest child's t = -a (|c - p| - r) lies in [-122, -86] (float64), uniform in t.  In [-104, -86] the terms are subnormal:
    the float32 exponential keeps them down to t = -103.97, so the sum is finite there.  Below -104 every term is flushed and the distance is
    +inf; the band is carried on to -122 so that both outcomes are well represented."""
    rng = np.random.default_rng(seed)
    a = blob.a
    c, r = blob.spheres[:, :3].astype(np.float64), blob.spheres[:, 3].astype(np.float64)
    keep, have = [], 0
    for _ in range(64):
        i = rng.integers(0, len(c), 4 * n)
        tau = rng.uniform(-FAR_T[1], -FAR_T[0], (4 * n, 1))
        cand = (c[i] + _directions(rng, 4 * n) * (r[i][:, None] + tau / a)).astype(F)
        t = blob.exact(cand)[3]
        keep.append(cand[(t >= FAR_T[0]) & (t <= FAR_T[1])])
        have += len(keep[-1])
        if have >= n:
            break
    pts = np.concatenate(keep)[:n]
    assert len(pts) == n, len(pts)
    return blocks(pts)


def lean_families(oracle, blob):
    """name -> points of every family the blob has (shell: only where a near region exists)"""
    O = oracle.Oracle()
    boundary = O.form_boundary(O.object_form(O.scene(blob.scene()).object))
    ordinary = ordinary_family(blob, boundary)
    fam = {"centres": centre_family(blob.spheres[:, :3]), "ordinary": ordinary, "guard": guard_family(ordinary), "far ring": far_ring_family(blob)}
    if blob.near_radius() > 0.0 and 86.0 / blob.a < 1e3:
        fam["shell"] = shell_family(blob.near_radius(), blob.spheres[:, :3])
    return fam


def assert_families_tell(oracle, blob, fam):
    """the conditions that keep a test from passing vacuously, from the oracle's values alone: at least 95 % of the centre, shell and ordinary points
    have a finite distance; of the far ring at least 20 % a finite one and at least 20 % +inf"""
    O = oracle.Oracle()
    form = O.object_form(O.scene(blob.scene()).object)
    for key, pts in fam.items():
        with np.errstate(all="ignore"):
            d = O.form_distance(form, pts)
        finite, inf = float(np.isfinite(d).mean()), float(np.isposinf(d).mean())
        if key == "far ring":
            assert finite >= 0.2 and inf >= 0.2, (key, finite, inf)
        elif key != "guard":
            assert finite >= 0.95, (key, finite)


# ---- ray buffers ---------------------------------------------------------------------------------------------------------------------------------------------
def rays_towards(points, focus, eps, scale=1.0):
    """rays born at `points`, aimed at `focus`: direction unit x scale, Length 30, Epsilon eps"""
    p = np.asarray(points, np.float64)
    d = np.asarray(focus, np.float64) - p
    n = np.linalg.norm(d, axis=1, keepdims=True)
    d = np.where(n > 0, d / np.where(n > 0, n, 1.0), [0.0, 0.0, 1.0]) * scale
    return np.ascontiguousarray(np.concatenate([p, d, np.full((len(p), 1), LEN), np.full((len(p), 1), eps)], axis=1), F)


def ray_buffer(oracle, families, focus, eps, cam):
    """the buffer of the lane evaluator (256 rays and more: one ray per lane): blocks of 64 rays born at the families' points — ordinary (unit),
    centres (x 0.9), the shell's antipode blocks where a shell exists (x 0.9), far ring (x 1.2), guard (unit), ordinary (unit) — then every 12th
    pixel ray of the scene's camera (view_of), so that lit and shadowed hits are among them"""
    parts = [(families["ordinary"][:64], 1.0), (np.resize(families["centres"][::2], (64, 3)), 0.9)]
    if "shell" in families:
        parts.append((np.resize(families["shell"][-ANTIPODE::9], (64, 3)), 0.9))
    parts += [(families["far ring"][:64], 1.2), (np.resize(guard_points(families), (64, 3)), 1.0), (families["ordinary"][64:128], 1.0)]
    return np.ascontiguousarray(np.concatenate([rays_towards(p, focus, eps, s) for p, s in parts] + [pixel_rays(oracle, cam, eps)[::12]]), F)


def pixel_rays(oracle, cam, eps):
    """the camera rays of the W x H frame, column by column"""
    c = cam.as_array()
    return np.stack([oracle.pixel_ray(c, W, H, x, y, eps, LEN) for x in range(W) for y in range(H)])


def guard_points(families):
    """the 18 points of the guard family's whole blocks, one per value (nextbelow(20000), 20000, nextabove(20000)), axis and sign, in that order"""
    return families["guard"][64::128]


def ray_packs(oracle, families, focus, eps, cam):
    """[(label, rays)]: the buffers of 1, 8 and 32 rays, which the packed latency evaluator takes whole (its regime is balloted over all rays of
    the pack).  Every family is born into every size:
    - one ray alone from each pool: a centre, the origin's neighbourhood of the shell inside and outside, the antipode, a guard point at each of the
      three values, the far ring, an ordinary point;
    - 8 and 32 rays dealt from the pools in turn (near, fast-only and exact rays in one pack);
    - 8 and 32 rays all on centres; where a shell exists, all inside it (the near regime for the whole pack);
    - 7 and 31 rays inside the shell plus one outside it, and 7 and 31 ordinary rays plus one at each guard value: exactly one ray of the pack
      fails near_point_ok or fast_point_ok, in a slot that moves;
    - 8 and 32 pixel rays of the scene's camera, so that the packs together hold lit and shadowed hits and misses.
    Directions point at `focus`, scaled by 1, 0.9 and 1.2 in turn."""
    pools = {"centre": families["centres"], "far ring": families["far ring"], "ordinary": families["ordinary"]}
    hot = guard_points(families)
    for k, v in enumerate(("below 20000", "at 20000", "above 20000")):
        pools["guard " + v] = hot[6 * k:6 * k + 6]
    if "shell" in families:
        sh, anti = families["shell"], families["shell"][-ANTIPODE:]
        n = len(SHELL)
        pools.update({"shell inside": sh[:128], "shell at 1": sh[128 * 3:128 * 4], "shell outside": sh[128 * (n - 1):128 * n],
                      "antipode inside": anti[64 * 3:64 * 4], "antipode outside": anti[64 * (n - 2):64 * (n - 1)]})        # factors 1 and 1.06
    scales = (1.0, 0.9, 1.2)

    def rays_of(points):
        points = np.asarray(points, F).reshape(-1, 3)
        return np.concatenate([rays_towards(points[i:i + 1], focus, eps, scales[i % 3]) for i in range(len(points))])

    def with_one(base, n, odd, slot):
        pts = np.asarray(base[:n], F).copy()
        pts[slot % n] = odd
        return pts

    packs = [("one ray: " + k, rays_of(v[len(v) // 3:len(v) // 3 + 1])) for k, v in pools.items()]
    names = list(pools)
    for n in (8, 32):
        packs.append((f"{n} rays dealt from every pool", rays_of([pools[names[i % len(names)]][(5 * i) % len(pools[names[i % len(names)]])] for i in range(n)])))
        packs.append((f"{n} rays on centres", rays_of(pools["centre"][:n])))
        for k, v in enumerate(("below 20000", "at 20000", "above 20000")):
            packs.append((f"{n - 1} ordinary rays and one {v}", rays_of(with_one(pools["ordinary"], n, pools["guard " + v][(k + n) % 6], 5 + 11 * k))))
        if "shell" in families:
            packs.append((f"{n} rays inside the shell", rays_of(pools["shell inside"][:n])))
            packs.append((f"{n - 1} rays inside the shell and one outside", rays_of(with_one(pools["shell inside"], n, pools["shell outside"][3], 13))))
            packs.append((f"{n - 1} rays inside the shell and one at the antipode outside", rays_of(with_one(pools["antipode inside"], n, pools["antipode outside"][7], 2))))
    px = pixel_rays(oracle, cam, eps)
    packs += [("8 pixel rays", px[40::96][:8]), ("32 pixel rays", px[7::24][:32])]
    return [(label, np.ascontiguousarray(r, F)) for label, r in packs]
