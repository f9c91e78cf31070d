"""Scenes, cameras and rays on which a ray is born with Length <= 0 where it matters: shared by the oracle's known answers
(tests/test_oracle_kat.py) and the GPU parity tests (tests/test_gpu_ray_length_edges.py).

The reference tests a ray's Length before it evaluates anything (SdfForm.fs:94-95, then :97), so an occlusion ray of ao_radius <= 0 and a
shadow ray of Length 0 are open whatever the distance at their origin is.  That only shows where the distance at the pulled-back hit position
is below epsilon — there a ray that does evaluate hits at once.  From a camera outside the scene that is rare; it holds on every pixel for a
camera inside a body, and on many for a camera in a carved cavity that looks at concave walls.  Everything here is chosen with the CPU oracle alone."""
import numpy as np

from fraytracer_amd import Camera, Lens, SdfForm, SdfLight, SdfMaterial, SdfObject, SdfScene
from fraytracer_amd import synthetic as syn

F = np.float32
EPS, LEN = syn.EPSILON, syn.RAY_LENGTH
W, H = 48, 40
LOOK_AT = (0.3, 0.2, 5.0)
CAVITY = (-0.5, 1.0, -2.0)                        # the centre of console_scene's subtracted sphere (Program.fs:74)


def camera_at(pos):
    return Camera.lookAt(Position=tuple(float(v) for v in pos), LookAt=LOOK_AT, Up=(0.0, 1.0, 0.0), Lens=Lens.create(60.0))


def interior_points(oracle, scene, seed, depth, count=1, radius=4.0, n=3000):
    """up to `count` points, in sample order, of a seeded sample of the cube of half-width `radius` at which the oracle's distance is below -depth"""
    O = oracle.Oracle()
    form = O.object_form(O.scene(scene).object)
    pts = (np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3)) * radius).astype(F)
    d = O.form_distance(form, pts)
    inside = pts[d < F(-depth)]
    assert len(inside) >= 1
    return [tuple(float(v) for v in p) for p in inside[:count]]


def interior_cameras(oracle, scene, seed, depth, count=1, **ext):
    """cameras at the first `count` interior points (interior_points) from which the oracle's frame with four occlusion rays of a subnormal radius
    differs from its frame without occlusion rays on at least 100 pixels: there an occlusion ray that evaluates at all hits at once, so whether a
    ray of radius <= 0 evaluates decides the pixel.  (A camera inside a glass body fails this: its paths leave the body and hit solids from outside.)"""
    os_ = oracle.Oracle().scene(scene)
    cams = []
    for p in interior_points(oracle, scene, seed, depth, count=12 * count):
        cam = camera_at(p)
        plain, _ = os_.render(EPS, LEN, W, H, cam.as_array(), **ext)
        tiny, _ = os_.render(EPS, LEN, W, H, cam.as_array(), ao_samples=4, ao_radius=1e-40, **ext)
        if (plain.view(np.uint32) != tiny.view(np.uint32)).any(-1).sum() >= 100:
            cams.append(cam)
            if len(cams) == count:
                return cams
    raise AssertionError("no interior camera found")


def pixel_rays(oracle, cam, w=W, h=H, eps=EPS, length=LEN):
    """the camera rays of a w x h frame, column by column (Image.fs:26-35)"""
    c = cam.as_array()
    return np.stack([oracle.pixel_ray(c, w, h, x, y, eps, length) for x in range(w) for y in range(h)])


def cached_distance(oracle, scene, rays):
    """per ray: (hit, the oracle's distance at the record's origin — the pulled-back hit position, where every secondary ray of that hit is born
    and whose distance the kernels keep from the normal's centre probe); shapes [n]"""
    O = oracle.Oracle()
    os_ = O.scene(scene)
    rec, _ = os_.object_try_trace(rays)
    hit = rec[:, 14].view(np.int32) == 1
    d = O.form_distance(O.object_form(os_.object), rec[:, 0:3])
    return hit, d


def self_hitting(oracle, scene, cam, w=W, h=H):
    """bool [w, h]: pixels that hit and whose cached distance is below epsilon — where a secondary ray that evaluates at all hits at once"""
    hit, d = cached_distance(oracle, scene, pixel_rays(oracle, cam, w, h))
    return (hit & (d < F(EPS))).reshape(w, h), hit.reshape(w, h)


def assert_not_vacuous(oracle, scene, cam, w=W, h=H):
    """at least 100 hit pixels, and at least 10 % of the hit pixels, have a cached distance below epsilon"""
    near, hit = self_hitting(oracle, scene, cam, w, h)
    assert near.sum() >= 100 and near.sum() * 10 >= hit.sum(), (int(near.sum()), int(hit.sum()))
    return near, hit


# ---- one scene per kernel family, each with a camera where the cached distance is below epsilon on many pixels -----------------------------------
def lean(oracle, count=1):
    """C3 (a smooth union of spheres), the camera inside the blob -> (scene, cameras, extension arguments)"""
    scene = syn.config3(n=64, size=W)[0]
    return scene, interior_cameras(oracle, scene, 1, 0.15, count), {}


def cavity(oracle=None, count=1):
    """the reference's own structure, the camera at the centre of the sphere it subtracts, looking at the concave walls"""
    assert count == 1
    return syn.console_scene(n=150, size=W)[0], [camera_at(CAVITY)], {}


def general(oracle, count=1):
    """every combinator and primitive nested (the general interpreter), the camera inside a body"""
    scene = syn.mixed_nested()[0]
    return scene, interior_cameras(oracle, scene, 1, 0.03, count), {}


def calls(oracle, count=1):
    """a union of combinator objects (on-demand sub-programs), the camera inside one of them"""
    scene = syn.combinator_crowd(n=60, size=W)[0]
    return scene, interior_cameras(oracle, scene, 2, 0.03, count), {}


def glass(oracle, count=1):
    """config 5 traced as paths (max_bounces = 4: Scene_trace_path shades through the same code), the camera inside a solid body"""
    scene = syn.config5(size=W)[0]
    return scene, interior_cameras(oracle, scene, 1, 0.03, count, max_bounces=4), dict(max_bounces=4)


FAMILIES = {"lean": lean, "cavity": cavity, "general": general, "calls": calls, "glass": glass}


# ---- the shadow ray of Length 0 ---------------------------------------------------------------------------------------------------------------------
# The ray starts at (0,0,0), ON sphere((0,0,1), 1): its first evaluation is a hit.  Its direction has length 1.7e-28, so the pull-back by epsilon
# (SdfObject.fs:66-78) moves the origin to exactly (1e-30, 1e-30, -1e-30).  A point light 3e-30 from there has distance2 = 9e-60 -> 0 in float32:
# direction diff / 0 = (+inf, +inf, -inf), cosine +inf > 0, so a shadow ray IS cast, with Length sqrt(0) = 0 (SdfLight.fs:27-37).
SHADOW_RAY = np.array([0, 0, 0, -1e-28, -1e-28, 1e-28, 30, 0.01], F)
SHADOW_ORIGIN = np.array([1e-30, 1e-30, -1e-30], F)
LIGHT_ZERO_LENGTH = ((2e-30, 3e-30, -3e-30), (1.0, 2.0, 3.0))      # cosine +inf: one shadow ray of Length 0, which misses: colour inf
LIGHT_CONTROL = ((2e-30, 3e-30, 3e-30), (1.0, 2.0, 3.0))           # cosine inf - inf = NaN, not > 0: no shadow ray, the unlit colour


def _the_sphere():
    return SdfObject.create(SdfMaterial.createSolid((0.8, 0.8, 0.8)), SdfForm.Primitive.sphere((0.0, 0.0, 1.0), 1.0))


def _solid(rgb, form):
    return SdfObject.create(SdfMaterial.createSolid(rgb), form)


def shadow_objects():
    """name -> scene.Object: the sphere alone and next to far bodies of each non-SHADE kernel family"""
    P = SdfForm.Primitive
    far = [_solid((0.2, 0.9, 0.1), P.sphere((20.0, 0.0, 5.0), 1.0)), _solid((0.1, 0.2, 0.9), P.torus((0.0, 25.0, 3.0), (0.0, 1.0, 0.0), 1.0, 0.3)),
           _solid((0.9, 0.2, 0.1), P.capsule((-22.0, 0.0, 4.0), (-22.0, 3.0, 4.0), 0.5))]
    blob = SdfForm.unionSmooth(0.25, [P.sphere((0.0, 0.0, 1.0), 1.0), P.sphere((0.0, 20.0, 1.0), 1.0)])
    def carved(k):                                # carved spheres on a ring of radius 20 around the z axis
        x, y = 20.0 * np.cos(0.7 * k), 20.0 * np.sin(0.7 * k)
        return SdfObject.subtract(_solid((0.3, 0.3, 0.9), P.sphere((x, y, 4.0), 2.0)), P.sphere((x, y, 2.5), 1.0))
    return {"sphere alone": _the_sphere(),
            "union with far primitives": SdfObject.union([_the_sphere()] + far),
            "unionSmooth with a far sphere": _solid((0.8, 0.8, 0.8), blob),
            "beside a combinator child": SdfObject.union([_the_sphere(), carved(0), far[0]]),
            "beside nine combinator children": SdfObject.union([_the_sphere()] + [carved(k) for k in range(9)])}


def shadow_scene(obj, light):
    return SdfScene(obj, syn.BACKGROUND, [SdfLight.point(*light)])


def shadow_buffer(n_edge=64, n_plain=37, seed=4):
    """(rays, index of the edge rays): a whole wave of the Length-0 construction, then a wave that mixes it with ordinary rays"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-3.0, 3.0, (n_plain, 3)) + np.array([0.0, 0.0, -6.0])
    t = rng.uniform(-0.8, 0.8, (n_plain, 3)) + np.array([0.0, 0.0, 1.0])
    d = (t - o) / np.linalg.norm(t - o, axis=1, keepdims=True)
    plain = np.concatenate([o, d, np.full((n_plain, 1), 30.0), np.full((n_plain, 1), 0.01)], axis=1).astype(F)
    tail = np.empty((2 * n_plain, 8), F)
    tail[0::2] = plain
    tail[1::2] = SHADOW_RAY
    rays = np.ascontiguousarray(np.concatenate([np.tile(SHADOW_RAY, (n_edge, 1)), tail]))
    edge = np.concatenate([np.arange(n_edge), n_edge + 1 + 2 * np.arange(n_plain)])
    return rays, edge
