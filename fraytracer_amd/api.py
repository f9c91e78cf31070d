"""Host-side mirror of FrayTracer's scene-composition API (the reference is F#; no .NET toolchain
exists in the build image, so the host layer above the C ABI is written in Python — INTEGRATION.md
shows the F# binding a maintainer would add).

Names, argument order and behaviour follow the reference modules:

    SdfForm.Primitive.sphere/capsule/torus/triangle   src/FrayTracer/SdfForm.fs:117-268
    SdfForm.union/subtract/intersect/unionSmooth      src/FrayTracer/SdfForm.fs:14-91
    SdfMaterial.createSolid                           src/FrayTracer/SdfMaterial.fs:4-7
    SdfObject.create/union/subtract/intersect         src/FrayTracer/SdfObject.fs:6-64
    SdfLight.directional/point                        src/FrayTracer/SdfLight.fs:6-42
    SdfScene (record) / SdfScene.trace                src/FrayTracer/Types.fs:74-79, SdfScene.fs:7-28
    Lens.create / Camera.lookAt                       src/FrayTracer/Camera.fs:11-42
    ImageSize / Image.render                          src/FrayTracer/Image.fs:8-35

Scene values are immutable descriptions (the reference's goal "immutable scenes", README.md:8).
They are realised through libfraytracer_hip's constructor twins the first time they are rendered
on a device.  The same descriptions can be realised on any object offering the small backend
protocol below (tests realise them on the CPU oracle to compare results).
"""
import contextlib
import ctypes as C
import threading

import numpy as np

from . import _lib
from ._lib import lib, check, FrayTracerError


def _v3(v):
    x, y, z = (float(np.float32(c)) for c in v)
    return (x, y, z)


class FColor(tuple):
    """FColor.fs:8-33 — an RGB triple of float32."""

    @staticmethod
    def ofRGB(r, g, b):
        return FColor(_v3((r, g, b)))


# --------------------------------------------------------------------------------------------------
# descriptions
# --------------------------------------------------------------------------------------------------
class _Desc:
    __slots__ = ("kind", "args", "kids", "__weakref__")

    def __init__(self, kind, args=(), kids=()):
        object.__setattr__(self, "kind", kind)
        object.__setattr__(self, "args", tuple(args))
        object.__setattr__(self, "kids", tuple(kids))

    def __setattr__(self, *_):
        raise AttributeError("scene descriptions are immutable")

    def __repr__(self):
        return f"<{type(self).__name__} {self.kind} kids={len(self.kids)}>"


class Form(_Desc):
    pass


class Material(_Desc):
    pass


class Object(_Desc):
    pass


class Light(_Desc):
    pass


class SdfForm:
    class Primitive:
        @staticmethod
        def sphere(Center, Radius):
            return Form("sphere", (_v3(Center), float(np.float32(Radius))))

        @staticmethod
        def capsule(From, To, Radius):
            return Form("capsule", (_v3(From), _v3(To), float(np.float32(Radius))))

        @staticmethod
        def torus(Center, Normal, MajorRadius, MinorRadius):
            return Form("torus", (_v3(Center), _v3(Normal), float(np.float32(MajorRadius)), float(np.float32(MinorRadius))))

        @staticmethod
        def triangle(V1, V2, V3, Radius):
            return Form("triangle", (_v3(V1), _v3(V2), _v3(V3), float(np.float32(Radius))))

        @staticmethod
        def box(Center, HalfExtent):
            """EXTENSION — not in the reference (BASELINE.json config 2 asks for boxes)."""
            return Form("box", (_v3(Center), _v3(HalfExtent)))

    @staticmethod
    def union(forms):
        forms = list(forms)
        if not forms:
            raise ValueError("No SdfObjects given.")            # SdfForm.fs:16
        return forms[0] if len(forms) == 1 else Form("union", (), forms)

    @staticmethod
    def subtract(a, b):
        return Form("subtract", (), (a, b))

    @staticmethod
    def intersect(forms):
        forms = list(forms)
        if not forms:
            raise ValueError("No SdfObjects given.")            # SdfForm.fs:53
        return forms[0] if len(forms) == 1 else Form("intersect", (), forms)

    @staticmethod
    def unionSmooth(strength, forms):
        forms = list(forms)
        if not forms:
            raise ValueError("blub")                            # SdfForm.fs:71
        return forms[0] if len(forms) == 1 else Form("unionSmooth", (float(np.float32(strength)),), forms)

    @staticmethod
    def tryTrace(form, rays, device=None):
        """SdfForm.tryTrace (SdfForm.fs:93-104) over a ray buffer on the GPU, see form_try_trace"""
        return form_try_trace(form, rays, device)

    @staticmethod
    def distance(form, points, device=None):
        """sdf.Distance at points [n, 3] on the GPU -> float32 [n]"""
        return _form_scene(form, device).eval_distance(points)[0]

    @staticmethod
    def tryDistance(form, points, device=None):
        """SdfForm.tryDistance (SdfForm.fs:7-12): sdf.Distance where SdfBoundary.isInside (DistanceSquared(Center, p) <
        Radius * Radius, SdfBoundary.fs:56), NaN standing for ValueNone elsewhere"""
        F = np.float32
        pts = np.ascontiguousarray(points, dtype=F).reshape(-1, 3)
        ds = _form_scene(form, device)
        b = ds.boundary()
        d = pts - np.asarray(b[0:3], F)
        inside = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) < F(b[3]) * F(b[3])
        out = ds.eval_distance(pts)[0]
        out[~inside] = np.nan
        return out

    @staticmethod
    def normal(form, epsilon, points, device=None):
        """SdfForm.normal sdf epsilon position (SdfForm.fs:106-112) at points [..., 3] -> float32 [..., 3], the four evaluations and the
        normalisation on the GPU (DeviceScene.sample_points)"""
        return _form_scene(form, device).sample_points(points, normal_epsilon=epsilon, distance=False).normal

    @staticmethod
    def sample(form, origin, step, counts, normal_epsilon=None, bounded=False, device=None):
        """sdf.Distance (and SdfForm.normal, with normal_epsilon) on the lattice lattice_points(origin, step, counts), computed on the GPU ->
        FieldSamples with distance float32 [nx, ny, nz] and normal float32 [nx, ny, nz, 3] or None; bounded: SdfForm.tryDistance, NaN
        standing for ValueNone (DeviceScene.sample_lattice)"""
        return _form_scene(form, device).sample_lattice(origin, step, counts, normal_epsilon=normal_epsilon, bounded=bounded)

    @staticmethod
    def mesh(form, origin, step, counts, iso=0.0, normal_epsilon=None, device=None, refine=None, shells=False, keep=None, measures=False):
        """the surface sdf.Distance = iso as triangles, extracted on the GPU from the lattice lattice_points(origin, step, counts) -> Mesh, with
        SdfForm.normal per vertex where normal_epsilon is given; refine: bisection rounds that move the vertices onto the surface
        (DeviceScene.mesh_lattice); shells, keep, measures: label the mesh's shells, keep some of them, measure them (DeviceScene.mesh_lattice)"""
        return _form_scene(form, device).mesh_lattice(origin, step, counts, iso=iso, normal_epsilon=normal_epsilon, refine=refine, shells=shells, keep=keep, measures=measures)

    @staticmethod
    def slice(form, origin, step, counts, axis=2, iso=0.0, normal_epsilon=None, device=None, refine=None, measures=False):
        """the contours sdf.Distance = iso of every lattice plane normal to `axis`, extracted and chained on the GPU from the lattice
        lattice_points(origin, step, counts) -> Contours, with SdfForm.normal per point where normal_epsilon is given; refine: bisection rounds
        that move the points onto the surface; measures: measure the polylines and the slices (DeviceScene.slice_lattice)"""
        return _form_scene(form, device).slice_lattice(origin, step, counts, axis=axis, iso=iso, normal_epsilon=normal_epsilon, refine=refine, measures=measures)

    @staticmethod
    def crossings(form, a, b, iso=0.0, steps=8, device=None):
        """where the segments from a [..., 3] to b [..., 3] cross sdf.Distance = iso, by bisection on the GPU -> (points float32 [..., 3], status
        int32 [...]; status 0: no bracket, the point is NaN) (DeviceScene.refine_segments)"""
        return _form_scene(form, device).refine_segments(a, b, iso=iso, steps=steps)

    @staticmethod
    def normalFromRay(form, rays, device=None):
        """SdfForm.normalFromRay (SdfForm.fs:106-115) at the position of each ray [n, 8] -> float32 [n, 3]: forward
        differences with h = Epsilon / 8 at Ray.get(-Epsilon), evaluated on the GPU"""
        F = np.float32
        r = np.ascontiguousarray(rays, dtype=F).reshape(-1, 8)
        p = r[:, 0:3] + r[:, 3:6] * (-r[:, 7:8])
        h = r[:, 7] * F(0.125)
        probes = np.repeat(p[:, None, :], 4, axis=1)
        for k in range(3):
            probes[:, k, k] = p[:, k] + h
        d = _form_scene(form, device).eval_distance(probes.reshape(-1, 3))[0].reshape(-1, 4)
        g = d[:, 0:3] - d[:, 3:4]
        with np.errstate(all="ignore"):
            return g / np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])[:, None]


_trace_cache = []          # most recent first: (description, light-less scene around it); a few entries


def _cached_scene(key, make):
    for i, (k, scene) in enumerate(_trace_cache):
        if k is key:
            if i:
                _trace_cache.insert(0, _trace_cache.pop(i))
            return scene
    scene = make()
    _trace_cache.insert(0, (key, scene))
    del _trace_cache[8:]
    return scene


def _object_scene(object, device):
    """device scene holding just `object` (no lights): what the tryTrace entries need"""
    scene = _cached_scene(object, lambda: SdfScene(object, (0.0, 0.0, 0.0), []))
    dev = device if device is not None else Device.default(0)
    return dev.scene(scene)


def _form_scene(form, device):
    scene = _cached_scene(form, lambda: SdfScene(SdfObject.create(SdfMaterial.createSolid((0.0, 0.0, 0.0)), form), (0.0, 0.0, 0.0), []))
    dev = device if device is not None else Device.default(0)
    return dev.scene(scene)


def form_try_trace(form, rays, device=None):
    """SdfForm.tryTrace sdf ray (SdfForm.fs:93-104) over rays [n, 8] on the GPU -> float32 [n, 10]
    (Ray at the hit, Distance, hit flag as int32 bits); a miss (ValueNone) is a row of zeros."""
    return _form_scene(form, device).form_try_trace(rays)[0]


class SdfMaterial:
    @staticmethod
    def createSolid(color):
        return Material("solid", (_v3(color),))

    @staticmethod
    def createGlass(tint, ior, dispersion=0.0):
        """EXTENSION (not in the reference): refracting material, Cauchy dispersion in um^2."""
        return Material("glass", (_v3(tint), float(np.float32(ior)), float(np.float32(dispersion))))


class SdfObject:
    @staticmethod
    def create(material, form):
        return Object("create", (), (material, form))

    @staticmethod
    def union(objects):
        objects = list(objects)
        if not objects:
            raise ValueError("No SdfObjects given.")            # SdfObject.fs:14
        return objects[0] if len(objects) == 1 else Object("union", (), objects)

    @staticmethod
    def subtract(object, form):
        return Object("subtract", (), (object, form))

    @staticmethod
    def intersect(object, forms):
        return Object("intersect", (), (object,) + tuple(forms))

    @staticmethod
    def tryTrace(object, rays, device=None):
        """SdfObject.tryTrace object ray (SdfObject.fs:66-78) over rays [n, 8] on the GPU -> float32 [n, 16]
        (Ray pulled back by epsilon, Normal, Color, hit flag as int32 bits, 0); a miss (ValueNone) is a row of zeros."""
        return _object_scene(object, device).object_try_trace(rays)[0]


class SdfLight:
    @staticmethod
    def directional(direction, color):
        return Light("directional", (_v3(direction), _v3(color)))

    @staticmethod
    def point(position, color):
        return Light("point", (_v3(position), _v3(color)))


class SdfScene:
    """Types.fs:74-79 record {Object; BackgroundColor; Lights}."""

    def __init__(self, Object, BackgroundColor, Lights=()):
        self.Object = Object
        self.BackgroundColor = _v3(BackgroundColor)
        self.Lights = tuple(Lights)
        self._realised = {}
        self._lock = threading.Lock()

    @staticmethod
    def trace(scene, device=None):
        """SdfScene.trace scene : Ray -> FColor (SdfScene.fs:7-8), evaluated on the GPU."""
        return SceneTrace(scene, device)

    @staticmethod
    def shade(scene, hits, device=None):
        """SdfScene.trace from its `| ValueSome result ->` arm on (SdfScene.fs:11-28) over hit records (SdfObjectTraceResult voption values:
        a PixelHits, float32 [..., 16] or a device tensor) -> colours [..., 3], evaluated on the GPU (ft_shade_hits)."""
        dev = device if device is not None else Device.default(0)
        return dev.scene(scene).shade_hits(hits)[0]

    @staticmethod
    def lightVisibility(scene, hits, select=None, previous=None, device=None):
        """Which lights reach each hit record: bit i of the uint32 mask is set where `scene.Lights.[i].Intensity scene.Object ray` is ValueSome
        for a light with lightCos > 0, i.e. where SdfScene.fs:23 executes (ft_light_visibility).  select / previous: re-march some lights only."""
        dev = device if device is not None else Device.default(0)
        return dev.scene(scene).light_visibility(hits, select, previous)[0]

    @staticmethod
    def shadeVisible(scene, hits, visibility, device=None):
        """SdfScene.shade with every shadow ray answered by the masks of lightVisibility: no march (ft_shade_visible)."""
        dev = device if device is not None else Device.default(0)
        return dev.scene(scene).shade_visible(hits, visibility)[0]


def realise(node, backend, memo=None):
    """Build `node` on a backend (libfraytracer_hip context or the test oracle); returns its handle."""
    memo = {} if memo is None else memo
    key = id(node)
    if key in memo:
        return memo[key]
    k = node.kind
    kids = [realise(c, backend, memo) for c in node.kids]
    if isinstance(node, Form):
        if k == "sphere": h = backend.sphere(*node.args)
        elif k == "capsule": h = backend.capsule(*node.args)
        elif k == "torus": h = backend.torus(*node.args)
        elif k == "triangle": h = backend.triangle(*node.args)
        elif k == "box": h = backend.box(*node.args)
        elif k == "union": h = backend.form_union(kids)
        elif k == "subtract": h = backend.form_subtract(kids[0], kids[1])
        elif k == "intersect": h = backend.form_intersect(kids)
        elif k == "unionSmooth": h = backend.form_union_smooth(node.args[0], kids)
        else: raise ValueError(k)
    elif isinstance(node, Material):
        h = backend.material_solid(node.args[0]) if k == "solid" else backend.material_glass(*node.args)
    elif isinstance(node, Object):
        if k == "create": h = backend.object_create(kids[0], kids[1])
        elif k == "union": h = backend.object_union(kids)
        elif k == "subtract": h = backend.object_subtract(kids[0], kids[1])
        elif k == "intersect": h = backend.object_intersect(kids[0], kids[1:])
        else: raise ValueError(k)
    elif isinstance(node, Light):
        h = backend.light_directional(*node.args) if k == "directional" else backend.light_point(*node.args)
    else:
        raise TypeError(type(node))
    memo[key] = h
    return h


# --------------------------------------------------------------------------------------------------
# libfraytracer_hip backend
# --------------------------------------------------------------------------------------------------
def _f3(v):
    return (C.c_float * 3)(*v)


def _handles(hs):
    return (C.c_int32 * len(hs))(*hs), len(hs)


def _vec(v):
    return _lib.Vec3(*v)


_GLIBC_PROBES = ((0x4202422F, 0x56FC9F1C, 0x56FC9F1B), (0xC27C65D9, 0x11FA2993, 0x11FA2992))   # expf input bits, FMA build's result, SSE2 build's result


def glibc_build_of_this_host():
    """FT_MATH_GLIBC_FMA (1) or FT_MATH_GLIBC_SSE2 (2): which build of expf / logf / powf the C runtime of this machine resolves to — the
    value to give Device.set_option("math", ...) for results that equal the reference's CPU path on this host.  Decided by asking the running
    libm: the two builds of glibc 2.35's expf differ on exactly two of the 2^32 inputs (found by comparing the restatements of
    csrc/ft_libm.h exhaustively; logf never differs), so expf of those two tells which one the ifunc resolver picked — whatever
    /proc/cpuinfo, GLIBC_TUNABLES or the OS's XSAVE state made it pick.  Raises if the answers match neither build (another libm: then
    neither glibc mode restates this host's arithmetic)."""
    import struct
    libm = C.CDLL("libm.so.6")
    libm.expf.restype, libm.expf.argtypes = C.c_float, [C.c_float]
    got = [struct.unpack("<I", struct.pack("<f", libm.expf(struct.unpack("<f", struct.pack("<I", x))[0])))[0] for x, _, _ in _GLIBC_PROBES]
    if got == [f for _, f, _ in _GLIBC_PROBES]:
        return _lib.FT_MATH_GLIBC_FMA
    if got == [s_ for _, _, s_ in _GLIBC_PROBES]:
        return _lib.FT_MATH_GLIBC_SSE2
    raise RuntimeError("this host's expf is neither build of glibc 2.35's (probe results %s): FT_OPT_MATH's glibc modes do not restate it" % [hex(g) for g in got])


class Device:
    """One ft_ctx: a GPU (index >= 0) or a host-only context (index -1: construction and
    introspection only — rendering raises, there is no CPU fallback)."""

    _default = {}
    _default_lock = threading.RLock()          # re-entrant: default() constructs a Device, whose __init__ takes the lock for its serial
    _serial = 0

    def __init__(self, index=0):
        p = C.c_void_p()
        check(lib.ft_ctx_create(int(index), C.byref(p)))
        self._ctx = p
        self.index = int(index)
        self._scenes = []                      # DeviceScenes created on this context (closed with it)
        with Device._default_lock:
            Device._serial += 1
            self.serial = Device._serial       # cache key for SdfScene._realised (id() values get reused)

    @classmethod
    def default(cls, index=0):
        with cls._default_lock:
            if index not in cls._default:
                cls._default[index] = Device(index)
            return cls._default[index]

    def close(self):
        if self._ctx:
            for s in self._scenes:             # scenes hold device memory of this context: release them first
                s.close()
            self._scenes = []
            lib.ft_ctx_destroy(self._ctx)
            self._ctx = None

    def host_register(self, array):
        """page-lock a numpy array that is reused as render(..., out=array) destination (ft_host_register)"""
        check(lib.ft_host_register(self._ctx, array.ctypes.data_as(C.c_void_p), array.nbytes))

    def host_unregister(self, array):
        check(lib.ft_host_unregister(self._ctx, array.ctypes.data_as(C.c_void_p)))

    def set_stream(self, hip_stream):
        check(lib.ft_ctx_set_stream(self._ctx, C.c_void_p(hip_stream)))
        self._adopted = hip_stream or None

    @contextlib.contextmanager
    def on_current_stream(self, tensor):
        """Order the context's launches inside the block with the caller's torch work, without a synchronise: they go to torch's current stream
        of the tensor's device (ft_ctx_set_stream), after the kernels that produced the tensor and before whatever the caller queues next.
        torch's default stream is the null stream, which a context cannot adopt (NULL gives it a stream of its own); the launches then go to
        a side stream of this Device that waits for the default stream before the block and that the default stream waits for after it."""
        import torch              # a device tensor was passed in: torch is loaded
        cur = torch.cuda.current_stream(tensor.device)
        side = None
        if int(cur.cuda_stream) == 0:
            side = self._side_stream = getattr(self, "_side_stream", None) or torch.cuda.Stream(tensor.device)
            side.wait_stream(cur)
        handle = int((side or cur).cuda_stream)
        if getattr(self, "_adopted", None) != handle:
            self.set_stream(handle)
        try:
            yield
        finally:
            if side is not None:
                cur.wait_stream(side)

    OPTIONS = {"refill_min": _lib.FT_OPT_REFILL_MIN, "max_blocks_per_cu": _lib.FT_OPT_MAX_BLOCKS_PER_CU,
               "host_chunks": _lib.FT_OPT_HOST_CHUNKS, "host_pin": _lib.FT_OPT_HOST_PIN, "math": _lib.FT_OPT_MATH,
               "tail_k": _lib.FT_OPT_TAIL_K, "guided": _lib.FT_OPT_GUIDED, "chunk": _lib.FT_OPT_CHUNK, "cull": _lib.FT_OPT_CULL, "escape": _lib.FT_OPT_ESCAPE, "lazy_union": _lib.FT_OPT_LAZY_UNION, "carved": _lib.FT_OPT_CARVED, "reuse": _lib.FT_OPT_REUSE,
               "cert": _lib.FT_OPT_CERT, "cert_policy": _lib.FT_OPT_CERT_POLICY,
               # changes only when work starts, never what a launch computes or counts:
               # FT_OPT_ORDER, 1 (default) heavy tiles of the last frame first, 2 record tile costs only, 0 off
               "order": _lib.FT_OPT_ORDER,
               # exact shortcuts like "cert" / "cert_policy" (same frame, counters and flags; sdf_evals falls):
               # FT_OPT_OCCL, the occlusion certificate (1 default, 0 off), and FT_OPT_OCCL_POLICY, its schedule word
               "occl": _lib.FT_OPT_OCCL, "occl_policy": _lib.FT_OPT_OCCL_POLICY}
    # options of a stream of frames, named like the ones above but kept apart from them (OPTIONS is the list the ABI test pins):
    # FT_OPT_TRY_HINT, 1 (default) a tile's bundle-certificate tries follow what its last frame recorded, 2 record only, 0 off; same frame, fewer sdf_evals
    # (tests/helpers.py options_left_at_defaults walks OPTIONS only: a test that changes one of these restores it itself, tests/test_try_hint.py checks its own)
    # FT_OPT_DEPART, 1 (default) the frames that follow try hints try their shadow rays' miss certificate at birth under a margin that grows along the ray,
    # 2 every camera launch of the lean family, 0 off; same frame, fewer sdf_evals (tests/test_gpu_departure_certificate.py checks its own)
    STREAM_OPTIONS = {"try_hint": _lib.FT_OPT_TRY_HINT, "depart": _lib.FT_OPT_DEPART}

    def set_option(self, name, value):
        """ft_ctx_set_option: per-context switches (the library reads no environment variables)"""
        check(lib.ft_ctx_set_option(self._ctx, self._option_id(name), int(value)))

    def get_option(self, name):
        v = C.c_int32()
        check(lib.ft_ctx_get_option(self._ctx, self._option_id(name), C.byref(v)))
        return int(v.value)

    def _option_id(self, name):
        return self.OPTIONS[name] if name in self.OPTIONS else self.STREAM_OPTIONS[name]

    # constructor twins ---------------------------------------------------------------------------
    def sphere(self, c, r): return check(lib.ft_form_sphere(self._ctx, C.byref(_lib.Sphere(_vec(c), r))))
    def capsule(self, a, b, r): return check(lib.ft_form_capsule(self._ctx, C.byref(_lib.Capsule(_vec(a), _vec(b), r))))
    def torus(self, c, n, R, r): return check(lib.ft_form_torus(self._ctx, C.byref(_lib.Torus(_vec(c), _vec(n), R, r))))
    def triangle(self, a, b, c, r): return check(lib.ft_form_triangle(self._ctx, C.byref(_lib.Triangle(_vec(a), _vec(b), _vec(c), r))))
    def box(self, c, h): return check(lib.ft_form_box(self._ctx, C.byref(_lib.Box(_vec(c), _vec(h)))))
    def form_union(self, hs): return check(lib.ft_form_union(self._ctx, *_handles(hs)))
    def form_subtract(self, a, b): return check(lib.ft_form_subtract(self._ctx, a, b))
    def form_intersect(self, hs): return check(lib.ft_form_intersect(self._ctx, *_handles(hs)))
    def form_union_smooth(self, k, hs): return check(lib.ft_form_union_smooth(self._ctx, k, *_handles(hs)))
    def material_solid(self, rgb): return check(lib.ft_material_solid(self._ctx, _f3(rgb)))
    def material_glass(self, tint, ior, dispersion): return check(lib.ft_material_glass(self._ctx, _f3(tint), ior, dispersion))
    def object_create(self, m, f): return check(lib.ft_object_create(self._ctx, m, f))
    def object_union(self, hs): return check(lib.ft_object_union(self._ctx, *_handles(hs)))
    def object_subtract(self, o, f): return check(lib.ft_object_subtract(self._ctx, o, f))
    def object_intersect(self, o, hs): return check(lib.ft_object_intersect(self._ctx, o, *_handles(hs)))
    def light_directional(self, d, c): return check(lib.ft_light_directional(self._ctx, _f3(d), _f3(c)))
    def light_point(self, p, c): return check(lib.ft_light_point(self._ctx, _f3(p), _f3(c)))

    def form_boundary(self, h):
        b = _lib.Boundary()
        check(lib.ft_form_boundary(self._ctx, h, C.byref(b)))
        return (b.center.x, b.center.y, b.center.z, b.radius)

    def object_form(self, h): return check(lib.ft_object_form(self._ctx, h))

    def scene(self, scene):
        """realise + flatten + upload an SdfScene; cached per device."""
        with scene._lock:
            got = scene._realised.get(self.serial)
            if got is None or got._scene is None:
                memo = {}
                obj = realise(scene.Object, self, memo)
                lights = [realise(l, self, memo) for l in scene.Lights]
                got = DeviceScene(self, obj, scene.BackgroundColor, lights)
                got.materials = _materials_by_handle(scene.Object, memo)
                scene._realised[self.serial] = got
                self._scenes.append(got)
            return got

    def mesh_values(self, values, origin, step, iso=0.0, shells=False, keep=None, measures=False):
        """ft_mesh_values: the surface {values = iso} of a float32 lattice [nx, ny, nz] (point (i, j, k) at lattice_points(origin, step,
        values.shape)) as triangles, extracted on the device -> Mesh without normals and materials.  A device tensor (see is_device_tensor;
        float32, contiguous) is meshed where it lies by ft_mesh_values_device on the caller's current stream, and the Mesh holds tensors of its
        device; the values are only read.  shells, keep, measures: as in DeviceScene.mesh_lattice."""
        on_device = is_device_tensor(values)
        if on_device:
            if str(values.dtype).rsplit(".", 1)[-1] != "float32" or not values.is_contiguous():
                raise ValueError("mesh_values: a device tensor must be float32 and contiguous (no silent copy on the device)")
            vals = values
        else:
            vals = np.ascontiguousarray(values, dtype=np.float32)
        if len(tuple(vals.shape)) != 3:
            raise ValueError(f"mesh_values: values must have shape [nx, ny, nz], not {list(vals.shape)}")
        lat, _ = _lattice(origin, step, tuple(int(d) for d in vals.shape))
        handle = C.c_void_p()
        if on_device:
            with self.on_current_stream(vals):
                check(lib.ft_mesh_values_device(self._ctx, C.byref(lat), _dptr(vals.data_ptr()), float(iso), C.byref(handle)))
                return _read_mesh(handle, vals, None, shells, keep, measures)
        check(lib.ft_mesh_values(self._ctx, C.byref(lat), _hptr(vals), float(iso), C.byref(handle)))
        return _read_mesh(handle, None, None, shells, keep, measures)

    def shells(self, triangles, n_vertices, like=None):
        """ft_shells_triangles: the shells (connected pieces, by shared vertex) of any indexed triangle mesh -> Shells.  triangles: int32 [nT, 3], every
        index in 0 .. n_vertices - 1 and the three of a triangle different (anything else is FT_ERR_INVALID); a numpy array, or a device tensor
        (int32, contiguous), which is labelled where it lies by ft_shells_triangles_device on the caller's current stream and gives tensors of its
        device.  like: a device tensor — a host triangle list then gives tensors of like's device as well."""
        on_device = is_device_tensor(triangles)
        if like is not None and not is_device_tensor(like):
            raise ValueError("like: a device tensor (see is_device_tensor) or None")
        if on_device:
            if str(triangles.dtype).rsplit(".", 1)[-1] != "int32" or not triangles.is_contiguous():
                raise ValueError("shells: a device tensor must be int32 and contiguous (no silent copy on the device)")
            tri = triangles
        else:
            tri = np.ascontiguousarray(triangles, dtype=np.int32)
        if len(tuple(tri.shape)) != 2 or int(tri.shape[1]) != 3:
            raise ValueError(f"shells: triangles must have shape [nT, 3], not {list(tri.shape)}")
        handle = C.c_void_p()
        nt, nv = int(tri.shape[0]), int(n_vertices)
        if on_device:
            with self.on_current_stream(tri):
                check(lib.ft_shells_triangles_device(self._ctx, _dptr(tri.data_ptr()), nt, nv, C.byref(handle)))
                return _read_shells(handle, tri)
        with (self.on_current_stream(like) if like is not None else contextlib.nullcontext()):
            check(lib.ft_shells_triangles(self._ctx, _hptr(tri), nt, nv, C.byref(handle)))
            return _read_shells(handle, like)

    def slice_values(self, values, origin, step, axis=2, iso=0.0, measures=False):
        """ft_slice_values: the contours {values = iso} of a float32 lattice [nx, ny, nz] in every lattice plane normal to `axis`, as ordered
        polylines chained on the device -> Contours without normals and materials.  A device tensor (see is_device_tensor; float32, contiguous) is
        sliced where it lies by ft_slice_values_device on the caller's current stream, and the Contours hold tensors of its device; the values are
        only read.  measures: as in DeviceScene.slice_lattice."""
        on_device = is_device_tensor(values)
        if on_device:
            if str(values.dtype).rsplit(".", 1)[-1] != "float32" or not values.is_contiguous():
                raise ValueError("slice_values: a device tensor must be float32 and contiguous (no silent copy on the device)")
            vals = values
        else:
            vals = np.ascontiguousarray(values, dtype=np.float32)
        if len(tuple(vals.shape)) != 3:
            raise ValueError(f"slice_values: values must have shape [nx, ny, nz], not {list(vals.shape)}")
        lat, _ = _lattice(origin, step, tuple(int(d) for d in vals.shape))
        handle = C.c_void_p()
        if on_device:
            with self.on_current_stream(vals):
                check(lib.ft_slice_values_device(self._ctx, C.byref(lat), _dptr(vals.data_ptr()), int(axis), float(iso), C.byref(handle)))
                return _read_slices(handle, vals, None, measures)
        check(lib.ft_slice_values(self._ctx, C.byref(lat), _hptr(vals), int(axis), float(iso), C.byref(handle)))
        return _read_slices(handle, None, None, measures)

    def selftest_libm(self, op, variant, y=0.0, lo_bits=0, n_chunks=256):
        """ft_selftest_libm: checksums of the device restatement of glibc's expf (op 0) / logf (1) / powf(x, y) (2) per 2^24 inputs"""
        sums = (C.c_uint64 * n_chunks)()
        check(lib.ft_selftest_libm(self._ctx, int(op), int(variant), float(y), int(lo_bits), int(n_chunks), sums))
        return np.array(sums, np.uint64)

    def selftest_fastmath(self):
        m = (C.c_uint64 * 3)()
        check(lib.ft_selftest_fastmath(self._ctx, m))
        return {"sqrt": int(m[0]), "exp": int(m[1]), "exp_near": int(m[2])}

    def math_eval(self, op, x, y=None):
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty_like(x)
        yp = None
        if y is not None:
            y = np.ascontiguousarray(y, dtype=np.float32)
            yp = y.ctypes.data_as(C.c_void_p)
        check(lib.ft_math_eval(self._ctx, op, x.ctypes.data_as(C.c_void_p), yp, x.size, out.ctypes.data_as(C.c_void_p)))
        return out


def _materials_by_handle(obj, memo):
    """handle -> SdfMaterial descriptor for every material of a realised object tree"""
    out, stack = {}, [obj]
    while stack:
        node = stack.pop()
        if isinstance(node, Material):
            out[memo[id(node)]] = node
        stack.extend(node.kids)
    return out


def _dptr(p):
    """a device address (int; None or 0: not asked for) as the void* of a C call"""
    return None if not p else C.c_void_p(p)


def _hptr(a):
    """a numpy array (None: not asked for) as the void* of a C call"""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _host_outputs(lead, image, records, material):
    """The host arrays a hits form fills, by flags: image float32 lead + (3,), records float32 lead + (16,), material int32 lead; None for
    what is not asked for -> ((image, records, material), their pointers in the C calls' order)"""
    arrays = (np.empty(lead + (3,), np.float32) if image else None, np.empty(lead + (16,), np.float32) if records else None,
              np.empty(lead, np.int32) if material else None)
    return arrays, tuple(_hptr(a) for a in arrays)


def is_device_tensor(x):
    """Duck-typed device tensor (a torch CUDA / HIP tensor, without importing torch): anything with data_ptr(), is_cuda, shape, dtype and
    is_contiguous() whose is_cuda is true.  The ray-buffer calls trace such a tensor where it lies."""
    return all(hasattr(x, k) for k in ("data_ptr", "is_cuda", "shape", "dtype", "is_contiguous")) and bool(x.is_cuda)


def _buffer(x):
    """the buffer behind a PixelHits (its records), an array-like or a device tensor: a device tensor or a numpy array as it is, anything else
    as a numpy array"""
    x = x.records if isinstance(x, PixelHits) else x
    return x if is_device_tensor(x) or isinstance(x, np.ndarray) else np.asarray(x)


def _empty(like, shape, kind="float32"):
    """An uninitialised output of `shape`: a numpy array where `like` is None, else a tensor of like's device (like.new_empty).  kind: "float32",
    "int32", or "mask" for visibility masks: uint32 in numpy, the same bits as int32 in torch, whose uint32 has no arithmetic."""
    if like is None:
        return np.empty(shape, {"float32": np.float32, "int32": np.int32, "mask": np.uint32}[kind])
    return like.new_empty(shape) if kind == "float32" else like.new_empty(shape, dtype=_torch_int32(like))


def check_device_rays(t):
    """n of a device ray buffer: float32, shape [n, 8], contiguous — anything else is a ValueError (no silent copy on the device)"""
    if str(t.dtype).rsplit(".", 1)[-1] != "float32":
        raise ValueError(f"device ray buffer: dtype must be float32, not {t.dtype}")
    shape = tuple(t.shape)
    if len(shape) != 2 or shape[1] != 8:
        raise ValueError(f"device ray buffer: shape must be [n, 8] (Origin, Direction, Length, Epsilon), not {list(shape)}")
    if not t.is_contiguous():
        raise ValueError("device ray buffer: the tensor must be contiguous (call .contiguous() first)")
    return int(shape[0])


def check_hit_records(t):
    """leading shape of a buffer of hit records (a numpy array or a device tensor): float32, shape [..., 16] (ft_object_trace_result), and for
    a device tensor contiguous — anything else is a ValueError (no silent conversion)"""
    if str(t.dtype).rsplit(".", 1)[-1] != "float32":
        raise ValueError(f"hit records: dtype must be float32, not {t.dtype}")
    shape = tuple(int(d) for d in t.shape)
    if len(shape) < 1 or shape[-1] != 16:
        raise ValueError(f"hit records: shape must be [..., 16] (Ray, Normal, Color, hit, 0), not {list(shape)}")
    if is_device_tensor(t) and not t.is_contiguous():
        raise ValueError("hit records: the tensor must be contiguous (call .contiguous() first)")
    return shape[:-1]


def check_visibility(m, lead, what="visibility"):
    """a buffer of visibility masks for records of leading shape `lead`: a uint32 numpy array or an int32 device tensor (the same bits; torch's
    uint32 has no arithmetic), contiguous, of exactly that shape — anything else is a ValueError (no silent conversion)"""
    want = "int32" if is_device_tensor(m) else "uint32"
    if str(m.dtype).rsplit(".", 1)[-1] != want:
        raise ValueError(f"{what}: dtype must be {want}, not {m.dtype}")
    if tuple(int(d) for d in m.shape) != tuple(lead):
        raise ValueError(f"{what}: shape must be {list(lead)} (the records' without their last axis), not {list(m.shape)}")
    if is_device_tensor(m) and not m.is_contiguous():
        raise ValueError(f"{what}: the tensor must be contiguous (call .contiguous() first)")


def check_device_points(t):
    """leading shape of a device point buffer: float32, shape [..., 3], contiguous — anything else is a ValueError (no silent copy on the device)"""
    if str(t.dtype).rsplit(".", 1)[-1] != "float32":
        raise ValueError(f"device point buffer: dtype must be float32, not {t.dtype}")
    shape = tuple(int(d) for d in t.shape)
    if len(shape) < 1 or shape[-1] != 3:
        raise ValueError(f"device point buffer: shape must be [..., 3] (x, y, z), not {list(shape)}")
    if not t.is_contiguous():
        raise ValueError("device point buffer: the tensor must be contiguous (call .contiguous() first)")
    return shape[:-1]


def lattice_points(origin, step, counts):
    """The points of the lattice ft_sample_lattice evaluates, float32 [nx, ny, nz, 3]: point (i, j, k) is origin + (i, j, k) * step per
    coordinate, as ONE float32 product, rounded, then ONE float32 sum, rounded (never fused).  Pure numpy: the definition, for callers and tests."""
    F = np.float32
    o, st = np.asarray(origin, F).reshape(3), np.asarray(step, F).reshape(3)
    n = _lattice_counts(counts)
    pts = np.empty(n + (3,), F)
    for a in range(3):
        prod = np.arange(n[a], dtype=F) * st[a]                       # (float)i is exact: counts are at most 2^24
        pts[..., a] = (o[a] + prod).reshape([-1 if b == a else 1 for b in range(3)])
    return pts


def _lattice_counts(counts):
    n = tuple(int(c) for c in counts)
    if len(n) != 3 or any(c < 1 or c > 16777216 for c in n):
        raise ValueError(f"lattice: counts must be three integers in 1 .. 16777216, not {counts!r}")
    return n


def _lattice(origin, step, counts):
    n = _lattice_counts(counts)
    o, st = _v3(origin), _v3(step)
    return _lib.Lattice(_lib.Vec3(*o), _lib.Vec3(*st), *n), n


class FieldSamples:
    """What sample_points / sample_lattice return: `distance` float32 [...], `normal` float32 [..., 3], `material` int32 [...] (the handle of the
    material object.Material.Color picks at the point; -1 where FT_FIELD_BOUNDED left the point out) — each None where not asked for; numpy
    arrays, or device tensors where the call was given one."""

    def __init__(self, distance=None, normal=None, material=None, materials=None):
        self.distance = distance
        self.normal = normal
        self.material = material
        self._materials = dict(materials or {})

    def descriptor(self, handle):
        """the SdfMaterial description (SdfMaterial.createSolid / createGlass value) a material handle was realised from; None for -1"""
        return self._materials.get(int(handle))


class Mesh:
    """What mesh_lattice / mesh_values return: `vertices` float32 [nv, 3], `triangles` int32 [nt, 3] (counter-clockwise seen from the outside),
    `normal` float32 [nv, 3] and `material` int32 [nv] (the handle of the material object.Material.Color picks at the vertex) — None where not
    asked for — and `skipped`, the tetrahedra left out for a non-finite corner value; numpy arrays, or device tensors where the call was given
    one.  The rule that fixes every bit of it is the header's ("Meshing")."""

    def __init__(self, vertices, triangles, normal=None, material=None, skipped=0, materials=None, shells=None, measure=None):
        self.vertices = vertices
        self.triangles = triangles
        self.normal = normal
        self.material = material
        self.skipped = int(skipped)
        self.shells = shells                                          # a Shells where the mesh was made with shells=True or keep=...; else None
        self.measure = measure                                        # a Measures of one record, the whole mesh's, where it was made with measures=True; else None
        self._materials = dict(materials or {})

    def descriptor(self, handle):
        """the SdfMaterial description (SdfMaterial.createSolid / createGlass value) a material handle was realised from; None for -1"""
        return self._materials.get(int(handle))

    @staticmethod
    def _host(a):
        return None if a is None else (a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a))

    def save_obj(self, path, groups=False):
        """Wavefront OBJ: v lines (9 significant digits: float32 round-trips), vn lines where the mesh has normals, f lines with 1-based indices.
        groups: where the mesh carries shells, the faces are written shell by shell, each under a line `g shell_<s>` (within a shell in their old order)"""
        v, t, n = self._host(self.vertices), self._host(self.triangles), self._host(self.normal)
        of = self._host(self.shells.triangle_shell) if groups and self.shells is not None else None
        with open(path, "w") as f:
            f.write(f"# {len(v)} vertices, {len(t)} triangles\n")
            for p in v:
                f.write("v %.9g %.9g %.9g\n" % tuple(float(c) for c in p))
            if n is not None:
                for p in n:
                    f.write("vn %.9g %.9g %.9g\n" % tuple(float(c) for c in p))
            if of is None:
                for a, b, c in (t + 1).tolist():
                    f.write(f"f {a}//{a} {b}//{b} {c}//{c}\n" if n is not None else f"f {a} {b} {c}\n")
                return
            for s in range(len(self.shells.records)):
                f.write(f"g shell_{s}\n")
                for a, b, c in (t[of == s] + 1).tolist():
                    f.write(f"f {a}//{a} {b}//{b} {c}//{c}\n" if n is not None else f"f {a} {b} {c}\n")

    def save_stl(self, path):
        """binary STL: per triangle its unit normal (from the vertices, float32; zero for a zero-area triangle) and its three corners"""
        v, t = self._host(self.vertices), self._host(self.triangles)
        corners = v[t.astype(np.int64)].astype(np.float32).reshape(-1, 3, 3)
        with np.errstate(all="ignore"):
            nrm = np.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0]).astype(np.float32)
            length = np.sqrt((nrm * nrm).sum(axis=1, dtype=np.float32))
            nrm = np.where(length[:, None] > 0, nrm / length[:, None], np.float32(0.0)).astype(np.float32)
        rec = np.zeros(len(t), np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("attr", "<u2")]))
        rec["n"], rec["v"] = nrm, corners
        with open(path, "wb") as f:
            f.write(b"fraytracer_amd mesh".ljust(80, b" "))
            f.write(np.uint32(len(t)).tobytes())
            f.write(rec.tobytes())


def _read_mesh(handle, like, materials, shells=False, keep=None, measures=False):
    """an ft_mesh -> Mesh of numpy arrays (like = None) or of tensors of like's device, through ft_mesh_read; the handle is destroyed.  shells: the
    Mesh carries its Shells, computed on the handle before it is destroyed; keep (implies shells): the shells to keep (_keep_mask) — the Mesh is then
    ft_mesh_select's, with the shells of the selected mesh; measures (implies shells): the Shells carry their Measures and the Mesh its own"""
    if keep is not None:
        selected = C.c_void_p()
        try:
            sh = C.c_void_p()
            check(lib.ft_mesh_shells(handle, C.byref(sh)))
            try:
                wanted = measures or (isinstance(keep, str) and keep == "bodies")
                mask = _keep_mask(_read_shells(sh, None, destroy=False, mesh=handle if wanted else None), keep)
                check(lib.ft_mesh_select(handle, sh, _hptr(mask), len(mask), C.byref(selected)))
            finally:
                lib.ft_shells_destroy(sh)
        finally:
            lib.ft_mesh_destroy(handle)
        return _read_mesh(selected, like, materials, shells=True, measures=measures)
    try:
        info = _lib.MeshInfo()
        check(lib.ft_mesh_get_info(handle, C.byref(info)))
        nv, nt = int(info.n_vertices), int(info.n_triangles)
        parts = (_empty(like, (nv, 3)), _empty(like, (nt, 3), "int32"), _empty(like, (nv, 3)) if info.has_normal else None,
                 _empty(like, (nv,), "int32") if info.has_material else None)
        ptr = _hptr if like is None else (lambda a: None if a is None else _dptr(a.data_ptr()))
        check(lib.ft_mesh_read(handle, *map(ptr, parts)))
        found = whole = None
        if shells or measures:
            sh = C.c_void_p()
            check(lib.ft_mesh_shells(handle, C.byref(sh)))
            found = _read_shells(sh, like, mesh=handle if measures else None)
        if measures:
            whole = _read_measures(like, 1 if nv or nt else 0, lambda out: lib.ft_mesh_measure(handle, out))
        return Mesh(*parts, skipped=info.n_skipped, materials=materials, shells=found, measure=whole)
    finally:
        lib.ft_mesh_destroy(handle)


class Shells:
    """What Device.shells and a mesh made with shells=True carry: `vertex_shell` int32 [nV] (-1: a vertex no triangle names), `triangle_shell` int32
    [nT], `records` int32 [S, 4] with the columns of ft_shell (first_vertex, n_vertices, n_triangles, n_border_edges) and `info`, a dict of
    ft_shells_info's six counts; numpy arrays, or device tensors where the call was given one.  Shells are numbered by their smallest vertex.  The
    rule that fixes every bit of it is the header's ("Shells").  `measures`: a Measures, one record per shell, where the mesh was made with
    measures=True; else None."""

    def __init__(self, vertex_shell, triangle_shell, records, info, measures=None):
        self.vertex_shell = vertex_shell
        self.triangle_shell = triangle_shell
        self.records = records
        self.info = dict(info)
        self.measures = measures

    def __len__(self):
        return int(self.info["n_shells"])

    @property
    def closed(self):
        """bool [S]: no border edge"""
        return Mesh._host(self.records).reshape(-1, 4)[:, 3] == 0

    @property
    def euler(self):
        """int64 [S]: V - (3 F + B) // 2 + F per shell, the Euler characteristic where no directed side occurs twice (every mesher output)"""
        r = Mesh._host(self.records).reshape(-1, 4).astype(np.int64)
        return r[:, 1] - (3 * r[:, 2] + r[:, 3]) // 2 + r[:, 2]


class Measures:
    """Per-shell measures (ft_shell_measure, the header's "Measures"): `records` is the [S] record array — a numpy structured array with the fields
    of ft_shell_measure, or, where the call was given a device tensor, a float32 tensor [S, 18] of its device holding the same 72 bytes per shell.
    The properties give numpy arrays (a device tensor is read back): area float64 [S], volume float64 [S] (positive for a closed body, negative
    for a closed cavity; no meaning for an open shell), moment float64 [S, 3] (the integral of x over the volume), bbox_min / bbox_max float32
    [S, 3], n_unmeasured int32 [S] (triangles with a non-finite coordinate), extent_exponent int.  Every bit of them is fixed by the rule;
    `centroid` = moment / volume is plain numpy and is not."""

    def __init__(self, records):
        self.records = records

    def __len__(self):
        return int(self.records.shape[0])

    def host(self):
        """the records as a numpy structured array [S]"""
        r = self.records
        if isinstance(r, np.ndarray):
            return r
        return np.ascontiguousarray(r.detach().cpu().numpy()).view(np.dtype(_lib.SHELL_MEASURE_DTYPE)).reshape(-1)

    area = property(lambda self: self.host()["area"])
    volume = property(lambda self: self.host()["volume"])
    moment = property(lambda self: self.host()["moment"])
    bbox_min = property(lambda self: self.host()["bbox_min"])
    bbox_max = property(lambda self: self.host()["bbox_max"])
    n_unmeasured = property(lambda self: self.host()["n_unmeasured"])

    @property
    def extent_exponent(self):
        e = self.host()["extent_exponent"]
        return int(e[0]) if len(e) else 0

    @property
    def centroid(self):
        """float64 [S, 3]: moment / volume (nan where the volume is 0)"""
        h = self.host()
        with np.errstate(all="ignore"):
            return h["moment"] / h["volume"][:, None]


def _read_measures(like, n, call):
    """n records written by call(out pointer) -> Measures over a numpy record array (like = None) or a float32 tensor [n, 18] of like's device"""
    if like is None:
        rec = np.zeros(n, np.dtype(_lib.SHELL_MEASURE_DTYPE))
        check(call(_hptr(rec) if n else None))
    else:
        rec = like.new_empty((n, 18), dtype=like.new_empty(0).float().dtype)
        check(call(_dptr(rec.data_ptr()) if n else None))
    return Measures(rec)


def _read_shells(handle, like, destroy=True, mesh=None):
    """an ft_shells -> Shells of numpy arrays (like = None) or of tensors of like's device, through ft_shells_read; the handle is destroyed.  mesh: the
    ft_mesh the shells were built from — the Shells then carry its shells' Measures (ft_shells_measure)"""
    try:
        info = _lib.ShellsInfo()
        check(lib.ft_shells_get_info(handle, C.byref(info)))
        parts = (_empty(like, (int(info.n_vertices),), "int32"), _empty(like, (int(info.n_triangles),), "int32"), _empty(like, (int(info.n_shells), 4), "int32"))
        ptr = _hptr if like is None else (lambda a: _dptr(a.data_ptr()))
        check(lib.ft_shells_read(handle, *map(ptr, parts)))
        found = None if mesh is None else _read_measures(like, int(info.n_shells), lambda out: lib.ft_shells_measure(mesh, handle, out))
        return Shells(*parts, info={k: int(getattr(info, k)) for k, _ in info._fields_}, measures=found)
    finally:
        if destroy:
            lib.ft_shells_destroy(handle)


def _keep_mask(shells, keep):
    """keep= of the mesh methods as one byte per shell: an int k (the k shells with the most triangles, ties going to the lower number), "closed",
    "bodies" (closed and of positive volume: needs the shells' measures), a bool array of length S, or a callable Shells -> bool array"""
    n = len(shells)
    if callable(keep):
        keep = keep(shells)
    if isinstance(keep, str):
        if keep not in ("closed", "bodies"):
            raise ValueError(f'keep: the names are "closed" and "bodies", not {keep!r}')
        if keep == "bodies" and shells.measures is None:
            raise ValueError('keep="bodies": these shells carry no measures')
        mask = shells.closed if keep == "closed" else shells.closed & (shells.measures.volume > 0)
    elif isinstance(keep, (int, np.integer)) and not isinstance(keep, (bool, np.bool_)):
        if keep < 0:
            raise ValueError("keep: a count of shells must be >= 0")
        tris = Mesh._host(shells.records).reshape(-1, 4)[:, 2]
        mask = np.zeros(n, bool)
        mask[sorted(range(n), key=lambda s: (-int(tris[s]), s))[:int(keep)]] = True
    else:
        mask = np.asarray(Mesh._host(keep))
        if mask.dtype != np.bool_ or mask.shape != (n,):
            raise ValueError(f"keep: a bool array of length {n} (one per shell), not {mask.dtype} {list(mask.shape)}")
    return np.ascontiguousarray(mask, dtype=np.uint8)


class Contours:
    """What slice_lattice / slice_values return: `points` float32 [n, 3] and `polylines` int32 [m, 4] with the columns of ft_polyline (first, count,
    slice, closed): polyline r is points[first : first + count] in slice `slice`, closed (a loop, its first point not repeated; counter-clockwise seen
    from +axis around the inside, clockwise around a hole) or open.  `normal` float32 [n, 3] and `material` int32 [n] are None where not asked for;
    `skipped` counts the triangles left out for a non-finite corner value; `axis` and `slices` say which planes.  numpy arrays, or device tensors
    where the call was given one.  The rule that fixes every bit of it is the header's ("Slicing").  `measures` (a ContourMeasures, one record per
    polyline) and `layer_measures` (one record per slice) where the contours were made with measures=True; else None."""

    def __init__(self, points, polylines, normal=None, material=None, skipped=0, closed=0, axis=2, slices=0, materials=None, measures=None, layer_measures=None):
        self.points = points
        self.polylines = polylines
        self.normal = normal
        self.material = material
        self.skipped = int(skipped)
        self.closed = int(closed)
        self.axis = int(axis)
        self.slices = int(slices)
        self.measures = measures
        self.layer_measures = layer_measures
        self._materials = dict(materials or {})

    def descriptor(self, handle):
        """the SdfMaterial description a material handle was realised from; None for -1"""
        return self._materials.get(int(handle))

    def layer(self, w):
        """the polylines of slice w in the rule's order: a list of (points float32 [m, 3], closed)"""
        pts, rec = Mesh._host(self.points), Mesh._host(self.polylines)
        return [(pts[first:first + count], bool(closed)) for first, count, plane, closed in rec.tolist() if plane == w]

    def write_svg(self, path, w, stroke=None):
        """slice w as an SVG drawing, u to the right and v up: one path per polyline (9 significant digits: float32 round-trips), closed ones
        ending in Z; filled by the even-odd rule, so that holes stay open"""
        u, v = (self.axis + 1) % 3, (self.axis + 2) % 3
        pts = Mesh._host(self.points)
        lines = self.layer(w)
        if len(pts):
            lo, hi = pts[:, [u, v]].min(axis=0).astype(float), pts[:, [u, v]].max(axis=0).astype(float)
        else:
            lo, hi = np.zeros(2), np.ones(2)
        size = np.maximum(hi - lo, 1e-9)
        width = float(stroke) if stroke is not None else float(size.max()) / 400.0
        with open(path, "w") as f:
            f.write('<svg xmlns="http://www.w3.org/2000/svg" viewBox="%.9g %.9g %.9g %.9g">\n' % (lo[0], -hi[1], size[0], size[1]))
            f.write('<g transform="scale(1,-1)" fill="#ccc" fill-rule="evenodd" stroke="#000" stroke-width="%.9g">\n' % width)
            for p, closed in lines:
                d = " L ".join("%.9g %.9g" % (float(q[u]), float(q[v])) for q in p)
                f.write('<path d="M %s%s"%s/>\n' % (d, " Z" if closed else "", "" if closed else ' fill="none"'))
            f.write("</g>\n</svg>\n")


class ContourMeasures:
    """Per-polyline or per-slice contour measures (ft_contour_measure / ft_slice_measure, the header's "Contour measures"): `records` is the record
    array — a numpy structured array with the struct's fields, or, where the call was given a device tensor, a float32 tensor [n, 14] (polylines)
    or [n, 18] (slices) of its device holding the same 56 or 72 bytes per record.  The properties give numpy arrays (a device tensor is read back):
    length float64 [n], area float64 [n] (per polyline positive for a closed outer boundary, negative for a closed hole, with positive steps in the
    plane; per slice the enclosed area, holes subtracted), moment float64 [n, 2] (the integral of (u, v) over the area), bbox_min / bbox_max float32
    [n, 2], n_unmeasured int32 [n], extent_exponent int; per slice also n_polylines, n_closed, n_outer, n_holes.  Every bit of them is fixed by the
    rule; `centroid` = moment / area is plain numpy and is not."""

    def __init__(self, records, per_slice=False):
        self.records = records
        self.per_slice = bool(per_slice)

    def __len__(self):
        return int(self.records.shape[0])

    def host(self):
        """the records as a numpy structured array [n]"""
        r = self.records
        if isinstance(r, np.ndarray):
            return r
        dtype = np.dtype(_lib.SLICE_MEASURE_DTYPE if self.per_slice else _lib.CONTOUR_MEASURE_DTYPE)
        return np.ascontiguousarray(r.detach().cpu().numpy()).view(dtype).reshape(-1)

    length = property(lambda self: self.host()["length"])
    area = property(lambda self: self.host()["area"])
    moment = property(lambda self: self.host()["moment"])
    bbox_min = property(lambda self: self.host()["bbox_min"])
    bbox_max = property(lambda self: self.host()["bbox_max"])
    n_unmeasured = property(lambda self: self.host()["n_unmeasured"])
    n_polylines = property(lambda self: self.host()["n_polylines"])      # the four counts: per-slice records only
    n_closed = property(lambda self: self.host()["n_closed"])
    n_outer = property(lambda self: self.host()["n_outer"])
    n_holes = property(lambda self: self.host()["n_holes"])

    @property
    def extent_exponent(self):
        e = self.host()["extent_exponent"]
        return int(e[0]) if len(e) else 0

    @property
    def centroid(self):
        """float64 [n, 2]: moment / area in the plane's (u, v) (nan where the area is 0)"""
        h = self.host()
        with np.errstate(all="ignore"):
            return h["moment"] / h["area"][:, None]


def _read_contour_measures(handle, like, n_polylines, n_slices):
    """ft_slices_measure of an ft_slices -> (ContourMeasures per polyline, ContourMeasures per slice) over numpy record arrays (like = None) or
    float32 tensors [n, 14] and [n, 18] of like's device"""
    if like is None:
        per_line, per_slice = np.zeros(n_polylines, np.dtype(_lib.CONTOUR_MEASURE_DTYPE)), np.zeros(n_slices, np.dtype(_lib.SLICE_MEASURE_DTYPE))
        check(lib.ft_slices_measure(handle, _hptr(per_line) if n_polylines else None, _hptr(per_slice) if n_slices else None))
    else:
        f32 = like.new_empty(0).float().dtype
        per_line, per_slice = like.new_empty((n_polylines, 14), dtype=f32), like.new_empty((n_slices, 18), dtype=f32)
        check(lib.ft_slices_measure(handle, _dptr(per_line.data_ptr()) if n_polylines else None, _dptr(per_slice.data_ptr()) if n_slices else None))
    return ContourMeasures(per_line), ContourMeasures(per_slice, per_slice=True)


def _read_slices(handle, like, materials, measures=False):
    """an ft_slices -> Contours of numpy arrays (like = None) or of tensors of like's device, through ft_slices_read; the handle is destroyed.
    measures: the Contours carry their ContourMeasures, computed on the handle before it is destroyed"""
    try:
        info = _lib.SlicesInfo()
        check(lib.ft_slices_get_info(handle, C.byref(info)))
        n, m = int(info.n_points), int(info.n_polylines)
        parts = (_empty(like, (n, 3)), _empty(like, (m, 4), "int32"), _empty(like, (n, 3)) if info.has_normal else None,
                 _empty(like, (n,), "int32") if info.has_material else None)
        ptr = _hptr if like is None else (lambda a: None if a is None else _dptr(a.data_ptr()))
        check(lib.ft_slices_read(handle, *map(ptr, parts)))
        per_line, per_slice = _read_contour_measures(handle, like, m, int(info.n_slices)) if measures else (None, None)
        return Contours(*parts, skipped=info.n_skipped, closed=info.n_closed, axis=info.axis, slices=info.n_slices, materials=materials,
                        measures=per_line, layer_measures=per_slice)
    finally:
        lib.ft_slices_destroy(handle)


def _torch_int32(t):
    import torch                  # a device tensor was passed in: torch is loaded
    return torch.int32


class PixelHits:
    """EXTENSION (ft_render_hits): SdfObject.tryTrace scene.Object of every pixel's camera ray (sample 0), laid out like the
    frame.  `records` is float32 [n_columns, Y, 16] in the layout of ft_object_trace_result — Ray pulled back by epsilon
    (Origin = Position, Direction, Length, Epsilon), Normal, Color, hit flag (int32 bits), 0; a miss (ValueNone) is all zero.
    `material` is int32 [n_columns, Y]: the handle of the material the hit picked, -1 on a miss (None if not asked for).
    ft_render_views_hits: every array has a leading view axis, [K, n_columns, Y, ...]; the properties keep it.
    ft_trace_rays_hits: one record per ray of a ray buffer, [n, 16] and [n]; device tensors where the rays were one."""

    def __init__(self, records, material=None, materials=None):
        self.records = records
        self.material = material
        self._materials = dict(materials or {})

    @property
    def ray(self): return self.records[..., 0:8]

    @property
    def position(self): return self.records[..., 0:3]

    @property
    def direction(self): return self.records[..., 3:6]

    @property
    def length(self):
        """remaining Length of the pulled-back ray: what is left of the ray's length, plus epsilon"""
        return self.records[..., 6]

    @property
    def normal(self): return self.records[..., 8:11]

    @property
    def color(self): return self.records[..., 11:14]

    @property
    def hit(self):
        flag = self.records[..., 14]
        return flag.view(np.int32 if isinstance(flag, np.ndarray) else _torch_int32(flag)) != 0

    def descriptor(self, handle):
        """the SdfMaterial description (SdfMaterial.createSolid / createGlass value) a material handle was realised from; None for -1"""
        return self._materials.get(int(handle))


class DeviceScene:
    """ft_scene: the flattened immutable scene resident in HBM."""

    def __init__(self, device, obj, bg, lights):
        self.device = device
        self._object = obj
        self.materials = {}               # material handle -> SdfMaterial description (filled by Device.scene)
        p = C.c_void_p()
        hs, n = _handles(lights)
        check(lib.ft_scene_create(device._ctx, obj, _f3(bg), hs, n, C.byref(p)))
        self._scene = p

    def close(self):
        if self._scene:
            lib.ft_scene_destroy(self._scene)
            self._scene = None

    def relight(self, BackgroundColor, Lights):
        """ft_scene_relight: a DeviceScene of the same Object under another background and other lights (SdfLight descriptions).  The flattened
        object — program, grids, support sphere, certificate clusters — is copied, not rebuilt; the result equals Device.scene(SdfScene(Object,
        BackgroundColor, Lights)) in every uploaded byte and is independent of this scene (either may be closed first)."""
        dev = self.device
        hs, n = _handles([realise(l, dev) for l in Lights])
        p = C.c_void_p()
        check(lib.ft_scene_relight(self._scene, _f3(_v3(BackgroundColor)), hs, n, C.byref(p)))
        new = DeviceScene.__new__(DeviceScene)
        new.device, new._object, new.materials, new._scene = dev, getattr(self, "_object", None), getattr(self, "materials", {}), p
        dev._scenes.append(new)
        return new

    def boundary(self):
        """scene.Object.Form.Boundary as (cx, cy, cz, radius)"""
        return self.device.form_boundary(self.device.object_form(self._object))

    def info(self):
        i = _lib.SceneInfo()
        check(lib.ft_scene_info_get(self._scene, C.byref(i)))
        return {k: getattr(i, k) for k, _ in i._fields_}

    def support_sphere(self):
        """(cx, cy, cz, radius) of the sphere outside of which (grown by epsilon) no evaluation can be a hit; radius < 0: none known"""
        cr = (C.c_float * 4)()
        check(lib.ft_scene_support_sphere(self._scene, cr))
        return tuple(float(v) for v in cr)

    def miss_certificate(self):
        """{margin, clip, rho2, len_factor, steps}: the constants of the smooth-union kernel's miss certificate (margin < 0: none)"""
        v = (C.c_float * 5)()
        check(lib.ft_scene_miss_certificate(self._scene, v))
        return dict(zip(("margin", "clip", "rho2", "len_factor", "steps"), (float(x) for x in v)))

    def occlusion_certificate(self):
        """{step, base, eps_min, cap, len_inv, near, reach}: the constants of the smooth-union kernel's occlusion certificate (base < 0: none)"""
        v = (C.c_float * 7)()
        check(lib.ft_scene_occlusion_certificate(self._scene, v))
        return dict(zip(("step", "base", "eps_min", "cap", "len_inv", "near", "reach"), (float(x) for x in v)))

    def departure_certificate(self):
        """{step, base, kappa, eps_min, clip, len_factor, steps}: the constants of the smooth-union kernel's departure certificate (base < 0: none)"""
        v = (C.c_float * 7)()
        check(lib.ft_scene_departure_certificate(self._scene, v))
        return dict(zip(("step", "base", "kappa", "eps_min", "clip", "len_factor", "steps"), (float(x) for x in v)))

    def miss_certificate_clusters(self):
        """(clusters, members): clusters a float32 array (K, 4) of centre xyz and radius, members a list of K arrays (n_c, 4) of the children
        (x, y, z, r) in cluster order; K = 0: the certificate sums every child"""
        k, n = C.c_int32(), C.c_int32()
        check(lib.ft_scene_miss_certificate_clusters(self._scene, C.byref(k), C.byref(n), None, 0))
        size = 8 * k.value + 4 * n.value
        buf = (C.c_float * max(size, 1))()
        check(lib.ft_scene_miss_certificate_clusters(self._scene, C.byref(k), C.byref(n), buf, size))
        a = np.frombuffer(buf, np.float32, size).copy()
        rec = a[:8 * k.value].reshape(-1, 8)
        kids = a[8 * k.value:].reshape(-1, 4)
        ints = rec[:, 4:6].copy().view(np.int32)
        return rec[:, :4].copy(), [kids[f:f + c] for c, f in ints]

    def grid(self, g=0):
        info = (C.c_float * 6)()
        counts = (C.c_int32 * 3)()
        nc, ni = C.c_int32(), C.c_int32()
        check(lib.ft_scene_grid_shape(self._scene, g, info, counts, C.byref(nc), C.byref(ni)))
        cell_start = np.empty(nc.value + 1, np.uint32)
        centers = np.empty((nc.value, 3), np.float32)
        lower = np.empty(ni.value, np.float32)
        child = np.empty(ni.value, np.int32)
        check(lib.ft_scene_grid_dump(self._scene, g, *(a.ctypes.data_as(C.c_void_p) for a in (cell_start, centers, lower, child))))
        return {"aabbMin": np.array(info[0:3], np.float32), "cellSizeInv": np.array(info[3:6], np.float32),
                "counts": tuple(counts), "cell_start": cell_start, "centers": centers, "lower": lower, "child": child}

    def _params(self, imageSize, epsilon, length, x0=0, n_columns=None, stripe_width=None, stripe_ranks=1, stripe_rank=0,
                spp=1, ao_samples=0, ao_radius=0.0, max_bounces=0, spectral=0):
        """spp / ao_samples / ao_radius / max_bounces / spectral are EXTENSIONS (not in the reference);
        defaults = the reference."""
        W, H = int(imageSize.X), int(imageSize.Y)
        if n_columns is None:
            n_columns = W - x0 if stripe_ranks == 1 else W // stripe_ranks
        if stripe_width is None:
            stripe_width = n_columns
        return _lib.RenderParams(W, H, int(x0), int(n_columns), int(stripe_width), int(stripe_ranks), int(stripe_rank),
                                 int(spp), float(epsilon), float(length), int(ao_samples), float(ao_radius),
                                 int(max_bounces), int(spectral))

    def _call(self, fn, *args):
        """fn(ctx, scene, *args, &stats) of a host form -> the stats dict"""
        st = _lib.Stats()
        check(fn(self.device._ctx, self._scene, *args, C.byref(st)))
        return st.as_dict()

    @staticmethod
    def _image(out, shape, what):
        """the float32 array a frame form renders into: a new one, or the caller's `out` if it has this shape"""
        if out is None:
            return np.empty(shape, np.float32)
        if out.dtype != np.float32 or out.shape != shape or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous float32 array of shape {what}")
        return out

    @staticmethod
    def _cameras(cameras):
        cams = list(cameras)
        arr = (_lib.CameraS * max(len(cams), 1))()
        for k, cam in enumerate(cams):
            arr[k] = cam._c
        return arr, len(cams)

    def render(self, epsilon, length, imageSize, camera, out=None, **tiling):
        """Image.render (Image.fs:26-35) -> (FColor[X,Y] as float32 [n_columns, Y, 3], stats dict).  `out`: a float32 array
        of that shape to render into (e.g. one page-locked with Device.host_register)."""
        p = self._params(imageSize, epsilon, length, **tiling)
        out = self._image(out, (p.n_columns, p.height, 3), "(n_columns, Y, 3)")
        return out, self._call(lib.ft_render, C.byref(camera._c), C.byref(p), _hptr(out))

    def render_device(self, epsilon, length, imageSize, camera, d_out_ptr, **tiling):
        """asynchronous render into device memory (pointer as int); pair with collect_stats()."""
        p = self._params(imageSize, epsilon, length, **tiling)
        check(lib.ft_render_device(self.device._ctx, self._scene, C.byref(camera._c), C.byref(p), _dptr(d_out_ptr)))
        return p.n_columns

    def render_hits(self, epsilon, length, imageSize, camera, shade=False, material=True, records=True, **tiling_and_ext):
        """EXTENSION ft_render_hits: per-pixel SdfObject.tryTrace of the camera rays -> (PixelHits, image or None, stats).
        shade: also render the frame (bit-identical to render() with the same parameters, same launch); without it one ray
        per pixel is traced and spp / ao_samples / max_bounces / spectral do not apply.  material / records: which planes to return."""
        p = self._params(imageSize, epsilon, length, **tiling_and_ext)
        (img, rec, mat), ptrs = _host_outputs((p.n_columns, p.height), shade, records, material)
        st = self._call(lib.ft_render_hits, C.byref(camera._c), C.byref(p), *ptrs)
        return PixelHits(rec, mat, self.materials), img, st

    def render_hits_device(self, epsilon, length, imageSize, camera, d_hits_ptr, d_material_ptr=None, d_out_ptr=None, **tiling_and_ext):
        """asynchronous ft_render_hits_device into device memory (pointers as int, None = not asked; the records 16-byte
        aligned, n_columns x Y x 16 float32); pair with collect_stats()."""
        p = self._params(imageSize, epsilon, length, **tiling_and_ext)
        check(lib.ft_render_hits_device(self.device._ctx, self._scene, C.byref(camera._c), C.byref(p), _dptr(d_out_ptr), _dptr(d_hits_ptr), _dptr(d_material_ptr)))
        return p.n_columns

    def render_views(self, epsilon, length, imageSize, cameras, out=None, **tiling_and_ext):
        """ft_render_views: Image.render of one scene from each camera of `cameras` in one job queue -> (float32 [K, n_columns, Y, 3],
        stats dict of the whole batch).  Block k is bit for bit render(..., cameras[k], **tiling_and_ext)[0].  `out`: a float32 array of
        that shape to render into."""
        p = self._params(imageSize, epsilon, length, **tiling_and_ext)
        arr, k = self._cameras(cameras)
        out = self._image(out, (k, p.n_columns, p.height, 3), "(n_views, n_columns, Y, 3)")
        return out, self._call(lib.ft_render_views, arr, k, C.byref(p), _hptr(out))

    def render_views_device(self, epsilon, length, imageSize, cameras, d_out_ptr, **tiling_and_ext):
        """asynchronous ft_render_views_device into device memory (pointer as int; n_views x n_columns x Y x 3 float32); pair with
        collect_stats()."""
        p = self._params(imageSize, epsilon, length, **tiling_and_ext)
        arr, k = self._cameras(cameras)
        check(lib.ft_render_views_device(self.device._ctx, self._scene, arr, k, C.byref(p), _dptr(d_out_ptr)))
        return p.n_columns

    def render_views_hits(self, epsilon, length, imageSize, cameras, shade=False, material=True, records=True, **tiling_and_ext):
        """EXTENSION ft_render_views_hits: render_hits of one scene from each camera of `cameras` in one job queue -> (PixelHits with
        records float32 [K, n_columns, Y, 16] and material int32 [K, n_columns, Y], image float32 [K, n_columns, Y, 3] or None, stats
        of the whole batch).  Block k of each is bit for bit render_hits(..., cameras[k], shade, **tiling_and_ext)'s."""
        p = self._params(imageSize, epsilon, length, **tiling_and_ext)
        arr, k = self._cameras(cameras)
        (img, rec, mat), ptrs = _host_outputs((k, p.n_columns, p.height), shade, records, material)
        st = self._call(lib.ft_render_views_hits, arr, k, C.byref(p), *ptrs)
        return PixelHits(rec, mat, self.materials), img, st

    def render_views_hits_device(self, epsilon, length, imageSize, cameras, d_hits_ptr, d_material_ptr=None, d_out_ptr=None, **tiling_and_ext):
        """asynchronous ft_render_views_hits_device into device memory (pointers as int, None = not asked; view-major, the records
        16-byte aligned, n_views x n_columns x Y x 16 float32); pair with collect_stats()."""
        p = self._params(imageSize, epsilon, length, **tiling_and_ext)
        arr, k = self._cameras(cameras)
        check(lib.ft_render_views_hits_device(self.device._ctx, self._scene, arr, k, C.byref(p), _dptr(d_out_ptr), _dptr(d_hits_ptr), _dptr(d_material_ptr)))
        return p.n_columns

    def collect_stats(self):
        st = _lib.Stats()
        check(lib.ft_collect_stats(self.device._ctx, C.byref(st)))
        return st.as_dict()

    def render_colors(self, epsilon, length, imageSize, camera, gamma=2.2, seed=None, bmp_order=False, **ext):
        """Program.fs:90-100 on the device: Image.render, then Image.toColors gamma (and, with bmp_order, the scan-line
        order of Image.toBitmap) — only 3 bytes per pixel leave the GPU.  seed None: no dithering noise (u = 0.5).
        Returns (uint8 [X, Y, 3] R,G,B — or [Y, X, 3] B,G,R rows from the top with bmp_order —, max, stats)."""
        p = self._params(imageSize, epsilon, length, **ext)
        tm = _tonemap_params(gamma, seed, bmp_order)
        out = np.empty((p.height, p.width, 3) if bmp_order else (p.width, p.height, 3), np.uint8)
        mx = C.c_float()
        st = self._call(lib.ft_render_colors, C.byref(camera._c), C.byref(p), C.byref(tm), _hptr(out), C.byref(mx))
        return out, float(mx.value), st

    # ---- ray buffers: host arrays (numpy) or device tensors ------------------------------------------------------------
    def _trace_buffer(self, rays, host_fn, device_fn, widths):
        """Where a ray-buffer method decides between a host array and a device tensor (see is_device_tensor) -> (outputs, stats); the record
        methods have _record_form, the field methods _field.  widths: per output of the C call its row width — float32 [n, w]; 0: int32 [n];
        None: not asked for.  A host array goes through host_fn (the ft_* host form), n = 0 included; a device tensor (checked: float32 [n, 8],
        contiguous) is traced where it lies by device_fn on the caller's current stream, n = 0 included, the outputs are tensors of its device
        and stats is None: fetch them with collect_stats() when needed."""
        like = rays if is_device_tensor(rays) else None
        if like is None:
            rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = rays.shape[0] if like is None else check_device_rays(rays)
        outs = [None if w is None else _empty(like, (n, w)) if w else _empty(like, (n,), "int32") for w in widths]
        if like is None:
            return outs, self._call(host_fn, _hptr(rays), n, *map(_hptr, outs))
        with self.device.on_current_stream(rays):
            device_fn(rays.data_ptr(), n, *(None if o is None else o.data_ptr() for o in outs))
        return outs, None

    def trace_rays(self, rays):
        """SdfScene.trace over n rays given as float32 [n, 8] (Origin, Direction, Length, Epsilon) -> (float32 [n, 3], stats).
        A device tensor (see is_device_tensor) is traced in place by ft_trace_rays_device on the caller's current stream and the colours come
        back as a tensor of the same device; stats is then None: fetch them with collect_stats() when needed."""
        (out,), st = self._trace_buffer(rays, lib.ft_trace_rays, self.trace_rays_device, (3,))
        return out, st

    def form_try_trace(self, rays):
        """SdfForm.tryTrace scene.Object.Form over rays [n, 8] (SdfForm.fs:93-104) -> float32 [n, 10]:
        Ray at the hit (8), Distance, hit flag (int32 bits; 0 = ValueNone, row is zeros).  Device tensors as in trace_rays."""
        (out,), st = self._trace_buffer(rays, lib.ft_form_try_trace, self.form_try_trace_device, (10,))
        return out, st

    def object_try_trace(self, rays):
        """SdfObject.tryTrace scene.Object over rays [n, 8] (SdfObject.fs:66-78) -> float32 [n, 16]:
        Ray pulled back by epsilon (8), Normal (3), Color (3), hit flag (int32 bits), 0.  Device tensors as in trace_rays."""
        (out,), st = self._trace_buffer(rays, lib.ft_object_try_trace, self.object_try_trace_device, (16,))
        return out, st

    def trace_rays_hits(self, rays, shade=True, records=True, material=True):
        """EXTENSION ft_trace_rays_hits: SdfScene.trace and SdfObject.tryTrace of every ray [n, 8] in one launch -> (PixelHits with records
        float32 [n, 16] and material int32 [n], colours float32 [n, 3] or None, stats).  Ray i: colours = trace_rays, records =
        object_try_trace, material = the handle render_hits reports for a pixel with that camera ray.  shade=False: hits only, no lighting
        and no shadow rays.  Device tensors as in trace_rays: results are tensors of the rays' device (material int32), stats is None."""
        if not (shade or records or material):
            raise ValueError("trace_rays_hits: no output asked for")
        widths = (3 if shade else None, 16 if records else None, 0 if material else None)
        (rgb, rec, mat), st = self._trace_buffer(rays, lib.ft_trace_rays_hits, self.trace_rays_hits_device, widths)
        return PixelHits(rec, mat, self.materials), rgb, st

    # raw device pointers (int; None = not asked): rays n x 32 B and object records 16-byte aligned, no scratch, no copy, asynchronous on the
    # context's stream; pair with collect_stats()
    def trace_rays_device(self, d_rays_ptr, n, d_out_ptr):
        """asynchronous ft_trace_rays_device: n x 3 float32 colours at d_out_ptr"""
        check(lib.ft_trace_rays_device(self.device._ctx, self._scene, _dptr(d_rays_ptr), n, _dptr(d_out_ptr)))

    def form_try_trace_device(self, d_rays_ptr, n, d_out_ptr):
        """asynchronous ft_form_try_trace_device: n x 10 dwords at d_out_ptr"""
        check(lib.ft_form_try_trace_device(self.device._ctx, self._scene, _dptr(d_rays_ptr), n, _dptr(d_out_ptr)))

    def object_try_trace_device(self, d_rays_ptr, n, d_out_ptr, d_material_ptr=None):
        """asynchronous ft_object_try_trace_device: n x 16 dwords at d_out_ptr and, if asked, n int32 material handles (-1: miss)"""
        check(lib.ft_object_try_trace_device(self.device._ctx, self._scene, _dptr(d_rays_ptr), n, _dptr(d_out_ptr), _dptr(d_material_ptr)))

    def trace_rays_hits_device(self, d_rays_ptr, n, d_out_ptr=None, d_hits_ptr=None, d_material_ptr=None):
        """asynchronous ft_trace_rays_hits_device: colours, records and material handles of n rays in one launch (any two may be None)"""
        check(lib.ft_trace_rays_hits_device(self.device._ctx, self._scene, _dptr(d_rays_ptr), n, _dptr(d_out_ptr), _dptr(d_hits_ptr),
                                            _dptr(d_material_ptr)))

    # ---- relighting: hit records in, colours out ------------------------------------------------------------------------
    def shade_hits(self, hits):
        """ft_shade_hits: SdfScene.trace from its hit on (SdfScene.fs:11-28) for every record of `hits` — a PixelHits, a float32 array
        [..., 16] or a device tensor of that shape (see is_device_tensor) -> (float32 [..., 3], stats).  Records written under a scene that
        shares this scene's Object (see relight) shade to what this scene's trace_rays / render gives, bit for bit, without a primary march;
        records are data and may be edited first (colour, normal; hit = 0 gives the background).  A device tensor is shaded where it lies
        by ft_shade_hits_device on the caller's current stream, the colours are a tensor of its device and stats is None."""
        rec, lead, n = self._records(hits)
        return self._record_form(rec, n, lead + (3,), "float32", lambda out: self._call(lib.ft_shade_hits, _hptr(rec), n, out),
                                 lambda out: self.shade_hits_device(rec.data_ptr(), n, out))

    def shade_hits_device(self, d_hits_ptr, n, d_out_ptr):
        """asynchronous ft_shade_hits_device: n records (64 B each, 16-byte aligned) at d_hits_ptr -> n x 3 float32 colours at d_out_ptr
        (pointers as int); no scratch, no copy; pair with collect_stats()."""
        check(lib.ft_shade_hits_device(self.device._ctx, self._scene, _dptr(d_hits_ptr), n, _dptr(d_out_ptr)))

    # ---- light visibility masks: the shadow marches kept as bits, and shading from the bits ------------------------------
    @staticmethod
    def _records(hits):
        """the record buffer of a PixelHits, an array or a device tensor (a host array made contiguous) -> (buffer, leading shape, record count)"""
        rec = _buffer(hits)
        lead = check_hit_records(rec)
        return rec if is_device_tensor(rec) else np.ascontiguousarray(rec), lead, int(np.prod(lead, dtype=np.int64))

    @staticmethod
    def _masks(m, rec, lead, what):
        """visibility masks for the records `rec`: checked (check_visibility) and lying where the records lie; a host array made contiguous"""
        m = _buffer(m)
        if is_device_tensor(rec) != is_device_tensor(m):
            raise ValueError(f"{what}: must lie where the records lie (device tensor or numpy array)")
        check_visibility(m, lead, what)
        return m if is_device_tensor(m) else np.ascontiguousarray(m)

    def _record_form(self, rec, n, shape, kind, host, device):
        """Where a record method (shade_hits, light_visibility, shade_visible) decides between host arrays and device tensors -> (output, stats).
        The output (_empty: shape, kind) lies where the n records `rec` lie.  Device tensor: device(output address) launches on the caller's
        current stream, only if there is a record, and stats is None.  Host array: host(output pointer) calls the ft_* host form and returns
        its stats; without a record there is no call and the stats are zero."""
        if is_device_tensor(rec):
            out = _empty(rec, shape, kind)
            if n:
                with self.device.on_current_stream(rec):
                    device(out.data_ptr())
            return out, None
        out = _empty(None, shape, kind)
        return out, host(_hptr(out)) if n else _lib.Stats().as_dict()

    def light_visibility(self, hits, select=None, previous=None):
        """ft_light_visibility: one shadow march per selected light and record of `hits` (a PixelHits, float32 [..., 16] or a device tensor,
        as for shade_hits) -> (uint32 masks shaped like the records without their last axis, stats): bit i is set where light i reaches the
        record, i.e. where SdfScene.fs:23 executes.  select: a bit mask of the lights to march (None: all); previous: masks whose other bits
        are kept (None: none), so that after one light has moved only its own shadow rays are cast.  The bits depend on the Object, the records
        and the lights' directions and positions, never on a colour.  Device records give an int32 tensor holding the same bits (previous: such
        a tensor), on the caller's current stream, and stats None."""
        rec, lead, n = self._records(hits)
        sel = 0xFFFFFFFF if select is None else int(select) & 0xFFFFFFFF
        prev = None if previous is None else self._masks(previous, rec, lead, "previous")
        return self._record_form(rec, n, lead, "mask", lambda out: self._call(lib.ft_light_visibility, _hptr(rec), n, sel, _hptr(prev), out),
                                 lambda out: self.light_visibility_device(rec.data_ptr(), n, out, sel, None if prev is None else prev.data_ptr()))

    def light_visibility_device(self, d_hits_ptr, n, d_vis_out_ptr, select=0xFFFFFFFF, d_vis_in_ptr=None):
        """asynchronous ft_light_visibility_device: n records (64 B each, 16-byte aligned) at d_hits_ptr -> n uint32 masks at d_vis_out_ptr;
        d_vis_in_ptr: masks to keep the unselected bits of (None: none; may be d_vis_out_ptr).  Pointers as int; pair with collect_stats()."""
        check(lib.ft_light_visibility_device(self.device._ctx, self._scene, _dptr(d_hits_ptr), n, select, _dptr(d_vis_in_ptr), _dptr(d_vis_out_ptr)))

    def shade_visible(self, hits, visibility):
        """ft_shade_visible: the colours of `hits` under this scene's lights and background with every shadow ray answered by `visibility`
        (what light_visibility returned for a scene with the same Object and the same light directions and positions) -> (float32 [..., 3],
        stats).  No march runs: a memory pass.  Equal bit for bit to shade_hits / trace_rays under this scene; records may be recoloured first.
        A mask is data: a set bit adds its light whatever the cosine.  Device records take an int32 mask tensor and give a tensor; stats None."""
        rec, lead, n = self._records(hits)
        vis = self._masks(visibility, rec, lead, "visibility")
        return self._record_form(rec, n, lead + (3,), "float32", lambda out: self._call(lib.ft_shade_visible, _hptr(rec), _hptr(vis), n, out),
                                 lambda out: self.shade_visible_device(rec.data_ptr(), vis.data_ptr(), n, out))

    def shade_visible_device(self, d_hits_ptr, d_visibility_ptr, n, d_out_ptr):
        """asynchronous ft_shade_visible_device: n records and n uint32 masks -> n x 3 float32 colours (pointers as int; records 16-byte
        aligned); a streaming kernel on the context's stream; pair with collect_stats()."""
        check(lib.ft_shade_visible_device(self.device._ctx, self._scene, _dptr(d_hits_ptr), _dptr(d_visibility_ptr), n, _dptr(d_out_ptr)))

    # ---- the distance field itself: lattices and point buffers ------------------------------------------------------------
    def _field(self, lead, like, launch_host, launch_device, normal_epsilon, distance, material, bounded):
        """Where a field method decides between host arrays and device tensors -> FieldSamples.  like: None (numpy outputs through launch_host,
        which is called whatever the point count: ft_sample_points itself has nothing to do for none) or a device tensor, whose device the
        outputs are allocated on and whose current stream launch_device runs on, only if there is a point."""
        normal = normal_epsilon is not None
        if not (distance or normal or material):
            raise ValueError("field: no output asked for")
        eps = float(normal_epsilon) if normal else 0.0
        flags = _lib.FT_FIELD_BOUNDED if bounded else 0
        outs = (_empty(like, lead) if distance else None, _empty(like, lead + (3,)) if normal else None,
                _empty(like, lead, "int32") if material else None)
        if like is None:
            launch_host(eps, flags, *map(_hptr, outs))
        elif int(np.prod(lead, dtype=np.int64)):
            with self.device.on_current_stream(like):
                launch_device(eps, flags, *(None if o is None else o.data_ptr() for o in outs))
        return FieldSamples(*outs, materials=self.materials)

    def sample_points(self, points, normal_epsilon=None, material=False, bounded=False, distance=True):
        """ft_sample_points: scene.Object.Form.Distance at points [..., 3] -> FieldSamples shaped like the points without their last axis.
        normal_epsilon: also SdfForm.normal sdf normal_epsilon p (SdfForm.fs:106-112); material: also the handle of the material
        object.Material.Color picks at p (FieldSamples.descriptor); bounded: SdfForm.tryDistance — outside SdfBoundary.isInside nothing is
        evaluated, distance and normal are NaN, the material -1.  A device tensor (see is_device_tensor; float32, contiguous) is sampled where
        it lies by ft_sample_points_device on the caller's current stream and the results are tensors of its device."""
        ctx, sc = self.device._ctx, self._scene
        if is_device_tensor(points):
            lead = check_device_points(points)
            n = int(np.prod(lead, dtype=np.int64))
            return self._field(lead, points, None, lambda e, f, *o: self.sample_points_device(points.data_ptr(), n, *o, normal_epsilon=e, flags=f),
                               normal_epsilon, distance, material, bounded)
        pts = np.ascontiguousarray(points, dtype=np.float32)
        if pts.ndim < 1 or pts.shape[-1] != 3:
            raise ValueError(f"points: shape must be [..., 3], not {list(pts.shape)}")
        n = pts.size // 3
        return self._field(pts.shape[:-1], None, lambda e, f, *o: check(lib.ft_sample_points(ctx, sc, _hptr(pts), n, e, f, *o)), None,
                           normal_epsilon, distance, material, bounded)

    def sample_lattice(self, origin, step, counts, normal_epsilon=None, material=False, bounded=False, distance=True, like=None):
        """ft_sample_lattice: sample_points on lattice_points(origin, step, counts) without any point array -> FieldSamples with distance
        [nx, ny, nz], normal [nx, ny, nz, 3], material [nx, ny, nz].  like: a device tensor — the results are then tensors of its device,
        written by ft_sample_lattice_device on the caller's current stream."""
        lat, n = _lattice(origin, step, counts)
        ctx, sc = self.device._ctx, self._scene
        if like is not None and not is_device_tensor(like):
            raise ValueError("like: a device tensor (see is_device_tensor) or None")
        return self._field(n, like, lambda e, f, *o: check(lib.ft_sample_lattice(ctx, sc, C.byref(lat), e, f, *o)),
                           lambda e, f, *o: check(lib.ft_sample_lattice_device(ctx, sc, C.byref(lat), e, f, *map(_dptr, o))),
                           normal_epsilon, distance, material, bounded)

    def mesh_lattice(self, origin, step, counts, iso=0.0, normal_epsilon=None, material=False, like=None, refine=None, shells=False, keep=None, measures=False):
        """ft_mesh_lattice: the surface scene.Object.Form.Distance = iso as triangles, extracted on the device from the distances on
        lattice_points(origin, step, counts) (never bounded) -> Mesh.  normal_epsilon: also SdfForm.normal sdf normal_epsilon v per vertex;
        material: also the handle of the material object.Material.Color picks at v (Mesh.descriptor) — both exactly what sample_points gives
        for the vertices.  like: a device tensor — the Mesh then holds tensors of its device, and the launches run on the caller's current
        stream.  refine: None, or the bisection rounds (0 .. 32) of ft_mesh_lattice_refined: every vertex moves along its lattice edge onto
        the surface, to within the edge's length * 2^-refine; triangles are unchanged, normals and materials are taken at the refined vertices.
        shells: the Mesh carries `.shells`, its connected pieces labelled on the device (ft_mesh_shells).  keep (implies shells): only some shells,
        through ft_mesh_select — an int k (the k shells with the most triangles, ties going to the lower number), "closed", a bool array of
        length S or a callable Shells -> bool array; `.shells` are then those of the selected mesh.  measures (implies shells): `.shells.measures`
        holds each shell's area, signed volume, first moment and box and `.measure` the whole mesh's, computed on the device (ft_shells_measure,
        ft_mesh_measure; with keep: of the selected mesh); the callable form of keep then receives Shells that carry their measures, and
        keep="bodies" keeps the closed shells of positive volume: no cavities, no debris of open pieces."""
        lat, _ = _lattice(origin, step, counts)
        if like is not None and not is_device_tensor(like):
            raise ValueError("like: a device tensor (see is_device_tensor) or None")
        flags = (_lib.FT_MESH_NORMAL if normal_epsilon is not None else 0) | (_lib.FT_MESH_MATERIAL if material else 0)
        eps = float(normal_epsilon) if normal_epsilon is not None else 0.0
        handle = C.c_void_p()
        with (self.device.on_current_stream(like) if like is not None else contextlib.nullcontext()):
            if refine is None:
                check(lib.ft_mesh_lattice(self.device._ctx, self._scene, C.byref(lat), float(iso), eps, flags, C.byref(handle)))
            else:
                check(lib.ft_mesh_lattice_refined(self.device._ctx, self._scene, C.byref(lat), float(iso), eps, flags, int(refine), C.byref(handle)))
            return _read_mesh(handle, like, self.materials, shells, keep, measures)

    def slice_lattice(self, origin, step, counts, axis=2, iso=0.0, normal_epsilon=None, material=False, like=None, refine=None, measures=False):
        """ft_slice_lattice: the contours scene.Object.Form.Distance = iso of every lattice plane normal to `axis` (0, 1, 2: x, y, z), extracted
        and chained on the device from the distances on lattice_points(origin, step, counts) (never bounded) -> Contours.  normal_epsilon: also
        SdfForm.normal per point; material: also the handle of the material object.Material.Color picks there (Contours.descriptor) — both
        exactly what sample_points gives for the points.  like: a device tensor — the Contours then hold tensors of its device, and the launches
        run on the caller's current stream.  refine: None, or the bisection rounds (0 .. 32) of ft_slice_lattice_refined: the points are then the
        refined mesh vertices of the same edges (mesh_lattice), the polylines unchanged.  measures: `.measures` holds each polyline's length, signed
        area, first moment and box in the plane and `.layer_measures` the same per slice, holes subtracted, with the slice's outer loops and holes
        counted, computed on the device (ft_slices_measure)."""
        lat, _ = _lattice(origin, step, counts)
        if like is not None and not is_device_tensor(like):
            raise ValueError("like: a device tensor (see is_device_tensor) or None")
        flags = (_lib.FT_SLICE_NORMAL if normal_epsilon is not None else 0) | (_lib.FT_SLICE_MATERIAL if material else 0)
        eps = float(normal_epsilon) if normal_epsilon is not None else 0.0
        handle = C.c_void_p()
        with (self.device.on_current_stream(like) if like is not None else contextlib.nullcontext()):
            if refine is None:
                check(lib.ft_slice_lattice(self.device._ctx, self._scene, C.byref(lat), int(axis), float(iso), eps, flags, C.byref(handle)))
            else:
                check(lib.ft_slice_lattice_refined(self.device._ctx, self._scene, C.byref(lat), int(axis), float(iso), eps, flags, int(refine), C.byref(handle)))
            return _read_slices(handle, like, self.materials, measures)

    def refine_segments(self, a, b, iso=0.0, steps=8):
        """ft_refine_segments: where the segments from a [..., 3] to b [..., 3] cross scene.Object.Form.Distance = iso -> (points float32 [..., 3],
        status int32 [...]).  status 1: exactly one end is inside (distance - iso < 0) and both distances are finite; the point is then the
        bracket's interpolation after `steps` (0 .. 32) bisection rounds, within |b - a| * 2^-steps of the surface: a crossing, not
        necessarily the first.  status 0: the point is three NaN.  Device tensors (see is_device_tensor; float32, contiguous, same shape) are
        refined where they lie by ft_refine_segments_device on the caller's current stream, and the results are tensors of their device."""
        ctx, sc = self.device._ctx, self._scene
        if is_device_tensor(a) or is_device_tensor(b):
            if not (is_device_tensor(a) and is_device_tensor(b)):
                raise ValueError("segments: both ends must be device tensors, or neither")
            lead = check_device_points(a)
            if check_device_points(b) != lead:
                raise ValueError(f"segments: the ends' shapes differ: {list(a.shape)} and {list(b.shape)}")
            n = int(np.prod(lead, dtype=np.int64))
            points, status = _empty(a, lead + (3,)), _empty(a, lead, "int32")
            if n:
                with self.device.on_current_stream(a):
                    self.refine_segments_device(a.data_ptr(), b.data_ptr(), n, points.data_ptr(), status.data_ptr(), iso=iso, steps=steps)
            return points, status
        pa, pb = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
        if pa.ndim < 1 or pa.shape[-1] != 3 or pa.shape != pb.shape:
            raise ValueError(f"segments: both shapes must be the same [..., 3], not {list(pa.shape)} and {list(pb.shape)}")
        points, status = np.empty(pa.shape, np.float32), np.empty(pa.shape[:-1], np.int32)
        check(lib.ft_refine_segments(ctx, sc, _hptr(pa), _hptr(pb), pa.size // 3, float(iso), int(steps), _hptr(points), _hptr(status)))
        return points, status

    def refine_segments_device(self, d_a_ptr, d_b_ptr, n, d_point_ptr=None, d_status_ptr=None, iso=0.0, steps=8):
        """asynchronous ft_refine_segments_device: n segments (ends 12 B apart at d_a_ptr, d_b_ptr) -> n x 3 float32 points, n int32 status
        (pointers as int, None = not asked; every buffer 4-byte aligned); on the context's stream, not synchronised"""
        check(lib.ft_refine_segments_device(self.device._ctx, self._scene, _dptr(d_a_ptr), _dptr(d_b_ptr), n, float(iso), int(steps),
                                            _dptr(d_point_ptr), _dptr(d_status_ptr)))

    def sample_points_device(self, d_points_ptr, n, d_distance_ptr=None, d_normal_ptr=None, d_material_ptr=None, normal_epsilon=0.0, flags=0):
        """asynchronous ft_sample_points_device: n points (12 B each) at d_points_ptr -> n float32 distances, n x 3 float32 normals, n int32
        material handles (pointers as int, None = not asked; every buffer 4-byte aligned); no scratch, no copy, on the context's stream"""
        check(lib.ft_sample_points_device(self.device._ctx, self._scene, _dptr(d_points_ptr), n, normal_epsilon, flags,
                                          _dptr(d_distance_ptr), _dptr(d_normal_ptr), _dptr(d_material_ptr)))

    def sample_lattice_device(self, origin, step, counts, d_distance_ptr=None, d_normal_ptr=None, d_material_ptr=None, normal_epsilon=0.0, flags=0):
        """asynchronous ft_sample_lattice_device: the lattice's nx x ny x nz results, k contiguous, at the given device addresses (as above)"""
        lat, _ = _lattice(origin, step, counts)
        check(lib.ft_sample_lattice_device(self.device._ctx, self._scene, C.byref(lat), normal_epsilon, flags,
                                           _dptr(d_distance_ptr), _dptr(d_normal_ptr), _dptr(d_material_ptr)))

    def eval_distance(self, points):
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        d = np.empty(pts.shape[0], np.float32)
        m = np.empty(pts.shape[0], np.int32)
        check(lib.ft_eval_distance(self.device._ctx, self._scene, pts.ctypes.data_as(C.c_void_p), pts.shape[0],
                                   d.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p)))
        return d, m


def _tonemap_params(gamma, seed, bmp_order):
    return _lib.TonemapParams(float(gamma), 0 if seed is None else 1, 0 if seed is None else int(seed) & 0xFFFFFFFF, 1 if bmp_order else 0)


def tone_map_device(device, d_frame_ptr, X, Y, gamma=2.2, seed=None, bmp_order=False, d_out_ptr=None):
    """Image.toColors on a frame that sits in HBM (pointer as int).  With d_out_ptr the 8-bit image stays on the device
    (asynchronous, returns None); otherwise it is copied to the host: (uint8 array, max)."""
    tm = _tonemap_params(gamma, seed, bmp_order)
    if d_out_ptr is not None:
        check(lib.ft_tone_map_device(device._ctx, C.c_void_p(d_frame_ptr), int(X), int(Y), C.byref(tm), C.c_void_p(d_out_ptr)))
        return None
    out = np.empty((Y, X, 3) if bmp_order else (X, Y, 3), np.uint8)
    mx = C.c_float()
    check(lib.ft_tone_map(device._ctx, C.c_void_p(d_frame_ptr), int(X), int(Y), C.byref(tm), out.ctypes.data_as(C.c_void_p), C.byref(mx)))
    return out, float(mx.value)


def spectral_table(nw):
    """EXTENSION: the library's wavelength table, float32 [nw, 4] = rgb weight, Cauchy term (ft_spectral_table)."""
    out = np.empty((int(nw), 4), np.float32)
    check(lib.ft_spectral_table(int(nw), out.ctypes.data_as(C.c_void_p)))
    return out


def render_multi(devices, scene, epsilon, length, imageSize, camera, stripe_width=16):
    """ft_render_multi: single-process multi-GPU render (one host thread + context per device inside the
    library, column stripes, ONE ncclGather to devices[0], de-interleave on the way to the host).
    Returns (float32 [X, Y, 3], stats)."""
    scenes = [devices[0].scene(scene)]
    for d in devices[1:]:
        p = C.c_void_p()
        check(lib.ft_scene_clone(scenes[0]._scene, d._ctx, C.byref(p)))
        clone = DeviceScene.__new__(DeviceScene)
        clone.device, clone._scene = d, p
        scenes.append(clone)
    n = len(devices)
    ctxs = (C.c_void_p * n)(*[d._ctx for d in devices])
    scs = (C.c_void_p * n)(*[s._scene for s in scenes])
    W, H = int(imageSize.X), int(imageSize.Y)
    p = _lib.RenderParams(W, H, 0, W, int(stripe_width), 1, 0, 1, float(epsilon), float(length), 0, 0.0, 0, 0)
    out = np.empty((W, H, 3), np.float32)
    st = _lib.Stats()
    try:
        check(lib.ft_render_multi(ctxs, scs, n, C.byref(camera._c), C.byref(p), out.ctypes.data_as(C.c_void_p), C.byref(st)))
    finally:
        for s in scenes[1:]:
            s.close()
    return out, st.as_dict()


class SceneTrace:
    """The value `SdfScene.trace scene`: callable on one ray (8 floats) -> FColor."""

    def __init__(self, scene, device=None):
        self.scene = scene
        self.device = device

    def resolve(self):
        dev = self.device if self.device is not None else Device.default(0)
        return dev.scene(self.scene)

    def __call__(self, ray):
        if is_device_tensor(ray):                                  # a ray buffer [n, 8] in device memory -> colours [n, 3] there
            return self.resolve().trace_rays(ray)[0]
        out, _ = self.resolve().trace_rays(np.asarray(ray, np.float32).reshape(1, 8))
        return FColor(tuple(float(c) for c in out[0]))


# --------------------------------------------------------------------------------------------------
# Camera.fs / Image.fs
# --------------------------------------------------------------------------------------------------
class Lens:
    def __init__(self, NearPlaneSize):
        self.NearPlaneSize = float(NearPlaneSize)

    @staticmethod
    def create(fieldOfView):
        """Camera.fs:11-14: sin(fov * 0.5) — radians, as in the reference (Program.fs:21 passes 60.0f)."""
        return Lens(lib.ft_lens_create(float(np.float32(fieldOfView))))


class Camera:
    def __init__(self, c):
        self._c = c

    @staticmethod
    def lookAt(Position, LookAt, Up, Lens):
        c = _lib.CameraS()
        check(lib.ft_camera_look_at(_f3(_v3(Position)), _f3(_v3(LookAt)), _f3(_v3(Up)), Lens.NearPlaneSize, C.byref(c)))
        return Camera(c)

    def as_array(self):
        return np.frombuffer(bytes(self._c), dtype=np.float32).copy()

    @staticmethod
    def uniformPixelToRay(epsilon, length, camera, position):
        """Camera.uniformPixelToRay (Camera.fs:44-54), host side, float32 operation by operation:
        Direction = normalize(Forward + (px - 0.5) * RightScaled + (py - 0.5) * UpScaled) -> ray as 8 floats
        (Origin, Direction, Length, Epsilon; Types.fs:9-17)."""
        F = np.float32
        a = camera.as_array()
        pos, fw, up, rt = a[0:3], a[3:6], a[6:9], a[9:12]
        px, py = F(position[0]), F(position[1])
        d = (fw + F(px - F(0.5)) * rt) + F(py - F(0.5)) * up
        d = d / np.sqrt(F(F(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
        return np.concatenate([pos, d, [F(length), F(epsilon)]]).astype(F)

    Position = property(lambda s: (s._c.position.x, s._c.position.y, s._c.position.z))
    Forward = property(lambda s: (s._c.forward.x, s._c.forward.y, s._c.forward.z))
    UpScaled = property(lambda s: (s._c.up_scaled.x, s._c.up_scaled.y, s._c.up_scaled.z))
    RightScaled = property(lambda s: (s._c.right_scaled.x, s._c.right_scaled.y, s._c.right_scaled.z))


class ImageSize:
    def __init__(self, X, Y):
        self.X, self.Y = int(X), int(Y)

    @staticmethod
    def getUniformPixelPos(size):
        """ImageSize.getUniformPixelPos (Image.fs:17-23): (x, y) -> (x / max(X, Y), y / max(X, Y)) in float32"""
        m = np.float32(max(size.X, size.Y))
        return lambda x, y: (np.float32(x) / m, np.float32(y) / m)


class Ray:
    """Ray.fs:6-15 on rays stored as 8 floats (Origin, Direction, Length, Epsilon)"""

    @staticmethod
    def get(length, ray):
        r = np.asarray(ray, np.float32)
        return r[0:3] + r[3:6] * np.float32(length)

    @staticmethod
    def move(length, ray):
        r = np.asarray(ray, np.float32).copy()
        r[0:3] = Ray.get(length, ray)
        r[6] = r[6] - np.float32(length)
        return r

    @staticmethod
    def setDirection(direction, ray):
        r = np.asarray(ray, np.float32).copy()
        r[3:6] = np.asarray(direction, np.float32)
        return r


class Image:
    @staticmethod
    def render(epsilon, length, imageSize, camera, trace):
        """Image.render epsilon length imageSize camera trace (Image.fs:26-35).  `trace` must be the
        value of SdfScene.trace (an opaque Python closure cannot run on the GPU); returns the
        FColor[X,Y] image as a float32 array [X, Y, 3]."""
        if not isinstance(trace, SceneTrace):
            raise TypeError("Image.render needs `SdfScene.trace scene`; arbitrary closures have no GPU form")
        img, _ = trace.resolve().render(epsilon, length, imageSize, camera)
        return img

    @staticmethod
    def renderScene(epsilon, length, imageSize, camera, scene, device=None):
        return Image.render(epsilon, length, imageSize, camera, SdfScene.trace(scene, device))

    @staticmethod
    def renderViews(epsilon, length, imageSize, cameras, scene, device=None):
        """Image.render of one scene from every camera of `cameras` in one launch (ft_render_views) -> float32 [K, X, Y, 3]; image k is
        Image.renderScene epsilon length imageSize cameras[k] scene."""
        dev = device if device is not None else Device.default(0)
        img, _ = dev.scene(scene).render_views(epsilon, length, imageSize, cameras)
        return img

    @staticmethod
    def renderHits(epsilon, length, imageSize, camera, scene, device=None):
        """EXTENSION: Image.render's pixel loop (Image.fs:26-35) over SdfObject.tryTrace scene.Object (SdfObject.fs:66-78) instead of
        SdfScene.trace: the SdfObjectTraceResult voption of every pixel as PixelHits (records [X, Y, 16], material handles)."""
        dev = device if device is not None else Device.default(0)
        hits, _, _ = dev.scene(scene).render_hits(epsilon, length, imageSize, camera)
        return hits

    @staticmethod
    def renderViewsHits(epsilon, length, imageSize, cameras, scene, device=None):
        """EXTENSION: Image.renderHits of one scene from every camera of `cameras` in one launch (ft_render_views_hits) -> PixelHits with
        records [K, X, Y, 16] and material handles [K, X, Y]; view k is Image.renderHits epsilon length imageSize cameras[k] scene."""
        dev = device if device is not None else Device.default(0)
        hits, _, _ = dev.scene(scene).render_views_hits(epsilon, length, imageSize, cameras)
        return hits

    @staticmethod
    def toColors(gamma, rng, image, device=None, bmp_order=False):
        """Image.toColors gamma rng image (Image.fs:37-50) on the GPU for a host FColor[X,Y] (float32 [X, Y, 3]) ->
        uint8 [X, Y, 3].  `rng`: None = no dithering noise (u = 0.5); an int = seed of the counter-based noise (the
        reference's shared System.Random is racy, so its low bit is not reproducible: +-1 LSB comparable)."""
        img = np.ascontiguousarray(image, dtype=np.float32)
        X, Y = img.shape[0], img.shape[1]
        dev = device if device is not None else Device.default(0)
        tm = _tonemap_params(gamma, rng, bmp_order)
        out = np.empty((Y, X, 3) if bmp_order else (X, Y, 3), np.uint8)
        check(lib.ft_tone_map_host(dev._ctx, img.ctypes.data_as(C.c_void_p), X, Y, C.byref(tm), out.ctypes.data_as(C.c_void_p), None))
        return out

    @staticmethod
    def saveBitmap(path, colors):
        """Image.saveBitmap (Image.fs:88-90) for the uint8 [X, Y, 3] value of toColors: 24-bpp BMP, host side"""
        from .postprocess import saveBitmap
        saveBitmap(path, colors)
