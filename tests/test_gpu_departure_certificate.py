"""The departure certificate on the device (FT_OPT_DEPART; capi.cpp departSchedule, kernels.hip ft_miss_certificate with a tilted margin).

Every frame is compared bit for bit with the CPU oracle, which has no shortcut at all: pixels, rays, hits and flags.  The counters that may move are
sdf_evals and wave_evals, and only where the option says so: with 1 a first frame counts exactly what it counts with 0."""
import contextlib
import functools
import os
import re

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import _lib
from fraytracer_amd import synthetic as syn
from helpers import COUNTERS, assert_bit_equal, assert_cpp_compiles, host, options, options_left_at_defaults, oracle_libm  # noqa: F401  (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS, LEN = 0.01, 30.0
EVERY_STEP = 255 | (0 << 8) | (1 << 16) | (1 << 24)     # FT_OPT_CERT_POLICY: primary rays never, shadow rays from step 0, one due lane, again after every step

# name -> (spheres, frame side, camera): C3 under the Program.fs lens (wide tiles), and the narrow-tiled cases of tests/test_try_hint.py
NARROW = {"n64-128": (64, 128, 0.08, 1.936798870563507), "n256-128": (256, 128, 0.08, 4.615188837051392)}
CASES = ["c3-96", "c3-160", "n64-128", "n256-128"]


def scene_of(case):
    return syn.config3(n=NARROW[case][0] if case in NARROW else 64, size=NARROW[case][1] if case in NARROW else int(case[3:]))[0]


def size_of(case):
    return NARROW[case][1] if case in NARROW else int(case[3:])


def camera_of(case):
    if case not in NARROW:
        return syn.default_camera()
    _, _, lens, x = NARROW[case]
    return ft.Camera.lookAt(Position=(0.0, 0.0, -10.0), LookAt=(x, 0.3, 0.0), Up=(0.0, 1.0, 0.0), Lens=ft.Lens.create(lens))


def tile_over_margin(ds, cam, size):
    """capi.cpp certSchedule: the side of an 8x8 pixel tile at the far side of the support sphere, over certM; <= 1: word 0 is the bundle alone"""
    ca, sup = cam.as_array().astype(np.float64), ds.support_sphere()
    n = lambda v: float(np.sqrt((v * v).sum()))
    return 8.0 * max(n(ca[6:9]), n(ca[9:12])) / size * (n(ca[0:3] - np.array(sup[:3])) + sup[3]) / n(ca[3:6]) / ds.miss_certificate()["margin"]


def narrow(ds, case):
    ratio = tile_over_margin(ds, camera_of(case), size_of(case))
    assert 0.5 < ratio <= 1.0, ("the case's tiles are no longer narrow: its second frame would follow no hint", ratio)


def oracle_render(case, scene, libm=False):
    from oracle import binding as ob
    size = size_of(case)
    with (oracle_libm(ob) if libm else contextlib.nullcontext()), np.errstate(all="ignore"):
        want, cnt = ob.Oracle().scene(scene).render(EPS, LEN, size, size, camera_of(case).as_array(), nthreads=16)
    want.setflags(write=False)
    return want, cnt


@functools.lru_cache(maxsize=None)
def oracle_frame(case, libm=False):
    """the oracle's frame and counters of a case, computed once and left unchanged"""
    return oracle_render(case, scene_of(case), libm)


@pytest.fixture(autouse=True)
def depart_left_at_default(request):
    """"depart" lives in Device.STREAM_OPTIONS, which helpers.options_left_at_defaults does not walk: this module checks its own option"""
    yield
    if "gpu" in request.fixturenames:
        gpu = request.getfixturevalue("gpu")
        left = gpu.get_option("depart")
        gpu.set_option("depart", 1)
        assert left == 1, f"depart left at {left} on the shared device (now back at 1)"


def frames(gpu, case, n, want, cnt, what, scene=None, **opts):
    """n frames of a fresh scene handle (its first is a first frame) under the options: each is the oracle's in pixels, rays, hits and flags -> their stats"""
    ds = gpu.scene(scene if scene is not None else scene_of(case))
    size = size_of(case)
    out = []
    with contextlib.closing(ds), options(gpu, **opts), np.errstate(all="ignore"):
        for i in range(n):
            got, st = ds.render(EPS, LEN, ft.ImageSize(size, size), camera_of(case))
            assert_bit_equal(got, want, f"{case} {what} frame {i + 1}")
            for k in COUNTERS:
                assert st[k] == cnt[k], (case, what, i, k, st[k], cnt[k])
            out.append(st)
    return out


SAME = ("sdf_evals", "wave_evals", "culled_fraction")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_frames_under_every_setting(gpu, oracle, case):
    want, cnt = oracle_frame(case)
    if case in NARROW:
        ds = gpu.scene(scene_of(case))
        with contextlib.closing(ds):
            narrow(ds, case)
    off = frames(gpu, case, 2, want, cnt, "depart 0", depart=0)
    one = frames(gpu, case, 2, want, cnt, "depart 1", depart=1)
    two = frames(gpu, case, 2, want, cnt, "depart 2", depart=2)
    every = frames(gpu, case, 1, want, cnt, "depart 2, every step", depart=2, cert_policy=EVERY_STEP)
    every_off = frames(gpu, case, 1, want, cnt, "depart 0, every step", depart=0, cert_policy=EVERY_STEP)
    frames(gpu, case, 1, want, cnt, "depart 2, latency mode", depart=2, tail_k=64)
    print(case, "sdf_evals off", [s["sdf_evals"] for s in off], "1", [s["sdf_evals"] for s in one], "2", [s["sdf_evals"] for s in two], "every step", every[0]["sdf_evals"], "against", every_off[0]["sdf_evals"])
    # 2 bites on every C3 case, first frames included; under an explicit word against the flat margin on the same word
    assert two[0]["sdf_evals"] < off[0]["sdf_evals"] and every[0]["sdf_evals"] < every_off[0]["sdf_evals"]
    # 1: a first frame counts exactly what it counts with the option off
    for k in SAME:
        assert one[0][k] == off[0][k], (case, k, one[0][k], off[0][k])
    if case in NARROW:                                                  # ... and the second frame, which follows try hints, counts fewer
        assert one[1]["sdf_evals"] < off[1]["sdf_evals"] and one[1]["sdf_evals"] < one[0]["sdf_evals"]
    else:                                                               # a wide-tiled frame follows no hint: nothing moves
        for k in SAME:
            assert one[1][k] == off[1][k], (case, k)
    # where no certificate runs nothing may be tried
    for name, o in (("escape 0", {"escape": 0}), ("cert 0", {"cert": 0})):
        a = frames(gpu, case, 1, want, cnt, name + " depart 0", depart=0, **o)[0]
        b = frames(gpu, case, 1, want, cnt, name + " depart 2", depart=2, **o)[0]
        c = frames(gpu, case, 1, want, cnt, name + " depart 2 every step", depart=2, cert_policy=EVERY_STEP, **o)[0]
        for k in SAME:
            assert a[k] == b[k] == c[k], (case, name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_glibc_arithmetic(gpu, oracle, case):
    want, cnt = oracle_frame(case, libm=True)
    math = ft.glibc_build_of_this_host()
    off = frames(gpu, case, 1, want, cnt, "glibc depart 0", depart=0, math=math)[0]
    two = frames(gpu, case, 1, want, cnt, "glibc depart 2", depart=2, math=math)[0]
    assert two["sdf_evals"] < off["sdf_evals"]


@pytest.mark.gpu
@pytest.mark.parametrize("light", ["point far", "point inside"])
def test_point_lights(gpu, oracle, light):
    """a point light's shadow ray has |dir| = 1 / distance.  Ten units away every ray is outside the gate and nothing moves; inside the cloud the rays
    whose light is 0.83 .. 1.11 away pass it, and the frame is the oracle's either way"""
    case = "c3-96"
    base = scene_of(case)
    pos = (3.0, 9.0, -4.0) if light == "point far" else (0.3, 0.2, -0.4)
    scene = ft.SdfScene(base.Object, syn.BACKGROUND, [ft.SdfLight.point(pos, (40.0, 30.0, 20.0))])
    want, cnt = oracle_render(case, scene)
    assert cnt["rays_shadow"] > 0
    off = frames(gpu, case, 1, want, cnt, light + " depart 0", scene=scene, depart=0)[0]
    two = frames(gpu, case, 1, want, cnt, light + " depart 2", scene=scene, depart=2)[0]
    every = frames(gpu, case, 1, want, cnt, light + " depart 2 every step", scene=scene, depart=2, cert_policy=EVERY_STEP)[0]
    ref = frames(gpu, case, 1, want, cnt, light + " depart 0 every step", scene=scene, depart=0, cert_policy=EVERY_STEP)[0]
    print(light, off["sdf_evals"], two["sdf_evals"], every["sdf_evals"], ref["sdf_evals"])
    # the gate's answer shows on the explicit word, whose tries are the shadow rays' alone (under word 0 a wide-tiled frame's primary tries tilt as well)
    if light == "point far":
        assert every["sdf_evals"] == ref["sdf_evals"]                  # the same tries, and every one fails the gate on |dir|^2 as the flat one does
    else:
        assert every["sdf_evals"] < ref["sdf_evals"]                   # some rays pass the gate, and the tilted margin ends them earlier than the flat one
    assert two["sdf_evals"] <= off["sdf_evals"]


def test_option_and_its_mirrors(host, tmp_path):
    header = open(os.path.join(ROOT, "include", "fraytracer_hip.h")).read()
    assert re.search(r"\bFT_OPT_DEPART\s*=\s*20\b", header)
    assert _lib.FT_OPT_DEPART == 20 and ft.Device.STREAM_OPTIONS["depart"] == 20
    assert "FT_OPT_DEPART" in open(os.path.join(ROOT, "host", "cpp", "FrayTracer.hpp")).read()
    assert_cpp_compiles(tmp_path, "depart.cpp", "void f(FrayTracer::Context& c) { c.setOption(FT_OPT_DEPART, 2); static_assert(FT_OPT_DEPART == 20, \"\"); (void)c.getOption(FT_OPT_DEPART); }\n")
    fs = open(os.path.join(ROOT, "host", "fsharp", "FrayTracer.Hip.fs")).read()
    assert re.search(r"let setDepart \(mode : int\) = if ft_ctx_set_option \(ctx\.Value, 20, mode\)", fs)
    assert host.get_option("depart") == 1
    for v in (0, 2, 1):
        host.set_option("depart", v)
        assert host.get_option("depart") == v
    for bad in (-1, 3):
        with pytest.raises(ft.FrayTracerError) as e:
            host.set_option("depart", bad)
        assert e.value.code == _lib.FT_ERR_INVALID and host.get_option("depart") == 1
