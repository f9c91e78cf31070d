"""Rays born with Length <= 0, on the frames where that decides the pixel (tests/edge_scenes.py): the reference tests the Length before it evaluates
anything (SdfForm.fs:94-95, then :97), so an occlusion ray of ao_radius <= 0, a shadow ray of Length 0 and a primary ray of length <= 0 end open
without an evaluation — also where the kernels already know the distance at the ray's origin (FT_OPT_REUSE: the normal's centre probe for the
secondary rays, the shared camera evaluation for the primary ones) and that distance is below epsilon.  Every frame, record and counter is the CPU
oracle's, bit for bit; for radii <= 0 the frame is also the one without occlusion rays, an expectation the oracle does not supply.

On the parent of the commit that added this file, with FT_OPT_REUSE on (the default), the cases with a radius <= 0 and the zero-Length shadow ray
fail; with it off they pass."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import synthetic as syn
import edge_scenes as edge
from helpers import assert_bit_equal, check_counts, glibc_mode, options, options_left_at_defaults  # noqa: F401  (glibc_mode, options_left_at_defaults: fixtures)

pytestmark = pytest.mark.gpu

EPS, LEN = syn.EPSILON, syn.RAY_LENGTH
W, H = edge.W, edge.H
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")

OPEN = [0.0, -0.0, -1.0, -INF]                    # the frame of ao_samples = 0 as well as the oracle's
TINY = [1.4e-45, 1e-40, 1.17549435e-38]           # smallest subnormal, a subnormal, the smallest normal: `Length <= 0` under the kernel's denormal mode
CONTROL = [1e-3, 0.5]
RADII = OPEN + TINY + CONTROL
LENGTHS = [0.0, -0.0, -1.0, 1e-40, 1.17549435e-38]
SAMPLING = [(1, 1), (1, 4), (4, 4), (4, 16)]      # (spp, ao_samples)
MODES = {"reuse on": dict(reuse=1), "reuse off": dict(reuse=0), "reuse on, no other shortcut": dict(reuse=1, escape=0, cert=0, occl=0)}
SMOOTH = ["lean", "general", "calls", "glass"]    # the scenes that hold a unionSmooth: the _libm twins of their kernels
VIEWS = {"lean": 2, "cavity": 1, "general": 2, "calls": 2, "glass": 2}      # cameras inside; one outside is added


_FAMILY, _WANT, _DS = {}, {}, {}


def family(oracle, name):
    """(scene, cameras: the ones inside first, the default camera outside last, extension arguments, oracle scene): chosen once"""
    if name not in _FAMILY:
        scene, cams, ext = edge.FAMILIES[name](oracle, VIEWS[name])
        _FAMILY[name] = (scene, cams + [syn.default_camera()], ext, oracle.Oracle().scene(scene))
    return _FAMILY[name]


def device_scene(gpu, oracle, name):
    if name not in _DS:
        _DS[name] = gpu.scene(family(oracle, name)[0])
    return _DS[name]


def want(oracle, name, cam=0, length=LEN, libm=0, x0=0, x1=None, bare=False, **kw):
    """the oracle's (frame, counters) of camera `cam` of a family, with the family's extension arguments unless `bare`: computed once, shared,
    never written to.  libm: the oracle is in its C-runtime mode (the caller holds the glibc_mode fixture)"""
    scene, cams, ext, os_ = family(oracle, name)
    kw = dict({} if bare else ext, **kw)
    key = (name, cam, float(length).hex(), libm, x0, x1) + tuple(sorted((k, float(v).hex()) for k, v in kw.items()))
    if key not in _WANT:
        frame, cnt = os_.render(EPS, length, W, H, cams[cam].as_array(), x0=x0, x1=x1, **kw)
        frame.setflags(write=False)
        _WANT[key] = (frame, cnt)
    return _WANT[key]


def want_records(oracle, name, cam=0, length=LEN):
    """the oracle's SdfObject.tryTrace records of a camera's pixel rays, [W, H, 16]"""
    key = ("records", name, cam, float(length).hex())
    if key not in _WANT:
        scene, cams, _, os_ = family(oracle, name)
        _WANT[key] = os_.object_try_trace(edge.pixel_rays(oracle, cams[cam], W, H, EPS, length))[0].reshape(W, H, 16)
    return _WANT[key]


def check(got, gst, wanted, what):
    frame, cnt = wanted
    assert_bit_equal(got, frame, what)
    check_counts(gst, cnt)
    assert gst["rays_ext"] == cnt["rays_ext"], (what, gst["rays_ext"], cnt["rays_ext"])


def total(counts):
    return {k: sum(c[k] for c in counts) for k in ("rays_primary", "rays_shadow", "rays_ext", "hits_primary", "hits_shadow", "flags")}


def rid(v):
    return repr(float(v))


def test_the_scenes_reach_every_family_and_cannot_pass_vacuously(gpu, oracle):
    """from the oracle alone: on each scene at least 100 hit pixels, and 10 % of them, have a cached distance below epsilon; the scenes run in the
    lean, the general and the call-capable kernels (and the carved scene's EXTENSION frames in the general one)"""
    families = {}
    for name in edge.FAMILIES:
        scene, cams, ext, _ = family(oracle, name)
        for cam in cams[:-1]:
            edge.assert_not_vacuous(oracle, scene, cam)
        plain, tiny = want(oracle, name)[0], want(oracle, name, ao_samples=4, ao_radius=1e-40)[0]
        assert (plain.view(np.uint32) != tiny.view(np.uint32)).any(-1).sum() >= 100, name
        families[name] = device_scene(gpu, oracle, name).info()["fast_path"]
    assert set(families.values()) >= {0, 1, 2}, families
    assert families["lean"] == 1 and families["general"] == 0 and families["calls"] == 2, families


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("radius", RADII, ids=rid)
@pytest.mark.parametrize("name", list(edge.FAMILIES))
def test_occlusion_rays(gpu, oracle, name, radius, mode):
    ds = device_scene(gpu, oracle, name)
    cam = family(oracle, name)[1][0]
    with options(gpu, **MODES[mode]):
        for spp, k in SAMPLING:
            kw = dict(spp=spp, ao_samples=k, ao_radius=radius)
            g, gst = ds.render(EPS, LEN, ft.ImageSize(W, H), cam, **dict(family(oracle, name)[2], **kw))
            what = f"{name}, ao_radius {radius!r}, spp {spp}, ao_samples {k}, {mode}"
            check(g, gst, want(oracle, name, **kw), what)
            if radius <= 0.0:
                assert_bit_equal(g, want(oracle, name, spp=spp)[0], what + ": the frame without occlusion rays")


@pytest.mark.parametrize("name", list(edge.FAMILIES))
def test_the_default_radius(gpu, oracle, name):
    """ao_samples alone: the Python default ao_radius = 0.0"""
    ds = device_scene(gpu, oracle, name)
    scene, cams, ext, _ = family(oracle, name)
    g, gst = ds.render(EPS, LEN, ft.ImageSize(W, H), cams[0], ao_samples=4, **ext)
    check(g, gst, want(oracle, name, ao_samples=4), f"{name}: ao_samples=4 and nothing else")
    assert_bit_equal(g, want(oracle, name)[0], f"{name}: the frame without occlusion rays")


@pytest.mark.parametrize("reuse", [1, 0])
@pytest.mark.parametrize("radius", [0.0, -0.0, -1.0, -INF, 1e-40, 0.5], ids=rid)
@pytest.mark.parametrize("name", list(edge.FAMILIES))
def test_occlusion_rays_through_the_other_entry_points(gpu, oracle, name, radius, reuse):
    """views (cameras inside bodies plus one outside), the frame of render_hits, a column range.  ft.render_multi takes no extension arguments: its
    single-process path runs in test_primary_rays_from_a_camera_inside_a_body"""
    ds = device_scene(gpu, oracle, name)
    scene, cams, ext, _ = family(oracle, name)
    kw = dict(spp=4, ao_samples=4, ao_radius=radius)
    full = dict(ext, **kw)
    what = f"{name}, ao_radius {radius!r}, reuse {reuse}"
    with options(gpu, reuse=reuse):
        g, gst = ds.render_views(EPS, LEN, ft.ImageSize(W, H), cams, **full)
        wants = [want(oracle, name, cam=c, **kw) for c in range(len(cams))]
        for c in range(len(cams)):
            assert_bit_equal(g[c], wants[c][0], f"{what}: view {c}")
            if radius <= 0.0:
                assert_bit_equal(g[c], want(oracle, name, cam=c, spp=4)[0], f"{what}: view {c}, the frame without occlusion rays")
        tot = total([w[1] for w in wants])
        check_counts(gst, tot)
        assert gst["rays_ext"] == tot["rays_ext"]
        hits, img, hst = ds.render_hits(EPS, LEN, ft.ImageSize(W, H), cams[0], shade=True, **full)
        check(img, hst, wants[0], what + ": render_hits")
        assert np.array_equal(hits.records.view(np.uint32), want_records(oracle, name).view(np.uint32)), what
        g, gst = ds.render(EPS, LEN, ft.ImageSize(W, H), cams[0], x0=5, n_columns=17, **full)
        cols = want(oracle, name, x0=5, x1=22, **kw)
        assert_bit_equal(cols[0], wants[0][0][5:22], "the oracle's column range")
        check(g, gst, cols, what + ": columns 5 .. 21")


def test_occlusion_rays_in_the_glibc_math_modes(gpu, oracle, glibc_mode):
    """the _libm twins of the kernels: the host's variant against the oracle calling the C runtime; the other variant against the frame without
    occlusion rays of the same variant"""
    for name in SMOOTH:
        ds = device_scene(gpu, oracle, name)
        scene, cams, ext, _ = family(oracle, name)
        for reuse in (1, 0):
            with options(gpu, reuse=reuse):
                for radius in (0.0, -1.0, 1e-40, 0.5):
                    kw = dict(spp=1, ao_samples=4, ao_radius=radius)
                    what = f"{name}, glibc mode, ao_radius {radius!r}, reuse {reuse}"
                    g, gst = ds.render(EPS, LEN, ft.ImageSize(W, H), cams[0], **dict(ext, **kw))
                    check(g, gst, want(oracle, name, libm=1, **kw), what)
                    if radius <= 0.0:
                        assert_bit_equal(g, want(oracle, name, libm=1)[0], what + ": the frame without occlusion rays")
                with options(gpu, math=3 - glibc_mode):
                    plain, pst = ds.render(EPS, LEN, ft.ImageSize(W, H), cams[0], **ext)
                    for radius in (0.0, -1.0):
                        g, gst = ds.render(EPS, LEN, ft.ImageSize(W, H), cams[0], **dict(ext, spp=1, ao_samples=4, ao_radius=radius))
                        assert_bit_equal(g, plain, f"{name}, the other glibc variant, ao_radius {radius!r}, reuse {reuse}")
                        check_counts(gst, pst)


# ---- primary rays: the shared camera evaluation (start_job: camKnown && s.len > 0) must not turn a ray of Length <= 0 into a hit at step 0 ---------
@pytest.mark.parametrize("reuse", [1, 0])
@pytest.mark.parametrize("length", LENGTHS, ids=rid)
@pytest.mark.parametrize("name", list(edge.FAMILIES))
def test_primary_rays_from_a_camera_inside_a_body(gpu, oracle, name, length, reuse):
    ds = device_scene(gpu, oracle, name)
    scene, cams, ext, _ = family(oracle, name)
    size = ft.ImageSize(W, H)
    what = f"{name}, length {length!r}, reuse {reuse}"
    wants = [want(oracle, name, cam=c, length=length) for c in range(len(cams))]
    recs = [want_records(oracle, name, c, length) for c in range(len(cams))]
    inside = name != "cavity"
    if length <= 0.0:                                              # SdfForm.fs:94-95 -> SdfScene.fs:10
        for frame, cnt in wants:
            assert_bit_equal(frame, np.broadcast_to(np.float32(syn.BACKGROUND), (W, H, 3)), "the oracle: background on every pixel")
            assert cnt["hits_primary"] == 0
        assert not any(r.any() for r in recs)
    elif inside:                                                   # every pixel is a hit at step 0
        assert wants[0][1]["hits_primary"] == W * H and (recs[0][..., 14].view(np.int32) == 1).all()
    with options(gpu, reuse=reuse):
        g, gst = ds.render(EPS, length, size, cams[0], **ext)
        check(g, gst, wants[0], what + ": render")
        hits, img, hst = ds.render_hits(EPS, length, size, cams[0], shade=True, **ext)
        check(img, hst, wants[0], what + ": render_hits")
        assert np.array_equal(hits.records.view(np.uint32), recs[0].view(np.uint32)), what
        assert (hits.material[~hits.hit] == -1).all() and (length > 0.0 or not hits.hit.any()), what
        g, gst = ds.render_views(EPS, length, size, cams, **ext)
        for c in range(len(cams)):
            assert_bit_equal(g[c], wants[c][0], f"{what}: view {c}")
        check_counts(gst, total([w[1] for w in wants]))
        hits, img, hst = ds.render_views_hits(EPS, length, size, cams, shade=True, **ext)
        for c in range(len(cams)):
            assert_bit_equal(img[c], wants[c][0], f"{what}: render_views_hits, view {c}")
            assert np.array_equal(hits.records[c].view(np.uint32), recs[c].view(np.uint32)), (what, c)
        check_counts(hst, total([w[1] for w in wants]))
        g, gst = ft.render_multi([gpu], scene, EPS, length, size, cams[0], stripe_width=16)
        check(g, gst, want(oracle, name, length=length, bare=True), what + ": render_multi")


# ---- the shadow ray of Length 0 (edge_scenes.SHADOW_RAY) -----------------------------------------------------------------------------------------------
def shadow_cases(oracle):
    """(name, scene, light name) of every object on which the oracle keeps the construction: the record's origin and the infinite colour"""
    out = []
    for name, obj in edge.shadow_objects().items():
        with np.errstate(all="ignore"):
            os_ = oracle.Oracle().scene(edge.shadow_scene(obj, edge.LIGHT_ZERO_LENGTH))
            rgb, cnt = os_.trace_rays(edge.SHADOW_RAY[None])
            rec, _ = os_.object_try_trace(edge.SHADOW_RAY[None])
        if np.array_equal(rec[0, 0:3], edge.SHADOW_ORIGIN) and np.isposinf(rgb[0]).all() and cnt["rays_shadow"] == 1 and cnt["hits_shadow"] == 0:
            out += [(name, edge.shadow_scene(obj, edge.LIGHT_ZERO_LENGTH), "zero-Length light"), (name, edge.shadow_scene(obj, edge.LIGHT_CONTROL), "control light")]
    return out


def test_shadow_ray_of_length_zero(gpu, oracle):
    """a point light whose distance2 underflows: the shadow ray is cast with Length 0 and misses without an evaluation — the light arrives (colour
    inf, no shadow hit counted).  64 copies (a whole wave) and 37 more between ordinary rays (a mixed wave), through ft_trace_rays and
    ft_trace_rays_hits, in the general, carved, lean and call-capable kernels"""
    cases = shadow_cases(oracle)
    assert len(cases) == 10
    rays, where = edge.shadow_buffer()
    families = set()
    for name, scene, light in cases:
        os_ = oracle.Oracle().scene(scene)
        with np.errstate(all="ignore"):
            want_rgb, cnt = os_.trace_rays(rays)
            want_rec, _ = os_.object_try_trace(rays)
        if light == "zero-Length light":
            assert np.isposinf(want_rgb[where]).all() and cnt["hits_shadow"] < cnt["rays_shadow"]
        ds = gpu.scene(scene)
        families.add(ds.info()["fast_path"])
        for reuse in (1, 0):
            what = f"{name}, {light}, reuse {reuse}"
            with options(gpu, reuse=reuse):
                rgb, st = ds.trace_rays(rays)
                assert_bit_equal(rgb, want_rgb, what + ": trace_rays")
                check_counts(st, cnt)
                hits, rgb, st = ds.trace_rays_hits(rays)
                assert_bit_equal(rgb, want_rgb, what + ": trace_rays_hits")
                check_counts(st, cnt)
                assert np.array_equal(hits.records.view(np.uint32), want_rec.view(np.uint32)), what
        ds.close()
    assert families >= {0, 1, 2, 3}, families


SHADOW_DEVICE_FORM = r"""
import json, sys
import numpy as np
import torch                              # before the library: torch's HIP runtime is the one the process loads first
import fraytracer_amd as ft
sys.path.insert(0, "tests")
import edge_scenes as edge
import test_gpu_ray_length_edges as T
from oracle import binding as oracle
dev = ft.Device(0)
rays, where = edge.shadow_buffer()
d_rays = torch.from_numpy(rays).cuda()
res = []
for name, scene, light in T.shadow_cases(oracle):
    with np.errstate(all="ignore"):
        want, cnt = oracle.Oracle().scene(scene).trace_rays(rays)
    ds = dev.scene(scene)
    for reuse in (1, 0):
        dev.set_option("reuse", reuse)
        d_rgb = torch.full((len(rays), 3), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ds.trace_rays_device(d_rays.data_ptr(), len(rays), d_rgb.data_ptr())
        st = ds.collect_stats()
        got = d_rgb.cpu().numpy()
        same = bool(((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all())
        res.append({"case": f"{name}, {light}, reuse {reuse}", "rgb": same,
                    "counters": all(st[k] == cnt[k] for k in ("rays_primary", "rays_shadow", "hits_primary", "hits_shadow", "flags"))})
    dev.set_option("reuse", 1)
dev.close()
print(json.dumps(res))
"""


def test_shadow_ray_of_length_zero_in_device_memory():
    """ft_trace_rays_device on the same buffer, in a child process that loads torch before the library (the idiom of tests/test_gpu_rays_device.py)"""
    out = subprocess.run([sys.executable, "-c", SHADOW_DEVICE_FORM], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert len(res) == 20
    failed = [r["case"] for r in res if not (r["rgb"] and r["counters"])]
    assert not failed, failed
