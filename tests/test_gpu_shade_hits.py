"""Relighting without re-tracing (ft_scene_relight, ft_shade_hits, ft_shade_hits_device), bit for bit.  The oracle defines every bit: for
scenes A and B that share their Object, shade(B, object_try_trace(A.Object, rays)) = trace_rays(B, rays).  The six scenes (one per kernel
family), frame sizes and rays are those of tests/test_gpu_rays_device.py: the pixel rays plus that file's seeded odd rays.

Evaluation counts measured on the MI355X with cert = 0 and reuse = 0 (test_evaluation_count asserts the identity and prints the figures), as
sdf_evals of shade_hits = trace_rays - object_try_trace: console_like 31450 = 42950 - 11500, config3 19801 = 35189 - 15388, mixed_nested
8248 = 16237 - 7989, console_scene 38757 = 54915 - 16158, config2 boxes 22937 = 35569 - 12632, config5 15654 = 26165 - 10511."""
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import synthetic as syn
from fraytracer_amd.api import Material, Object
from helpers import COUNTERS, assert_bit_equal, options, options_left_at_defaults  # noqa: F401  (options_left_at_defaults: a fixture)
from test_gpu_rays_device import EPS, LEN, ray_buffer, same_bits, scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BG = (0.02, 0.03, 0.05)
LIGHTS = (ft.SdfLight.directional((0.6, -1.0, -0.3), (0.9, 0.8, 0.7)), ft.SdfLight.point((3.0, 4.0, -6.0), (30.0, 40.0, 50.0)),
          ft.SdfLight.directional((0.0, 1.0, 0.2), (0.3, 0.3, 0.3)))
N_SCENES = 6
FAST_PATH = {1: 1, 3: 3}                                      # config3: lean; console_scene: carved


def whitened(obj):
    """the object with every material replaced by solid white: same geometry, same hits, Color = (1, 1, 1)"""
    white, memo = ft.SdfMaterial.createSolid((1.0, 1.0, 1.0)), {}

    def walk(node):
        if isinstance(node, Material):
            return white
        if not isinstance(node, Object):
            return node                                       # forms carry no material
        if id(node) not in memo:
            memo[id(node)] = Object(node.kind, node.args, [walk(k) for k in node.kids])
        return memo[id(node)]
    return walk(obj)


class Case:
    """one scene: its rays, the oracle's records under the scene as it is and the oracle's colours and counters under the relit scene — computed
    once, shared by every test, never written to.  The conditions on the inputs are asserted here, on the oracle's own outputs."""

    def __init__(self, oracle, device, k):
        self.k = k
        self.name, self.scene, self.W, self.H = scenes()[k]
        self.relit_scene = ft.SdfScene(self.scene.Object, BG, LIGHTS)
        self.rays, self.npx = ray_buffer(oracle, device.scene(self.scene), k, self.W, self.H)
        self.rec, _ = oracle.Oracle().scene(self.scene).object_try_trace(self.rays)
        self.want, self.cnt = oracle.Oracle().scene(self.relit_scene).trace_rays(self.rays)
        self.hit = self.rec[:, 14].view(np.int32) != 0
        hits = int(self.hit.sum())
        assert 0.10 <= hits / len(self.rays) <= 0.90, (self.name, hits, len(self.rays))
        assert 0.05 <= self.cnt["hits_shadow"] / self.cnt["rays_shadow"] <= 0.95, (self.name, self.cnt)
        assert 0.2 <= self.cnt["rays_shadow"] / (3 * hits) <= 0.9, (self.name, self.cnt, hits)       # some lights face away
        assert self.cnt["flags"] == 0 and self.cnt["hits_primary"] == hits, (self.name, self.cnt)
        for a in (self.rays, self.rec, self.want):
            a.setflags(write=False)


_CASES = {}


def _case(k, device):
    """the case of scene k; `device` (any Device: the rays need the scene's boundary only) is used the first time"""
    if k not in _CASES:
        from oracle import binding
        _CASES[k] = Case(binding, device, k)
    return _CASES[k]


@pytest.fixture(params=range(N_SCENES), ids=lambda k: scenes()[k][0].split(" ")[0])
def case(request, gpu):
    return _case(request.param, gpu)


def relit_of(gpu, c):
    return gpu.scene(c.scene).relight(BG, LIGHTS)


def test_against_the_oracle(gpu, case):
    c = case
    ds = gpu.scene(c.scene)
    relit = ds.relight(BG, LIGHTS)
    try:
        rgb, st = relit.shade_hits(c.rec)
        assert rgb.shape == (len(c.rays), 3)
        assert_bit_equal(rgb, c.want, f"{c.name}: shade(relit, oracle records) = oracle trace_rays(relit)")
        assert st["rays_shadow"] == c.cnt["rays_shadow"] and st["hits_shadow"] == c.cnt["hits_shadow"] and st["flags"] == 0, (c.name, st, c.cnt)
        assert st["rays_primary"] == 0 and st["hits_primary"] == 0 and st["rays_ext"] == 0, (c.name, st)
        # the library's own records: of the ray buffer, and of a frame (a PixelHits keeps its [X, Y] shape)
        hits, _, _ = ds.trace_rays_hits(c.rays, shade=False, material=False)
        assert same_bits(hits.records, c.rec), c.name
        want_rgb, want_st = relit.trace_rays(c.rays)
        assert_bit_equal(want_rgb, c.want, f"{c.name}: relit.trace_rays = oracle")
        rgb2, st2 = relit.shade_hits(hits)
        assert_bit_equal(rgb2, want_rgb, f"{c.name}: shade(trace_rays_hits records) = relit.trace_rays")
        for key in ("rays_shadow", "hits_shadow", "flags"):
            assert st2[key] == want_st[key], (c.name, key)
        cam = syn.default_camera()
        frame_hits, _, _ = ds.render_hits(EPS, LEN, ft.ImageSize(c.W, c.H), cam)
        img, img_st = relit.render(EPS, LEN, ft.ImageSize(c.W, c.H), cam)
        rgb3, st3 = relit.shade_hits(frame_hits)
        assert rgb3.shape == (c.W, c.H, 3)
        assert_bit_equal(rgb3, img, f"{c.name}: shade(render_hits records) = relit.render")
        assert_bit_equal(rgb3.reshape(-1, 3), c.want[:c.npx], f"{c.name}: ... = oracle, pixel rays")
        for key in ("rays_shadow", "hits_shadow", "flags"):
            assert st3[key] == img_st[key], (c.name, key)
        assert relit.info()["fast_path"] == ds.info()["fast_path"] == FAST_PATH.get(c.k, ds.info()["fast_path"]), c.name
    finally:
        relit.close()


def test_evaluation_count(gpu, case):
    """no centre probe ran, so every shadow ray's first evaluation is computed: with the certificate and the reuse off for all three calls,
    sdf_evals(shade_hits) = sdf_evals(trace_rays) - sdf_evals(object_try_trace) on the relit scene"""
    c = case
    relit = relit_of(gpu, c)
    with contextlib.closing(relit), options(gpu, cert=0, reuse=0) as set_:
        _, st = relit.shade_hits(c.rec)
        _, tr = relit.trace_rays(c.rays)
        _, ob = relit.object_try_trace(c.rays)
        print(f"{c.name}: sdf_evals shade_hits {st['sdf_evals']} trace_rays {tr['sdf_evals']} object_try_trace {ob['sdf_evals']}")
        assert st["sdf_evals"] == tr["sdf_evals"] - ob["sdf_evals"], (c.name, st["sdf_evals"], tr["sdf_evals"], ob["sdf_evals"])
        assert st["sdf_evals"] > 0
        set_(reuse=1)                                         # the option does not reach ft_shade_hits: there is nothing to reuse
        _, st1 = relit.shade_hits(c.rec)
        assert st1["sdf_evals"] == st["sdf_evals"], c.name


SHORTCUTS = [("escape", 0), ("cert", 0), ("cert_policy", 0x01010100), ("cull", 0), ("lazy_union", 0), ("carved", 0), ("tail_k", 64)]


@pytest.mark.parametrize("option,value", SHORTCUTS, ids=[f"{o}={v:#x}" for o, v in SHORTCUTS])
def test_shortcuts_do_not_change_the_colours(gpu, option, value):
    for k in range(N_SCENES):
        c = _case(k, gpu)
        relit = relit_of(gpu, c)
        with options(gpu, **{option: value}):
            rgb, st = relit.shade_hits(c.rec)
        assert_bit_equal(rgb, c.want, f"{option} = {value:#x}, {c.name}")
        assert st["rays_shadow"] == c.cnt["rays_shadow"] and st["hits_shadow"] == c.cnt["hits_shadow"], (option, c.name)
        relit.close()


@pytest.mark.parametrize("math", [1, 2], ids=["glibc_fma", "glibc_sse2"])
def test_shortcuts_in_glibc_arithmetic(gpu, math):
    """config3 under FT_MATH_GLIBC_*: the *_libm twin of the lean kernel, every shortcut off in turn; the records and the reference colours are the
    library's own in that arithmetic"""
    c = _case(1, gpu)
    ds = gpu.scene(c.scene)
    relit = ds.relight(BG, LIGHTS)
    with contextlib.closing(relit), options(gpu, math=math):
        rec, _ = ds.object_try_trace(c.rays)
        want, want_st = relit.trace_rays(c.rays)
        rgb, st = relit.shade_hits(rec)
        assert_bit_equal(rgb, want, f"math {math}: shade = trace_rays")
        assert st["rays_shadow"] == want_st["rays_shadow"] and st["hits_shadow"] == want_st["hits_shadow"]
        for option, value in SHORTCUTS:
            with options(gpu, **{option: value}):
                got, _ = relit.shade_hits(rec)
            assert_bit_equal(got, want, f"math {math}, {option} = {value:#x}")


def test_records_are_data(gpu, case, oracle):
    c = case
    relit = relit_of(gpu, c)
    try:
        # recoloured: Color * (lightColor * piInv), and lightColor * piInv is the white scene's colour (1 * x is exact)
        white = ft.SdfScene(whitened(c.scene.Object), BG, LIGHTS)
        s, _ = oracle.Oracle().scene(white).trace_rays(c.rays)
        colour = np.random.default_rng(7000 + c.k).uniform(0.0, 2.0, (len(c.rays), 3)).astype(np.float32)
        rec = c.rec.copy()
        rec[:, 11:14] = colour
        rgb, _ = relit.shade_hits(rec)
        want = np.where(c.hit[:, None], colour * s, np.asarray(BG, np.float32)[None, :]).astype(np.float32)
        assert_bit_equal(rgb, want, f"{c.name}: recoloured records")
        # hit = 0 is background whatever else the record holds
        rec = c.rec.copy()
        rec[::3, 14] = 0.0
        rgb, st = relit.shade_hits(rec)
        want = c.want.copy()
        want[::3] = np.asarray(BG, np.float32)
        assert_bit_equal(rgb, want, f"{c.name}: every third record switched off")
        assert st["rays_shadow"] < c.cnt["rays_shadow"], c.name
    finally:
        relit.close()


def test_relight_equals_a_scene_built_from_scratch(gpu, case):
    c = case
    cam, size = syn.default_camera(), ft.ImageSize(c.W, c.H)
    src = gpu.scene(c.scene)
    relit = src.relight(BG, LIGHTS)
    src.close()                                               # releasing the source first must not matter
    fresh = gpu.scene(c.relit_scene)
    with contextlib.closing(relit), options(gpu, cert=0):     # sdf_evals is compared too
        img, st = relit.render(EPS, LEN, size, cam)
        want, want_st = fresh.render(EPS, LEN, size, cam)
        assert_bit_equal(img, want, f"{c.name}: relit.render = render of ft_scene_create's scene")
        assert_bit_equal(img.reshape(-1, 3), c.want[:c.npx], f"{c.name}: ... = oracle")
        for key in COUNTERS + ("sdf_evals", "rays_ext"):
            assert st[key] == want_st[key], (c.name, key, st[key], want_st[key])
        assert relit.info() == fresh.info(), c.name


DEVICE_FORMS = r"""
import json, sys
import numpy as np
import torch                              # before the library: torch's HIP runtime is the one the process loads first
import fraytracer_amd as ft
sys.path.insert(0, "tests")
import test_gpu_shade_hits as T
bits = lambda t: t.detach().cpu().numpy().view(np.uint32)
same = lambda t, a: bool(np.array_equal(bits(t), np.ascontiguousarray(a).view(np.uint32)))
dev = ft.Device(0)
res = []
for k in range(T.N_SCENES):
    c = T._case(k, dev)
    relit = dev.scene(c.scene).relight(T.BG, T.LIGHTS)
    n = len(c.rays) - 5                   # odd, and no multiple of 64
    assert n % 64 != 0 and n % 2 == 1
    r = {"scene": c.name}
    d_rec = torch.from_numpy(c.rec[:n].copy()).cuda()
    d_rgb = torch.full((n, 3), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    relit.shade_hits_device(d_rec.data_ptr(), n, d_rgb.data_ptr())
    st = relit.collect_stats()
    r["device"] = same(d_rgb, c.want[:n]) and st["rays_primary"] == 0 and st["rays_shadow"] > 0
    # n = 0 and the refusals launch nothing and write nothing
    d_rgb.fill_(float("nan")); torch.cuda.synchronize()
    relit.shade_hits_device(d_rec.data_ptr(), 0, d_rgb.data_ptr())
    for bad in ((d_rec.data_ptr() + 4, n - 1, d_rgb.data_ptr()), (d_rec.data_ptr(), n, d_rec.data_ptr())):
        try:
            relit.shade_hits_device(*bad)
            r["refused"] = False
        except ft.FrayTracerError as e:
            r.setdefault("refused", e.code == -1)
    st = relit.collect_stats()
    r["nothing_launched"] = st["rays_shadow"] == 0 and bool(torch.isnan(d_rgb).all())
    # the tensor front end on a side stream, between torch kernels: records [a, b, 16] -> colours [a, b, 3]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        big = torch.from_numpy(c.rec[:c.npx].reshape(c.W, c.H, 16).copy()).cuda()
        for _ in range(20):
            big = big * 1.0
        rgb, none = relit.shade_hits(big)
        rgb2 = rgb + 0.0
    side.synchronize()
    r["tensor"] = none is None and rgb.is_cuda and tuple(rgb.shape) == (c.W, c.H, 3) and same(rgb2, c.want[:c.npx].reshape(c.W, c.H, 3))
    rgb0, _ = relit.shade_hits(ft.PixelHits(d_rec * 1.0))                                      # the default stream, through a PixelHits
    r["tensor_default_stream"] = same(rgb0 + 0.0, c.want[:n])
    relit.collect_stats()
    for bad, why in ((d_rec.double(), "float32"), (d_rec[:, :15].contiguous(), "16]"), (d_rec[::2], "contiguous")):
        try:
            relit.shade_hits(bad)
            r["refuses " + why] = False
        except ValueError as e:
            r["refuses " + why] = why in str(e)
    res.append(r)
dev.close()
print(json.dumps(res))
"""


def test_device_forms_equal_the_oracle():
    """ft_shade_hits_device and the tensor front end on all six scenes, in a child process that loads torch before the library"""
    out = subprocess.run([sys.executable, "-c", DEVICE_FORMS], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert len(res) == N_SCENES
    for r in res:
        failed = [k for k, v in r.items() if k != "scene" and v is not True]
        assert not failed, (r["scene"], failed)
