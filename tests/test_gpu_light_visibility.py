"""Light visibility masks (ft_light_visibility, ft_shade_visible and their *_device forms), bit for bit.  The oracle defines every bit: bit i
of ray r is set iff the ray's colour under the whitened Object, a black background and light i alone, white, is above zero — the one case in
which SdfScene.fs:23 executed.  The six scenes (one per kernel family), rays, records and the three relight lights are those of
tests/test_gpu_shade_hits.py, computed once there and shared.  Every comparison is exact."""
import contextlib
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import _lib
from fraytracer_amd import synthetic as syn
from helpers import assert_bit_equal, glibc_math, host_ptr as ptr, options, options_left_at_defaults  # noqa: F401  (options_left_at_defaults: a fixture)
from test_gpu_rays_device import EPS, LEN, pixel_rays, same_bits, scenes
from test_gpu_shade_hits import BG, LIGHTS, N_SCENES, SHORTCUTS, _case, whitened

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLACK, WHITE = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
# identity (b): the same three lights, other colours (one of them black), another background
BG2 = (0.11, 0.0, 0.07)
COLOURS2 = ((0.2, 1.7, 0.4), (0.0, 0.0, 0.0), (55.0, 3.0, 21.0))
# identity (c): the point light somewhere else
MOVED = (-4.0, 2.5, -5.0)
PI_INV = np.float32(1.0) / np.float32(3.14159274101257324)


def recoloured(light, colour):
    make = ft.SdfLight.directional if light.kind == "directional" else ft.SdfLight.point
    return make(light.args[0], colour)


def oracle_bits(oracle, obj, rays, lights):
    """(uint32 mask per ray, per-light counters) from one single-light oracle trace per light: bit i = max(rgb) > 0 under the whitened object, a
    black background and light i in white"""
    white = whitened(obj)
    mask, cnts = np.zeros(len(rays), np.uint32), []
    for i, l in enumerate(lights):
        rgb, cnt = oracle.Oracle().scene(ft.SdfScene(white, BLACK, [recoloured(l, WHITE)])).trace_rays(rays)
        mask |= (rgb.max(axis=1) > 0.0).astype(np.uint32) << np.uint32(i)
        cnts.append(cnt)
    return mask, cnts


class VisCase:
    """the shade tests' case of scene k plus the oracle's masks under LIGHTS and under LIGHTS with the point light moved; computed once, never
    written to.  What makes max(rgb) > 0 a definition of the bit is asserted here, on the oracle's outputs alone."""

    def __init__(self, oracle, device, k):
        self.c = c = _case(k, device)
        self.mask, self.cnts = oracle_bits(oracle, c.scene.Object, c.rays, LIGHTS)
        lit = [int(((self.mask >> np.uint32(i)) & 1).sum()) for i in range(3)]
        # every shadow ray that missed lit its ray, and nothing else did: the counts of three single-light traces sum to those of the full trace
        assert sum(lit) == c.cnt["rays_shadow"] - c.cnt["hits_shadow"], (c.name, lit, c.cnt)
        for i in range(3):
            assert lit[i] == self.cnts[i]["rays_shadow"] - self.cnts[i]["hits_shadow"] and lit[i] > 0, (c.name, i, lit, self.cnts[i])
        assert sum(n["rays_shadow"] for n in self.cnts) == c.cnt["rays_shadow"], c.name
        assert not (self.mask[~c.hit] != 0).any(), c.name                 # no lit ray is a miss
        self.lights2 = (LIGHTS[0], ft.SdfLight.point(MOVED, LIGHTS[1].args[1]), LIGHTS[2])
        self.mask2, self.cnts2 = oracle_bits(oracle, c.scene.Object, c.rays, self.lights2)
        assert same_bits(self.mask2 & np.uint32(0b101), self.mask & np.uint32(0b101)), c.name
        assert ((self.mask2 ^ self.mask) & np.uint32(0b010)).any(), (c.name, "the moved light must change some bit")
        self.mask.setflags(write=False)
        self.mask2.setflags(write=False)


_VIS = {}


def _vis(k, device):
    if k not in _VIS:
        from oracle import binding
        _VIS[k] = VisCase(binding, device, k)
    return _VIS[k]


@pytest.fixture(params=range(N_SCENES), ids=lambda k: scenes()[k][0].split(" ")[0])
def vc(request, gpu):
    return _vis(request.param, gpu)


COUNTERS = ("rays_primary", "hits_primary", "rays_ext", "rays_shadow", "hits_shadow", "sdf_evals", "flags")


def test_mask_against_the_oracle(gpu, vc):
    c = vc.c
    relit = gpu.scene(c.scene).relight(BG, LIGHTS)
    with contextlib.closing(relit), options(gpu) as set_:
        vis, st = relit.light_visibility(c.rec)
        assert vis.shape == (len(c.rays),) and vis.dtype == np.uint32
        assert same_bits(vis, vc.mask), (c.name, int((vis != vc.mask).sum()))
        assert not (vis >> np.uint32(3)).any(), c.name
        assert st["rays_primary"] == 0 and st["hits_primary"] == 0 and st["rays_ext"] == 0, (c.name, st)
        assert st["rays_shadow"] == c.cnt["rays_shadow"] and st["hits_shadow"] == c.cnt["hits_shadow"] and st["flags"] == 0, (c.name, st, c.cnt)
        set_(cert=0)                                          # sdf_evals is compared too
        _, sh = relit.shade_hits(c.rec)
        vis0, st0 = relit.light_visibility(c.rec)
        assert same_bits(vis0, vc.mask), c.name
        for key in COUNTERS:
            assert st0[key] == sh[key], (c.name, key, st0[key], sh[key])
        assert st0["sdf_evals"] > 0


def test_identity_a_host_forms_and_frames(gpu, vc):
    """shade_visible(B, rec, light_visibility(B, rec)) = shade_hits(B, rec) = trace_rays(B, rays)"""
    c = vc.c
    ds = gpu.scene(c.scene)
    relit = ds.relight(BG, LIGHTS)
    try:
        vis, _ = relit.light_visibility(c.rec)
        rgb, st = relit.shade_visible(c.rec, vis)
        assert rgb.shape == (len(c.rays), 3)
        assert_bit_equal(rgb, c.want, f"{c.name}: shade_visible = oracle trace_rays(relit)")
        sh, _ = relit.shade_hits(c.rec)
        assert_bit_equal(rgb, sh, f"{c.name}: shade_visible = shade_hits")
        for key in COUNTERS:
            assert st[key] == 0, (c.name, key, st)
        assert st["kernel_ms"] > 0.0, (c.name, st)
        # a frame of hits keeps its [X, Y] shape through both calls
        cam = syn.default_camera()
        frame_hits, _, _ = ds.render_hits(EPS, LEN, ft.ImageSize(c.W, c.H), cam)
        img, img_st = relit.render(EPS, LEN, ft.ImageSize(c.W, c.H), cam)
        fvis, fst = relit.light_visibility(frame_hits)
        assert fvis.shape == (c.W, c.H) and same_bits(fvis.reshape(-1), vc.mask[:c.npx]), c.name
        frgb, _ = relit.shade_visible(frame_hits, fvis)
        assert frgb.shape == (c.W, c.H, 3)
        assert_bit_equal(frgb, img, f"{c.name}: shade_visible(render_hits records) = relit.render")
        for key in ("rays_shadow", "hits_shadow", "flags"):
            assert fst[key] == img_st[key], (c.name, key)
    finally:
        relit.close()


def test_identity_b_recoloured_lights_background_and_records(gpu, vc, oracle):
    """the masks of B shade under B' — B's lights at the same places in other colours, another background — and for recoloured records"""
    c = vc.c
    lights2 = [recoloured(l, col) for l, col in zip(LIGHTS, COLOURS2)]
    relit = gpu.scene(c.scene).relight(BG, LIGHTS)
    other = relit.relight(BG2, lights2)
    try:
        vis, _ = relit.light_visibility(c.rec)
        want, _ = oracle.Oracle().scene(ft.SdfScene(c.scene.Object, BG2, lights2)).trace_rays(c.rays)
        rgb, _ = other.shade_visible(c.rec, vis)
        assert_bit_equal(rgb, want, f"{c.name}: shade_visible(B', rec, vis(B)) = oracle trace_rays(B')")
        rec = c.rec.copy()
        rec[:, 11:14] = np.random.default_rng(9000 + c.k).uniform(0.0, 2.0, (len(c.rays), 3)).astype(np.float32)
        rec[::3, 14] = 0.0
        want2, _ = other.shade_hits(rec)
        rgb2, _ = other.shade_visible(rec, vis)
        assert_bit_equal(rgb2, want2, f"{c.name}: edited records, shade_visible = shade_hits under B'")
        assert_bit_equal(rgb2[::3], np.broadcast_to(np.asarray(BG2, np.float32), rgb2[::3].shape), f"{c.name}: switched off = background")
    finally:
        other.close()
        relit.close()


def test_identity_c_and_selection(gpu, vc):
    """one light moved: re-marching that light alone, in place, gives the moved scene's masks and casts only that light's shadow rays"""
    c = vc.c
    relit = gpu.scene(c.scene).relight(BG, LIGHTS)
    moved = relit.relight(BG, vc.lights2)
    try:
        base, _ = relit.light_visibility(c.rec)
        full, _ = moved.light_visibility(c.rec)
        assert same_bits(full, vc.mask2), c.name
        # in place through the C call: vis_in == vis_out
        v, st, rec = base.copy(), _lib.Stats(), np.ascontiguousarray(c.rec)
        _lib.check(_lib.lib.ft_light_visibility(gpu._ctx, moved._scene, ptr(rec), len(rec), 0b010, ptr(v), ptr(v), C.byref(st)))
        assert same_bits(v, vc.mask2), c.name
        # the shadow rays cast are the moved light's: the hit records whose cosine to it is > 0 (the oracle's single-light trace)
        assert st.rays_shadow == vc.cnts2[1]["rays_shadow"] and st.hits_shadow == vc.cnts2[1]["hits_shadow"], (c.name, st.rays_shadow, vc.cnts2[1])
        assert 0 < st.rays_shadow < c.cnt["rays_shadow"] and st.rays_primary == 0
        # the Python layer: previous is left alone, the result is new
        upd, ust = moved.light_visibility(c.rec, select=0b010, previous=base)
        assert same_bits(upd, vc.mask2) and same_bits(base, vc.mask) and ust["rays_shadow"] == st.rays_shadow, c.name
        one, _ = moved.light_visibility(c.rec, select=0b010)
        assert same_bits(one, vc.mask2 & np.uint32(0b010)), c.name
        # nothing selected: the kept bits, no ray; junk in bits that are no light comes out cleared
        junk = base | np.uint32(0xFFFFFFF8)
        kept, kst = moved.light_visibility(c.rec, select=0, previous=junk)
        assert same_bits(kept, vc.mask) and kst["rays_shadow"] == 0 and kst["sdf_evals"] == 0, (c.name, kst)
        none, nst = moved.light_visibility(c.rec, select=0)
        assert not none.any() and nst["rays_shadow"] == 0, c.name
        upd2, _ = moved.light_visibility(c.rec, select=0xFFFFFFF2, previous=junk)         # select bits beyond the lights select nothing
        assert same_bits(upd2, vc.mask2), c.name
    finally:
        moved.close()
        relit.close()


@pytest.mark.parametrize("option,value", SHORTCUTS, ids=[f"{o}={v:#x}" for o, v in SHORTCUTS])
def test_shortcuts_do_not_change_the_masks(gpu, option, value):
    for k in range(N_SCENES):
        v = _vis(k, gpu)
        relit = gpu.scene(v.c.scene).relight(BG, LIGHTS)
        with options(gpu, **{option: value}):
            vis, st = relit.light_visibility(v.c.rec)
        assert same_bits(vis, v.mask), (option, value, v.c.name)
        assert st["rays_shadow"] == v.c.cnt["rays_shadow"] and st["hits_shadow"] == v.c.cnt["hits_shadow"], (option, v.c.name)
        relit.close()


def test_glibc_arithmetic(gpu, oracle):
    """config3 under FT_OPT_MATH = glibc (the *_libm_vis twin of the lean kernel) against the oracle calling this host's expf / logf"""
    c = _case(1, gpu)
    ds = gpu.scene(c.scene)
    relit = ds.relight(BG, LIGHTS)
    with contextlib.closing(relit), glibc_math(gpu, oracle):
        rec, _ = oracle.Oracle().scene(c.scene).object_try_trace(c.rays)
        want_rgb, cnt = oracle.Oracle().scene(c.relit_scene).trace_rays(c.rays)
        want, _ = oracle_bits(oracle, c.scene.Object, c.rays, LIGHTS)
        assert int(sum(((want >> np.uint32(i)) & 1).sum() for i in range(3))) == cnt["rays_shadow"] - cnt["hits_shadow"]
        vis, st = relit.light_visibility(rec)
        assert same_bits(vis, want), int((vis != want).sum())
        assert st["rays_shadow"] == cnt["rays_shadow"] and st["hits_shadow"] == cnt["hits_shadow"]
        rgb, _ = relit.shade_visible(rec, vis)
        assert_bit_equal(rgb, want_rgb, "glibc: shade_visible = oracle trace_rays with libm")


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_counts(gpu, n):
    """a single record, one short of a wave, a wave, one more: both kernels guard their tail"""
    v = _vis(0, gpu)
    c = v.c
    first = int(np.flatnonzero(v.mask == 7)[0]) if (v.mask == 7).any() else int(np.flatnonzero(v.mask)[0])
    first = min(first, len(c.rays) - n)
    assert v.mask[first:first + n].any()
    relit = gpu.scene(c.scene).relight(BG, LIGHTS)
    try:
        rec = np.ascontiguousarray(c.rec[first:first + n])
        vis, st = relit.light_visibility(rec)
        assert vis.shape == (n,) and same_bits(vis, v.mask[first:first + n]), n
        rgb, _ = relit.shade_visible(rec, vis)
        assert_bit_equal(rgb, c.want[first:first + n], f"n = {n}")
    finally:
        relit.close()


def test_no_lights(gpu):
    c = _case(2, gpu)
    dark = gpu.scene(c.scene).relight(BG, [])
    try:
        vis, st = dark.light_visibility(c.rec)
        assert not vis.any() and st["rays_shadow"] == 0
        junk = np.full(len(c.rec), 0xFFFFFFFF, np.uint32)
        vis, _ = dark.light_visibility(c.rec, previous=junk)
        assert not vis.any()
        rgb, _ = dark.shade_visible(c.rec, junk)                  # bits that are no light are ignored
        bg = np.asarray(BG, np.float32)
        want = np.where(c.hit[:, None], c.rec[:, 11:14] * (bg * PI_INV)[None, :], bg[None, :]).astype(np.float32)
        assert_bit_equal(rgb, want, "no lights: Color * (BackgroundColor * piInv)")
    finally:
        dark.close()


def test_thirty_two_lights(gpu, oracle):
    """one sphere under 32 directional lights on a spiral from -z (behind the sphere, as the camera sees it) to +z: every bit against its own
    single-light oracle trace, bit 31 among them"""
    i = np.arange(32)
    z = 2.0 * (i + 0.5) / 32.0 - 1.0
    phi = i * 2.399963229728653
    dirs = np.stack([np.sqrt(1.0 - z * z) * np.cos(phi), np.sqrt(1.0 - z * z) * np.sin(phi), z], axis=1)
    lights = [ft.SdfLight.directional(tuple(float(x) for x in d), (0.1 + 0.01 * k, 0.2, 0.3)) for k, d in enumerate(dirs)]
    obj = ft.SdfObject.create(ft.SdfMaterial.createSolid((0.8, 0.5, 0.3)), ft.SdfForm.Primitive.sphere((0.3, -0.2, 0.0), 2.5))
    scene = ft.SdfScene(obj, BG, lights)
    rays = np.ascontiguousarray(pixel_rays(oracle, 15, 14))
    rec, _ = oracle.Oracle().scene(scene).object_try_trace(rays)
    want_rgb, cnt = oracle.Oracle().scene(scene).trace_rays(rays)
    want, _ = oracle_bits(oracle, obj, rays, lights)
    assert int(sum(((want >> np.uint32(k)) & 1).sum() for k in range(32))) == cnt["rays_shadow"] - cnt["hits_shadow"]
    assert ((want >> np.uint32(31)) & 1).any() and ((want >> np.uint32(0)) & 1).sum() < (rec[:, 14].view(np.int32) != 0).sum()
    ds = gpu.scene(scene)
    vis, st = ds.light_visibility(rec)
    assert same_bits(vis, want), int((vis != want).sum())
    assert st["rays_shadow"] == cnt["rays_shadow"] and st["hits_shadow"] == cnt["hits_shadow"]
    rgb, _ = ds.shade_visible(rec, vis)
    assert_bit_equal(rgb, want_rgb, "32 lights: shade_visible = oracle trace_rays")
    top, tst = ds.light_visibility(rec, select=1 << 31, previous=vis & np.uint32(0x7FFFFFFF))
    assert same_bits(top, want) and tst["rays_shadow"] == int(((want >> np.uint32(31)) & 1).sum()) + tst["hits_shadow"]
    ds.close()


def test_a_mask_is_data(gpu):
    """a set bit contributes whatever the cosine: one directional light, every bit set, the expectation from the stated formula in float32"""
    c = _case(0, gpu)
    d, col = -np.asarray(LIGHTS[0].args[0], np.float32), np.asarray(LIGHTS[0].args[1], np.float32)
    d = d / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])           # the light's Direction: -direction |> Vector3.normalize (SdfLight.fs:7)
    assert d.dtype == np.float32
    one = gpu.scene(c.scene).relight(BG, [LIGHTS[0]])
    try:
        n = c.rec[:, 8:11]
        cos = ((n[:, 0] * d[0] + n[:, 1] * d[1]) + n[:, 2] * d[2]).astype(np.float32)
        assert (cos[c.hit] <= 0).any() and (cos[c.hit] > 0).any()
        bg = np.asarray(BG, np.float32)
        lacc = (bg[None, :] + col[None, :] * cos[:, None]).astype(np.float32)
        want = np.where(c.hit[:, None], c.rec[:, 11:14] * (lacc * PI_INV), bg[None, :]).astype(np.float32)
        rgb, _ = one.shade_visible(c.rec, np.full(len(c.rec), 0xFFFFFFFF, np.uint32))
        assert_bit_equal(rgb, want, "every bit set: Color * ((bg + colour * cos) * piInv), cos <= 0 included")
    finally:
        one.close()


DEVICE_FORMS = r"""
import json, sys
import numpy as np
import torch                              # before the library: torch's HIP runtime is the one the process loads first
import fraytracer_amd as ft
sys.path.insert(0, "tests")
import test_gpu_light_visibility as T
ibits = lambda t: t.detach().cpu().numpy().view(np.uint32)
same = lambda t, a: bool(np.array_equal(ibits(t), np.ascontiguousarray(a).view(np.uint32)))
dev = ft.Device(0)
res = []
for k in range(T.N_SCENES):
    v = T._vis(k, dev)
    c = v.c
    relit = dev.scene(c.scene).relight(T.BG, T.LIGHTS)
    moved = relit.relight(T.BG, v.lights2)
    n = len(c.rays) - 5                   # odd, and no multiple of 64
    assert n % 64 != 0 and n % 2 == 1
    r = {"scene": c.name}
    d_rec = torch.from_numpy(c.rec[:n].copy()).cuda()
    d_vis = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d_rgb = torch.full((n, 3), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    relit.light_visibility_device(d_rec.data_ptr(), n, d_vis.data_ptr())
    st = relit.collect_stats()
    r["masks"] = same(d_vis, v.mask[:n]) and st["rays_primary"] == 0 and st["rays_shadow"] > 0
    relit.shade_visible_device(d_rec.data_ptr(), d_vis.data_ptr(), n, d_rgb.data_ptr())
    st = relit.collect_stats()
    r["colours"] = same(d_rgb, c.want[:n]) and st["rays_shadow"] == 0 and st["sdf_evals"] == 0 and st["kernel_ms"] > 0
    # identity (c) in place: vis_in == vis_out
    moved.light_visibility_device(d_rec.data_ptr(), n, d_vis.data_ptr(), 0b010, d_vis.data_ptr())
    st = moved.collect_stats()
    r["in_place"] = same(d_vis, v.mask2[:n]) and 0 < st["rays_shadow"]
    # n = 0 and the refusals launch nothing and write nothing
    d_rgb.fill_(float("nan")); d_vis.fill_(-1); torch.cuda.synchronize()
    relit.light_visibility_device(d_rec.data_ptr(), 0, d_vis.data_ptr())
    relit.shade_visible_device(d_rec.data_ptr(), d_vis.data_ptr(), 0, d_rgb.data_ptr())
    r["refused"] = True
    for call, bad in ((relit.light_visibility_device, (d_rec.data_ptr() + 4, n - 1, d_vis.data_ptr())), (relit.light_visibility_device, (d_rec.data_ptr(), n, d_rec.data_ptr())),
                      (relit.shade_visible_device, (d_rec.data_ptr(), d_vis.data_ptr(), n, d_vis.data_ptr())), (relit.shade_visible_device, (d_rec.data_ptr(), d_vis.data_ptr() + 2, n, d_rgb.data_ptr()))):
        try:
            call(*bad)
            r["refused"] = False
        except ft.FrayTracerError as e:
            r["refused"] = r["refused"] and e.code == -1
    st = relit.collect_stats()
    r["nothing_launched"] = st["rays_shadow"] == 0 and bool(torch.isnan(d_rgb).all()) and bool((d_vis == -1).all())
    # the tensor front end on a side stream, between torch kernels: records [a, b, 16] -> masks [a, b] -> colours [a, b, 3]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        big = torch.from_numpy(c.rec[:c.npx].reshape(c.W, c.H, 16).copy()).cuda()
        for _ in range(20):
            big = big * 1.0
        vis, none = relit.light_visibility(big)
        vis2 = vis | 0
        rgb, none2 = relit.shade_visible(big, vis2)
        rgb2 = rgb + 0.0
    side.synchronize()
    r["tensor"] = (none is None and none2 is None and vis.is_cuda and vis.dtype == torch.int32 and tuple(vis.shape) == (c.W, c.H)
                   and same(vis2, v.mask[:c.npx].reshape(c.W, c.H)) and tuple(rgb.shape) == (c.W, c.H, 3) and same(rgb2, c.want[:c.npx].reshape(c.W, c.H, 3)))
    d_all, _ = relit.light_visibility(ft.PixelHits(d_rec * 1.0))                               # the default stream, through a PixelHits
    upd, _ = moved.light_visibility(d_rec, select=0b010, previous=d_all)
    r["tensor_default_stream"] = same(d_all | 0, v.mask[:n]) and same(upd | 0, v.mask2[:n])
    relit.collect_stats()
    for bad, why in ((d_all.to(torch.int64), "int32"), (d_all[:-1].contiguous(), "shape"), (torch.zeros((2 * n,), dtype=torch.int32, device="cuda")[::2], "contiguous"),
                     (d_all.cpu().numpy().view(np.uint32), "where the records lie")):
        try:
            relit.shade_visible(d_rec, bad)
            r["refuses " + why] = False
        except ValueError as e:
            r["refuses " + why] = why in str(e)
    res.append(r)
dev.close()
print(json.dumps(res))
"""


def test_device_forms_equal_the_oracle():
    """the *_device forms and the tensor front end on all six scenes, in a child process that loads torch before the library"""
    out = subprocess.run([sys.executable, "-c", DEVICE_FORMS], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert len(res) == N_SCENES
    for r in res:
        failed = [k for k, v in r.items() if k != "scene" and v is not True]
        assert not failed, (r["scene"], failed)
