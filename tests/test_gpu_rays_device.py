"""Ray buffers with hit records and materials in one pass, in host and in device memory (ft_trace_rays_hits*, ft_*_device): per ray the
colour of SdfScene.trace, the SdfObject.tryTrace record and the material handle, bit for bit against the CPU oracle and the existing entry
points.  The rays are the pixel rays of a small frame plus rays no camera makes: origins inside and outside the scene's boundary, non-unit
directions, Length <= 0 and the point-light form of a shadow ray (direction diff / distance^2, Length = distance; SdfLight.fs:27-37)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import synthetic as syn
from helpers import COUNTERS, assert_bit_equal, options, options_left_at_defaults  # noqa: F401  (options_left_at_defaults: a fixture)

pytestmark = pytest.mark.gpu

EPS, LEN = syn.EPSILON, syn.RAY_LENGTH
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scenes():
    """one scene per kernel family, the list of tests/test_gpu_hits.py, with the size of the frame whose pixel rays are used"""
    return [("console_like (general)", syn.console_like(n=300)[0], 36, 27),
            ("config3 (lean)", syn.config3(n=64)[0], 36, 27),
            ("mixed_nested (general, nested combinators)", syn.mixed_nested()[0], 31, 24),
            ("console_scene (carved -> general)", syn.console_scene(n=200)[0], 40, 37),
            ("config2 boxes", syn.config2(boxes=True)[0], 36, 27),
            ("config5 (glass; on-demand calls)", syn.config5()[0], 32, 29)]


def pixel_rays(oracle, W, H):
    cam = syn.default_camera().as_array()
    return np.stack([oracle.pixel_ray(cam, W, H, x, y, EPS, LEN) for x in range(W) for y in range(H)])


def odd_rays(boundary, seed, n=384):
    """seeded rays no camera makes, around the scene's boundary sphere (cx, cy, cz, r): a third start inside it, the rest up to 3 r away;
    most aim at a point inside the sphere; directions of length 0.25 .. 4; every 12th ray has Length <= 0; every 5th is the point-light
    form (direction diff / distance^2, Length = distance: it travels one unit per unit of Length)"""
    rng = np.random.default_rng(seed)
    c, r = np.asarray(boundary[:3], np.float64), float(boundary[3])
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    rad = np.where(np.arange(n) % 3 == 0, rng.uniform(0.0, 1.0, n), rng.uniform(1.0, 3.0, n)) * r
    o = c + unit(rng.normal(size=(n, 3))) * rad[:, None]
    target = c + unit(rng.normal(size=(n, 3))) * (rng.uniform(0.0, 0.8, n) * r)[:, None]
    aimed = np.arange(n) % 4 != 3
    d = np.where(aimed[:, None], unit(target - o), unit(rng.normal(size=(n, 3)))) * rng.uniform(0.25, 4.0, n)[:, None]
    length = rng.uniform(0.5, 6.0, n) * r
    eps = np.where(np.arange(n) % 7 == 0, 4.0 * EPS, EPS)
    light = np.arange(n) % 5 == 0
    diff = target - o
    dist2 = (diff * diff).sum(-1)
    d[light] = diff[light] / dist2[light, None]
    length[light] = np.sqrt(dist2[light])
    dead = np.arange(n) % 12 == 5
    length[dead] = np.where(np.arange(n)[dead] % 24 == 5, 0.0, -1.0)
    return np.concatenate([o, d, length[:, None], eps[:, None]], axis=1).astype(np.float32)


def ray_buffer(oracle, ds, k, W, H):
    """(rays, number of pixel rays in front): the frame's pixel rays, then the odd ones"""
    px = pixel_rays(oracle, W, H)
    return np.ascontiguousarray(np.concatenate([px, odd_rays(ds.boundary(), 1000 + k)])), len(px)


def oracle_results(oracle, scene, rays):
    """(rgb, records, counters of trace_rays) of the oracle; asserts the condition on the inputs: 10 % .. 90 % of the rays hit"""
    o = oracle.Oracle().scene(scene)
    rgb, cnt = o.trace_rays(rays)
    rec, _ = o.object_try_trace(rays)
    frac = float((rec[:, 14].view(np.int32) == 1).mean())
    assert 0.10 <= frac <= 0.90, f"the ray set must exercise both store sites: {frac:.2f} of the rays hit"
    return rgb, rec, cnt


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_shade_records_and_material_in_one_launch(gpu, oracle):
    with options(gpu, cert=0):                               # sdf_evals is compared too
        for k, (name, scene, W, H) in enumerate(scenes()):
            ds = gpu.scene(scene)
            rays, _ = ray_buffer(oracle, ds, k, W, H)
            want_rgb, want_rec, _ = oracle_results(oracle, scene, rays)
            hits, rgb, st = ds.trace_rays_hits(rays)
            assert rgb.shape == (len(rays), 3) and hits.records.shape == (len(rays), 16) and hits.material.shape == (len(rays),)
            assert_bit_equal(rgb, want_rgb, f"{name}: rgb = oracle trace_rays")
            assert same_bits(hits.records, want_rec), name                                   # all 16 dwords, misses included
            ref_rgb, ref_st = ds.trace_rays(rays)
            assert_bit_equal(rgb, ref_rgb, f"{name}: rgb = ft_trace_rays")
            for c in COUNTERS + ("sdf_evals",):
                assert st[c] == ref_st[c], (name, c, st[c], ref_st[c])
            assert st["rays_primary"] == len(rays) and st["hits_primary"] == int(hits.hit.sum()), name
    ds = gpu.scene(scenes()[1][1])                           # certificate on (the lean kernel's default): every counter but sdf_evals
    rays, _ = ray_buffer(oracle, ds, 1, 36, 27)
    _, _, st = ds.trace_rays_hits(rays)
    _, ref_st = ds.trace_rays(rays)
    for c in COUNTERS:
        assert st[c] == ref_st[c], (c, st[c], ref_st[c])


def test_hits_only(gpu, oracle):
    with options(gpu, cert=0):
        for k, (name, scene, W, H) in enumerate(scenes()):
            ds = gpu.scene(scene)
            rays, _ = ray_buffer(oracle, ds, k, W, H)
            _, want_rec, _ = oracle_results(oracle, scene, rays)
            hits, rgb, st = ds.trace_rays_hits(rays, shade=False)
            assert rgb is None
            assert same_bits(hits.records, want_rec), name
            ref_rec, ref_st = ds.object_try_trace(rays)
            assert same_bits(ref_rec, want_rec), name
            for c in COUNTERS + ("sdf_evals",):
                assert st[c] == ref_st[c], (name, c, st[c], ref_st[c])
            assert st["rays_shadow"] == 0 and st["hits_shadow"] == 0, name
            only, _, _ = ds.trace_rays_hits(rays, shade=False, records=False)
            assert only.records is None and np.array_equal(only.material, hits.material), name


def test_materials(gpu, oracle):
    cam = syn.default_camera()
    for k, (name, scene, W, H) in enumerate(scenes()):
        ds = gpu.scene(scene)
        rays, npx = ray_buffer(oracle, ds, k, W, H)
        _, want_rec, _ = oracle_results(oracle, scene, rays)
        hits, _, _ = ds.trace_rays_hits(rays)
        frame, _, _ = ds.render_hits(EPS, LEN, ft.ImageSize(W, H), cam)
        assert np.array_equal(hits.material[:npx], frame.material.reshape(-1)), name         # pixel rays: what ft_render_hits reports
        hit = want_rec[:, 14].view(np.int32) == 1
        assert np.array_equal(hits.material == -1, ~hit), name                                # -1 exactly where the oracle misses
        for i in np.nonzero(hit)[0]:
            desc = hits.descriptor(hits.material[i])
            assert desc is not None, (name, i)
            if desc.kind == "solid":
                assert tuple(np.float32(v) for v in desc.args[0]) == tuple(want_rec[i, 11:14]), (name, i)
        shaded, _, _ = ds.trace_rays_hits(rays, shade=True, records=False)
        assert np.array_equal(shaded.material, hits.material), name


@pytest.mark.parametrize("option", ["cull", "escape", "lazy_union", "carved", "reuse", "cert"])
def test_shortcuts_do_not_change_the_results(gpu, oracle, option):
    for k, (name, scene, W, H) in enumerate(scenes()):
        ds = gpu.scene(scene)
        rays, _ = ray_buffer(oracle, ds, k, W, H)
        want, want_rgb, _ = ds.trace_rays_hits(rays)
        want_only, _, _ = ds.trace_rays_hits(rays, shade=False)
        with options(gpu, **{option: 0}):
            got, rgb, _ = ds.trace_rays_hits(rays)
            got_only, _, _ = ds.trace_rays_hits(rays, shade=False)
        for a, b in ((got, want), (got_only, want_only), (got_only, want)):
            assert same_bits(a.records, b.records), (option, name)
            assert np.array_equal(a.material, b.material), (option, name)
        assert_bit_equal(rgb, want_rgb, f"{option} = 0, {name}: rgb")


def test_plain_trace_rays_stays_on_the_carved_kernels(gpu, oracle):
    scene = syn.console_scene(n=200)[0]
    ds = gpu.scene(scene)
    assert ds.info()["fast_path"] == 3
    rays = pixel_rays(oracle, 40, 37)
    rgb, _ = ds.trace_rays(rays)
    assert ds.info()["fast_path"] == 3
    want, _ = oracle.Oracle().scene(scene).trace_rays(rays)
    assert_bit_equal(rgb, want, "carved scene, ft_trace_rays")


DEVICE_FORMS = r"""
import json, sys
import numpy as np
import torch                              # before the library: torch's HIP runtime is the one the process loads first
import fraytracer_amd as ft
from fraytracer_amd import synthetic as syn
sys.path.insert(0, "tests")
import test_gpu_rays_device as T
from oracle import binding as oracle
bits = lambda t: t.detach().cpu().numpy().view(np.uint32)
same = lambda t, a: bool(np.array_equal(bits(t), np.ascontiguousarray(a).view(np.uint32)))
KEYS = ("rays_primary", "rays_shadow", "hits_primary", "hits_shadow", "flags")
dev = ft.Device(0)
res = []
for k in (1, 3, 5):                       # lean, carved -> general, on-demand calls
    name, scene, W, H = T.scenes()[k]
    ds = dev.scene(scene)
    rays, _ = T.ray_buffer(oracle, ds, k, W, H)
    rays = rays[:len(rays) - 5]           # odd, and no multiple of 64
    n = len(rays)
    assert n % 64 != 0 and n % 2 == 1
    want, want_rgb, want_st = ds.trace_rays_hits(rays)
    want_form, _ = ds.form_try_trace(rays)
    want_obj, obj_st = ds.object_try_trace(rays)
    nan = float("nan")
    d_rays = torch.from_numpy(rays).cuda()
    new = lambda *shape: torch.full(shape, nan, dtype=torch.float32, device="cuda")
    d_rgb, d_rec, d_form, d_obj = new(n, 3), new(n, 16), new(n, 10), new(n, 16)
    d_mat = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    d_mat2 = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    r = {"scene": name}
    ds.trace_rays_hits_device(d_rays.data_ptr(), n, d_rgb.data_ptr(), d_rec.data_ptr(), d_mat.data_ptr())
    st = ds.collect_stats()
    r["hits_rgb"], r["hits_rec"], r["hits_mat"] = same(d_rgb, want_rgb), same(d_rec, want.records), bool(np.array_equal(d_mat.cpu().numpy(), want.material))
    r["hits_stats"] = all(st[c] == want_st[c] for c in KEYS)
    d_rgb.fill_(nan); torch.cuda.synchronize()
    ds.trace_rays_device(d_rays.data_ptr(), n, d_rgb.data_ptr())
    st = ds.collect_stats()
    r["rgb"] = same(d_rgb, want_rgb) and all(st[c] == want_st[c] for c in KEYS)
    ds.form_try_trace_device(d_rays.data_ptr(), n, d_form.data_ptr())
    ds.object_try_trace_device(d_rays.data_ptr(), n, d_obj.data_ptr(), d_mat2.data_ptr())
    st = ds.collect_stats()
    r["form"], r["object"] = same(d_form, want_form), same(d_obj, want_obj)
    r["object_mat"] = bool(np.array_equal(d_mat2.cpu().numpy(), want.material))
    r["object_stats"] = st["rays_primary"] == 2 * n and st["hits_primary"] == 2 * obj_st["hits_primary"] and st["rays_shadow"] == 0
    d_obj.fill_(nan); torch.cuda.synchronize()
    ds.object_try_trace_device(d_rays.data_ptr(), n, d_obj.data_ptr())                       # no material plane: ft_object_try_trace itself
    ds.collect_stats()
    r["object_plain"] = same(d_obj, want_obj)
    # hits only through the device form: nothing is written to an image
    d_rec.fill_(nan); torch.cuda.synchronize()
    ds.trace_rays_hits_device(d_rays.data_ptr(), n, None, d_rec.data_ptr())
    st = ds.collect_stats()
    r["hits_only"] = same(d_rec, want.records) and st["rays_shadow"] == 0
    # n = 0: nothing launched, nothing written; a misaligned ray buffer is refused, nothing launched
    d_rgb.fill_(nan); torch.cuda.synchronize()
    ds.trace_rays_hits_device(d_rays.data_ptr(), 0, d_rgb.data_ptr(), d_rec.data_ptr(), d_mat.data_ptr())
    try:
        ds.trace_rays_device(d_rays.data_ptr() + 4, n - 1, d_rgb.data_ptr())
        r["misaligned"] = False
    except ft.FrayTracerError as e:
        r["misaligned"] = e.code == -1
    st = ds.collect_stats()
    r["nothing_launched"] = st["rays_primary"] == 0 and bool(torch.isnan(d_rgb).all())
    # the tensor front end on a side stream, behind the torch kernel that makes the rays: the stream hand-over
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        big = d_rays.repeat(1, 1)
        for _ in range(20):
            big = big * 1.0                # torch kernels queued in front of the trace on the same stream
        hits, rgb, none = ds.trace_rays_hits(big)
        rgb2 = rgb + 0.0                   # and one behind it
        rec1, none1 = ds.object_try_trace(big)
        form1, _ = ds.form_try_trace(big)
        rgb1, _ = ds.trace_rays(big)
    side.synchronize()
    r["tensor"] = none is None and none1 is None and same(rgb, want_rgb) and same(rgb2, want_rgb) and same(hits.records, want.records) \
        and bool(np.array_equal(hits.material.cpu().numpy(), want.material)) and same(rec1, want_obj) and same(form1, want_form) and same(rgb1, want_rgb)
    r["tensor_types"] = rgb.is_cuda and hits.material.dtype == torch.int32 and bool(np.array_equal(hits.hit.cpu().numpy(), want.hit))
    st = ds.collect_stats()
    r["tensor_stats"] = st["rays_primary"] == 4 * n
    # the default stream works as well
    hits0, rgb0, _ = ds.trace_rays_hits(d_rays * 1.0)
    r["tensor_default_stream"] = same(rgb0 + 0.0, want_rgb) and same(hits0.records, want.records)
    ds.collect_stats()
    for bad, why in ((d_rays.double(), "float32"), (d_rays[:, :7].contiguous(), "[n, 8]"), (d_rays[::2], "contiguous")):
        try:
            ds.trace_rays_hits(bad)
            r["refuses " + why] = False
        except ValueError as e:
            r["refuses " + why] = why in str(e)
    res.append(r)
dev.close()
print(json.dumps(res))
"""


def test_device_forms_equal_the_host_forms():
    """the *_device entry points and the tensor front end, in a child process that loads torch before the library"""
    out = subprocess.run([sys.executable, "-c", DEVICE_FORMS], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert len(res) == 3
    for r in res:
        failed = [k for k, v in r.items() if k != "scene" and v is not True]
        assert not failed, (r["scene"], failed)
