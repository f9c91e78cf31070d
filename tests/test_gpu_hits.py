"""Per-pixel hit buffers (ft_render_hits / ft_render_hits_device, DeviceScene.render_hits): SdfObject.tryTrace scene.Object of every
pixel's camera ray (SdfObject.fs:66-78 in Image.render's pixel loop, Image.fs:26-35), bit for bit against the CPU oracle, with and without
the shaded frame of the same launch."""
import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import SdfForm, SdfLight, SdfMaterial, SdfObject, SdfScene
from fraytracer_amd import synthetic as syn
from helpers import assert_bit_equal, options, options_left_at_defaults  # noqa: F401  (options_left_at_defaults: a fixture)

pytestmark = pytest.mark.gpu

EPS, LEN = syn.EPSILON, syn.RAY_LENGTH
COUNTERS = ("rays_primary", "rays_shadow", "rays_ext", "hits_primary", "hits_shadow", "sdf_evals", "flags")


def scenes():
    """one scene per kernel family the hit buffers run in"""
    return [("console_like (general)", syn.console_like(n=300)[0], 72, 53),
            ("config3 (lean)", syn.config3(n=64)[0], 72, 53),
            ("mixed_nested (general, nested combinators)", syn.mixed_nested()[0], 61, 47),
            ("console_scene (carved -> general)", syn.console_scene(n=200)[0], 200, 193),
            ("config2 boxes", syn.config2(boxes=True)[0], 72, 53),
            ("config5 (glass; on-demand calls)", syn.config5()[0], 64, 57)]


def oracle_hits(oracle, scene, W, H, cols=None):
    cam = syn.default_camera().as_array()
    cols = range(W) if cols is None else cols
    rays = np.stack([oracle.pixel_ray(cam, W, H, x, y, EPS, LEN) for x in cols for y in range(H)])
    rec, cnt = oracle.Oracle().scene(scene).object_try_trace(rays)
    return rays, rec.reshape(len(cols), H, 16), cnt


def test_hits_only_equal_the_oracle(gpu, oracle):
    cam = syn.default_camera()
    for name, scene, W, H in scenes():
        ds = gpu.scene(scene)
        hits, img, st = ds.render_hits(EPS, LEN, ft.ImageSize(W, H), cam)
        assert img is None
        rays, want, _ = oracle_hits(oracle, scene, W, H)
        assert hits.records.shape == (W, H, 16) and hits.records.dtype == np.float32
        assert np.array_equal(hits.records.view(np.uint32), want.view(np.uint32)), name       # all 16 dwords, misses included
        assert_bit_equal(hits.records.reshape(-1, 16), ds.object_try_trace(rays)[0], f"{name}: = ft_object_try_trace")
        assert 0 < hits.hit.sum() < W * H, name
        assert (hits.records[..., 15] == 0).all()


def shaded_cases():
    c2 = syn.config2(boxes=True)[0]
    return [("config2 spp 4", c2, dict(spp=4)), ("config2 ao", c2, dict(ao_samples=4, ao_radius=0.75)),
            ("config5 glass spectral", syn.config5()[0], dict(spp=4, max_bounces=4, spectral=4)),
            ("mixed_nested", syn.mixed_nested()[0], {}), ("config3", syn.config3(n=64)[0], {})]


def test_shade_and_hits_equal_render_and_oracle(gpu, oracle):
    cam = syn.default_camera()
    W, H = 72, 53
    for name, scene, ext in shaded_cases():
        ds = gpu.scene(scene)
        want_img, want_st = ds.render(EPS, LEN, ft.ImageSize(W, H), cam, **ext)
        hits, img, st = ds.render_hits(EPS, LEN, ft.ImageSize(W, H), cam, shade=True, **ext)
        assert_bit_equal(img, want_img, f"{name}: image = render")
        for k in COUNTERS:
            assert st[k] == want_st[k], (name, k, st[k], want_st[k])
        orc, _ = oracle.Oracle().scene(scene).render(EPS, LEN, W, H, cam.as_array(), **ext)
        assert_bit_equal(img, orc, f"{name}: image = oracle")
        alone, _, _ = ds.render_hits(EPS, LEN, ft.ImageSize(W, H), cam)
        assert np.array_equal(hits.records.view(np.uint32), alone.records.view(np.uint32)), name
        assert np.array_equal(hits.material, alone.material), name
        _, want, _ = oracle_hits(oracle, scene, W, H)
        assert np.array_equal(hits.records.view(np.uint32), want.view(np.uint32)), name


def test_material_plane_names_the_hit_material(gpu, oracle):
    colours = [(0.9, 0.1, 0.1), (0.1, 0.9, 0.1), (0.1, 0.1, 0.9), (0.8, 0.8, 0.1), (0.1, 0.8, 0.8), (0.8, 0.1, 0.8)]
    objs = [SdfObject.create(SdfMaterial.createSolid(c), SdfForm.Primitive.sphere((-5.0 + 2.0 * i, 0.3 * i - 0.7, 0.5 * i), 1.1))
            for i, c in enumerate(colours)]
    scene = SdfScene(SdfObject.union(objs), syn.BACKGROUND, [SdfLight.directional((0.3, -1.0, 0.5), (1.0, 1.0, 1.0))])
    cam = syn.default_camera()
    W, H = 96, 64
    ds = gpu.scene(scene)
    hits, _, _ = ds.render_hits(EPS, LEN, ft.ImageSize(W, H), cam)
    _, want, _ = oracle_hits(oracle, scene, W, H)
    assert np.array_equal(hits.records.view(np.uint32), want.view(np.uint32))
    m = hits.material
    assert (m[~hits.hit] == -1).all() and (m[hits.hit] >= 0).all()
    by_colour = {tuple(np.float32(v) for v in c): h for h, d in ds.materials.items() for c in [d.args[0]]}
    seen = set()
    for x, y in zip(*np.nonzero(hits.hit)):
        h = int(m[x, y])
        desc = hits.descriptor(h)
        assert desc is not None and desc.kind == "solid"
        assert tuple(np.float32(v) for v in desc.args[0]) == tuple(hits.color[x, y]), (x, y)
        assert by_colour[tuple(want[x, y, 11:14])] == h, (x, y)      # the handle the oracle's colour names
        seen.add(h)
    assert len(seen) >= 4
    only, img, _ = ds.render_hits(EPS, LEN, ft.ImageSize(W, H), cam, records=False)
    assert only.records is None and img is None and np.array_equal(only.material, m)
    # glass materials are named as well
    ds5 = gpu.scene(syn.config5()[0])
    h5, _, _ = ds5.render_hits(EPS, LEN, ft.ImageSize(64, 57), cam)
    kinds = {ds5.materials[int(h)].kind for h in np.unique(h5.material[h5.hit])}
    assert kinds == {"solid", "glass"}


def test_tiling_cuts_the_full_buffers(gpu):
    cam = syn.default_camera()
    W, H = 96, 40
    ds = gpu.scene(syn.console_like(n=300)[0])
    full, img, _ = ds.render_hits(EPS, LEN, ft.ImageSize(W, H), cam, shade=True)
    part, pimg, _ = ds.render_hits(EPS, LEN, ft.ImageSize(W, H), cam, shade=True, x0=24, n_columns=40)
    assert np.array_equal(part.records.view(np.uint32), full.records[24:64].view(np.uint32))
    assert np.array_equal(part.material, full.material[24:64])
    assert_bit_equal(pimg, img[24:64], "x0 / n_columns image")
    for r in range(3):
        got, gimg, _ = ds.render_hits(EPS, LEN, ft.ImageSize(W, H), cam, shade=True, stripe_width=16, stripe_ranks=3, stripe_rank=r)
        xs = [(c // 16) * 48 + r * 16 + c % 16 for c in range(W // 3)]
        assert np.array_equal(got.records.view(np.uint32), full.records[xs].view(np.uint32)), r
        assert np.array_equal(got.material, full.material[xs]), r
        assert_bit_equal(gimg, img[xs], f"stripe rank {r} image")


@pytest.mark.parametrize("option,off", [("cull", 0), ("escape", 0), ("lazy_union", 0), ("carved", 0), ("reuse", 0), ("chunk", 32), ("tail_k", 0)])
def test_options_do_not_change_the_buffers(gpu, option, off):
    cam = syn.default_camera()
    W, H = 72, 53
    cases = [syn.console_scene(n=200)[0], syn.config3(n=64)[0], syn.mixed_nested()[0], syn.config5()[0]]
    for scene in cases:
        ds = gpu.scene(scene)
        want, want_img, _ = ds.render_hits(EPS, LEN, ft.ImageSize(W, H), cam, shade=True)
        want_only, _, _ = ds.render_hits(EPS, LEN, ft.ImageSize(W, H), cam)
        with options(gpu, **{option: off}):
            got, img, _ = ds.render_hits(EPS, LEN, ft.ImageSize(W, H), cam, shade=True)
            got_only, _, _ = ds.render_hits(EPS, LEN, ft.ImageSize(W, H), cam)
        for a, b in ((got, want), (got_only, want_only), (got_only, want)):
            assert np.array_equal(a.records.view(np.uint32), b.records.view(np.uint32)), option
            assert np.array_equal(a.material, b.material), option
        assert_bit_equal(img, want_img, f"{option} = {off}: image")


def test_hits_only_statistics(gpu, oracle):
    cam = syn.default_camera()
    for name, scene, W, H in scenes()[:3]:
        ds = gpu.scene(scene)
        hits, _, st = ds.render_hits(EPS, LEN, ft.ImageSize(W, H), cam, spp=4, ao_samples=4, ao_radius=0.5)   # EXTENSION fields do not apply
        _, want, cnt = oracle_hits(oracle, scene, W, H)
        assert st["rays_primary"] == W * H and st["rays_shadow"] == 0 and st["rays_ext"] == 0, name
        assert st["hits_primary"] == int((want[..., 14].view(np.int32) == 1).sum()) == int(hits.hit.sum()), name
        assert st["flags"] == 0 and st["hits_shadow"] == 0, name
        assert np.array_equal(hits.records.view(np.uint32), want.view(np.uint32)), name


DEVICE_FORM = r"""
import json, sys
import numpy as np
import torch                              # before the library, as bench.py and the tools do: torch's HIP runtime is the one the process loads first
import fraytracer_amd as ft
from fraytracer_amd import synthetic as syn
EPS, LEN, W, H = syn.EPSILON, syn.RAY_LENGTH, 72, 53
dev = ft.Device(0)
cam = syn.default_camera()
res = []
for scene in (syn.config3(n=64)[0], syn.console_like(n=300)[0]):
    ds = dev.scene(scene)
    want, want_img, want_st = ds.render_hits(EPS, LEN, ft.ImageSize(W, H), cam, shade=True, spp=4)
    d_hits = torch.empty((W, H, 16), dtype=torch.float32, device="cuda")
    d_mat = torch.empty((W, H), dtype=torch.int32, device="cuda")
    d_img = torch.empty((W, H, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ds.render_hits_device(EPS, LEN, ft.ImageSize(W, H), cam, d_hits.data_ptr(), d_mat.data_ptr(), d_img.data_ptr(), spp=4)
    st = ds.collect_stats()
    r = {"records": bool(np.array_equal(d_hits.cpu().numpy().view(np.uint32), want.records.view(np.uint32))),
         "material": bool(np.array_equal(d_mat.cpu().numpy(), want.material)),
         "image": bool(np.array_equal(d_img.cpu().numpy().view(np.uint32), want_img.view(np.uint32))),
         "stats": st["rays_primary"] == want_st["rays_primary"] and st["hits_primary"] == want_st["hits_primary"]}
    d_hits.zero_()
    torch.cuda.synchronize()
    ds.render_hits_device(EPS, LEN, ft.ImageSize(W, H), cam, d_hits.data_ptr())          # hits only, no material plane
    ds.collect_stats()
    r["hits_only"] = bool(np.array_equal(d_hits.cpu().numpy().view(np.uint32), want.records.view(np.uint32)))
    try:
        ds.render_hits_device(EPS, LEN, ft.ImageSize(W, H), cam, None)                   # nothing asked for
        r["refused"] = False
    except ft.FrayTracerError:
        r["refused"] = True
    res.append(r)
dev.close()
print(json.dumps(res))
"""


def test_device_form_equals_host_form():
    """render_hits_device into torch tensors = the host form; in a child process that loads torch before the library"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", DEVICE_FORM], cwd=root, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert len(res) == 2 and all(all(r.values()) for r in res), res


def test_full_size_c3_shade_and_hits(gpu, oracle):
    scene, size = syn.config3()
    cam = syn.default_camera()
    ds = gpu.scene(scene)
    want_img, want_st = ds.render(EPS, LEN, size, cam)
    hits, img, st = ds.render_hits(EPS, LEN, size, cam, shade=True, material=False)
    assert_bit_equal(img, want_img, "C3 4096^2 image")
    del want_img, img
    assert int(hits.hit.sum()) == st["hits_primary"] == want_st["hits_primary"]
    rng = np.random.default_rng(2024)
    xs, ys = rng.integers(0, size.X, 2000), rng.integers(0, size.Y, 2000)
    c = cam.as_array()
    rays = np.stack([oracle.pixel_ray(c, size.X, size.Y, int(x), int(y), EPS, LEN) for x, y in zip(xs, ys)])
    want, _ = oracle.Oracle().scene(scene).object_try_trace(rays)
    assert np.array_equal(hits.records[xs, ys].view(np.uint32), want.view(np.uint32))
