"""Batches of camera views (ft_render_views / ft_render_views_device, DeviceScene.render_views): one launch over K cameras of one scene.
Block k of the batch is bit for bit the single render of camera k, in every trace kernel family, with the EXTENSION parameters, under every
option, across the 64-view split, with column tiling; the counters are the sums of the single renders'."""
import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import synthetic as syn
from helpers import assert_bit_equal, options, options_left_at_defaults  # noqa: F401  (options_left_at_defaults: a fixture)
from test_gpu_hits import scenes

pytestmark = pytest.mark.gpu

EPS, LEN = syn.EPSILON, syn.RAY_LENGTH
COUNTERS = ("rays_primary", "rays_shadow", "rays_ext", "hits_primary", "hits_shadow", "sdf_evals", "flags")
EXACT = ("rays_primary", "rays_shadow", "rays_ext", "hits_primary", "hits_shadow", "flags")


def look(pos, at, up=(0.0, 1.0, 0.0)):
    return ft.Camera.lookAt(Position=pos, LookAt=at, Up=up, Lens=ft.Lens.create(60.0))


def inside_point(ds):
    """a point inside the scene's object (Distance < 0 there): a camera there hits at its own position"""
    g = np.linspace(-3.0, 3.0, 13, dtype=np.float32)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    d, _ = ds.eval_distance(pts)
    inside = np.flatnonzero(d < -EPS)
    return tuple(float(v) for v in pts[inside[len(inside) // 2]]) if len(inside) else (0.0, 0.0, 0.0)


def cameras(ds):
    """the Program.fs camera, an orbit position, one inside the object (or the support sphere), one looking away (every ray misses), one grazing"""
    return [syn.default_camera(),
            look((7.0, 3.0, -7.0), (0.0, 0.0, 0.0)),
            look(inside_point(ds), (4.0, 1.0, 2.0)),
            look((0.0, 0.0, -10.0), (0.0, 0.0, -20.0)),
            look((4.6, 0.4, -9.0), (4.2, 0.1, 9.0))]


def singles(ds, W, H, cams, **kw):
    out = [ds.render(EPS, LEN, ft.ImageSize(W, H), c, **kw) for c in cams]
    return [img for img, _ in out], {k: sum(st[k] for _, st in out) for k in COUNTERS}, [st for _, st in out]


def check_views(ds, W, H, cams, what, exact_evals=True, **kw):
    imgs, st = ds.render_views(EPS, LEN, ft.ImageSize(W, H), cams, **kw)
    want, total, _ = singles(ds, W, H, cams, **kw)
    assert imgs.shape == (len(cams),) + want[0].shape and imgs.dtype == np.float32
    for k, w in enumerate(want):
        assert_bit_equal(imgs[k], w, f"{what}: view {k} = render")
    for k in EXACT:
        assert st[k] == total[k], (what, k, st[k], total[k])
    if exact_evals:
        assert st["sdf_evals"] == total["sdf_evals"], (what, st["sdf_evals"], total["sdf_evals"])
    else:
        assert st["sdf_evals"] <= total["sdf_evals"] * 1.05 + 1000, (what, st["sdf_evals"], total["sdf_evals"])
    return imgs, st, total


def test_every_kernel_family_equals_single_renders_and_the_oracle(gpu, oracle):
    families = set()
    for name, scene, W, H in scenes():
        ds = gpu.scene(scene)
        fp = ds.info()["fast_path"]
        families.add(fp)
        cams = cameras(ds)
        with options(gpu, cert=0):                             # the certificate's firing depends on how waves are packed: counted below
            imgs, _, _ = check_views(ds, W, H, cams, name)
        imgs_c, st_c = ds.render_views(EPS, LEN, ft.ImageSize(W, H), cams)
        want, total, _ = singles(ds, W, H, cams)
        for k in range(len(cams)):
            assert_bit_equal(imgs_c[k], want[k], f"{name}: view {k} = render (certificate on)")
        for k in EXACT:
            assert st_c[k] == total[k], (name, k)
        with options(gpu, cert=0):
            _, total_off, _ = singles(ds, W, H, cams)
        assert st_c["sdf_evals"] <= total_off["sdf_evals"], name
        orc, _ = oracle.Oracle().scene(scene).render(EPS, LEN, W, H, cams[0].as_array())
        assert_bit_equal(imgs[0], orc, f"{name}: Program.fs camera = oracle")
        assert (imgs[3] == imgs[3][0, 0]).all(), f"{name}: looking away, every ray misses"
    assert families >= {0, 1, 2, 3}, families                 # general, lean smooth spheres, calls, carved


def test_counters_are_the_sums_with_the_certificate_off(gpu):
    for scene, W, H in ((syn.config3(n=64)[0], 72, 53), (syn.console_scene(n=200)[0], 96, 71), (syn.mixed_nested()[0], 61, 47),
                        (syn.config5()[0], 64, 57)):
        ds = gpu.scene(scene)
        cams = cameras(ds)
        with options(gpu, cert=0) as set_:
            for reuse in (1, 0):
                set_(reuse=reuse)
                check_views(ds, W, H, cams, f"fast_path {ds.info()['fast_path']} reuse {reuse}")


def test_extension_params_per_view(gpu, oracle):
    c2 = syn.config2(boxes=True)[0]
    cases = [("config2 spp 4", c2, dict(spp=4)), ("config2 ao 4", c2, dict(ao_samples=4, ao_radius=0.75)),
             ("config3 spp 4 (lean EXTENSION)", syn.config3(n=64)[0], dict(spp=4)),
             ("config5 glass", syn.config5()[0], dict(spp=4, max_bounces=4, spectral=4))]
    W, H = 64, 57
    for name, scene, ext in cases:
        ds = gpu.scene(scene)
        cams = cameras(ds)[:3]
        imgs, _, _ = check_views(ds, W, H, cams, name, **ext)
        orc, _ = oracle.Oracle().scene(scene).render(EPS, LEN, W, H, cams[1].as_array(), **ext)
        assert_bit_equal(imgs[1], orc, f"{name}: orbit camera = oracle")


OPTIONS = [("reuse", 0), ("cert", 0), ("escape", 0), ("cull", 0), ("carved", 0), ("chunk", 16), ("chunk", 32), ("guided", 1),
           ("tail_k", 64), ("tail_k", 0)]


def test_options_leave_every_view_unchanged(gpu):
    for scene, W, H in ((syn.config3(n=64)[0], 72, 53), (syn.console_scene(n=200)[0], 96, 71), (syn.mixed_nested()[0], 61, 47)):
        ds = gpu.scene(scene)
        cams = cameras(ds)
        base, _, _ = singles(ds, W, H, cams)
        for opt, v in OPTIONS + ([("math", ft.glibc_build_of_this_host())] if ds.info()["fast_path"] == 1 else []):
            with options(gpu, **{opt: v}):
                imgs, _ = ds.render_views(EPS, LEN, ft.ImageSize(W, H), cams)
                want = base if opt != "math" else singles(ds, W, H, cams)[0]
            for k in range(len(cams)):
                assert_bit_equal(imgs[k], want[k], f"fast_path {ds.info()['fast_path']} {opt}={v}: view {k}")


def test_guided_hand_out_with_part_tiles(gpu):
    """the guided hand-out's chunk sizes change under a race and may let a chunk straddle two views: every view still renders right"""
    ds = gpu.scene(syn.config3(n=64)[0])
    cams = [look((8.0 * np.cos(a), 1.0, 8.0 * np.sin(a)), (0.0, 0.0, 0.0)) for a in np.linspace(0.0, 6.0, 12)]
    want, _, _ = singles(ds, 200, 193, cams)
    for chunk in (64, 32):
        with options(gpu, guided=1, chunk=chunk):
            imgs, _ = ds.render_views(EPS, LEN, ft.ImageSize(200, 193), cams)
        for k in range(len(cams)):
            assert_bit_equal(imgs[k], want[k], f"guided chunk {chunk}: view {k}")


def test_batches_split_at_64_views(gpu):
    for scene in (syn.config3(n=64)[0], syn.console_scene(n=200)[0]):
        ds = gpu.scene(scene)
        for K in (65, 130):
            cams = [look((9.0 * np.cos(a), 2.0 * np.sin(3 * a), 9.0 * np.sin(a)), (0.0, 0.0, 0.0)) for a in np.linspace(0.0, 6.2, K)]
            check_views(ds, 16, 16, cams, f"K={K}", exact_evals=ds.info()["fast_path"] != 1)


def test_column_tiling_per_view(gpu):
    W, H = 72, 53
    for scene in (syn.config3(n=64)[0], syn.console_scene(n=200)[0]):
        ds = gpu.scene(scene)
        cams = cameras(ds)[:4]
        for tiling in (dict(x0=8, n_columns=40), dict(x0=3, n_columns=21), dict(n_columns=24, stripe_width=8, stripe_ranks=3, stripe_rank=1)):
            imgs, _, _ = check_views(ds, W, H, cams, f"tiling {tiling}", exact_evals=ds.info()["fast_path"] != 1, **tiling)
            assert imgs.shape == (4, tiling["n_columns"], H, 3)


def test_one_view_is_render(gpu):
    for name, scene, W, H in scenes():
        ds = gpu.scene(scene)
        cam = cameras(ds)[1]
        imgs, st = ds.render_views(EPS, LEN, ft.ImageSize(W, H), [cam])
        img, want = ds.render(EPS, LEN, ft.ImageSize(W, H), cam)
        assert_bit_equal(imgs[0], img, name)
        for k in COUNTERS + ("wave_evals",):
            assert st[k] == want[k], (name, k, st[k], want[k])


def test_out_buffer_and_image_render_views(gpu):
    scene = syn.config3(n=64)[0]
    ds = gpu.scene(scene)
    cams = cameras(ds)[:3]
    out = np.full((3, 40, 30, 3), np.nan, np.float32)
    imgs, _ = ds.render_views(EPS, LEN, ft.ImageSize(40, 30), cams, out=out)
    assert imgs is out
    want, _, _ = singles(ds, 40, 30, cams)
    for k in range(3):
        assert_bit_equal(out[k], want[k], f"out view {k}")
    with pytest.raises(ValueError):
        ds.render_views(EPS, LEN, ft.ImageSize(40, 30), cams, out=np.empty((2, 40, 30, 3), np.float32))
    via_image = ft.Image.renderViews(EPS, LEN, ft.ImageSize(40, 30), cams, scene, device=gpu)
    assert_bit_equal(via_image, out, "Image.renderViews")
    with pytest.raises(ft.FrayTracerError):
        ds.render_views(EPS, LEN, ft.ImageSize(40, 30), [])


def test_job_limit_is_refused_and_the_context_still_renders(gpu):
    scene = syn.config3(n=64)[0]
    ds = gpu.scene(scene)
    cams = cameras(ds)[:4]
    with pytest.raises(ft.FrayTracerError) as e:
        ds.render_views_device(EPS, LEN, ft.ImageSize(4096, 4096), cams, 256, spp=64)
    assert e.value.code == ft._lib.FT_ERR_UNSUPPORTED
    check_views(ds, 72, 53, cams, "after the refusal", exact_evals=False)


DEVICE_FORM = r"""
import json
import numpy as np
import torch                              # before the library, as bench.py and the tools do: torch's HIP runtime is the one the process loads first
import fraytracer_amd as ft
from fraytracer_amd import synthetic as syn
EPS, LEN, W, H = syn.EPSILON, syn.RAY_LENGTH, 72, 53
dev = ft.Device(0)
lens = ft.Lens.create(60.0)
cams = [ft.Camera.lookAt(Position=p, LookAt=(0.0, 0.0, 0.0), Up=(0.0, 1.0, 0.0), Lens=lens) for p in ((0.0, 0.0, -10.0), (7.0, 3.0, -7.0), (-6.0, -2.0, 8.0))]
res = []
dev.set_option("cert", 0)
for scene, ext in ((syn.config3(n=64)[0], {}), (syn.console_scene(n=200)[0], {}), (syn.config2(boxes=True)[0], dict(spp=4))):
    ds = dev.scene(scene)
    want, want_st = ds.render_views(EPS, LEN, ft.ImageSize(W, H), cams, **ext)
    d_out = torch.full((len(cams), W, H, 3), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ds.render_views_device(EPS, LEN, ft.ImageSize(W, H), cams, d_out.data_ptr(), **ext)
    st = ds.collect_stats()
    res.append({"image": bool(np.array_equal(d_out.cpu().numpy().view(np.uint32), want.view(np.uint32))),
                "stats": all(st[k] == want_st[k] for k in ("rays_primary", "rays_shadow", "hits_primary", "hits_shadow", "sdf_evals", "flags"))})
dev.close()
print(json.dumps(res))
"""


def test_device_form_equals_host_form():
    """render_views_device into a torch buffer + collect_stats = the host form; in a child process that loads torch before the library"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", DEVICE_FORM], cwd=root, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert len(res) == 3 and all(all(r.values()) for r in res), res
