"""Hit buffers of batches of camera views (ft_render_views_hits / ft_render_views_hits_device, DeviceScene.render_views_hits): view k's
records, material plane and image are bit for bit ft_render_hits for camera k, in every kernel family, with the EXTENSION parameters,
across the 64-view split, with column tiling, under every option; the counters are the sums of the single calls'."""
import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import synthetic as syn
from helpers import assert_bit_equal, options, options_left_at_defaults  # noqa: F401  (options_left_at_defaults: a fixture)
from test_gpu_hits import scenes
from test_gpu_views import cameras, look

pytestmark = pytest.mark.gpu

EPS, LEN = syn.EPSILON, syn.RAY_LENGTH
COUNTERS = ("rays_primary", "rays_shadow", "rays_ext", "hits_primary", "hits_shadow", "sdf_evals", "flags")
EXACT = ("rays_primary", "rays_shadow", "rays_ext", "hits_primary", "hits_shadow", "flags")


def singles(ds, W, H, cams, **kw):
    out = [ds.render_hits(EPS, LEN, ft.ImageSize(W, H), c, **kw) for c in cams]
    return out, {k: sum(st[k] for _, _, st in out) for k in COUNTERS}


def check_views_hits(ds, W, H, cams, what, exact_evals=True, shade=False, **kw):
    """the batch against one render_hits per camera: records, material plane, image and counters"""
    hits, img, st = ds.render_views_hits(EPS, LEN, ft.ImageSize(W, H), cams, shade=shade, **kw)
    want, total = singles(ds, W, H, cams, shade=shade, **kw)
    n = kw.get("n_columns", W)
    assert hits.records.shape == (len(cams), n, H, 16) and hits.material.shape == (len(cams), n, H)
    assert (img is None) == (not shade)
    for k, (h, i, _) in enumerate(want):
        assert np.array_equal(hits.records[k].view(np.uint32), h.records.view(np.uint32)), f"{what}: view {k} records"
        assert np.array_equal(hits.material[k], h.material), f"{what}: view {k} material"
        if shade:
            assert_bit_equal(img[k], i, f"{what}: view {k} image")
    for k in EXACT:
        assert st[k] == total[k], (what, k, st[k], total[k])
    if exact_evals:
        assert st["sdf_evals"] == total["sdf_evals"], (what, st["sdf_evals"], total["sdf_evals"])
    else:
        assert st["sdf_evals"] <= total["sdf_evals"] * 1.05 + 1000, (what, st["sdf_evals"], total["sdf_evals"])
    return hits, img, st


def test_each_view_equals_a_single_call_and_the_oracle(gpu, oracle):
    families = set()
    for name, scene, W, H in scenes():
        ds = gpu.scene(scene)
        families.add(ds.info()["fast_path"])
        cams = cameras(ds)
        with options(gpu, cert=0):                             # the certificate's firing depends on how waves are packed: counted below
            hits, _, _ = check_views_hits(ds, W, H, cams, f"{name} hits only")
            check_views_hits(ds, W, H, cams, f"{name} shaded", shade=True)
        got, _, st_c = ds.render_views_hits(EPS, LEN, ft.ImageSize(W, H), cams)
        assert np.array_equal(got.records.view(np.uint32), hits.records.view(np.uint32)), f"{name}: certificate on"
        assert np.array_equal(got.material, hits.material), f"{name}: certificate on"
        _, total = singles(ds, W, H, cams)
        for k in EXACT:
            assert st_c[k] == total[k], (name, k)
        for k, cam in enumerate(cams):                         # hits only = the oracle's object_try_trace of that camera's pixel rays
            c = cam.as_array()
            rays = np.stack([oracle.pixel_ray(c, W, H, x, y, EPS, LEN) for x in range(W) for y in range(H)])
            rec, _ = oracle.Oracle().scene(scene).object_try_trace(rays)
            assert np.array_equal(hits.records[k].view(np.uint32), rec.reshape(W, H, 16).view(np.uint32)), f"{name}: view {k} = oracle"
        assert not hits.hit[3].any() and (hits.material[3] == -1).all(), f"{name}: looking away, every ray misses"
    assert families >= {0, 1, 2, 3}, families                 # general, lean smooth spheres, calls, carved


def test_shading_and_extension_params(gpu):
    """images = render_views, records = the sample-0 records of hits only (ao_radius > 0)"""
    c2 = syn.config2(boxes=True)[0]
    cases = [("config2 spp 4", c2, dict(spp=4)), ("config2 ao 4", c2, dict(ao_samples=4, ao_radius=0.75)),
             ("config3 spp 4 (lean EXTENSION)", syn.config3(n=64)[0], dict(spp=4)),
             ("config5 glass spectral", syn.config5()[0], dict(spp=4, max_bounces=4, spectral=4))]
    W, H = 64, 57
    with options(gpu, cert=0):
        for name, scene, ext in cases:
            ds = gpu.scene(scene)
            cams = cameras(ds)[:3]
            hits, img, st = check_views_hits(ds, W, H, cams, name, shade=True, **ext)
            want_img, want_st = ds.render_views(EPS, LEN, ft.ImageSize(W, H), cams, **ext)
            assert_bit_equal(img, want_img, f"{name}: images = render_views")
            for k in COUNTERS:
                assert st[k] == want_st[k], (name, k, st[k], want_st[k])
            only, _, _ = ds.render_views_hits(EPS, LEN, ft.ImageSize(W, H), cams)
            assert np.array_equal(hits.records.view(np.uint32), only.records.view(np.uint32)), name
            assert np.array_equal(hits.material, only.material), name


def test_batches_split_at_64_views(gpu):
    for scene in (syn.config3(n=64)[0], syn.console_scene(n=200)[0]):
        ds = gpu.scene(scene)
        exact = ds.info()["fast_path"] != 1
        for K in (65, 130):
            cams = [look((9.0 * np.cos(a), 2.0 * np.sin(3 * a), 9.0 * np.sin(a)), (0.0, 0.0, 0.0)) for a in np.linspace(0.0, 6.2, K)]
            check_views_hits(ds, 16, 16, cams, f"K={K}", exact_evals=exact)
        check_views_hits(ds, 16, 16, cams[:66], "K=66 shaded spp 4", exact_evals=exact, shade=True, spp=4)


def test_column_tiling_per_view(gpu):
    W, H = 72, 53
    for scene in (syn.config3(n=64)[0], syn.console_scene(n=200)[0]):
        ds = gpu.scene(scene)
        cams = cameras(ds)[:4]
        full, full_img, _ = ds.render_views_hits(EPS, LEN, ft.ImageSize(W, H), cams, shade=True)
        for tiling in (dict(x0=8, n_columns=40), dict(x0=3, n_columns=21), dict(n_columns=24, stripe_width=8, stripe_ranks=3, stripe_rank=1)):
            hits, img, _ = check_views_hits(ds, W, H, cams, f"tiling {tiling}", exact_evals=ds.info()["fast_path"] != 1, shade=True, **tiling)
            if "x0" in tiling:
                xs = list(range(tiling["x0"], tiling["x0"] + tiling["n_columns"]))
            else:
                xs = [(c // 8) * 24 + 8 + c % 8 for c in range(24)]
            assert np.array_equal(hits.records.view(np.uint32), full.records[:, xs].view(np.uint32)), tiling
            assert np.array_equal(hits.material, full.material[:, xs]), tiling
            assert_bit_equal(img, full_img[:, xs], f"tiling {tiling}: image")


OPTIONS = [("reuse", 0), ("cert", 0), ("escape", 0), ("cull", 0), ("lazy_union", 0), ("carved", 0), ("chunk", 32), ("guided", 1),
           ("tail_k", 64), ("tail_k", 0)]


def test_options_and_glibc_math_change_no_bit(gpu):
    W, H = 72, 53
    for scene in (syn.config3(n=64)[0], syn.console_scene(n=200)[0], syn.mixed_nested()[0], syn.config5()[0]):
        ds = gpu.scene(scene)
        cams = cameras(ds)
        base, base_img, _ = ds.render_views_hits(EPS, LEN, ft.ImageSize(W, H), cams, shade=True)
        base_only, _, _ = ds.render_views_hits(EPS, LEN, ft.ImageSize(W, H), cams)
        assert np.array_equal(base.records.view(np.uint32), base_only.records.view(np.uint32))
        for opt, v in OPTIONS + [("math", ft.glibc_build_of_this_host())]:
            with options(gpu, **{opt: v}):
                got, img, _ = ds.render_views_hits(EPS, LEN, ft.ImageSize(W, H), cams, shade=True)
                only, _, _ = ds.render_views_hits(EPS, LEN, ft.ImageSize(W, H), cams)
                if opt == "math":                              # glibc math: its own bits, the same in the batch and in single calls
                    want = singles(ds, W, H, cams, shade=True)[0]
                    want_rec = np.stack([h.records for h, _, _ in want])
                    want_mat = np.stack([h.material for h, _, _ in want])
                    want_img = np.stack([i for _, i, _ in want])
                else:
                    want_rec, want_mat, want_img = base.records, base.material, base_img
            what = f"fast_path {ds.info()['fast_path']} {opt}={v}"
            assert np.array_equal(got.records.view(np.uint32), want_rec.view(np.uint32)), f"{what}: records"
            assert np.array_equal(only.records.view(np.uint32), want_rec.view(np.uint32)), f"{what}: hits only"
            assert np.array_equal(got.material, want_mat) and np.array_equal(only.material, want_mat), what
            assert_bit_equal(img, want_img, f"{what}: images")


def test_one_view_is_render_hits(gpu):
    for name, scene, W, H in scenes():
        ds = gpu.scene(scene)
        cam = cameras(ds)[1]
        for shade in (False, True):
            hits, img, st = ds.render_views_hits(EPS, LEN, ft.ImageSize(W, H), [cam], shade=shade)
            want, want_img, want_st = ds.render_hits(EPS, LEN, ft.ImageSize(W, H), cam, shade=shade)
            assert np.array_equal(hits.records[0].view(np.uint32), want.records.view(np.uint32)), name
            assert np.array_equal(hits.material[0], want.material), name
            if shade:
                assert_bit_equal(img[0], want_img, name)
            for k in COUNTERS:                                 # (wave_evals: wave rounds, which depend on how racing waves take their chunks)
                assert st[k] == want_st[k], (name, shade, k, st[k], want_st[k])


def test_partial_outputs_and_image_render_views_hits(gpu):
    scene = syn.config5()[0]
    ds = gpu.scene(scene)
    cams = cameras(ds)[:3]
    full, _, _ = ds.render_views_hits(EPS, LEN, ft.ImageSize(40, 30), cams)
    only_mat, img, _ = ds.render_views_hits(EPS, LEN, ft.ImageSize(40, 30), cams, records=False)
    assert only_mat.records is None and img is None and np.array_equal(only_mat.material, full.material)
    only_rec, _, _ = ds.render_views_hits(EPS, LEN, ft.ImageSize(40, 30), cams, material=False)
    assert only_rec.material is None and np.array_equal(only_rec.records.view(np.uint32), full.records.view(np.uint32))
    kinds = {ds.materials[int(h)].kind for h in np.unique(full.material[full.hit])}
    assert kinds == {"solid", "glass"}
    via_image = ft.Image.renderViewsHits(EPS, LEN, ft.ImageSize(40, 30), cams, scene, device=gpu)
    assert np.array_equal(via_image.records.view(np.uint32), full.records.view(np.uint32))
    assert np.array_equal(via_image.material, full.material)
    with pytest.raises(ft.FrayTracerError):
        ds.render_views_hits(EPS, LEN, ft.ImageSize(40, 30), [])
    with pytest.raises(ft.FrayTracerError):
        ds.render_views_hits(EPS, LEN, ft.ImageSize(40, 30), cams, material=False, records=False)


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
K = len(cams)
res = []
dev.set_option("cert", 0)
for scene, ext in ((syn.config3(n=64)[0], {}), (syn.console_scene(n=200)[0], {}), (syn.config2(boxes=True)[0], dict(spp=4))):
    ds = dev.scene(scene)
    want, want_img, want_st = ds.render_views_hits(EPS, LEN, ft.ImageSize(W, H), cams, shade=True, **ext)
    d_hits = torch.full((K, W, H, 16), float("nan"), dtype=torch.float32, device="cuda")
    d_mat = torch.full((K, W, H), -7, dtype=torch.int32, device="cuda")
    d_img = torch.full((K, W, H, 3), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ds.render_views_hits_device(EPS, LEN, ft.ImageSize(W, H), cams, d_hits.data_ptr(), d_mat.data_ptr(), d_img.data_ptr(), **ext)
    st = ds.collect_stats()
    r = {"records": bool(np.array_equal(d_hits.cpu().numpy().view(np.uint32), want.records.view(np.uint32))),
         "material": bool(np.array_equal(d_mat.cpu().numpy(), want.material)),
         "image": bool(np.array_equal(d_img.cpu().numpy().view(np.uint32), want_img.view(np.uint32))),
         "stats": all(st[k] == want_st[k] for k in ("rays_primary", "rays_shadow", "hits_primary", "hits_shadow", "sdf_evals", "flags"))}
    d_hits.fill_(float("nan"))
    torch.cuda.synchronize()
    ds.render_views_hits_device(EPS, LEN, ft.ImageSize(W, H), cams, d_hits.data_ptr())                 # hits only, no material plane
    ds.collect_stats()
    r["hits_only"] = bool(np.array_equal(d_hits.cpu().numpy().view(np.uint32), want.records.view(np.uint32)))
    try:
        ds.render_views_hits_device(EPS, LEN, ft.ImageSize(W, H), cams, None)                          # nothing asked for
        r["refused"] = False
    except ft.FrayTracerError:
        r["refused"] = True
    res.append(r)
# across the 64-view split: the second launch writes at view 64's offset in each of the three buffers
many = [ft.Camera.lookAt(Position=(9.0 * np.cos(a), 2.0 * np.sin(3 * a), 9.0 * np.sin(a)), LookAt=(0.0, 0.0, 0.0), Up=(0.0, 1.0, 0.0), Lens=lens)
        for a in np.linspace(0.0, 6.2, 70)]
for scene, ext in ((syn.config3(n=64)[0], {}), (syn.console_scene(n=200)[0], dict(spp=4))):
    ds = dev.scene(scene)
    want, want_img, want_st = ds.render_views_hits(EPS, LEN, ft.ImageSize(24, 17), many, shade=True, **ext)
    d_hits = torch.full((70, 24, 17, 16), float("nan"), dtype=torch.float32, device="cuda")
    d_mat = torch.full((70, 24, 17), -7, dtype=torch.int32, device="cuda")
    d_img = torch.full((70, 24, 17, 3), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ds.render_views_hits_device(EPS, LEN, ft.ImageSize(24, 17), many, d_hits.data_ptr(), d_mat.data_ptr(), d_img.data_ptr(), **ext)
    st = ds.collect_stats()
    res.append({"split_records": bool(np.array_equal(d_hits.cpu().numpy().view(np.uint32), want.records.view(np.uint32))),
                "split_material": bool(np.array_equal(d_mat.cpu().numpy(), want.material)),
                "split_image": bool(np.array_equal(d_img.cpu().numpy().view(np.uint32), want_img.view(np.uint32))),
                "split_stats": all(st[k] == want_st[k] for k in ("rays_primary", "rays_shadow", "hits_primary", "hits_shadow", "sdf_evals", "flags"))})
dev.close()
print(json.dumps(res))
"""


def test_device_form_equals_host_form():
    """render_views_hits_device into torch tensors + collect_stats = the host form; in a child process that loads torch before the library"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", DEVICE_FORM], cwd=root, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert len(res) == 5 and all(all(r.values()) for r in res), res
