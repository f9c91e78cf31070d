"""Hit buffers of batches of camera views (ft_render_views_hits / ft_render_views_hits_device): the parts that need no GPU — the ABI, the
refusals that come before any device work, PixelHits over stacked views, the C++ mirror's renderViewsHits and the F# binding."""
import ctypes as C
import os
import re

import numpy as np

import fraytracer_amd as ft
from fraytracer_amd import _lib
from fraytracer_amd import synthetic as syn
from helpers import HEADER, ROOT, assert_cpp_compiles, assert_declared_exported_bound, dev_ptr, host_ctx, host_ptr, render_params as _params  # noqa: F401  (host_ctx: a fixture)

EPS, LEN = syn.EPSILON, syn.RAY_LENGTH
NAMES = ("ft_render_views_hits", "ft_render_views_hits_device")


def test_symbols_are_declared_exported_and_bound():
    assert_declared_exported_bound(NAMES)


def test_abi_version_is_unchanged():
    assert _lib.lib.ft_abi_version() == 5


def _host(ctx, cams, n, p, rgb=None, hits=None, mat=None):
    st = _lib.Stats()
    return _lib.lib.ft_render_views_hits(ctx, None, cams, n, p, host_ptr(rgb), host_ptr(hits), host_ptr(mat), C.byref(st))


def _device(ctx, cams, n, p, rgb=None, hits=None, mat=None):
    return _lib.lib.ft_render_views_hits_device(ctx, None, cams, n, p, dev_ptr(rgb), dev_ptr(hits), dev_ptr(mat))


def test_host_only_context_has_no_view_hit_buffers(host_ctx):
    cams = (_lib.CameraS * 3)()
    p = C.byref(_params())
    hits = np.empty((3, 8, 8, 16), np.float32)
    mat = np.empty((3, 8, 8), np.int32)
    img = np.empty((3, 8, 8, 3), np.float32)
    assert _host(host_ctx, cams, 3, p, hits=hits) == _lib.FT_ERR_NO_DEVICE
    assert _host(host_ctx, cams, 3, p, img, hits, mat) == _lib.FT_ERR_NO_DEVICE
    assert _host(host_ctx, cams, 3, p, mat=mat) == _lib.FT_ERR_NO_DEVICE
    assert _device(host_ctx, cams, 3, p, hits=256) == _lib.FT_ERR_NO_DEVICE
    assert _device(host_ctx, cams, 3, p, 256, 512, 1024) == _lib.FT_ERR_NO_DEVICE
    assert _device(host_ctx, cams, 1, p, hits=256) == _lib.FT_ERR_NO_DEVICE


def test_bad_batches_are_refused_before_device_work(host_ctx):
    """a host-only context has no device: FT_ERR_INVALID can only come from checks that run before any device call"""
    cams = (_lib.CameraS * 2)()
    p = C.byref(_params())
    hits = np.empty((2, 8, 8, 16), np.float32)
    for n in (0, -1):
        assert _host(host_ctx, cams, n, p, hits=hits) == _lib.FT_ERR_INVALID
        assert _device(host_ctx, cams, n, p, hits=256) == _lib.FT_ERR_INVALID
    assert _host(host_ctx, None, 2, p, hits=hits) == _lib.FT_ERR_INVALID                    # NULL cameras
    assert _device(host_ctx, None, 2, p, hits=256) == _lib.FT_ERR_INVALID
    assert _host(host_ctx, cams, 2, p) == _lib.FT_ERR_INVALID                               # no output at all
    assert _device(host_ctx, cams, 2, p) == _lib.FT_ERR_INVALID
    assert _host(host_ctx, cams, 2, None, hits=hits) == _lib.FT_ERR_INVALID                 # no params
    assert _host(None, cams, 2, p, hits=hits) == _lib.FT_ERR_INVALID                        # no context
    bad = _params()
    bad.spp = 3                                                                             # not a square, even for hits only
    assert _host(host_ctx, cams, 2, C.byref(bad), hits=hits) == _lib.FT_ERR_INVALID
    # the alignment rules of ft_render_hits_device: records 16 bytes, image and material plane 4 bytes
    for rgb, h, m in ((None, 264, None), (None, 260, 512), (258, 256, None), (None, 256, 514), (None, None, 2)):
        assert _device(host_ctx, cams, 2, p, rgb, h, m) == _lib.FT_ERR_INVALID, (rgb, h, m)
    assert _device(host_ctx, cams, 2, p, 260, 272, 516) == _lib.FT_ERR_NO_DEVICE           # aligned: passes the checks


def test_batch_job_limit_is_refused_before_device_work(host_ctx):
    """2^32 jobs over the whole batch.  With the image, spp counts: 4096^2 at spp 64 is 2^30 jobs a view.  Hits only trace one ray
    per pixel, so spp does not count there"""
    many = (_lib.CameraS * 8)()
    big = C.byref(_params(4096, 4096, 64))
    for n, want in ((3, _lib.FT_ERR_NO_DEVICE), (4, _lib.FT_ERR_UNSUPPORTED), (8, _lib.FT_ERR_UNSUPPORTED)):
        assert _device(host_ctx, many, n, big, 256, 512, 1024) == want, n
        assert _device(host_ctx, many, n, big, hits=512) == _lib.FT_ERR_NO_DEVICE, n
    # hits only, many views: 2^32 / 4096^2 = 256 views of 4096^2
    n = (1 << 32) // (4096 * 4096)
    cams = (_lib.CameraS * n)()
    one = C.byref(_params(4096, 4096, 1))
    assert _device(host_ctx, cams, n, one, hits=512) == _lib.FT_ERR_UNSUPPORTED
    assert _device(host_ctx, cams, n, one, mat=512) == _lib.FT_ERR_UNSUPPORTED
    assert _device(host_ctx, cams, n - 1, one, hits=512) == _lib.FT_ERR_NO_DEVICE
    hits = np.empty(16, np.float32)                                                         # never written: refused first
    assert _host(host_ctx, cams, n, one, hits=hits) == _lib.FT_ERR_UNSUPPORTED


def test_header_documents_the_layout():
    text = open(HEADER).read()
    m = re.search(r"/\*(?:(?!\*/).)*?\*/\s*int ft_render_views_hits\(", text, flags=re.S)
    assert m and "view-major" in m.group(0) and "n_views" in m.group(0) and "ft_render_hits" in m.group(0)
    m = re.search(r"/\*(?:(?!\*/).)*?\*/\s*int ft_render_views_hits_device\(", text, flags=re.S)
    assert m and "16-byte aligned" in m.group(0)


def test_python_api_has_the_batch_forms():
    assert callable(ft.Image.renderViewsHits)
    for name in ("render_views_hits", "render_views_hits_device"):
        assert callable(getattr(ft.DeviceScene, name))


def test_pixel_hits_over_stacked_views(oracle):
    """PixelHits of a batch: oracle records of K cameras' pixel rays stacked [K, X, Y, 16]; every property keeps the view axis"""
    scene, _ = syn.config2(boxes=True)
    lens = ft.Lens.create(60.0)
    cams = [syn.default_camera().as_array()] + [ft.Camera.lookAt(Position=p, LookAt=(0.0, 0.0, 0.0), Up=(0.0, 1.0, 0.0), Lens=lens).as_array()
                                                for p in ((7.0, 3.0, -7.0), (0.0, 0.0, -10.0))]
    K, W, H = len(cams), 12, 9
    rays = np.stack([oracle.pixel_ray(c, W, H, x, y, EPS, LEN) for c in cams for x in range(W) for y in range(H)])
    rec, _ = oracle.Oracle().scene(scene).object_try_trace(rays)
    rec = rec.reshape(K, W, H, 16)
    mat = np.where(rec[..., 14].view(np.int32) == 1, 7, -1).astype(np.int32)
    desc = ft.SdfMaterial.createSolid((0.25, 0.5, 0.75))
    h = ft.PixelHits(rec, mat, {7: desc})
    assert h.ray.shape == (K, W, H, 8) and h.normal.shape == h.color.shape == h.position.shape == h.direction.shape == (K, W, H, 3)
    assert h.length.shape == h.hit.shape == (K, W, H) and h.hit.dtype == np.bool_
    assert np.array_equal(h.hit, rec[..., 14].view(np.int32) == 1)
    for k in range(K):                                                                      # view k = the single camera's PixelHits
        one = ft.PixelHits(rec[k], mat[k], {7: desc})
        for prop in ("ray", "position", "direction", "length", "normal", "color", "hit"):
            assert np.array_equal(getattr(h, prop)[k], getattr(one, prop)), (k, prop)
        assert 0 < h.hit[k].sum() < W * H or k == 2, k
    assert np.shares_memory(h.position, rec)
    assert np.array_equal(h.direction[h.hit], rays.reshape(K, W, H, 8)[h.hit][:, 3:6])
    assert not rec[~h.hit].any() and (h.material[~h.hit] == -1).all()
    assert h.descriptor(7) is desc and h.descriptor(-1) is None


def test_cpp_render_views_hits_compiles(tmp_path):
    assert_cpp_compiles(tmp_path, "views_hits.cpp",
                        "std::vector<ft_object_trace_result> f(const FrayTracer::SdfScene& s, const std::vector<ft_camera>& c, std::vector<int32_t>* m,\n"
                        "                                      ft_stats* st) {\n"
                        "    return FrayTracer::Image::renderViewsHits(0.01f, 100.0f, FrayTracer::ImageSize{64, 48}, c, s, m, st);\n"
                        "}\n")


def test_fsharp_binding_has_render_views_hits():
    fs = open(os.path.join(ROOT, "host", "fsharp", "FrayTracer.Hip.fs")).read()
    for name in NAMES:
        assert re.search(r"extern int " + name + r"\(", fs), name
    assert re.search(r"let renderViewsHits .*\(cameras : Camera\[\]\).*: SdfObjectTraceResult voption\[,\]\[\] =", fs)
