"""Batches of camera views (ft_render_views / ft_render_views_device): the parts that need no GPU — the ABI, the refusals that come before
any device work, the Python argument checks and the C++ mirror's renderViews."""
import ctypes as C
import os
import re

import numpy as np

import fraytracer_amd as ft
from fraytracer_amd import _lib
from fraytracer_amd import synthetic as syn
from helpers import HEADER, ROOT, assert_cpp_compiles, assert_declared_exported_bound, dev_ptr, host_ctx, host_ptr, render_params as _params  # noqa: F401  (host_ctx: a fixture)

EPS, LEN = syn.EPSILON, syn.RAY_LENGTH


def test_symbols_are_declared_exported_and_bound():
    assert_declared_exported_bound(("ft_render_views", "ft_render_views_device"))


def test_abi_version_is_unchanged():
    assert _lib.lib.ft_abi_version() == 5


def test_host_only_context_renders_no_views(host_ctx):
    cams = (_lib.CameraS * 3)()
    p = _params()
    out = np.empty((3, 8, 8, 3), np.float32)
    st = _lib.Stats()
    rc = _lib.lib.ft_render_views(host_ctx, None, cams, 3, C.byref(p), host_ptr(out), C.byref(st))
    assert rc == _lib.FT_ERR_NO_DEVICE
    rc = _lib.lib.ft_render_views_device(host_ctx, None, cams, 3, C.byref(p), dev_ptr(256))
    assert rc == _lib.FT_ERR_NO_DEVICE


def test_bad_batches_are_refused_before_device_work(host_ctx):
    """a host-only context has no device: these codes can only come from checks that run before any device call"""
    cams = (_lib.CameraS * 2)()
    p = _params()
    out = np.empty((2, 8, 8, 3), np.float32)
    o = host_ptr(out)
    st = _lib.Stats()
    for n in (0, -1):
        assert _lib.lib.ft_render_views(host_ctx, None, cams, n, C.byref(p), o, C.byref(st)) == _lib.FT_ERR_INVALID
        assert _lib.lib.ft_render_views_device(host_ctx, None, cams, n, C.byref(p), dev_ptr(256)) == _lib.FT_ERR_INVALID
    assert _lib.lib.ft_render_views(host_ctx, None, None, 2, C.byref(p), o, C.byref(st)) == _lib.FT_ERR_INVALID
    assert _lib.lib.ft_render_views_device(host_ctx, None, None, 2, C.byref(p), dev_ptr(256)) == _lib.FT_ERR_INVALID
    assert _lib.lib.ft_render_views(host_ctx, None, cams, 2, None, o, C.byref(st)) == _lib.FT_ERR_INVALID
    assert _lib.lib.ft_render_views(host_ctx, None, cams, 2, C.byref(p), None, C.byref(st)) == _lib.FT_ERR_INVALID
    assert _lib.lib.ft_render_views_device(host_ctx, None, cams, 2, C.byref(p), None) == _lib.FT_ERR_INVALID
    assert _lib.lib.ft_render_views(None, None, cams, 2, C.byref(p), o, C.byref(st)) == _lib.FT_ERR_INVALID
    bad = _params()
    bad.spp = 3                                                # not a square
    assert _lib.lib.ft_render_views(host_ctx, None, cams, 2, C.byref(bad), o, C.byref(st)) == _lib.FT_ERR_INVALID


def test_batch_job_limit_is_refused_before_device_work(host_ctx):
    """2^32 jobs over the whole batch: 4096^2 at spp 64 is 2^30 jobs a view, legal alone, refused from four views on"""
    many = (_lib.CameraS * 8)()
    big = _params(4096, 4096, 64)
    for n, want in ((3, _lib.FT_ERR_NO_DEVICE), (4, _lib.FT_ERR_UNSUPPORTED), (8, _lib.FT_ERR_UNSUPPORTED)):
        assert _lib.lib.ft_render_views_device(host_ctx, None, many, n, C.byref(big), dev_ptr(256)) == want, n
    # smaller frames, many views: 2^32 / (64^2 x 64) views of 64 x 64 at spp 64
    small = _params(64, 64, 64)
    n = (1 << 32) // (64 * 64 * 64)
    cams = (_lib.CameraS * n)()
    assert _lib.lib.ft_render_views_device(host_ctx, None, cams, n, C.byref(small), dev_ptr(256)) == _lib.FT_ERR_UNSUPPORTED
    assert _lib.lib.ft_render_views_device(host_ctx, None, cams, n - 1, C.byref(small), dev_ptr(256)) == _lib.FT_ERR_NO_DEVICE


def test_header_documents_the_layout():
    text = open(HEADER).read()
    m = re.search(r"/\*(?:(?!\*/).)*?\*/\s*int ft_render_views\(", text, flags=re.S)
    assert m and "view-major" in m.group(0) and "n_views" in m.group(0)


def test_python_api_has_the_batch_forms():
    assert callable(ft.Image.renderViews)
    for name in ("render_views", "render_views_device"):
        assert callable(getattr(ft.DeviceScene, name))


def test_cpp_render_views_compiles(tmp_path):
    assert_cpp_compiles(tmp_path, "views.cpp",
                        "std::vector<float> f(const FrayTracer::SdfScene& s, const std::vector<ft_camera>& c, ft_stats* st) {\n"
                        "    return FrayTracer::Image::renderViews(0.01f, 100.0f, FrayTracer::ImageSize{64, 48}, c, s, st);\n"
                        "}\n")


def test_fsharp_binding_has_render_views():
    fs = open(os.path.join(ROOT, "host", "fsharp", "FrayTracer.Hip.fs")).read()
    assert re.search(r"extern int ft_render_views\(", fs) and re.search(r"extern int ft_render_views_device\(", fs)
    assert re.search(r"let renderViews .*\(cameras : Camera\[\]\).*: FColor\[,\]\[\] =", fs)
