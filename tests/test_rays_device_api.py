"""Ray buffers in device memory, with hit records and materials in one pass (ft_trace_rays_device, ft_form_try_trace_device,
ft_object_try_trace_device, ft_trace_rays_hits, ft_trace_rays_hits_device): the parts that need no GPU — the ABI, the refusals that come
before any device work, the duck-typed device-tensor check, PixelHits over the records of a ray buffer, the C++ and F# mirrors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import _lib, api
from fraytracer_amd import synthetic as syn
from helpers import HEADER, ROOT, assert_cpp_compiles, assert_declared_exported_bound, dev_ptr as _p, host_ctx, host_ptr as ptr  # noqa: F401  (host_ctx: a fixture)

EPS, LEN = syn.EPSILON, syn.RAY_LENGTH
NAMES = ("ft_trace_rays_device", "ft_form_try_trace_device", "ft_object_try_trace_device", "ft_trace_rays_hits", "ft_trace_rays_hits_device")


def test_symbols_are_declared_exported_and_bound():
    assert_declared_exported_bound(NAMES)


def test_abi_version_is_unchanged():
    assert _lib.lib.ft_abi_version() == 5


def test_header_is_still_plain_c99(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER])
    src = tmp_path / "use.c"
    src.write_text('#include "fraytracer_hip.h"\n'
                   "int f(ft_ctx* c, const ft_scene* s, const ft_ray* r, void* d, float* rgb, ft_object_trace_result* h, int32_t* m, ft_stats* st) {\n"
                   "    return ft_trace_rays_device(c, s, d, 1, d) + ft_form_try_trace_device(c, s, d, 1, d) + ft_object_try_trace_device(c, s, d, 1, d, d)\n"
                   "         + ft_trace_rays_hits(c, s, r, 1, rgb, h, m, st) + ft_trace_rays_hits_device(c, s, d, 1, d, d, d);\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_header_states_the_contract():
    text = open(HEADER).read()
    m = re.search(r"/\*(?:(?!\*/).)*?\*/\s*int ft_trace_rays_device\(", text, flags=re.S)
    assert m and "16-byte aligned" in m.group(0) and "must not overlap" in m.group(0) and "scratch" in m.group(0)
    m = re.search(r"/\*(?:(?!\*/).)*?\*/\s*int ft_trace_rays_hits\(", text, flags=re.S)
    assert m and "ft_object_try_trace" in m.group(0) and "-1 on a miss" in m.group(0)


def test_host_only_context_traces_no_ray_buffer(host_ctx):
    L = _lib.lib
    assert L.ft_trace_rays_device(host_ctx, None, _p(256), 4, _p(1024)) == _lib.FT_ERR_NO_DEVICE
    assert L.ft_form_try_trace_device(host_ctx, None, _p(256), 4, _p(1024)) == _lib.FT_ERR_NO_DEVICE
    assert L.ft_object_try_trace_device(host_ctx, None, _p(256), 4, _p(1024), None) == _lib.FT_ERR_NO_DEVICE
    assert L.ft_object_try_trace_device(host_ctx, None, _p(256), 4, _p(1024), _p(2048)) == _lib.FT_ERR_NO_DEVICE
    assert L.ft_trace_rays_hits_device(host_ctx, None, _p(256), 4, _p(1024), _p(2048), _p(4096)) == _lib.FT_ERR_NO_DEVICE
    assert L.ft_trace_rays_hits_device(host_ctx, None, _p(256), 4, None, _p(2048), None) == _lib.FT_ERR_NO_DEVICE
    rays = np.zeros((4, 8), np.float32)
    rgb, rec, mat = np.empty((4, 3), np.float32), np.empty((4, 16), np.float32), np.empty(4, np.int32)
    st = _lib.Stats()
    assert L.ft_trace_rays_hits(host_ctx, None, ptr(rays), 4, ptr(rgb), ptr(rec), ptr(mat), C.byref(st)) == _lib.FT_ERR_NO_DEVICE
    assert L.ft_trace_rays_hits(host_ctx, None, ptr(rays), 4, None, ptr(rec), None, C.byref(st)) == _lib.FT_ERR_NO_DEVICE
    for fn in (L.ft_trace_rays_device, L.ft_form_try_trace_device):
        assert fn(None, None, _p(256), 4, _p(1024)) == _lib.FT_ERR_INVALID                  # no context at all


class FakeTensor:
    """what api.is_device_tensor looks for, without torch"""

    def __init__(self, shape=(5, 8), dtype="torch.float32", contiguous=True, is_cuda=True):
        self.shape, self.dtype, self._contiguous, self.is_cuda = shape, dtype, contiguous, is_cuda

    def data_ptr(self): return 4096

    def is_contiguous(self): return self._contiguous


def test_device_tensor_check_is_duck_typed_and_strict():
    assert api.is_device_tensor(FakeTensor())
    assert not api.is_device_tensor(FakeTensor(is_cuda=False))                              # a CPU tensor is host data
    assert not api.is_device_tensor(np.zeros((5, 8), np.float32)) and not api.is_device_tensor([[0.0] * 8])
    assert api.check_device_rays(FakeTensor()) == 5
    assert api.check_device_rays(FakeTensor(shape=(0, 8))) == 0
    with pytest.raises(ValueError, match="float32"):
        api.check_device_rays(FakeTensor(dtype="torch.float64"))
    with pytest.raises(ValueError, match=r"\[n, 8\]"):
        api.check_device_rays(FakeTensor(shape=(5, 7)))
    with pytest.raises(ValueError, match=r"\[n, 8\]"):
        api.check_device_rays(FakeTensor(shape=(40,)))
    with pytest.raises(ValueError, match="contiguous"):
        api.check_device_rays(FakeTensor(contiguous=False))


def test_python_api_has_the_ray_buffer_forms():
    for name in ("trace_rays_device", "form_try_trace_device", "object_try_trace_device", "trace_rays_hits", "trace_rays_hits_device"):
        assert callable(getattr(ft.DeviceScene, name)), name
    assert callable(ft.Device.on_current_stream)


def test_pixel_hits_over_a_ray_buffer(oracle):
    """PixelHits over [n, 16] records, as trace_rays_hits returns them: the accessors index the last axis only"""
    scene, _ = syn.config2(boxes=True)
    cam = syn.default_camera().as_array()
    W, H = 12, 9
    rays = np.stack([oracle.pixel_ray(cam, W, H, x, y, EPS, LEN) for x in range(W) for y in range(H)])
    rec, _ = oracle.Oracle().scene(scene).object_try_trace(rays)
    assert rec.shape == (W * H, 16)
    flag = rec[:, 14].view(np.int32)
    mat = np.where(flag == 1, 3, -1).astype(np.int32)
    h = ft.PixelHits(rec, mat, {})
    assert np.array_equal(h.position, rec[:, 0:3]) and np.array_equal(h.direction, rec[:, 3:6]) and np.array_equal(h.ray, rec[:, 0:8])
    assert np.array_equal(h.normal, rec[:, 8:11]) and np.array_equal(h.color, rec[:, 11:14]) and np.array_equal(h.length, rec[:, 6])
    assert h.hit.shape == (W * H,) and h.hit.dtype == np.bool_ and np.array_equal(h.hit, flag != 0)
    assert 0 < h.hit.sum() < W * H
    assert not rec[~h.hit].any() and (h.material[~h.hit] == -1).all()


def test_cpp_trace_rays_hits_compiles(tmp_path):
    assert_cpp_compiles(tmp_path, "rays_hits.cpp",
                        "std::vector<ft_object_trace_result> f(const FrayTracer::SdfScene& s, const std::vector<ft_ray>& r, std::vector<float>* c,\n"
                        "                                      std::vector<int32_t>* m, ft_stats* st) {\n"
                        "    return FrayTracer::Image::traceRaysHits(r, s, c, m, st);\n"
                        "}\n")


def test_fsharp_binding_imports_the_ray_buffer_forms():
    fs = open(os.path.join(ROOT, "host", "fsharp", "FrayTracer.Hip.fs")).read()
    for name in NAMES:
        assert re.search(r"extern int " + name + r"\(", fs), name
