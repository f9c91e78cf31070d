"""Relighting without re-tracing (ft_scene_relight, ft_shade_hits, ft_shade_hits_device): the parts that need no GPU — the ABI, a relit
scene against one flattened from scratch on a host-only context, the refusals (all made before the device is asked for), the Python layer's
checks, the C++ and F# mirrors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import _lib, api
from fraytracer_amd import synthetic as syn
from helpers import HEADER, ROOT, assert_cpp_compiles, assert_declared_exported_bound, dev_ptr as _p, host_ptr as ptr, host  # noqa: F401  (host: a fixture)

NAMES = ("ft_scene_relight", "ft_shade_hits", "ft_shade_hits_device")
BG = (0.02, 0.03, 0.05)
LIGHTS = (ft.SdfLight.directional((0.6, -1.0, -0.3), (0.9, 0.8, 0.7)), ft.SdfLight.point((3.0, 4.0, -6.0), (30.0, 40.0, 50.0)),
          ft.SdfLight.directional((0.0, 1.0, 0.2), (0.3, 0.3, 0.3)))
INVALID, NO_DEVICE, UNSUPPORTED = _lib.FT_ERR_INVALID, _lib.FT_ERR_NO_DEVICE, _lib.FT_ERR_UNSUPPORTED


def test_symbols_are_declared_exported_and_bound():
    assert_declared_exported_bound(NAMES)


def test_abi_version_is_unchanged():
    assert _lib.lib.ft_abi_version() == 5
    assert "#define FT_ABI_VERSION 5" in open(HEADER).read()


def test_header_is_still_plain_c99_and_states_the_contract(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER])
    src = tmp_path / "use.c"
    src.write_text('#include "fraytracer_hip.h"\n'
                   "int f(ft_ctx* c, const ft_scene* s, const float* bg, const ft_handle* l, const ft_object_trace_result* h, void* d, float* rgb, ft_stats* st) {\n"
                   "    ft_scene* r = 0;\n"
                   "    return ft_scene_relight(s, bg, l, 3, &r) + ft_shade_hits(c, r, h, 1, rgb, st) + ft_shade_hits_device(c, r, d, 1, d);\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    text = open(HEADER).read()
    m = re.search(r"/\*(?:(?!\*/).)*?\*/\s*int ft_shade_hits\(", text, flags=re.S)
    assert m and "FT_OPT_REUSE = 0" in m.group(0) and "rays_primary" in m.group(0) and "hit == 0" in m.group(0)
    m = re.search(r"/\*(?:(?!\*/).)*?\*/\s*int ft_shade_hits_device\(", text, flags=re.S)
    assert m and "16-byte aligned" in m.group(0) and "must not overlap" in m.group(0) and "scratch" in m.group(0)


def scenes():
    return [("console_like (general)", syn.console_like(n=120)[0]), ("config3 (lean, clustered certificate)", syn.config3(n=64)[0]),
            ("console_scene (carved)", syn.console_scene(n=100)[0]), ("config5 (on-demand calls)", syn.config5()[0])]


def test_a_relit_scene_equals_one_flattened_from_scratch(host):
    for name, scene in scenes():
        src = host.scene(scene)
        relit = src.relight(BG, LIGHTS)
        fresh = host.scene(ft.SdfScene(scene.Object, BG, LIGHTS))
        info = relit.info()
        assert info == fresh.info(), name
        assert info["n_lights"] == 3 and src.info()["n_lights"] == len(scene.Lights), name
        assert {k: v for k, v in info.items() if k != "n_lights"} == {k: v for k, v in src.info().items() if k != "n_lights"}, name
        for g in range(info["n_grids"]):
            a, b = relit.grid(g), fresh.grid(g)
            assert a["counts"] == b["counts"], (name, g)
            for k in ("aabbMin", "cellSizeInv", "cell_start", "centers", "lower", "child"):
                assert np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k],
                                      b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k]), (name, g, k)
        assert relit.support_sphere() == fresh.support_sphere() and relit.miss_certificate() == fresh.miss_certificate(), name
        (ca, ma), (cb, mb) = relit.miss_certificate_clusters(), fresh.miss_certificate_clusters()
        assert np.array_equal(ca, cb) and len(ma) == len(mb) and all(np.array_equal(x, y) for x, y in zip(ma, mb)), name
        # independent of its source, and a source of further relit scenes itself
        src.close()
        again = relit.relight((0.0, 0.0, 0.0), [])
        assert again.info()["n_lights"] == 0 and relit.info() == info, name


def test_relight_refuses_bad_arguments(host):
    L = _lib.lib
    ds = host.scene(scenes()[0][1])
    lights = [api.realise(l, host) for l in LIGHTS]
    bg = (C.c_float * 3)(*BG)
    out = C.c_void_p()

    def call(src, bgp, hs, n, outp):
        arr = None if hs is None else (C.c_int32 * max(len(hs), 1))(*hs)
        return L.ft_scene_relight(src, bgp, arr, n, outp)

    assert call(ds._scene, bg, lights, 3, C.byref(out)) == _lib.FT_OK and out.value
    L.ft_scene_destroy(out)
    assert call(ds._scene, bg, [], 0, C.byref(out)) == _lib.FT_OK                              # no lights at all is a scene
    L.ft_scene_destroy(out)
    assert call(ds._scene, bg, None, 0, C.byref(out)) == _lib.FT_OK                            # NULL with a count of 0, as in ft_scene_create
    L.ft_scene_destroy(out)
    for bad in ([lights[0], 9999, lights[2]], [-1, lights[1], lights[2]], [lights[0], lights[1], len(lights) + 1000]):
        assert call(ds._scene, bg, bad, 3, C.byref(out)) == INVALID and not out.value, bad
        assert "light" in _lib.last_error()
    assert call(None, bg, lights, 3, C.byref(out)) == INVALID
    assert call(ds._scene, None, lights, 3, C.byref(out)) == INVALID
    assert call(ds._scene, bg, None, 3, C.byref(out)) == INVALID
    assert call(ds._scene, bg, lights, -1, C.byref(out)) == INVALID
    assert call(ds._scene, bg, lights, 3, None) == INVALID


def test_shade_hits_statuses_come_before_the_device(host):
    """a host-only context: whatever is not FT_ERR_NO_DEVICE was decided before any device work"""
    L = _lib.lib
    relit = host.scene(scenes()[1][1]).relight(BG, LIGHTS)
    ctx, sc = host._ctx, relit._scene
    other = ft.Device(-1)
    try:
        foreign = other.scene(scenes()[1][1])._scene
        rec, rgb, st = np.zeros((4, 16), np.float32), np.empty((4, 3), np.float32), _lib.Stats()
        # sound arguments: there is no CPU fallback
        assert L.ft_shade_hits_device(ctx, sc, _p(4096), 4, _p(8192)) == NO_DEVICE
        assert L.ft_shade_hits_device(ctx, sc, _p(4096), 4, _p(8196)) == NO_DEVICE            # colours on 4 bytes
        assert L.ft_shade_hits(ctx, sc, ptr(rec), 4, ptr(rgb), C.byref(st)) == NO_DEVICE
        assert L.ft_shade_hits(ctx, sc, ptr(rec), 4, ptr(rgb), None) == NO_DEVICE
        # misaligned
        for hits, out in ((4096 + 4, 8192), (4096 + 8, 8192), (4096, 8192 + 2), (4096, 8192 + 1)):
            assert L.ft_shade_hits_device(ctx, sc, _p(hits), 4, _p(out)) == INVALID, (hits, out)
        assert "aligned" in _lib.last_error()
        # NULL, a negative count, a scene of another context, no context
        assert L.ft_shade_hits_device(ctx, sc, None, 4, _p(8192)) == INVALID
        assert L.ft_shade_hits_device(ctx, sc, _p(4096), 4, None) == INVALID
        assert L.ft_shade_hits_device(ctx, None, _p(4096), 4, _p(8192)) == INVALID
        assert L.ft_shade_hits_device(ctx, foreign, _p(4096), 4, _p(8192)) == INVALID
        assert L.ft_shade_hits_device(None, sc, _p(4096), 4, _p(8192)) == INVALID
        assert L.ft_shade_hits_device(ctx, sc, _p(4096), -1, _p(8192)) == INVALID
        assert L.ft_shade_hits(ctx, sc, None, 4, ptr(rgb), C.byref(st)) == INVALID
        assert L.ft_shade_hits(ctx, sc, ptr(rec), 4, None, C.byref(st)) == INVALID
        assert L.ft_shade_hits(ctx, foreign, ptr(rec), 4, ptr(rgb), C.byref(st)) == INVALID
        assert L.ft_shade_hits(ctx, sc, ptr(rec), -1, ptr(rgb), C.byref(st)) == INVALID
        # identical pointers
        assert L.ft_shade_hits_device(ctx, sc, _p(4096), 4, _p(4096)) == INVALID and "overlap" in _lib.last_error()
        assert L.ft_shade_hits(ctx, sc, ptr(rec), 4, ptr(rec), C.byref(st)) == INVALID
        # n = 0: nothing to do; the statistics of nothing
        st.rays_shadow = 7
        assert L.ft_shade_hits_device(ctx, sc, _p(4096), 0, _p(8192)) == _lib.FT_OK
        assert L.ft_shade_hits(ctx, sc, ptr(rec), 0, ptr(rgb), C.byref(st)) == _lib.FT_OK and st.rays_shadow == 0
        # the 32-bit job counter
        for n in (0xFFFF0000, 1 << 32, 1 << 40):
            assert L.ft_shade_hits_device(ctx, sc, _p(4096), n, _p(8192)) == UNSUPPORTED, n
            assert L.ft_shade_hits(ctx, sc, ptr(rec), n, ptr(rgb), C.byref(st)) == UNSUPPORTED, n
        assert L.ft_shade_hits_device(ctx, sc, _p(4096), 0xFFFF0000 - 1, _p(8192)) == NO_DEVICE
    finally:
        other.close()


class FakeTensor:
    """what api.is_device_tensor looks for, without torch"""

    def __init__(self, shape=(5, 16), dtype="torch.float32", contiguous=True):
        self.shape, self.dtype, self._contiguous, self.is_cuda = shape, dtype, contiguous, True

    def data_ptr(self): return 4096

    def is_contiguous(self): return self._contiguous


def test_python_layer_checks_shape_and_dtype(host):
    relit = host.scene(scenes()[0][1]).relight(BG, LIGHTS)
    assert api.check_hit_records(np.zeros((3, 4, 16), np.float32)) == (3, 4)
    assert api.check_hit_records(FakeTensor(shape=(7, 16))) == (7,)
    for bad, why in ((np.zeros((5, 15), np.float32), r"\[\.\.\., 16\]"), (np.zeros((5, 16), np.float64), "float32"), (np.zeros((), np.float32), r"\[\.\.\., 16\]"),
                     (np.zeros((5, 16), np.int32), "float32"), (FakeTensor(shape=(5, 8)), r"\[\.\.\., 16\]"), (FakeTensor(dtype="torch.float16"), "float32"),
                     (FakeTensor(contiguous=False), "contiguous"), (ft.PixelHits(np.zeros((2, 2, 12), np.float32)), r"\[\.\.\., 16\]")):
        with pytest.raises(ValueError, match=why):
            relit.shade_hits(bad)
    # sound records reach the library, which has no device here; an empty buffer is answered without it
    with pytest.raises(ft.FrayTracerError) as e:
        relit.shade_hits(np.zeros((2, 3, 16), np.float32))
    assert e.value.code == NO_DEVICE
    out, st = relit.shade_hits(np.zeros((0, 16), np.float32))
    assert out.shape == (0, 3) and st["rays_shadow"] == 0
    for name in ("relight", "shade_hits", "shade_hits_device"):
        assert callable(getattr(ft.DeviceScene, name)), name
    assert callable(ft.SdfScene.shade)


def test_cpp_mirror_compiles(tmp_path):
    assert_cpp_compiles(tmp_path, "shade_hits.cpp",
                        "std::vector<float> f(const FrayTracer::SdfScene& s, const std::vector<ft_object_trace_result>& h, ft_stats* st) {\n"
                        "    return FrayTracer::Image::shadeHits(h, s, st);\n"
                        "}\n"
                        "std::vector<std::vector<float>> g(const FrayTracer::SdfScene& s, const std::vector<ft_object_trace_result>& h, const std::vector<FrayTracer::SdfScene>& lit) {\n"
                        "    return FrayTracer::Image::shadeHitsRelit(h, s, lit);\n"
                        "}\n")


def test_fsharp_binding_imports_the_three_functions():
    fs = open(os.path.join(ROOT, "host", "fsharp", "FrayTracer.Hip.fs")).read()
    for name in NAMES:
        assert re.search(r"extern int " + name + r"\(", fs), name
