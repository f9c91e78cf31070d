"""Light visibility masks (ft_light_visibility, ft_shade_visible and their *_device forms): the parts that need no GPU — the ABI, the refusals
(all made before the device is asked for, so a host-only context shows every one), the 32-light limit, the Python layer's checks, the C++ and
F# mirrors."""
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

NAMES = ("ft_light_visibility", "ft_light_visibility_device", "ft_shade_visible", "ft_shade_visible_device")
BG = (0.02, 0.03, 0.05)
LIGHTS = (ft.SdfLight.directional((0.6, -1.0, -0.3), (0.9, 0.8, 0.7)), ft.SdfLight.point((3.0, 4.0, -6.0), (30.0, 40.0, 50.0)),
          ft.SdfLight.directional((0.0, 1.0, 0.2), (0.3, 0.3, 0.3)))
OK, INVALID, NO_DEVICE, UNSUPPORTED = _lib.FT_OK, _lib.FT_ERR_INVALID, _lib.FT_ERR_NO_DEVICE, _lib.FT_ERR_UNSUPPORTED
ALL = 0xFFFFFFFF
REC, VIN, VOUT, RGB = 4096, 8192, 12288, 16384                # device addresses that are never touched: no device exists


def lit(host, n_lights=3):
    lights = [ft.SdfLight.directional((0.1 * i - 1.0, -1.0, 0.3), (1.0, 1.0, 1.0)) for i in range(n_lights)] if n_lights != 3 else LIGHTS
    return host.scene(syn.config3(n=64)[0]).relight(BG, lights)


def test_symbols_are_declared_exported_and_bound():
    assert_declared_exported_bound(NAMES)


def test_abi_version_is_unchanged():
    assert _lib.lib.ft_abi_version() == 5
    assert "#define FT_ABI_VERSION 5" in open(HEADER).read()


def test_header_is_still_plain_c99_and_states_the_contract(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER])
    src = tmp_path / "use.c"
    src.write_text('#include "fraytracer_hip.h"\n'
                   "int f(ft_ctx* c, const ft_scene* s, const ft_object_trace_result* h, void* d, uint32_t* v, float* rgb, ft_stats* st) {\n"
                   "    return ft_light_visibility(c, s, h, 1, 0xFFFFFFFFu, v, v, st) + ft_light_visibility_device(c, s, d, 1, 2u, d, d)\n"
                   "         + ft_shade_visible(c, s, h, v, 1, rgb, st) + ft_shade_visible_device(c, s, d, d, 1, d);\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    text = open(HEADER).read()
    m = re.search(r"/\*(?:(?!\*/).)*?\*/\s*int ft_light_visibility\(", text, flags=re.S)
    assert m, "ft_light_visibility has no comment"
    for phrase in ("SdfScene.fs:23", "SdfScene.fs:15-17", "SdfLight.fs:17-20, 38-41", "select & (2^L - 1)", "vis_in[r] & ~sel & (2^L - 1)", "bits >= L",
                   "may\n * equal vis_out", "rays_primary", "more than 32 lights"):
        assert phrase in m.group(0), phrase
    m = re.search(r"/\*(?:(?!\*/).)*?\*/\s*int ft_shade_visible\(", text, flags=re.S)
    assert m, "ft_shade_visible has no comment"
    for phrase in ("hit == 0", "SdfScene.fs:28", "SdfLight.fs:25, 28, 40", "(a)", "(b)", "(c)", "cosine is <= 0", "every counter\n * is 0", "kernel_ms"):
        assert phrase in m.group(0), phrase


def test_light_visibility_statuses_come_before_the_device(host):
    """a host-only context: whatever is not FT_ERR_NO_DEVICE was decided before any device work"""
    L = _lib.lib
    ctx, sc = host._ctx, lit(host)._scene
    other = ft.Device(-1)
    try:
        foreign = lit(other)._scene
        rec, vis, vin, st = np.zeros((4, 16), np.float32), np.zeros(4, np.uint32), np.zeros(4, np.uint32), _lib.Stats()
        dev = lambda c=ctx, s=sc, h=REC, n=4, sel=ALL, vi=VIN, vo=VOUT: L.ft_light_visibility_device(c, s, _p(h), n, sel, _p(vi), _p(vo))
        hst = lambda c=ctx, s=sc, h=rec, n=4, sel=ALL, vi=vin, vo=vis, stats=st: L.ft_light_visibility(
            c, s, ptr(h), n, sel, ptr(vi), ptr(vo), None if stats is None else C.byref(stats))
        # sound arguments: there is no CPU fallback
        assert dev() == NO_DEVICE and hst() == NO_DEVICE and hst(stats=None) == NO_DEVICE
        assert dev(vi=None) == NO_DEVICE and hst(vi=None) == NO_DEVICE                         # vis_in may be NULL ...
        assert dev(vi=VOUT) == NO_DEVICE and hst(vi=vis) == NO_DEVICE                          # ... and may be vis_out
        assert dev(vi=VIN + 4, vo=VOUT + 4) == NO_DEVICE                                        # masks on 4 bytes
        assert dev(sel=0) == NO_DEVICE and dev(sel=0b010) == NO_DEVICE
        # misaligned (device forms only)
        for h, vi, vo in ((REC + 4, VIN, VOUT), (REC + 8, VIN, VOUT), (REC, VIN + 2, VOUT), (REC, VIN, VOUT + 1), (REC, None, VOUT + 2)):
            assert dev(h=h, vi=vi, vo=vo) == INVALID, (h, vi, vo)
            assert "aligned" in _lib.last_error()
        # NULL, a negative count, a scene of another context, no context
        assert dev(h=None) == INVALID and dev(vo=None) == INVALID and dev(s=None) == INVALID and dev(s=foreign) == INVALID
        assert dev(c=None) == INVALID and dev(n=-1) == INVALID
        assert hst(h=None) == INVALID and hst(vo=None) == INVALID and hst(s=None) == INVALID and hst(s=foreign) == INVALID
        assert hst(c=None) == INVALID and hst(n=-1) == INVALID
        # the records identical to the output
        assert dev(vo=REC) == INVALID and "overlap" in _lib.last_error()
        assert L.ft_light_visibility(ctx, sc, ptr(rec), 4, ALL, None, ptr(rec), C.byref(st)) == INVALID
        # n = 0: nothing to do; the statistics of nothing
        st.rays_shadow = 7
        assert dev(n=0) == OK and hst(n=0) == OK and st.rays_shadow == 0
        # the 32-bit job counter
        for n in (0xFFFF0000, 1 << 32, 1 << 40):
            assert dev(n=n) == UNSUPPORTED and hst(n=n) == UNSUPPORTED, n
        assert dev(n=0xFFFF0000 - 1) == NO_DEVICE
    finally:
        other.close()


def test_shade_visible_statuses_come_before_the_device(host):
    L = _lib.lib
    ctx, sc = host._ctx, lit(host)._scene
    other = ft.Device(-1)
    try:
        foreign = lit(other)._scene
        rec, vis, rgb, st = np.zeros((4, 16), np.float32), np.zeros(4, np.uint32), np.empty((4, 3), np.float32), _lib.Stats()
        dev = lambda c=ctx, s=sc, h=REC, v=VIN, n=4, o=RGB: L.ft_shade_visible_device(c, s, _p(h), _p(v), n, _p(o))
        hst = lambda c=ctx, s=sc, h=rec, v=vis, n=4, o=rgb, stats=st: L.ft_shade_visible(
            c, s, ptr(h), ptr(v), n, ptr(o), None if stats is None else C.byref(stats))
        assert dev() == NO_DEVICE and hst() == NO_DEVICE and hst(stats=None) == NO_DEVICE
        assert dev(v=VIN + 4, o=RGB + 4) == NO_DEVICE                                           # masks and colours on 4 bytes
        for h, v, o in ((REC + 4, VIN, RGB), (REC + 8, VIN, RGB), (REC, VIN + 2, RGB), (REC, VIN, RGB + 1), (REC, VIN + 1, RGB + 2)):
            assert dev(h=h, v=v, o=o) == INVALID, (h, v, o)
            assert "aligned" in _lib.last_error()
        assert dev(h=None) == INVALID and dev(v=None) == INVALID and dev(o=None) == INVALID and dev(s=None) == INVALID
        assert dev(s=foreign) == INVALID and dev(c=None) == INVALID and dev(n=-1) == INVALID
        assert hst(h=None) == INVALID and hst(v=None) == INVALID and hst(o=None) == INVALID and hst(s=None) == INVALID
        assert hst(s=foreign) == INVALID and hst(c=None) == INVALID and hst(n=-1) == INVALID
        # the records identical to the output, the masks identical to the output
        assert dev(o=REC) == INVALID and "overlap" in _lib.last_error()
        assert dev(o=VIN) == INVALID and "overlap" in _lib.last_error()
        assert L.ft_shade_visible(ctx, sc, ptr(rec), ptr(vis), 4, ptr(rec), C.byref(st)) == INVALID
        assert L.ft_shade_visible(ctx, sc, ptr(rec), ptr(vis), 4, ptr(vis), C.byref(st)) == INVALID
        st.rays_shadow = 7
        assert dev(n=0) == OK and hst(n=0) == OK and st.rays_shadow == 0
        for n in (0xFFFF0000, 1 << 32, 1 << 40):
            assert dev(n=n) == UNSUPPORTED and hst(n=n) == UNSUPPORTED, n
        assert dev(n=0xFFFF0000 - 1) == NO_DEVICE
    finally:
        other.close()


def test_a_mask_holds_32_lights(host):
    """33 lights: FT_ERR_UNSUPPORTED from both calls, in both forms; 32 pass every check and reach the device question"""
    L = _lib.lib
    rec, vis, rgb, st = np.zeros((4, 16), np.float32), np.zeros(4, np.uint32), np.empty((4, 3), np.float32), _lib.Stats()
    for n_lights, status in ((32, NO_DEVICE), (33, UNSUPPORTED), (40, UNSUPPORTED)):
        ds = lit(host, n_lights)
        assert ds.info()["n_lights"] == n_lights
        ctx, sc = host._ctx, ds._scene
        assert L.ft_light_visibility_device(ctx, sc, _p(REC), 4, ALL, None, _p(VOUT)) == status, n_lights
        assert L.ft_light_visibility(ctx, sc, ptr(rec), 4, ALL, None, ptr(vis), C.byref(st)) == status, n_lights
        assert L.ft_shade_visible_device(ctx, sc, _p(REC), _p(VIN), 4, _p(RGB)) == status, n_lights
        assert L.ft_shade_visible(ctx, sc, ptr(rec), ptr(vis), 4, ptr(rgb), C.byref(st)) == status, n_lights
        if status == UNSUPPORTED:
            assert "32 lights" in _lib.last_error()
            assert L.ft_light_visibility_device(ctx, sc, _p(REC), 4, 1, None, _p(VOUT)) == UNSUPPORTED    # whatever is selected
            assert L.ft_light_visibility_device(ctx, sc, None, 4, ALL, None, _p(VOUT)) == INVALID         # a bad argument is still a bad argument


class FakeTensor:
    """what api.is_device_tensor looks for, without torch"""

    def __init__(self, shape=(5, 16), dtype="torch.float32", contiguous=True):
        self.shape, self.dtype, self._contiguous, self.is_cuda = shape, dtype, contiguous, True

    def data_ptr(self): return 4096

    def is_contiguous(self): return self._contiguous


def test_python_layer_checks_shape_and_dtype(host):
    ds = lit(host)
    frame = ft.PixelHits(np.zeros((3, 4, 16), np.float32))
    # masks are shaped like the records without their last axis: [X, Y] for a frame of hits
    api.check_visibility(np.zeros((3, 4), np.uint32), (3, 4))
    api.check_visibility(FakeTensor(shape=(3, 4), dtype="torch.int32"), (3, 4))
    empty = ft.PixelHits(np.zeros((0, 4, 16), np.float32))
    vis, st = ds.light_visibility(empty)
    assert vis.shape == (0, 4) and vis.dtype == np.uint32 and st["rays_shadow"] == 0
    rgb, st = ds.shade_visible(empty, vis)
    assert rgb.shape == (0, 4, 3) and rgb.dtype == np.float32 and st["rays_shadow"] == 0
    # sound arguments reach the library, which has no device here
    for call in (lambda: ds.light_visibility(frame), lambda: ds.light_visibility(frame, select=0b010, previous=np.zeros((3, 4), np.uint32)),
                 lambda: ds.shade_visible(frame, np.zeros((3, 4), np.uint32)), lambda: ds.shade_visible(np.zeros((5, 16), np.float32), np.zeros(5, np.uint32))):
        with pytest.raises(ft.FrayTracerError) as e:
            call()
        assert e.value.code == NO_DEVICE
    # the records' checks are shade_hits'
    for bad, why in ((np.zeros((5, 15), np.float32), r"\[\.\.\., 16\]"), (np.zeros((5, 16), np.float64), "float32"), (FakeTensor(contiguous=False), "contiguous")):
        with pytest.raises(ValueError, match=why):
            ds.light_visibility(bad)
        with pytest.raises(ValueError, match=why):
            ds.shade_visible(bad, np.zeros(5, np.uint32))
    # the masks': dtype, shape, where they lie
    for bad, why in ((np.zeros((3, 4), np.int32), "uint32"), (np.zeros((3, 4), np.float32), "uint32"), (np.zeros((3, 4), np.uint64), "uint32"),
                     (np.zeros((4, 3), np.uint32), "shape"), (np.zeros(12, np.uint32), "shape"), (np.zeros((3, 4, 1), np.uint32), "shape"),
                     (FakeTensor(shape=(3, 4), dtype="torch.int32"), "where the records lie")):
        with pytest.raises(ValueError, match=why):
            ds.shade_visible(frame, bad)
        with pytest.raises(ValueError, match=why):
            ds.light_visibility(frame, previous=bad)
    for bad, why in ((FakeTensor(shape=(5,), dtype="torch.uint32"), "int32"), (FakeTensor(shape=(5,), dtype="torch.float32"), "int32"),
                     (FakeTensor(shape=(6,), dtype="torch.int32"), "shape"), (FakeTensor(shape=(5,), dtype="torch.int32", contiguous=False), "contiguous"),
                     (np.zeros(5, np.uint32), "where the records lie")):
        with pytest.raises(ValueError, match=why):
            ds.shade_visible(FakeTensor(), bad)
        with pytest.raises(ValueError, match=why):
            ds.light_visibility(FakeTensor(), previous=bad)
    for name in ("light_visibility", "light_visibility_device", "shade_visible", "shade_visible_device"):
        assert callable(getattr(ft.DeviceScene, name)), name
    assert callable(ft.SdfScene.lightVisibility) and callable(ft.SdfScene.shadeVisible)


def test_cpp_mirror_compiles(tmp_path):
    assert_cpp_compiles(tmp_path, "light_visibility.cpp",
                        "std::vector<uint32_t> f(const FrayTracer::SdfScene& s, const std::vector<ft_object_trace_result>& h, const std::vector<uint32_t>& prev, ft_stats* st) {\n"
                        "    std::vector<uint32_t> all = FrayTracer::Image::lightVisibility(h, s);\n"
                        "    return FrayTracer::Image::lightVisibility(h, s, 2u, &prev, st);\n"
                        "}\n"
                        "std::vector<float> g(const FrayTracer::SdfScene& s, const std::vector<ft_object_trace_result>& h, const std::vector<uint32_t>& v, ft_stats* st) {\n"
                        "    return FrayTracer::Image::shadeVisible(h, v, s, st);\n"
                        "}\n")


def test_fsharp_binding_imports_the_four_functions():
    fs = open(os.path.join(ROOT, "host", "fsharp", "FrayTracer.Hip.fs")).read()
    for name in NAMES:
        assert re.search(r"extern int " + name + r"\(", fs), name
