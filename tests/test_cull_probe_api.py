"""The internal entry points behind tests/test_gpu_wave_primitives.py and tests/test_gpu_cull_pass.py, as far as they go without a GPU: they are exported
but not declared in the header, refuse a context without a device, and ft_scene_cull_site reports the scene's own children in list order."""
import ctypes as C

import numpy as np

import fraytracer_amd as ft
from fraytracer_amd import _lib
from fraytracer_amd import synthetic as syn
from helpers import HEADER, host, host_ctx  # noqa: F401  (fixtures)

F = np.float32
L = _lib.lib


def test_the_probes_are_internal_and_need_a_device(host_ctx):
    text = open(HEADER).read()
    for name in ("ft_selftest_wave", "ft_selftest_cull", "ft_scene_cull_site"):
        assert name not in text and name not in _lib.SYMBOLS
        getattr(L, name)                                                                   # exported all the same
    wave, cull = L.ft_selftest_wave, L.ft_selftest_cull
    wave.restype, wave.argtypes = C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_float, C.c_int32, C.c_void_p]
    cull.restype, cull.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    x = np.zeros(64, F)
    assert wave(host_ctx, 0, x.ctypes.data_as(C.c_void_p), 1.0, 1, x.ctypes.data_as(C.c_void_p)) == _lib.FT_ERR_NO_DEVICE
    assert cull(host_ctx, None, None, None, 1, None, None) == _lib.FT_ERR_NO_DEVICE
    assert wave(None, 0, None, 1.0, 1, None) == _lib.FT_ERR_INVALID and cull(None, None, None, None, 1, None, None) == _lib.FT_ERR_INVALID


def test_the_cull_site_is_the_scenes_own_run(host):
    site = L.ft_scene_cull_site
    site.restype, site.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    head = np.zeros(3, np.uint32)
    for n, strength in ((31, 0.25), (32, 0.25), (257, 0.1)):
        ds = host.scene(syn.config3(n=n, size=64, strength=strength)[0])
        rec = np.full((n, 4), np.nan, F)
        assert site(ds._scene, head.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p), n) == 0
        if n < 32:
            assert head[0] == 0 and np.isnan(rec).all() and ds.info()["cull_pc"] == -1
            continue
        rng = syn.Rng(3)                                                                   # config3's own draws, in its order
        want = np.array([list(rng.pointInBall(4.0)) + [rng.range(0.1, 0.5)] for _ in range(n)], F)
        assert head[0] == n and head[1] & 1 and head[2:3].view(F)[0] == F(-1.0) / F(strength)
        assert np.array_equal(rec.view(np.uint32), want.view(np.uint32))
        short = np.full((5, 4), np.nan, F)
        assert site(ds._scene, head.ctypes.data_as(C.c_void_p), short.ctypes.data_as(C.c_void_p), 5) == 0 and np.array_equal(short, want[:5])
        assert site(ds._scene, None, None, 0) == _lib.FT_ERR_INVALID and site(None, head.ctypes.data_as(C.c_void_p), None, 0) == _lib.FT_ERR_INVALID
        assert site(ds._scene, head.ctypes.data_as(C.c_void_p), None, 3) == _lib.FT_ERR_INVALID
