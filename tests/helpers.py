import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fraytracer_hip.h")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bit_equal(got, want, what=""):
    got = np.ascontiguousarray(got, dtype=np.float32)
    want = np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    g, w = got.view(np.uint32), want.view(np.uint32)
    # NaNs compare by NaN-ness (payload is not part of the contract), everything else bit for bit
    same = (g == w) | (np.isnan(got) & np.isnan(want))
    if not same.all():
        idx = np.argwhere(~same)
        first = tuple(idx[0])
        raise AssertionError(f"{what}: {len(idx)} of {got.size} values differ; first at {first}: "
                             f"got {got[first]!r} ({g[first]:#010x}) want {want[first]!r} ({w[first]:#010x})")


# ---- shared by the CPU tests of the C ABI's render and ray-buffer forms (tests/test_*_api.py, tests/test_refusal_matrix.py) ----


@pytest.fixture
def host_ctx():
    """a host-only context (ft_ctx_create(-1)): it has no device, so whatever a call returns on it other than FT_ERR_NO_DEVICE comes from a
    check that runs before any device work.  Import it into the test module that uses it."""
    from fraytracer_amd import _lib
    ctx = C.c_void_p()
    _lib.check(_lib.lib.ft_ctx_create(-1, C.byref(ctx)))
    yield ctx
    _lib.lib.ft_ctx_destroy(ctx)


def render_params(w=8, h=8, spp=1):
    """ft_render_params of a whole w x h frame, the reference's sampling unless spp says otherwise"""
    from fraytracer_amd import _lib
    from fraytracer_amd import synthetic as syn
    return _lib.RenderParams(w, h, 0, w, w, 1, 0, spp, syn.EPSILON, syn.RAY_LENGTH, 0, 0.0, 0, 0)


def host_ptr(a):
    """a numpy array (or None) as the void* of a host buffer"""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def dev_ptr(a):
    """an integer (or None) as the void* of a device buffer: refused calls never dereference it"""
    return None if a is None else C.c_void_p(a)


def assert_declared_exported_bound(names):
    """every name is declared in the header (outside comments), exported by the library and bound by fraytracer_amd._lib"""
    from fraytracer_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for name in names:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert re.search(r"\bT " + name + r"\b", out), name
        assert name in _lib.SYMBOLS
        getattr(_lib.lib, name)


def assert_cpp_compiles(tmp_path, name, body):
    """`body` after #include "FrayTracer.hpp" passes the C++17 syntax check"""
    src = tmp_path / name
    src.write_text('#include "FrayTracer.hpp"\n' + body)
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "host", "cpp"), "-I", os.path.join(ROOT, "include"), str(src)])
