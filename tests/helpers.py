import contextlib
import ctypes as C
import functools
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


def seg_dist(P, a, b):
    """distance of each point of P from the segment a .. b (the certificate tests' float64 restatement)"""
    ab = b - a
    t = np.clip(((P - a) @ ab) / (ab @ ab), 0.0, 1.0)
    return np.linalg.norm(P - (a + t[:, None] * ab), axis=1)


COUNTERS = ("rays_primary", "rays_shadow", "hits_primary", "hits_shadow", "flags")


def check_counts(gst, ocnt):
    """the five COUNTERS of a launch equal the oracle's, and neither side raised a flag"""
    assert gst["rays_primary"] == ocnt["rays_primary"]
    assert gst["rays_shadow"] == ocnt["rays_shadow"]
    assert gst["hits_primary"] == ocnt["hits_primary"]
    assert gst["hits_shadow"] == ocnt["hits_shadow"]
    assert gst["flags"] == ocnt["flags"] == 0


# ---- the state that tests share: the session's `gpu` device and the oracle's process-wide libm flag.  Each has one writer, here ----


@contextlib.contextmanager
def options(dev, **opts):
    """set per-context options for the block and put back the values found (not the defaults).  Yields set_(**more), which changes further
    options inside the block under the same promise.  Every value is read before any is set: an unknown name raises with nothing changed."""
    old = {}

    def set_(**more):
        for k in more:
            old.setdefault(k, dev.get_option(k))
        for k, v in more.items():
            dev.set_option(k, v)
    try:
        set_(**opts)
        yield set_
    finally:
        for k, v in old.items():
            dev.set_option(k, v)


@contextlib.contextmanager
def oracle_libm(oracle):
    """the oracle on the C runtime's expf / logf / powf.  The flag is global to the process and has no getter: this is its only writer in the
    tests, and 0 is what it leaves behind"""
    oracle.lib.orc_set_libm(1)
    try:
        yield
    finally:
        oracle.lib.orc_set_libm(0)


@contextlib.contextmanager
def glibc_math(gpu, oracle):
    """FT_OPT_MATH = the glibc build this host's libm resolves to, with the oracle switched to the C runtime's expf / logf / powf"""
    import fraytracer_amd as ft
    variant = ft.glibc_build_of_this_host()
    with options(gpu, math=variant), oracle_libm(oracle):
        yield variant


@pytest.fixture
def glibc_mode(gpu, oracle):
    """glibc_math for the whole test.  Import it into the test module that uses it."""
    with glibc_math(gpu, oracle) as variant:
        yield variant


@functools.lru_cache(maxsize=None)
def option_defaults():
    """every option's default, asked of the library itself: a fresh host-only context holds them"""
    import fraytracer_amd as ft
    dev = ft.Device(-1)
    try:
        return {k: dev.get_option(k) for k in ft.Device.OPTIONS}
    finally:
        dev.close()


@pytest.fixture(autouse=True)
def options_left_at_defaults(request):
    """a test that leaves an option changed on the shared `gpu` device fails itself, not the tests after it.  Import it into every module
    that uses the `gpu` fixture."""
    yield
    if "gpu" not in request.fixturenames:
        return
    gpu = request.getfixturevalue("gpu")
    left = {k: gpu.get_option(k) for k, v in option_defaults().items() if gpu.get_option(k) != v}
    for k in left:
        gpu.set_option(k, option_defaults()[k])
    assert not left, f"options left changed on the shared device (now back at their defaults): {left}"


@pytest.fixture(scope="module")
def host():
    """a host-only device (no GPU): flattening, scene info and every check that runs before device work"""
    import fraytracer_amd as ft
    dev = ft.Device(-1)
    yield dev
    dev.close()


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
