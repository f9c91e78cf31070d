"""Tile order (FT_OPT_ORDER; kernels.hip "Tile order", capi.cpp launchTrace): a frame records what each 8x8 tile cost in evaluation rounds, and the
scene's next frame of the same grid hands out first the tiles that cost at least the mean, most expensive first, the others in index order.

Only the moment a tile starts may depend on it.  GPU: frames, counters and flags of reordered launches against index-order launches and the oracle,
bit for bit, every destination filled with NaN before each launch (a tile left out shows); the order read back against the rule restated here;
slots that must not be used for another grid; two scenes on one context; the option's three values.  CPU: the option itself."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import _lib
from fraytracer_amd import synthetic as syn
from helpers import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS, LEN = 0.01, 30.0
COUNTERS = ("rays_primary", "rays_shadow", "hits_primary", "sdf_evals", "flags")
ORACLE_COUNTERS = ("rays_primary", "rays_shadow", "hits_primary", "flags")     # the oracle has no shortcuts: its sdf_evals are another number
W, H = 200, 136                                                                 # 25 x 17 tiles, partial ones on both edges


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------

def test_option_values_and_its_number_in_every_layer():
    host = ft.Device(-1)
    try:
        assert host.get_option("order") == 1
        for v in (0, 2, 1):
            host.set_option("order", v)
            assert host.get_option("order") == v
        with pytest.raises(ft.FrayTracerError) as e:
            host.set_option("order", 3)
        assert e.value.code == _lib.FT_ERR_INVALID and host.get_option("order") == 1
        with pytest.raises(ft.FrayTracerError):
            host.set_option("order", -1)
    finally:
        host.close()
    header = open(os.path.join(ROOT, "include", "fraytracer_hip.h")).read()
    assert re.search(r"\bFT_OPT_ORDER\s*=\s*16\b", header)
    assert _lib.FT_OPT_ORDER == 16 and ft.Device.SCHEDULE_OPTIONS["order"] == 16
    assert "FT_OPT_ORDER" in open(os.path.join(ROOT, "host", "cpp", "FrayTracer.hpp")).read()      # the C++ layer takes the header's enumerator
    fs = open(os.path.join(ROOT, "host", "fsharp", "FrayTracer.Hip.fs")).read()
    assert re.search(r"let setTileOrder \(mode : int\) = if ft_ctx_set_option \(ctx\.Value, 16, mode\)", fs)
    assert "ft_ctx_set_option (ctx.Value, 16, mode)" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------

class DeviceFrames:
    """device buffers of the runtime the library is linked against (already loaded: the same instance), filled with NaN before every launch"""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so.7")
        self.ptr, self.bytes = C.c_void_p(), 0

    def render(self, gpu, ds, size, cam, eps=EPS, **tiling):
        """one ft_render_device launch into a NaN-filled buffer -> (float32 [n_columns, Y, 3], the launch's stats)"""
        p = ds._params(size, eps, LEN, **tiling)
        shape = (p.n_columns, p.height, 3)
        need = int(np.prod(shape)) * 4
        if need > self.bytes:
            if self.ptr:
                assert self.hip.hipFree(self.ptr) == 0
            assert self.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(need)) == 0
            self.bytes = need
        assert self.hip.hipMemset(self.ptr, 0xFF, C.c_size_t(need)) == 0            # 0xFFFFFFFF: a NaN
        assert self.hip.hipDeviceSynchronize() == 0
        ds.render_device(eps, LEN, size, cam, self.ptr.value, **tiling)
        st = ds.collect_stats()                                                      # waits for the context's stream
        out = np.empty(shape, np.float32)
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.ptr, C.c_size_t(need), 2) == 0     # hipMemcpyDeviceToHost
        return out, st

    def close(self):
        if self.ptr:
            self.hip.hipFree(self.ptr)


@pytest.fixture(scope="module")
def frames():
    f = DeviceFrames()
    yield f
    f.close()


@pytest.fixture(autouse=True)
def defaults_again(request):
    yield
    if "gpu" in request.fixturenames:
        g = request.getfixturevalue("gpu")
        for k, v in (("order", 1), ("guided", 0), ("math", 0)):
            g.set_option(k, v)


def read_slot(ds, which):
    """ft_scene_tile_costs / ft_scene_tile_order (internal): the scene's lane-0 slot -> uint32 array, None where the slot holds none"""
    fn = getattr(_lib.lib, "ft_scene_tile_" + which)
    fn.restype, fn.argtypes = C.c_longlong, [C.c_void_p, C.c_void_p, C.c_longlong]
    n = fn(ds._scene, None, 0)
    assert n >= 0, _lib.last_error()
    if n == 0:
        return None
    out = np.empty(n, np.uint32)
    assert fn(ds._scene, out.ctypes.data_as(C.c_void_p), n) == n
    return out


def used_order(ds):
    """ft_scene_tile_order_used (internal): did the scene's last recording launch on lane 0 hand its tiles out in a built order?"""
    fn = _lib.lib.ft_scene_tile_order_used
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p]
    return bool(fn(ds._scene))


def c3():
    return syn.config3(n=256, size=W)[0]


@pytest.fixture(scope="module")
def c3_oracle(oracle):
    """the oracle's whole C3 frame at W x H, computed once: (pixels [W, H, 3], counters)"""
    want, cnt = oracle.Oracle().scene(c3()).render(EPS, LEN, W, H, syn.default_camera().as_array(), nthreads=16)
    want.setflags(write=False)
    return want, cnt


def launches(gpu, frames, ds, size, cam, want, what, reorders=True, **tiling):
    """three launches with option 1 (index order, then twice reordered — the launch itself says whether it was), one with option 0: all four frames
    equal `want` bit for bit and their counters are equal per launch -> the four stats"""
    sts = []
    for i, order in enumerate((1, 1, 1, 0)):
        gpu.set_option("order", order)
        got, st = frames.render(gpu, ds, size, cam, **tiling)
        assert_bit_equal(got, want, f"{what}, launch {len(sts)} (order {order})")
        assert used_order(ds) == (reorders and i in (1, 2)), (what, i)
        sts.append(st)
    for i, st in enumerate(sts):
        print(what, i, {k: st[k] for k in COUNTERS})
    for k in COUNTERS:
        assert len({st[k] for st in sts}) == 1, (what, k, [st[k] for st in sts])
    return sts


@pytest.mark.gpu
def test_frame_and_counters_do_not_depend_on_the_order(gpu, frames, c3_oracle):
    want, cnt = c3_oracle
    ds = gpu.scene(c3())
    try:
        sts = launches(gpu, frames, ds, ft.ImageSize(W, H), syn.default_camera(), want, "C3 200x136")
        for k in ORACLE_COUNTERS:
            assert sts[0][k] == cnt[k], (k, sts[0][k], cnt[k])
    finally:
        ds.close()


@pytest.mark.gpu
def test_striped_share(gpu, frames, c3_oracle):
    """rank 1 of 3, stripes of 16 columns, 52 columns (no multiple of 8: a partial tile column): the share's pixels are the whole frame's"""
    want, _ = c3_oracle
    n, sw, ranks, rank = 52, 16, 3, 1
    xs = [(cl // sw) * sw * ranks + rank * sw + cl % sw for cl in range(n)]
    ds = gpu.scene(c3())
    try:
        sts = launches(gpu, frames, ds, ft.ImageSize(W, H), syn.default_camera(), want[xs], "C3 striped share",
                       n_columns=n, stripe_width=sw, stripe_ranks=ranks, stripe_rank=rank)
        assert sts[0]["rays_primary"] == n * H
    finally:
        ds.close()


@pytest.mark.gpu
def test_glibc_arithmetic(gpu, frames, oracle):
    build = ft.glibc_build_of_this_host()
    gpu.set_option("math", build)
    oracle.lib.orc_set_libm(1)
    try:
        want, _ = oracle.Oracle().scene(c3()).render(EPS, LEN, W, H, syn.default_camera().as_array(), nthreads=16)
        ds = gpu.scene(c3())
        try:
            launches(gpu, frames, ds, ft.ImageSize(W, H), syn.default_camera(), want, "C3 glibc")
        finally:
            ds.close()
    finally:
        oracle.lib.orc_set_libm(0)
        gpu.set_option("math", 0)


@pytest.mark.gpu
def test_carved_kernel(gpu, frames, oracle):
    """The carved kernels keep no tile bookkeeping: this only checks that option 1 leaves such a scene's launches, frames and slot alone."""
    scene = syn.console_scene(size=120)[0]
    cam = syn.default_camera()
    want, _ = oracle.Oracle().scene(scene).render(EPS, LEN, 120, 120, cam.as_array(), nthreads=16)
    ds = gpu.scene(scene)
    try:
        assert ds.info()["fast_path"] == 3
        launches(gpu, frames, ds, ft.ImageSize(120, 120), cam, want, "console scene 120^2", reorders=False)
        assert read_slot(ds, "costs") is None and read_slot(ds, "order") is None
    finally:
        ds.close()


def rule(cost):
    """the order the rule asks for, up to ties: (heavy tiles sorted by clamped cost descending then index, light tiles ascending)"""
    heavy = np.flatnonzero(cost.astype(np.uint64) * len(cost) >= cost.astype(np.uint64).sum())      # cost >= mean, exactly
    light = np.setdiff1d(np.arange(len(cost)), heavy)
    return heavy, light


@pytest.mark.gpu
def test_order_is_what_the_rule_says(gpu, frames, c3_oracle):
    want, _ = c3_oracle
    size, cam = ft.ImageSize(W, H), syn.default_camera()
    nTiles = ((W + 7) // 8) * ((H + 7) // 8)
    ds = gpu.scene(c3())
    try:
        for i in range(2):
            got, _ = frames.render(gpu, ds, size, cam)
            assert_bit_equal(got, want, "C3")
            assert used_order(ds) == (i == 1)
        cost, order = read_slot(ds, "costs"), read_slot(ds, "order")
        assert cost is not None and order is not None and len(cost) == len(order) == nTiles
        assert np.array_equal(np.sort(order), np.arange(nTiles))                    # a permutation of all tiles
        heavy, light = rule(cost)
        print("tiles", nTiles, "mean cost", cost.mean(), "max", cost.max(), "heavy", len(heavy))
        assert 0 < len(heavy) < nTiles
        head, tail = order[:len(heavy)], order[len(heavy):]
        assert np.array_equal(np.sort(head), heavy)                                 # exactly the tiles at or above the mean,
        clamped = np.minimum(cost[head], 255).astype(np.int64)
        assert (np.diff(clamped) <= 0).all()                                        # in non-increasing clamped cost;
        assert np.array_equal(tail, light)                                          # then the others in ascending index
        got, _ = frames.render(gpu, ds, size, cam)
        assert_bit_equal(got, want, "C3, third launch")
        assert used_order(ds)
        again = read_slot(ds, "costs")
        print("tiles whose cost moved between the second and the third launch:", int((again != cost).sum()))
        assert np.array_equal(again, cost)                                          # rounds are counts: the same tile costs the same
    finally:
        ds.close()


@pytest.mark.gpu
def test_a_slot_is_never_used_for_another_grid(gpu, frames):
    """160x160, 96x200, a column range of 160x160 (each changes the key: index order), then 160x160 from a moved camera (same key: the launch runs on
    an order built for another view).  Each frame is its option-0 frame."""
    moved = ft.Camera.lookAt(Position=(0.5, 0.0, -10.0), LookAt=(0.0, 0.0, 0.0), Up=(0.0, 1.0, 0.0), Lens=ft.Lens.create(60.0))
    cam = syn.default_camera()
    seq = [(ft.ImageSize(160, 160), cam, {}), (ft.ImageSize(96, 200), cam, {}), (ft.ImageSize(160, 160), cam, {"x0": 8, "n_columns": 64}),
           (ft.ImageSize(160, 160), cam, {}), (ft.ImageSize(160, 160), moved, {})]
    ds = gpu.scene(syn.config3(n=256, size=160)[0])
    try:
        gpu.set_option("order", 0)
        plain = [frames.render(gpu, ds, size, c, **t) for size, c, t in seq]
        assert read_slot(ds, "costs") is None
        gpu.set_option("order", 1)
        for i, (size, c, t) in enumerate(seq):
            got, st = frames.render(gpu, ds, size, c, **t)
            assert_bit_equal(got, plain[i][0], f"launch {i}")
            for k in COUNTERS:
                assert st[k] == plain[i][1][k], (i, k, st[k], plain[i][1][k])
            tiles = ((t.get("n_columns", size.X) + 7) // 8) * ((size.Y + 7) // 8)
            assert len(read_slot(ds, "order")) == tiles                             # the slot follows the launch's grid
            assert used_order(ds) == (i == 4), i                                    # only the moved camera finds its key in the slot
    finally:
        ds.close()


@pytest.mark.gpu
def test_two_scenes_on_one_context(gpu, frames):
    scenes = [syn.config3(n=256, size=96)[0], syn.config3(seed=5, n=64, size=96)[0]]
    size, cam = ft.ImageSize(96, 104), syn.default_camera()
    dss = [gpu.scene(s) for s in scenes]
    try:
        gpu.set_option("order", 0)
        plain = [frames.render(gpu, ds, size, cam) for ds in dss]
        gpu.set_option("order", 1)
        for rep in range(3):
            for i, ds in enumerate(dss):
                got, st = frames.render(gpu, ds, size, cam)
                assert_bit_equal(got, plain[i][0], f"scene {i}, launch {rep}")
                assert used_order(ds) == (rep > 0), (i, rep)
                for k in COUNTERS:
                    assert st[k] == plain[i][1][k], (i, rep, k)
    finally:
        for ds in dss:
            ds.close()


@pytest.mark.gpu
def test_options_0_and_2_and_the_guided_hand_out_keep_index_order(gpu, frames, c3_oracle):
    want, _ = c3_oracle
    size, cam = ft.ImageSize(W, H), syn.default_camera()
    nTiles = ((W + 7) // 8) * ((H + 7) // 8)
    ds = gpu.scene(c3())
    try:
        gpu.set_option("order", 0)
        for _ in range(2):
            plain, st0 = frames.render(gpu, ds, size, cam)
            assert_bit_equal(plain, want, "option 0")
            assert read_slot(ds, "costs") is None and read_slot(ds, "order") is None
        gpu.set_option("order", 2)
        for _ in range(2):
            got, _ = frames.render(gpu, ds, size, cam)
            assert_bit_equal(got, want, "option 2")
            assert len(read_slot(ds, "costs")) == nTiles and read_slot(ds, "order") is None and not used_order(ds)
        gpu.set_option("order", 0)
        frames.render(gpu, ds, size, cam)
        assert read_slot(ds, "costs") is None                                       # option 0 forgets what was recorded
        gpu.set_option("order", 1)
        gpu.set_option("guided", 1)
        for _ in range(3):
            got, st = frames.render(gpu, ds, size, cam)
            assert_bit_equal(got, plain, "guided hand-out with option 1")
            assert read_slot(ds, "order") is None and not used_order(ds)            # never combined: index order, nothing recorded
            for k in ("rays_primary", "rays_shadow", "hits_primary", "flags"):
                assert st[k] == st0[k], k
    finally:
        ds.close()
