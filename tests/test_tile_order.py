"""Tile order (FT_OPT_ORDER; kernels.hip "Tile order", capi.cpp launchTrace): a frame records what each 8x8 tile cost in evaluation rounds, and the
scene's next frame of the same grid hands out first the tiles that cost at least the mean, most expensive first, the others in index order.

Only the moment a tile starts may depend on it.  GPU: frames, counters and flags of reordered launches against index-order launches and the oracle,
bit for bit, every destination filled with NaN before each launch (a tile left out shows); the order read back against the rule restated here;
slots that must not be used for another grid; two scenes on one context; the option's three values; the three order kernels on their own, on costs made
here, at every size where their index arithmetic changes; frames whose order takes two workgroups, under four rules; the recorded costs against the
launch's own round count.  CPU: the option itself, and the checker against orders that are wrong on purpose."""
import ctypes as C
import functools
import os
import re
import time

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import _lib
from fraytracer_amd import synthetic as syn
from helpers import assert_bit_equal, glibc_math, options, options_left_at_defaults  # noqa: F401  (options_left_at_defaults: a fixture)

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
    assert _lib.FT_OPT_ORDER == 16 and ft.Device.OPTIONS["order"] == 16
    assert "FT_OPT_ORDER" in open(os.path.join(ROOT, "host", "cpp", "FrayTracer.hpp")).read()      # the C++ layer takes the header's enumerator
    fs = open(os.path.join(ROOT, "host", "fsharp", "FrayTracer.Hip.fs")).read()
    assert re.search(r"let setTileOrder \(mode : int\) = if ft_ctx_set_option \(ctx\.Value, 16, mode\)", fs)
    assert "ft_ctx_set_option (ctx.Value, 16, mode)" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def heavy_tiles(cost, num=1, den=1):
    """bool per tile: cost * n * den >= sum(cost) * num, exactly (kernels.hip ft_tile_is_heavy).  Both sides must fit 64 bits, which is the kernel's own
    precondition: asserted in Python integers, so that no case passes by wrapping the way the kernel would"""
    assert cost.dtype == np.uint32 and cost.ndim == 1 and len(cost) > 0
    n, total, top = len(cost), int(cost.sum(dtype=np.uint64)), int(cost.max())
    assert top * n * den < 2 ** 64 and total * num < 2 ** 64, ("outside the kernel's precondition", top, n, den, total, num)
    return cost.astype(np.uint64) * np.uint64(n * den) >= np.uint64(total * num)


def check_order(cost, order, num=1, den=1):
    """AssertionError unless `order` is what the rule asks for from `cost` (uint32 arrays) -> the number of heavy tiles.  A permutation of 0 .. n-1;
    its head is exactly the heavy tiles, in non-increasing cost clamped to 255 (equal clamped costs in any order: their ranks come from atomics);
    its tail is the light tiles in ascending index."""
    assert order.dtype == np.uint32 and order.shape == cost.shape, (order.dtype, order.shape, cost.shape)
    n = len(cost)
    heavy = heavy_tiles(cost, num, den)
    assert int(order.max()) < n, ("an entry outside the frame", int(order.max()), n)
    seen = np.zeros(n, bool)
    seen[order] = True
    assert seen.all(), ("not a permutation: tiles never handed out (so others twice)", np.flatnonzero(~seen)[:8], int((~seen).sum()))
    k = int(heavy.sum())
    head, tail = order[:k], order[k:]
    assert heavy[head].all(), ("light tiles among the first %d" % k, head[~heavy[head]][:8])      # k distinct heavy tiles: exactly the heavy set
    clamped = np.minimum(cost[head], 255).astype(np.int64)
    rising = np.flatnonzero(np.diff(clamped) > 0)
    assert len(rising) == 0, ("clamped cost rises along the head at positions", rising[:8], clamped[rising[:8]], clamped[rising[:8] + 1])
    assert np.array_equal(tail, np.flatnonzero(~heavy)), "the light tiles are not in ascending index"
    return k


def test_the_checker_rejects_wrong_orders():
    """What shows that the GPU tests below can fail: every kind of wrong order is refused, a right one with its ties shuffled is not."""
    cost = np.array([3, 900, 0, 40, 40, 2, 255, 40, 1, 300, 7, 40], np.uint32)             # mean 135.7: heavy are 1, 6, 9 (900, 255, 300: all clamp to 255)
    good = np.array([9, 1, 6, 0, 2, 3, 4, 5, 7, 8, 10, 11], np.uint32)
    assert check_order(cost, good) == 3
    assert check_order(cost, np.array([6, 9, 1, 0, 2, 3, 4, 5, 7, 8, 10, 11], np.uint32)) == 3     # the three clamp to 255: any order
    # every tile sorted (0 / 1): ties at 40 (tiles 3, 4, 7, 11) in any order, and 900, 300, 255 share the clamped bucket
    by_cost = np.array([6, 1, 9, 3, 4, 7, 11, 10, 0, 5, 8, 2], np.uint32)
    shuffled = np.array([9, 6, 1, 11, 7, 3, 4, 10, 0, 5, 8, 2], np.uint32)
    assert check_order(cost, by_cost, 0, 1) == 12 and check_order(cost, shuffled, 0, 1) == 12
    assert check_order(cost, np.arange(12, dtype=np.uint32), 1000000, 1) == 0                # no tile heavy: the identity
    assert check_order(np.zeros(5, np.uint32), np.array([4, 0, 3, 1, 2], np.uint32)) == 5   # a sum of 0: every tile heavy, all tied

    def wrong(order, num=1, den=1, c=cost):
        with pytest.raises(AssertionError):
            check_order(c, np.array(order, np.uint32), num, den)

    wrong([9, 1, 6, 0, 2, 3, 4, 5, 7, 8, 10, 10])                                           # a duplicated entry (11 never handed out)
    wrong([9, 1, 1, 0, 2, 3, 4, 5, 7, 8, 10, 11])                                           # ... in the head
    wrong([9, 1, 6, 0, 2, 3, 4, 5, 7, 8, 10, 12])                                           # an entry equal to n
    wrong([9, 1, 6, 0, 2, 3, 4, 5, 7, 8, 10, 0xFFFFFFFF])                                   # a position never written
    wrong([9, 1, 0, 6, 2, 3, 4, 5, 7, 8, 10, 11])                                           # heavy 6 and light 0 swapped across the boundary
    wrong([9, 1, 6, 0, 2, 4, 3, 5, 7, 8, 10, 11])                                           # two light tiles swapped
    wrong([9, 1, 6, 0, 2, 3, 4, 5, 7, 8, 10])                                               # one entry short
    wrong(by_cost[[0, 1, 2, 3, 4, 5, 6, 8, 7, 9, 10, 11]], 0, 1)                            # head: cost 3 (tile 0) before cost 7 (tile 10)
    wrong([1, 3, 0, 2], c=np.array([5, 200, 1, 254], np.uint32))                            # two head tiles in increasing clamped cost (mean 115: 1 and 3 are heavy)
    assert check_order(np.array([5, 200, 1, 254], np.uint32), np.array([3, 1, 0, 2], np.uint32)) == 2
    wrong(list(range(12)))                                                                   # the identity where three tiles are heavy
    wrong(good, 0, 1)                                                                        # a 1 / 1 order under the rule that sorts every tile
    with pytest.raises(AssertionError):                                                      # the precondition: (2^32 - 1) x 4 x 2^31 does not fit 64 bits
        heavy_tiles(np.full(4, 0xFFFFFFFF, np.uint32), 1, 2 ** 31)
    with pytest.raises(AssertionError):                                                      # ... nor does a sum of 2^34 - 4 times 2^31
        heavy_tiles(np.full(4, 0xFFFFFFFF, np.uint32), 2 ** 31, 1)


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
    with options(gpu) as set_:
        for i, order in enumerate((1, 1, 1, 0)):
            set_(order=order)
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
    with glibc_math(gpu, oracle):
        want, _ = oracle.Oracle().scene(c3()).render(EPS, LEN, W, H, syn.default_camera().as_array(), nthreads=16)
        ds = gpu.scene(c3())
        try:
            launches(gpu, frames, ds, ft.ImageSize(W, H), syn.default_camera(), want, "C3 glibc")
        finally:
            ds.close()


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


def rule(cost, num=1, den=1):
    """the order the rule asks for, up to ties: (heavy tiles, light tiles), each in ascending index"""
    heavy = heavy_tiles(cost, num, den)
    return np.flatnonzero(heavy), np.flatnonzero(~heavy)


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
        heavy, light = rule(cost)
        print("tiles", nTiles, "mean cost", cost.mean(), "max", cost.max(), "heavy", len(heavy))
        assert 0 < len(heavy) < nTiles and len(heavy) + len(light) == nTiles
        # a permutation of all tiles: exactly the tiles at or above the mean, in non-increasing clamped cost, then the others in ascending index
        assert check_order(cost, order) == len(heavy)
        assert np.array_equal(np.sort(order[:len(heavy)]), heavy) and np.array_equal(order[len(heavy):], light)
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
        with options(gpu, order=0) as set_:
            plain = [frames.render(gpu, ds, size, c, **t) for size, c, t in seq]
            assert read_slot(ds, "costs") is None
            set_(order=1)
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
        with options(gpu, order=0) as set_:
            plain = [frames.render(gpu, ds, size, cam) for ds in dss]
            set_(order=1)
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
        with options(gpu, order=0) as set_:
            for _ in range(2):
                plain, st0 = frames.render(gpu, ds, size, cam)
                assert_bit_equal(plain, want, "option 0")
                assert read_slot(ds, "costs") is None and read_slot(ds, "order") is None
            set_(order=2)
            for _ in range(2):
                got, _ = frames.render(gpu, ds, size, cam)
                assert_bit_equal(got, want, "option 2")
                assert len(read_slot(ds, "costs")) == nTiles and read_slot(ds, "order") is None and not used_order(ds)
            set_(order=0)
            frames.render(gpu, ds, size, cam)
            assert read_slot(ds, "costs") is None                                       # option 0 forgets what was recorded
            set_(order=1, guided=1)
            for _ in range(3):
                got, st = frames.render(gpu, ds, size, cam)
                assert_bit_equal(got, plain, "guided hand-out with option 1")
                assert read_slot(ds, "order") is None and not used_order(ds)            # never combined: index order, nothing recorded
                for k in ("rays_primary", "rays_shadow", "hits_primary", "flags"):
                    assert st[k] == st0[k], k
    finally:
        ds.close()


# ------------------------------------------------ the order kernels on their own ------------------------------------------------
# ft_launch_tile_order and ft_tile_order_work_bytes (kernels.hip; internal, not in the header) on costs made here, so that the sizes, the costs and the
# rule are the test's and not what one C3 frame happens to record.

ORDER_TILES = 1024                                      # FT_ORDER_TILES: tiles per workgroup of the order kernels
WORK_HEADER = 4 * 256 + 4 * 256 + 8 + 4 * 4             # FtTileOrderWork: hist[256], cursor[256], sum (64 bits), ticketCount, ticketHeavy, nHeavy, pad
GUARD = 256                                             # bytes behind `order` and behind `work` that no launch may touch
RULES = ((1, 1), (0, 1), (2, 1), (3, 2), (1000000, 1))
SMALL = (1, 2, 63, 64, 255, 256, 257,                   # one workgroup: around a wave and around the 256 threads
         1023, 1024, 1025, 2049)                        # around FT_ORDER_TILES: one, two and three workgroups, the last one with a single tile
LARGE = (262144, 262145,                                # 256 and 257 workgroups: one thread of the last workgroup owns 1 and 2 of them
         1048576, 1048583)                              # an 8192^2 frame's count: 4 and 5 of them, the last workgroup partial
PATTERNS = ("zeros", "sevens", "all 255", "thousands", "i % 300", "geometric", "around the clamp", "mean above 255", "2^31 on the last",
            "2^32 - 1 on the first", "heavy in the first 1024", "heavy behind the last 1024")


@functools.lru_cache(maxsize=None)
def pattern(name, n):
    """n costs (uint32, read-only).  The names say what the tiles are under the rule 1 / 1."""
    i = np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(1000 * PATTERNS.index(name) + n % 997)
    if name == "zeros": c = np.zeros(n)                                                  # a sum of 0: every tile is heavy, all tied
    elif name == "sevens": c = np.full(n, 7)                                             # all equal: every tile heavy
    elif name == "all 255": c = np.full(n, 255)                                          # the clamped bucket alone
    elif name == "thousands": c = np.full(n, 1000)                                       # ... with a mean above it
    elif name == "i % 300": c = i % 300                                                  # every bucket, 255 .. 299 share the last
    elif name == "geometric": c = rng.geometric(1.0 / 50.0, n)                           # mean about 50, a long tail: what C3 records
    elif name == "around the clamp": c = rng.integers(200, 601, n)
    elif name == "mean above 255": c = np.where(i % 3 == 0, 4000, 300)                   # light tiles inside the clamped bucket
    elif name == "2^31 on the last": c = np.where(i == n - 1, 2 ** 31, 0)
    elif name == "2^32 - 1 on the first": c = np.where(i == 0, 2 ** 32 - 1, 3)
    elif name == "heavy in the first 1024": c = np.where((i < ORDER_TILES) & (i % 3 == 0), 50 + i % 5, 1)
    elif name == "heavy behind the last 1024": c = np.where((i >= (n - 1) // ORDER_TILES * ORDER_TILES) & (i % 2 == 0), 40 + i % 3, 1)   # n = 1025, 2049: one tile
    else: raise KeyError(name)
    c = c.astype(np.uint32)
    c.setflags(write=False)
    return c


class OrderBuffers:
    """cost, order and work on the device for up to `cap` tiles, through the runtime handle DeviceFrames opened; order and work GUARD bytes longer than asked"""

    def __init__(self, hip, cap):
        self.hip, self.cap = hip, cap
        self.launch = _lib.lib.ft_launch_tile_order
        self.launch.restype, self.launch.argtypes = C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        self.work_bytes = _lib.lib.ft_tile_order_work_bytes
        self.work_bytes.restype, self.work_bytes.argtypes = C.c_size_t, [C.c_uint32]
        self.cost, self.order, self.work = C.c_void_p(), C.c_void_p(), C.c_void_p()
        for ptr, size in ((self.cost, 4 * cap), (self.order, 4 * cap + GUARD), (self.work, self.work_bytes(cap) + GUARD)):
            assert hip.hipMalloc(C.byref(ptr), C.c_size_t(size)) == 0

    def fill(self, ptr, nbytes):
        assert self.hip.hipMemset(ptr, 0xFF, C.c_size_t(nbytes)) == 0
        assert self.hip.hipDeviceSynchronize() == 0

    def read(self, ptr, nbytes):
        out = np.empty(nbytes, np.uint8)
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), ptr, C.c_size_t(nbytes), 2) == 0          # hipMemcpyDeviceToHost
        return out

    def run(self, cost, n, num, den, fill_work=True):
        """0xFF everywhere, one ft_launch_tile_order on stream 0 over the first n tiles -> (its return value, order's n words and guard, work's
        ft_tile_order_work_bytes(n) bytes and guard)"""
        assert len(cost) <= self.cap and n <= len(cost)
        size = max(n, 1)
        wb = self.work_bytes(size)
        assert wb == WORK_HEADER + 4 * ((size + ORDER_TILES - 1) // ORDER_TILES)
        assert self.hip.hipMemcpy(self.cost, cost.ctypes.data_as(C.c_void_p), C.c_size_t(4 * len(cost)), 1) == 0   # hipMemcpyHostToDevice
        self.fill(self.order, 4 * size + GUARD)
        if fill_work:
            self.fill(self.work, wb + GUARD)
        rc = self.launch(self.cost, n, num, den, self.order, self.work, None)
        assert self.hip.hipDeviceSynchronize() == 0
        return rc, self.read(self.order, 4 * size + GUARD), self.read(self.work, wb + GUARD)

    def close(self):
        for ptr in (self.cost, self.order, self.work):
            self.hip.hipFree(ptr)


@pytest.fixture(scope="module")
def order_buffers(frames):
    b = OrderBuffers(frames.hip, max(LARGE))
    yield b
    b.close()


def launch_and_check(bufs, cost, num, den, fill_work=True):
    """one launch of the three kernels; the order against the rule, the guards, and what the work area must hold afterwards -> heavy tiles"""
    n = len(cost)
    rc, order_raw, work_raw = bufs.run(cost, n, num, den, fill_work)
    assert rc == 0, rc
    assert (order_raw[4 * n:] == 0xFF).all(), "a store behind order[n - 1]"
    assert (work_raw[-GUARD:] == 0xFF).all(), "a store behind the work area"
    order = order_raw[:4 * n].view(np.uint32)
    unwritten = np.flatnonzero(order == 0xFFFFFFFF)
    assert len(unwritten) == 0, ("positions of the order never written", unwritten[:8], len(unwritten))
    k = check_order(cost, order, num, den)
    # the work area: counts and sums, which no order of the atomics changes
    heavy = heavy_tiles(cost, num, den)
    blocks = (n + ORDER_TILES - 1) // ORDER_TILES
    per_block = np.add.reduceat(heavy.astype(np.int64), np.arange(0, n, ORDER_TILES))
    want_prefix = np.concatenate(([0], np.cumsum(per_block)[:-1])).astype(np.uint32)
    words = work_raw[:WORK_HEADER + 4 * blocks].view(np.uint32)
    prefix = words[WORK_HEADER // 4:]
    assert len(prefix) == blocks and np.array_equal(prefix, want_prefix), ("heavy tiles before each workgroup", np.flatnonzero(prefix != want_prefix)[:8])
    hist = words[:256]
    assert np.array_equal(hist, np.bincount(np.minimum(cost, 255), minlength=256)), "histogram of the clamped costs"
    total = int(work_raw[2048:2056].view(np.uint64)[0])
    assert total == int(cost.sum(dtype=np.uint64)), (total, int(cost.sum(dtype=np.uint64)))
    tickets_and_heavy = [int(v) for v in words[514:517]]
    assert tickets_and_heavy == [blocks, blocks, k], (tickets_and_heavy, blocks, k)
    return k


SMALL_CASES = [(n, p) for n in SMALL for p in PATTERNS]
# above 2049 every pattern at every size, each with one rule, the rules rotating with the pattern and the size: all five at each size
LARGE_CASES = [(n, p, RULES[(PATTERNS.index(p) + LARGE.index(n)) % len(RULES)]) for n in LARGE for p in PATTERNS]


@pytest.mark.gpu
@pytest.mark.parametrize("n,name", SMALL_CASES, ids=[f"{n}-{p}" for n, p in SMALL_CASES])
def test_order_kernels_small(gpu, order_buffers, n, name):
    """one to three workgroups: every size, every pattern, every rule"""
    cost = pattern(name, n)
    for num, den in RULES:
        launch_and_check(order_buffers, cost, num, den)


@pytest.mark.gpu
@pytest.mark.parametrize("n,name,rule_", LARGE_CASES, ids=[f"{n}-{p}-rule {r[0]}:{r[1]}" for n, p, r in LARGE_CASES])
def test_order_kernels_large(gpu, order_buffers, n, name, rule_):
    """256, 257, 1024 and 1025 workgroups: the prefix over the workgroups, of which one thread owns 1, 2, 4 and 5"""
    t0 = time.perf_counter()
    k = launch_and_check(order_buffers, pattern(name, n), *rule_)
    print(f"n {n} {name} rule {rule_[0]}/{rule_[1]}: heavy {k}, {time.perf_counter() - t0:.3f} s")


def test_the_cases_cover_what_they_must():
    """the direct cases hold every size, pattern and rule, each pattern and rule above 256 workgroups, and a launch of 2, 257 and 1025 workgroups; every
    input is inside the kernels' precondition under every rule it is run with (heavy_tiles asserts it)"""
    assert {n for n, _ in SMALL_CASES} == set(SMALL) and {p for _, p in SMALL_CASES} == set(PATTERNS)
    big = [(n, p, r) for n, p, r in LARGE_CASES if n > 256 * ORDER_TILES]
    assert {p for _, p, _ in big} == set(PATTERNS) and {r for _, _, r in big} == set(RULES)
    for n in LARGE:
        assert {r for m, _, r in LARGE_CASES if m == n} == set(RULES)
    groups = {(n + ORDER_TILES - 1) // ORDER_TILES for n in SMALL + LARGE}
    assert {1, 2, 3, 256, 257, 1024, 1025} <= groups
    for n in (1, 257, 2049):
        for p in PATTERNS:
            for num, den in RULES:
                heavy_tiles(pattern(p, n), num, den)
    for n, p, (num, den) in LARGE_CASES:
        if n in (262145, 1048583):
            heavy_tiles(pattern(p, n), num, den)
    # the names keep their word under 1 / 1
    assert heavy_tiles(pattern("heavy behind the last 1024", 2049)).nonzero()[0].tolist() == [2048]
    assert heavy_tiles(pattern("heavy behind the last 1024", 1025)).nonzero()[0].tolist() == [1024]
    assert heavy_tiles(pattern("heavy in the first 1024", 2049)).nonzero()[0].max() < 1024
    assert heavy_tiles(pattern("mean above 255", 2049)).sum() == 683 and pattern("mean above 255", 2049).min() == 300
    assert heavy_tiles(pattern("zeros", 257)).all() and heavy_tiles(pattern("sevens", 257)).all()
    assert not heavy_tiles(pattern("sevens", 257), 2, 1).any() and not heavy_tiles(pattern("geometric", 2049), 1000000, 1).any()


@pytest.mark.gpu
def test_one_work_area_three_launches(gpu, order_buffers):
    """2049 tiles, three cost arrays, the work area filled once before the first: each launch rewinds both tickets, the histogram, the sum and the cursors"""
    for i, name in enumerate(("geometric", "mean above 255", "i % 300")):
        launch_and_check(order_buffers, pattern(name, 2049), 1, 1, fill_work=i == 0)
    for num, den in ((0, 1), (3, 2)):
        launch_and_check(order_buffers, pattern("around the clamp", 2049), num, den, fill_work=False)


@pytest.mark.gpu
def test_the_launcher_refuses_no_tiles_and_no_denominator(gpu, order_buffers):
    cost = pattern("geometric", 2049)
    for n, num, den in ((0, 1, 1), (2049, 1, 0), (0, 0, 0)):
        rc, order_raw, work_raw = order_buffers.run(cost, n, num, den)
        assert rc != 0, (n, num, den)
        assert (order_raw == 0xFF).all() and (work_raw == 0xFF).all(), (n, num, den)         # nothing written


# ------------------------------------------------ frames on an order of two workgroups ------------------------------------------------

W2, H2 = 260, 268                                       # 33 x 34 = 1122 tiles: two order workgroups, partial tiles on both edges
TILES2 = ((W2 + 7) // 8) * ((H2 + 7) // 8)
MOVED = dict(Position=(0.5, 0.0, -10.0), LookAt=(0.0, 0.0, 0.0), Up=(0.0, 1.0, 0.0))


def c3_small():
    return syn.config3(n=64, size=W2)[0]


@pytest.fixture(scope="module")
def c3_small_oracle(oracle):
    """the oracle's frame of the 64-sphere C3 scene at 260 x 268, computed once: (pixels [W2, H2, 3], counters)"""
    want, cnt = oracle.Oracle().scene(c3_small()).render(EPS, LEN, W2, H2, syn.default_camera().as_array(), nthreads=16)
    want.setflags(write=False)
    return want, cnt


def set_rule(gpu, num, den):
    """ft_ctx_tile_order_rule (internal): tiles are heavy from num / den of the mean cost on"""
    fn = _lib.lib.ft_ctx_tile_order_rule
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]
    assert fn(gpu._ctx, num, den) == 0, _lib.last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("num,den", [(1, 1), (0, 1), (2, 1), (1000000, 1)], ids=["1:1", "0:1", "2:1", "1000000:1"])
def test_frames_on_an_order_of_two_workgroups(gpu, frames, c3_small_oracle, num, den):
    """three launches under each rule: every frame and its counters are the oracle's, the second and third run on a built order, and the order in the
    slot is what the rule makes of the costs in the slot.  0 / 1 sorts every tile; 1000000 / 1 leaves none heavy: the identity."""
    want, cnt = c3_small_oracle
    ds = gpu.scene(c3_small())
    try:
        set_rule(gpu, num, den)
        for i in range(3):
            got, st = frames.render(gpu, ds, ft.ImageSize(W2, H2), syn.default_camera())
            assert_bit_equal(got, want, f"rule {num}/{den}, launch {i}")
            for k in ORACLE_COUNTERS:
                assert st[k] == cnt[k], (i, k, st[k], cnt[k])
            assert used_order(ds) == (i > 0), i
            cost, order = read_slot(ds, "costs"), read_slot(ds, "order")
            assert cost is not None and order is not None and len(cost) == len(order) == TILES2
            heavy = check_order(cost, order, num, den)
            print(f"rule {num}/{den}, launch {i}: {TILES2} tiles, mean cost {cost.mean():.2f}, max {cost.max()}, heavy {heavy}")
            if (num, den) == (0, 1):
                assert heavy == TILES2
            elif (num, den) == (1000000, 1):
                assert heavy == 0 and np.array_equal(order, np.arange(TILES2))
            else:
                assert 0 < heavy < TILES2
    finally:
        set_rule(gpu, 1, 1)
        ds.close()


# ------------------------------------------------ the costs themselves ------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("reuse", [1, 0])
def test_costs_add_up_to_the_rounds_of_the_launch(gpu, frames, order, reuse):
    """A wave's grab writes the cost of the tile it took before: its evaluation rounds since that grab; the grab that finds the queue empty writes the
    last one.  The lean kernel refills only when its 64 lanes are idle, so the costs of a launch telescope to the rounds its waves spent from their first
    grab on.  Every tile's cost written exactly once <=> that sum; a tile never written keeps an older frame's value, one written twice another wave's.

    Which rounds belong to no tile: with FT_OPT_REUSE (the default) every wave first evaluates the scene at the camera position in all lanes (PH_CAM:
    kernels.hip, "one scene-SDF evaluation per active lane"), one round before its first grab — also in a wave that then finds the queue empty.  So
        reuse = 0:  sum(costs) == wave_evals
        reuse = 1:  sum(costs) == wave_evals - waves of the launch (whole workgroups of FT_BLOCK / 64 = 4 waves, at most one wave per tile + 3).
    Measured on an MI355X, 1122 tiles: reuse 0 gives 17414 == 17414 (moved camera 17531, glibc 17424); reuse 1 gives 16657 against 17781, 1124 = 4 x 281
    waves apart, in all eight launches."""
    size, cam = ft.ImageSize(W2, H2), syn.default_camera()
    moved = ft.Camera.lookAt(Lens=ft.Lens.create(60.0), **MOVED)
    ds = gpu.scene(c3_small())
    try:
        with options(gpu, order=order, reuse=reuse) as set_:
            def launch(what, camera, reordered):
                _, st = frames.render(gpu, ds, size, camera)
                cost = read_slot(ds, "costs")
                assert cost is not None and len(cost) == TILES2
                assert used_order(ds) == reordered, what
                total, rounds = int(cost.sum(dtype=np.uint64)), st["wave_evals"]
                print(f"order {order} reuse {reuse}, {what}: sum of costs {total}, wave_evals {rounds}, difference {rounds - total}")
                assert total <= rounds, (what, total, rounds)
                if reuse == 0:
                    assert total == rounds, (what, total, rounds)
                else:
                    waves = rounds - total
                    assert waves % 4 == 0 and 0 < waves <= 4 * ((TILES2 * 64 + 255) // 256), (what, total, rounds)
                return cost, rounds - total

            first, waves = launch("first launch of a fresh scene", cam, False)
            other, w = launch("moved camera", moved, order == 1)                       # the same key: the slot's order, built for another view
            assert w == waves
            assert not np.array_equal(first, other)                                     # other costs
            set_(tail_k=64)
            _, w = launch("tail_k 64", cam, order == 1)
            assert w == waves
            set_(tail_k=-1, math=ft.glibc_build_of_this_host())
            launch("glibc arithmetic", cam, False)                                      # another kernel: another key, index order
    finally:
        ds.close()
