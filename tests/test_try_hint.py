"""Try hints (FT_OPT_TRY_HINT; kernels.hip "Try hints", ft_kernels.h, capi.cpp tileOrder): a frame of the lean kernel records per 8x8 tile the
earliest of the tile's evaluation rounds on which the bundle certificate of its primary rays and that of its shadow rays held, and the scene's next
frame of the same grid tries each tile's bundles around those rounds.  Only when a try runs may depend on it.

CPU: the word's packing and clamp, the option's number in every layer, the schedule rule restated here against a table.
GPU: C3 with 64 and 256 spheres at 128^2 and 192^2 under a lens so narrow that word 0 of FT_OPT_CERT_POLICY leaves the per-lane tries out (asserted: the
case cannot silently become unhinted), the camera on the cloud's silhouette so that the frame holds tiles that are all sky and tiles that are all
cloud.  Repeated frames, a camera turned to the opposite silhouette, hint words no frame could have left, the options 0 and 2 against counts recorded
from the commit before the hints, and the launches that must stay unhinted."""
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import _lib
from fraytracer_amd import synthetic as syn
from helpers import assert_bit_equal, assert_cpp_compiles, options, options_left_at_defaults  # noqa: F401  (options_left_at_defaults: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS, LEN = 0.01, 30.0
RAYS = ("rays_primary", "rays_shadow", "hits_primary", "hits_shadow", "flags")
NONE, MAX, IDLE, AFTER = 255, 254, 4, 2                                          # ft_kernels.h FT_HINT_NONE, FT_HINT_MAX, FT_HINT_IDLE, FT_HINT_AFTER


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------

def pack(primary, shadow):
    """ft_kernels.h ft_hint_pack: bits 0-7 the primary family's round, 8-15 the shadow family's"""
    return (primary & 255) | (shadow & 255) << 8


def note(word, primary, r):
    """ft_kernels.h ft_hint_note: the word after a bundle of one family held on round r of the tile — rounds from 254 on are 254, the smaller stays"""
    v, p, s = min(r, MAX), word & 255, (word >> 8) & 255
    return pack(min(v, p), s) if primary else pack(p, min(v, s))


def due(h, r, n=NONE):
    """kernels.hip ft_try_due: every 4th round of the tile whatever the hint; with a hinted round h also at h - 1 and h; then every 2nd round, counted
    from the round n the family's bundle first held on in this frame, or from h while none has"""
    if r % IDLE == 0:
        return True
    if h != NONE and (r + 1 == h or r == h):
        return True
    start = n if n != NONE else h
    return start != NONE and r > start and (r - start) % AFTER == 0


def test_word_packing_and_clamp():
    w = pack(NONE, NONE)
    assert w == 0xffff
    w = note(w, True, 7)
    assert w == 0xff07
    w = note(w, True, 9)                       # a later round does not replace an earlier one
    assert w == 0xff07
    w = note(w, True, 0)
    assert w == 0xff00
    w = note(w, False, 300)                    # clamped to 254: 255 stays "none held"
    assert w == 0xfe00 and (w >> 8) & 255 == MAX
    w = note(w, False, 254)
    assert w == 0xfe00
    w = note(w, False, 253)
    assert w == 0xfd00
    assert note(pack(NONE, NONE), False, 2 ** 32 - 1) == pack(NONE, MAX)
    # the header's own statement of the same constants and functions
    text = open(os.path.join(ROOT, "fraytracer_amd", "csrc", "ft_kernels.h")).read()
    for name, v in (("FT_HINT_NONE", NONE), ("FT_HINT_MAX", MAX), ("FT_HINT_IDLE", IDLE), ("FT_HINT_AFTER", AFTER)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(v) + r"u\b", text), name
    assert "return (primary & 255u) | (shadow & 255u) << 8;" in text
    assert "r < FT_HINT_MAX ? r : FT_HINT_MAX" in text


def test_option_values_and_its_number_in_every_layer(tmp_path):
    host = ft.Device(-1)
    try:
        assert host.get_option("try_hint") == 1
        for v in (0, 2, 1):
            host.set_option("try_hint", v)
            assert host.get_option("try_hint") == v
        for bad in (3, -1):
            with pytest.raises(ft.FrayTracerError) as e:
                host.set_option("try_hint", bad)
            assert e.value.code == _lib.FT_ERR_INVALID and host.get_option("try_hint") == 1
    finally:
        host.close()
    header = open(os.path.join(ROOT, "include", "fraytracer_hip.h")).read()
    assert re.search(r"\bFT_OPT_TRY_HINT\s*=\s*19\b", header)
    assert _lib.FT_OPT_TRY_HINT == 19 and ft.Device.STREAM_OPTIONS["try_hint"] == 19
    assert "FT_OPT_TRY_HINT" in open(os.path.join(ROOT, "host", "cpp", "FrayTracer.hpp")).read()      # the C++ layer names it and takes the header's enumerator:
    assert_cpp_compiles(tmp_path, "try_hint.cpp", "void f(FrayTracer::Context& c) { c.setOption(FT_OPT_TRY_HINT, 2); static_assert(FT_OPT_TRY_HINT == 19, \"\"); (void)c.getOption(FT_OPT_TRY_HINT); }\n")
    fs = open(os.path.join(ROOT, "host", "fsharp", "FrayTracer.Hip.fs")).read()
    assert re.search(r"let setTryHint \(mode : int\) = if ft_ctx_set_option \(ctx\.Value, 19, mode\)", fs)
    assert "ft_ctx_set_option (ctx.Value, 19, mode)" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert _lib.lib.ft_abi_version() == 5


def test_schedule_rule_against_a_table():
    """(hint, rounds 0 .. 11 of the tile) -> try (1) or no try (0), written out by hand from the rule's wording"""
    table = {
        0:    "1 0 1 0 1 0 1 0 1 0 1 0",       # held at once last time: round 0, then every 2nd (the shipped period)
        1:    "1 1 0 1 1 1 0 1 1 1 0 1",       # h - 1 = 0 and h = 1, then 3, 5, 7 ... and every 4th (4, 8)
        2:    "1 1 1 0 1 0 1 0 1 0 1 0",
        3:    "1 0 1 1 1 1 0 1 1 1 0 1",
        6:    "1 0 0 0 1 1 1 0 1 0 1 0",
        9:    "1 0 0 0 1 0 0 0 1 1 0 1",
        NONE: "1 0 0 0 1 0 0 0 1 0 0 0",       # no bundle of the family held: every 4th round
    }
    for h, row in table.items():
        assert [int(due(h, r)) for r in range(12)] == [int(x) for x in row.split()], h
    # after a hold on round n of this frame the every-2nd-round tries count from n, whichever of h - 1 and h it came on (rounds before n: nothing noted yet)
    held = {
        (3, 2):    "- - - 1 1 0 1 0 1 0 1 0",       # hinted 3, held on 2: round 3 is the hinted round itself, then 4, 6, 8 ...
        (3, 3):    "- - - - 1 1 0 1 1 1 0 1",       # held on 3: 5, 7, 9 ... and every 4th
        (2, 2):    "- - - 0 1 0 1 0 1 0 1 0",       # the next frame of the first row: the same rounds from 4 on
        (NONE, 4): "- - - - - 0 1 0 1 0 1 0",       # no hint, yet the bundle held on a 4th round: the shipped period from there
        (9, 4):    "- - - - - 0 1 0 1 1 1 0",       # held long before the hinted round: 6, 8, 10 and the hinted 8, 9
    }
    for (h, n), row in held.items():
        for r, x in enumerate(row.split()):
            assert x == "-" or int(due(h, r, n)) == int(x), (h, n, r)
    # the far end: 254 stands for every round from 254 on
    assert [r for r in range(250, 262) if due(MAX, r)] == [252, 253, 254, 256, 258, 260]
    assert [r for r in range(250, 262) if due(NONE, r)] == [252, 256, 260]
    # whatever the hint, a tile is tried on its first round and at least every 4th: what a wrong hint can cost is bounded
    for h in range(256):
        assert due(h, 0)
        gaps = np.diff([r for r in range(600) if due(h, r)])
        assert gaps.max() <= IDLE, (h, gaps.max())
    # the kernel's wording of the rule
    text = open(os.path.join(ROOT, "fraytracer_amd", "csrc", "kernels.hip")).read()
    body = text[text.index("bool ft_try_due(uint32_t h, uint32_t n, uint32_t r) {"):]
    body = body[:body.index("\n}\n")]
    assert "if (r % FT_HINT_IDLE == 0u) return true;" in body and "if (h != FT_HINT_NONE && (r + 1u == h || r == h)) return true;" in body
    assert "const uint32_t from = n != FT_HINT_NONE ? n : h;" in body
    assert "return from != FT_HINT_NONE && r > from && (r - from) % FT_HINT_AFTER == 0u;" in body


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------

@pytest.fixture(autouse=True)
def try_hint_left_at_default(request):
    """helpers.options_left_at_defaults walks Device.OPTIONS only, and "try_hint" lives in Device.STREAM_OPTIONS: this module checks its own option"""
    yield
    if "gpu" in request.fixturenames:
        gpu = request.getfixturevalue("gpu")
        left = gpu.get_option("try_hint")
        gpu.set_option("try_hint", 1)
        assert left == 1, f"try_hint left at {left} on the shared device (now back at 1)"


# spheres, frame side, lens in degrees, x of the cloud's silhouette at y = 0.3 seen from the Program.fs position towards +x (camera A) and -x (camera B)
CASES = {"n64-128": (64, 128, 0.08, 1.936798870563507, -4.373418569518254), "n64-192": (64, 192, 0.12, 1.936798870563507, -4.373418569518254),
         "n256-128": (256, 128, 0.08, 4.615188837051392, -4.669646024657414), "n256-192": (256, 192, 0.12, 4.615188837051392, -4.669646024657414)}


def scene_of(case):
    return syn.config3(n=CASES[case][0], size=CASES[case][1])[0]


def camera_of(case, which):
    _, _, lens, xa, xb = CASES[case]
    return ft.Camera.lookAt(Position=(0.0, 0.0, -10.0), LookAt=(xa if which == "A" else xb, 0.3, 0.0), Up=(0.0, 1.0, 0.0), Lens=ft.Lens.create(lens))


@functools.lru_cache(maxsize=None)
def oracle_frame(case, which):
    """the oracle's frame and counters, computed once per (case, camera) and left unchanged"""
    from oracle import binding as ob
    size = CASES[case][1]
    want, cnt = ob.Oracle().scene(scene_of(case)).render(EPS, LEN, size, size, camera_of(case, which).as_array(), nthreads=16)
    want.setflags(write=False)
    return want, cnt


def tile_classes(want, cnt):
    """-> (all-sky tiles, all-cloud tiles) as tile indices (tile = tx * tilesY + ty, kernels.hip start_job) from the oracle's frame [X, Y, 3]: a pixel
    whose ray missed holds the background colour exactly, and the count of such pixels is the oracle's own count of misses"""
    sky = (want == np.asarray(syn.BACKGROUND, np.float32)).all(axis=2)
    assert int(sky.sum()) == cnt["rays_primary"] - cnt["hits_primary"]
    X, Y = sky.shape
    t = sky.reshape(X // 8, 8, Y // 8, 8).sum(axis=(1, 3)).reshape(-1)
    return np.flatnonzero(t == 64), np.flatnonzero(t == 0)


def tile_over_margin(ds, cam, size):
    """capi.cpp certSchedule: the side of an 8x8 pixel tile at the far side of the support sphere, over certM; <= 1: word 0 is the bundle alone"""
    ca, sup = cam.as_array().astype(np.float64), ds.support_sphere()
    n = lambda v: float(np.sqrt((v * v).sum()))
    return 8.0 * max(n(ca[6:9]), n(ca[9:12])) / size * (n(ca[0:3] - np.array(sup[:3])) + sup[3]) / n(ca[3:6]) / ds.miss_certificate()["margin"]


def slot_words(ds, name):
    """ft_scene_tile_costs / ft_selftest_try_hints (internal): the scene's lane-0 slot -> uint32 array, None where the slot holds none"""
    fn = getattr(_lib.lib, name)
    fn.restype, fn.argtypes = C.c_longlong, [C.c_void_p, C.c_void_p, C.c_longlong]
    n = fn(ds._scene, None, 0)
    assert n >= 0, _lib.last_error()
    if n == 0:
        return None
    out = np.empty(n, np.uint32)
    assert fn(ds._scene, out.ctypes.data_as(C.c_void_p), n) == n
    return out


def fill_hints(ds, mode, value):
    """ft_selftest_try_hints_fill (internal): every word = value (mode 0) or words from a generator seeded with value (mode 1) -> the tile count"""
    fn = _lib.lib.ft_selftest_try_hints_fill
    fn.restype, fn.argtypes = C.c_longlong, [C.c_void_p, C.c_int32, C.c_uint32]
    n = fn(ds._scene, mode, value)
    assert n >= 0, _lib.last_error()
    return n


def hinted(ds):
    """ft_selftest_try_hints_used (internal): did the scene's last recording launch on lane 0 follow the hints it found?"""
    fn = _lib.lib.ft_selftest_try_hints_used
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p]
    return bool(fn(ds._scene))


def frame(ds, case, which="A", **ext):
    size = CASES[case][1]
    with np.errstate(all="ignore"):
        return ds.render(EPS, LEN, ft.ImageSize(size, size), camera_of(case, which), **ext)


def narrow(ds, case, which="A"):
    ratio = tile_over_margin(ds, camera_of(case, which), CASES[case][1])
    assert 0.5 < ratio <= 1.0, ("the case's tiles are no longer narrow: word 0 would keep the per-lane tries and the launch would be unhinted", ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_repeated_frames(gpu, oracle, case):
    """Four frames of one scene: each equals the oracle's on every pixel (so each equals frame 1), rays, hits and flags are the oracle's in all four,
    sdf_evals falls from frame 1 to frame 2 and never rises after.  Frame 1 is unhinted, the others follow hints.  Tiles that are all cloud never see
    their primary bundle hold and cost at least a march's step and the four probes; of the tiles that are all sky some see it hold, and none costs
    more than one round more under its hint than without."""
    want, cnt = oracle_frame(case, "A")
    sky, cloud = tile_classes(want, cnt)
    assert len(sky) > 0 and len(cloud) > 0, (len(sky), len(cloud))
    ds = gpu.scene(scene_of(case))
    try:
        narrow(ds, case)
        sts, costs, hints = [], [], []
        for i in range(4):
            got, st = frame(ds, case)
            assert_bit_equal(got, want, f"{case} frame {i + 1}")
            for k in RAYS:
                assert st[k] == cnt[k], (case, i, k, st[k], cnt[k])
            assert hinted(ds) == (i > 0), (case, i)
            sts.append(st); costs.append(slot_words(ds, "ft_scene_tile_costs")); hints.append(slot_words(ds, "ft_selftest_try_hints"))
        ev = [st["sdf_evals"] for st in sts]
        print(case, "sdf_evals", ev, "wave_evals", [st["wave_evals"] for st in sts], "tiles sky / cloud", len(sky), len(cloud))
        assert ev[1] < ev[0] and ev[2] <= ev[1] and ev[3] <= ev[2], ev
        for i in range(4):
            assert len(costs[i]) == len(hints[i]) == (CASES[case][1] // 8) ** 2
            assert (hints[i] >> 16 == 0).all()
            assert ((hints[i][cloud] & 255) == NONE).all(), (case, i)                   # no bundle of rays that hit can be proved to miss
            assert costs[i][cloud].min() >= 5, (case, i, costs[i][cloud].min())          # a step, three probes and the centre probe at the very least
            assert ((hints[i][sky] & 255) != NONE).any(), (case, i)                      # some bundle of rays that all miss is proved to
            if i > 0:
                # the camera stands still, so a first hold is found on its round or the one before, where frame 1 found it on its round or the one
                # after; every later hold at most one round after it became possible, in either schedule
                assert (costs[i][sky].astype(np.int64) <= costs[0][sky].astype(np.int64) + 1).all(), (case, i)
    finally:
        ds.close()


MAX_SHIFT = 16.0                                                                  # capi.cpp FT_HINT_MAX_SHIFT: hints are followed up to this many pixels of image motion


def camera_shift(ds, p, q, size):
    """capi.cpp cameraShiftPixels, restated: the turn of the forward direction, the change of up and right at the frame's edge and the move of the
    position seen from the near side of the support sphere, in pixels"""
    p, q, sup = p.as_array().astype(np.float64), q.as_array().astype(np.float64), ds.support_sphere()
    n = lambda v: float(np.sqrt((v * v).sum()))
    side = max(n(q[6:9]), n(q[9:12]))
    pixel = side / size / n(q[3:6])
    near = max(n(q[0:3] - np.array(sup[:3])) - sup[3], 0.1 * sup[3])
    moved = n(q[0:3] - p[0:3])
    return n(q[3:6] / n(q[3:6]) - p[3:6] / n(p[3:6])) / pixel + (n(q[6:9] - p[6:9]) + n(q[9:12] - p[9:12])) / side * 0.5 * size + (moved / near / pixel if moved > 0 else 0.0)


def look_at_x(case, x):
    return ft.Camera.lookAt(Position=(0.0, 0.0, -10.0), LookAt=(x, 0.3, 0.0), Up=(0.0, 1.0, 0.0), Lens=ft.Lens.create(CASES[case][2]))


def fresh_frame(case, cam):
    """the frame and stats of a fresh context's first launch: nothing recorded, nothing followed"""
    size = CASES[case][1]
    fresh = ft.Device(0)
    try:
        fs = fresh.scene(scene_of(case))
        with np.errstate(all="ignore"):
            ref, rst = fs.render(EPS, LEN, ft.ImageSize(size, size), cam)
        assert not hinted(fs)
        fs.close()
    finally:
        fresh.close()
    return ref, rst


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_stale_hints(gpu, oracle, case):
    """Camera A; then a camera turned by about ten pixels, which follows A's hints; then camera B on the opposite silhouette (the cloud fills the other
    half of the frame), which is too far from A to follow them (more than FT_HINT_MAX_SHIFT pixels) — and B once more with A's words written under it,
    which does.  Each frame equals a fresh context's frame of the same camera bit for bit, with the same rays, hits and flags, and B's the oracle's."""
    want, cnt = oracle_frame(case, "B")
    size, xa = CASES[case][1], CASES[case][3]
    cam_a, cam_b = camera_of(case, "A"), camera_of(case, "B")
    ds = gpu.scene(scene_of(case))
    try:
        narrow(ds, case, "A"); narrow(ds, case, "B")
        per_unit = camera_shift(ds, cam_a, look_at_x(case, xa + 1e-3), size) / 1e-3
        cam_c = look_at_x(case, xa - 10.0 / per_unit)
        assert 5.0 < camera_shift(ds, cam_a, cam_c, size) < MAX_SHIFT < camera_shift(ds, cam_a, cam_b, size)
        ref_c, rst_c = fresh_frame(case, cam_c)
        ref_b, rst_b = fresh_frame(case, cam_b)
        assert_bit_equal(ref_b, want, f"{case} fresh frame B")
        frame(ds, case, "A"); frame(ds, case, "A")
        words_a = slot_words(ds, "ft_selftest_try_hints")
        with np.errstate(all="ignore"):
            got, st = ds.render(EPS, LEN, ft.ImageSize(size, size), cam_c)
        assert hinted(ds)
        assert_bit_equal(got, ref_c, f"{case} ten pixels on under A's hints")
        for k in RAYS:
            assert st[k] == rst_c[k], (case, k, st[k], rst_c[k])
        got, st = frame(ds, case, "B")
        assert not hinted(ds)                                                            # too far: recorded, not followed
        assert_bit_equal(got, ref_b, f"{case} frame B after A")
        write = _lib.lib.ft_selftest_try_hints_write
        write.restype, write.argtypes = C.c_longlong, [C.c_void_p, C.c_void_p, C.c_longlong]
        assert write(ds._scene, words_a.ctypes.data_as(C.c_void_p), len(words_a)) == len(words_a), _lib.last_error()
        got, st = frame(ds, case, "B")
        assert hinted(ds)
        assert_bit_equal(got, ref_b, f"{case} frame B under A's hints")
        for k in RAYS:
            assert st[k] == rst_b[k] == cnt[k], (case, k, st[k], rst_b[k], cnt[k])
    finally:
        ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_wrong_hints(gpu, oracle, case):
    """Hint words no frame could have left — all 0, all 254, all 255, two seeded random fills (every byte value) — and the next frame is the oracle's
    each time: a hint only ever moves a try, the rule's every-4th-round tries cannot be switched off by any word"""
    want, cnt = oracle_frame(case, "A")
    ds = gpu.scene(scene_of(case))
    try:
        narrow(ds, case)
        _, first = frame(ds, case)
        evals = {}
        for name, mode, value in (("all 0", 0, 0), ("all 254", 0, pack(MAX, MAX)), ("all 255", 0, pack(NONE, NONE)), ("all ones", 0, 0xffffffff),
                                  ("random 1", 1, 1), ("random 2", 1, 20240607)):
            assert fill_hints(ds, mode, value) == (CASES[case][1] // 8) ** 2
            if mode == 0:
                assert (slot_words(ds, "ft_selftest_try_hints") == value).all()
            got, st = frame(ds, case)
            assert hinted(ds), name
            assert_bit_equal(got, want, f"{case} after {name}")
            for k in RAYS:
                assert st[k] == cnt[k], (case, name, k, st[k], cnt[k])
            assert (slot_words(ds, "ft_selftest_try_hints") >> 16 == 0).all()            # the frame wrote every tile's word anew
            evals[name] = st["sdf_evals"]
        print(case, "sdf_evals unhinted", first["sdf_evals"], evals)
    finally:
        ds.close()


@functools.lru_cache(maxsize=None)
def parent_counts():
    """sdf_evals, wave_evals and culled_fraction of four repeated frames per case, recorded from the commit before the hints (tools/try_hint_probe.py
    says nothing about them: they are a test vector)"""
    return json.load(open(os.path.join(ROOT, "tests", "golden", "try_hint_parent_counters.json")))


@pytest.mark.gpu
@pytest.mark.parametrize("option", [0, 2])
@pytest.mark.parametrize("case", list(CASES))
def test_options_off_and_record_only_count_what_the_parent_counts(gpu, oracle, case, option):
    want, cnt = oracle_frame(case, "A")
    ds = gpu.scene(scene_of(case))
    try:
        with options(gpu, try_hint=option):
            for i, rec in enumerate(parent_counts()[case]):
                got, st = frame(ds, case)
                assert_bit_equal(got, want, f"{case} option {option} frame {i + 1}")
                assert not hinted(ds)
                print(case, option, i, st["sdf_evals"], st["wave_evals"], st["culled_fraction"], rec)
                assert st["sdf_evals"] == rec["sdf_evals"] and st["wave_evals"] == rec["wave_evals"], (case, option, i, st, rec)
                assert np.float32(st["culled_fraction"]) == np.float32(rec["culled_fraction"]), (case, option, i, st["culled_fraction"], rec["culled_fraction"])
                words = slot_words(ds, "ft_selftest_try_hints")
                if option == 0:
                    assert words is None
                else:                                                                    # record only: the words are filled, and not followed
                    _, cloud = tile_classes(want, cnt)
                    assert words is not None and (words >> 16 == 0).all() and ((words & 255) != NONE).any() and ((words[cloud] & 255) == NONE).all()
    finally:
        ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["wide tiles", "explicit word", "views", "extension"])
def test_unhinted_launches_count_the_same_twice(gpu, what):
    """A wide-tiled frame (C3 at 96^2 under the Program.fs lens), an explicit policy word on a narrow-tiled frame, a views launch and an EXTENSION
    launch: the second launch of each counts what the first counted, and follows no hint"""
    case = "n64-128"
    size = ft.ImageSize(CASES[case][1], CASES[case][1])
    scene = syn.config3(n=64, size=96)[0] if what == "wide tiles" else scene_of(case)
    ds = gpu.scene(scene)
    try:
        opts = {"cert_policy": 255 | (255 << 8) | (16 << 16) | (6 << 24)} if what == "explicit word" else {}
        with options(gpu, **opts):
            sts = []
            for _ in range(2):
                with np.errstate(all="ignore"):
                    if what == "wide tiles":
                        assert tile_over_margin(ds, syn.default_camera(), 96) > 2.0
                        _, st = ds.render(EPS, LEN, ft.ImageSize(96, 96), syn.default_camera())
                    elif what == "views":
                        _, st = ds.render_views(EPS, LEN, size, [camera_of(case, "A"), camera_of(case, "B")])
                    elif what == "extension":
                        _, st = frame(ds, case, spp=4)
                    else:
                        narrow(ds, case)
                        _, st = frame(ds, case)
                assert not hinted(ds), what
                sts.append(st)
        for k in RAYS + ("sdf_evals", "wave_evals", "culled_fraction"):
            assert sts[0][k] == sts[1][k], (what, k, sts[0][k], sts[1][k])
    finally:
        ds.close()
