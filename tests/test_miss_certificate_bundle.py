"""The lean kernel's bundle certificate (kernels.hip ft_bundle_certificate; FT_OPT_CERT_POLICY bits 30-31): one miss certificate for all the primary
rays, or all the shadow rays, of a wave, with the children spread over the lanes.

CPU: a float64 restatement of the kernel's bound — axis, width W, interval I, with the kernel's own paddings — whose sum must be >= the flat
per-lane certificate sum of every member (so a bundle that holds implies that every member's own certificate holds), and the policy word.
GPU: colours, ray / hit counters and flags against the oracle (which has no certificate at all), bit for bit, with the bundle alone on every round,
with the bundle and the per-lane certificate on every round and step, with the bundle off, the certificates off and the escape shortcut off."""
import numpy as np
import pytest

import fraytracer_amd as ft
from fraytracer_amd import synthetic as syn
from helpers import assert_bit_equal, glibc_math, host, options, options_left_at_defaults, seg_dist  # noqa: F401  (host, options_left_at_defaults: fixtures)

EPS, LEN = 0.01, 30.0


def s32(v):
    """a 32-bit policy word as the int32 the option takes"""
    return v - (1 << 32) if v >= (1 << 31) else v


EVERY_STEP = 0 | (1 << 8) | (1 << 16) | (1 << 24)                 # per-lane: every lane, every step (tests/test_miss_certificate.py)
SHIPPED_LANES = 0 | (6 << 8) | (16 << 16) | (6 << 24)             # the per-lane schedule of word 0
BUNDLE_ONLY = s32(255 | (255 << 8) | (1 << 16) | (1 << 30))       # bundle every round from one member on, per-lane never
BUNDLE_AND_LANES = s32(EVERY_STEP | (1 << 30))                    # bundle every round + per-lane every step
BUNDLE_OFF = s32(SHIPPED_LANES | (3 << 30))
COLS = {"bundle_only": {"cert": 1, "cert_policy": BUNDLE_ONLY}, "bundle_and_lanes": {"cert": 1, "cert_policy": BUNDLE_AND_LANES},
        "bundle_off": {"cert": 1, "cert_policy": BUNDLE_OFF}, "cert_off": {"cert": 0, "cert_policy": BUNDLE_ONLY},
        "escape_off": {"cert": 1, "cert_policy": BUNDLE_AND_LANES, "escape": 0}}


# ---------------------------------------------------------------- CPU: the bound ----------------------------------------------------------------

def children(n, seed=3, two_groups=False):
    rng = syn.Rng(seed)
    C, R = [], []
    for _ in range(n):
        C.append(rng.pointInBall(4.0)); R.append(rng.range(0.1, 0.5))
    C, R = np.array(C, np.float32), np.array(R, np.float32)
    if two_groups:
        C = C * np.float32(0.5)
        C[::2, 0] += np.float32(-12.0); C[1::2, 0] += np.float32(12.0)
    return C, R


def scene_of(C, R, strength, lights=None):
    forms = [syn.SdfForm.Primitive.sphere(Center=tuple(float(v) for v in c), Radius=float(r)) for c, r in zip(C, R)]
    obj = syn.SdfObject.create(syn.SdfMaterial.createSolid((0.9, 0.6, 0.3)), syn.SdfForm.unionSmooth(strength, forms))
    return syn.SdfScene(obj, syn.BACKGROUND, lights or [syn.SdfLight.directional((-0.5, -1.0, 1.0), (0.5, 0.5, 0.5))])


def lane_segment(K, o, d, eps, length):
    """ft_cert_segment: (t0, t1) of the lane's clipped segment, or None where the gate or the clip leaves the lane out"""
    w = o - K["c"]
    ww, dd, b = w @ w, d @ d, w @ d
    if not (0.0 <= eps <= K["escR"] and 0.0 < length < 1e9 and 0.81 <= dd <= 1.44 and ww <= K["rho2"]):
        return None
    R = (K["escR"] + eps + K["clip"]) * 1.001
    disc = b * b - dd * (ww - R * R)
    if not disc > 0.0:
        return None
    sq = np.sqrt(disc)
    t0, t1 = max((-b - sq) / dd, 0.0), min((sq - b) / dd, length * K["lenF"])
    return (t0, t1) if t1 > t0 else None


def bundle_bound(K, C, R, k, lanes, axis):
    """ft_bundle_certificate in float64: lanes = [(o, dir, eps, length)] in lane order -> (members, bundle sum, eps max) or None without a member.
    axis "lane": the kernel's (the first member at or after lane 27, else the first); "mean": the members' mean origin and mean direction."""
    mem = [(i, l, lane_segment(K, *l)) for i, l in enumerate(lanes)]
    mem = [(i, l, s) for i, l, s in mem if s is not None]
    if not mem:
        return None
    if axis == "lane":
        first = [m for m in mem if m[0] >= 27]
        oc, dc = (first[0] if first else mem[0])[1][:2]
    else:
        oc, dc = np.mean([m[1][0] for m in mem], axis=0), np.mean([m[1][1] for m in mem], axis=0)
    W, lo, hi, epsMax = 0.0, np.inf, -np.inf, 0.0
    for _, (o, d, eps, _), (t0, t1) in mem:
        g = o - oc
        s = (g @ dc) / (dc @ dc)
        a, b = np.linalg.norm(g - s * dc), np.linalg.norm(d - dc)
        W, lo, hi, epsMax = max(W, a + b * t1), min(lo, s + t0), max(hi, s + t1), max(epsMax, eps)
    Rc = (K["escR"] + epsMax + K["clip"]) * 1.001
    W = W * 1.001 + (1e-6 + 4e-6 * Rc)
    if not W <= K["escR"]:
        return [m[0] for m in mem], np.inf, epsMax                    # the kernel gives up: no bound
    lo, hi = lo - 4e-6 * Rc, hi + 4e-6 * Rc
    total = np.exp(-k * (seg_dist(C, oc + lo * dc, oc + hi * dc) - W - R)).sum()
    return [m[0] for m in mem], total, epsMax


def flat_sum(C, R, k, o, d, t0, t1):
    return np.exp(-k * (seg_dist(C, o + t0 * d, o + t1 * d) - R)).sum()


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def make_bundle(family, rs, K):
    """64 lanes (o, dir, eps, length) of one family; -> (lanes, indices that must be left out)"""
    cam = syn.default_camera().as_array().astype(np.float64)
    eps = lambda: float(rs.choice([0.0, 0.01, 0.05]))
    out = set()
    if family in ("cone96", "cone4096"):
        size = 96 if family == "cone96" else 4096
        tx, ty = rs.integers(0, size // 8, 2)
        lanes = []
        adv = rs.uniform(0.0, 9.0) if rs.random() < 0.7 else 0.0
        for i in range(64):
            px, py = (tx * 8 + (i >> 3)) / size, (ty * 8 + (i & 7)) / size
            d = unit(cam[3:6] + (px - 0.5) * cam[9:12] + (py - 0.5) * cam[6:9])
            t = adv + rs.uniform(0.0, 0.5) if adv else 0.0             # marched to different depths
            lanes.append((cam[0:3] + t * d, d, eps(), LEN - t))
    elif family == "parallel":
        d = unit(rs.normal(size=3))
        u = unit(np.cross(d, rs.normal(size=3)))
        v = np.cross(d, u)
        base = K["c"] + (u * rs.normal() + v * rs.normal()) * K["escR"] * 0.6 - d * K["escR"] * 1.5
        lanes = [(base + u * rs.uniform(-0.05, 0.05) + v * rs.uniform(-0.05, 0.05) + d * rs.uniform(0.0, 5.0), d, eps(), LEN) for _ in range(64)]
    elif family == "straddle":                                        # through the gap between two far groups, or along the line through both
        d = unit(np.array([0.0, 1.0, 0.0]) + rs.normal(size=3) * 0.02) if rs.random() < 0.5 else unit(np.array([1.0, 0.0, 0.0]) + rs.normal(size=3) * 0.02)
        base = K["c"] - d * K["escR"] * 1.4 + rs.normal(size=3) * 0.5
        lanes = [(base + rs.normal(size=3) * 0.03, unit(d + rs.normal(size=3) * 0.002), eps(), LEN) for _ in range(64)]
    elif family == "one":
        d = unit(rs.normal(size=3))
        o = K["c"] + rs.normal(size=3) * K["escR"] * 0.5 - d * K["escR"]
        lanes = [(o, d, eps(), LEN)] + [(o, d * 3.0, 0.01, LEN)] * 63     # |dir| = 3: outside the gate
        out = set(range(1, 64))
        pos = int(rs.integers(0, 64))
        lanes[0], lanes[pos] = lanes[pos], lanes[0]
        out = set(range(64)) - {pos}
    elif family == "identical":
        d = unit(rs.normal(size=3))
        o = K["c"] + rs.normal(size=3) * K["escR"] * 0.5 - d * K["escR"]
        lanes = [(o, d, 0.01, LEN)] * 64
    elif family == "empty":                                           # half the lanes pass the clip ball by, or have no Length left: no segment
        d = unit(rs.normal(size=3))
        u = unit(np.cross(d, rs.normal(size=3)))
        base = K["c"] - d * K["escR"] * 1.5
        lanes = []
        for i in range(64):
            kind = i % 4
            if kind == 0: lanes.append((base + u * (K["escR"] * 1.2 + rs.uniform(0.0, 1.0)), d, 0.01, LEN)); out.add(i)
            elif kind == 1: lanes.append((base + u * rs.uniform(0.0, 0.05), d, 0.01, 0.5 * K["escR"] * 0.4)); out.add(i)   # ends before the ball
            else: lanes.append((base + u * rs.uniform(0.0, 0.05), d, 0.01, LEN))
    return lanes, out


SCENES = [(31, s, False) for s in (0.05, 0.25, 1.0)] + [(257, s, False) for s in (0.05, 0.25, 1.0)] + [(600, s, False) for s in (0.05, 0.25, 1.0)] + \
         [(257, 0.25, True)]
FAMILIES = ["cone96", "cone4096", "parallel", "straddle", "one", "identical", "empty"]


@pytest.mark.parametrize("axis", ["lane", "mean"])
def test_bundle_sum_bounds_every_members_flat_sum(host, axis):
    """2 000 and more random bundles per axis choice: the bundle's sum is >= the flat certificate sum of every member, lanes outside the gate or without
    a clipped segment are no members, and on C3's own camera cones the bundle does hold for some tiles (the test is not vacuous)."""
    rs = np.random.default_rng(17)
    checked = held = 0
    for n, strength, two in SCENES:
        C, R = children(n, two_groups=two)
        ds = host.scene(scene_of(C, R, strength))
        try:
            cx, cy, cz, escR = ds.support_sphere()
            cert = ds.miss_certificate()
        finally:
            ds.close()
        assert escR > 0 and cert["margin"] > 0
        K = {"c": np.array([cx, cy, cz], np.float64), "escR": escR, "clip": cert["clip"], "rho2": cert["rho2"], "lenF": cert["len_factor"]}
        Cd, Rd, k = C.astype(np.float64), R.astype(np.float64), 1.0 / strength
        for family in FAMILIES:
            if (family == "straddle") != two and (family == "straddle" or two):
                continue
            for _ in range(40 if not two else 240):
                lanes, out = make_bundle(family, rs, K)
                res = bundle_bound(K, Cd, Rd, k, lanes, axis)
                if res is None:
                    continue
                members, total, epsMax = res
                assert not (set(members) & out), (family, sorted(set(members) & out))
                if family in ("one", "identical", "empty"):
                    assert set(members) == set(range(64)) - out, family
                thr = np.exp(-k * (epsMax + cert["margin"])) * 0.9999
                for i in members:
                    o, d, e, length = lanes[i]
                    t0, t1 = lane_segment(K, o, d, e, length)
                    flat = flat_sum(Cd, Rd, k, o, d, t0, t1)
                    assert total >= flat * (1 - 1e-12), (n, strength, family, axis, i, total, flat)
                    assert thr <= np.exp(-k * (e + cert["margin"])) * 0.9999 * (1 + 1e-12)      # the strictest member's threshold
                checked += 1
                if family.startswith("cone") and n == 257 and not two and total < thr:
                    held += 1
    assert checked >= 2000, checked
    assert held > 0


def test_policy_word(host):
    """bits 30-31 select the bundle's schedule; every word refused before is refused, the new bits come back as set, word 0 reads back as 0"""
    with options(host) as set_:
        assert host.get_option("cert_policy") == 0
        for bad in (1, 65 << 16, s32(1 | (1 << 30)), s32((65 << 16) | (2 << 30)), s32(3 << 30), s32((255 << 16) | (3 << 30)), 0x00FF0000):
            with pytest.raises(ft.FrayTracerError) as e:
                host.set_option("cert_policy", bad)
            assert e.value.code == -1, bad
            assert host.get_option("cert_policy") == 0
        for word in (BUNDLE_ONLY, BUNDLE_AND_LANES, BUNDLE_OFF, s32(SHIPPED_LANES | (2 << 30)), EVERY_STEP, SHIPPED_LANES, 0x01010100, 1 | (6 << 8) | (16 << 16)):
            set_(cert_policy=word)
            assert host.get_option("cert_policy") == word
        set_(cert_policy=0)
        assert host.get_option("cert_policy") == 0


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------

def run_columns(gpu, call, want, ocnt, counters, cols=COLS, extra=None):
    """call() under every policy column -> {column: stats}; every float and every counter equal to the oracle's"""
    out = {}
    with options(gpu) as set_:
        for name, o in cols.items():
            set_(**dict(o, **(extra or {})))
            with np.errstate(all="ignore"):
                got, st = call()
            assert_bit_equal(got, want, name)
            for k in counters:
                assert st[k] == ocnt[k], (name, k, st[k], ocnt[k])
            out[name] = st
    return out


FRAME_COUNTERS = ("rays_primary", "rays_shadow", "hits_primary", "hits_shadow", "flags")
RAY_COUNTERS = ("rays_shadow", "hits_primary", "hits_shadow", "flags")


def render_columns(gpu, oracle, scene, W, H, eps=EPS, cols=COLS, extra=None, counters=FRAME_COUNTERS, cam=None, **ext):
    cam = cam or syn.default_camera()
    want, ocnt = oracle.Oracle().scene(scene).render(eps, LEN, W, H, cam.as_array(), nthreads=16, **ext)
    ds = gpu.scene(scene)
    try:
        return run_columns(gpu, lambda: ds.render(eps, LEN, ft.ImageSize(W, H), cam, **ext), want, ocnt, counters, cols, extra)
    finally:
        ds.close()


def look(pos, at):
    return ft.Camera.lookAt(Position=pos, LookAt=at, Up=(0.0, 1.0, 0.0), Lens=ft.Lens.create(60.0))


@pytest.mark.gpu
@pytest.mark.parametrize("strength", [0.05, 0.25, 1.0])
def test_c3_frames(gpu, oracle, strength):
    """C3 at 96^2.  At strength 0.05 the frame of the Program.fs camera holds no march at all: 10 units from the cloud every term exp(-20 d) is
    below 2^-149, the float32 sum is 0 and the first step is infinite, so every ray ends after the camera's own evaluation (which a wave makes once
    and sdf_evals does not count) and there is nothing a certificate could save.  That frame is compared all the same; the count is asserted on the
    frame of a camera 7.5 units from the centre, where the rays do march."""
    scene = syn.config3(n=256, size=96, strength=strength)[0]
    if strength == 0.05:
        st = render_columns(gpu, oracle, scene, 96, 96)
        assert {v["sdf_evals"] for v in st.values()} == {0}, st
    st = render_columns(gpu, oracle, scene, 96, 96, cam=look((0.0, 0.0, -7.5), (0.0, 0.0, 0.0)) if strength == 0.05 else None)
    print(strength, {k: v["sdf_evals"] for k, v in st.items()})
    assert st["bundle_only"]["sdf_evals"] < st["cert_off"]["sdf_evals"]           # the bundle certificate fires
    assert st["bundle_and_lanes"]["sdf_evals"] <= st["bundle_off"]["sdf_evals"] <= st["cert_off"]["sdf_evals"]


@pytest.mark.gpu
def test_c3_frame_glibc_arithmetic(gpu, oracle):
    with glibc_math(gpu, oracle) as variant:
        st = render_columns(gpu, oracle, syn.config3(n=256, size=96)[0], 96, 96, extra={"math": variant})
    assert st["bundle_only"]["sdf_evals"] < st["cert_off"]["sdf_evals"]


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(8, 8), (13, 9), (1, 1)])
def test_tiny_and_ragged_frames(gpu, oracle, W, H):
    """one tile, ragged tiles with idle lanes, one pixel"""
    render_columns(gpu, oracle, syn.config3(n=256, size=16)[0], W, H)


@pytest.mark.gpu
@pytest.mark.parametrize("tail_k", [64, 0])
def test_latency_mode_forced_and_off(gpu, oracle, tail_k):
    render_columns(gpu, oracle, syn.config3(n=256, size=64)[0], 64, 64, extra={"tail_k": tail_k})


@pytest.mark.gpu
@pytest.mark.parametrize("eps", ["-0.01", "0", "0.01", "beyond"])
def test_epsilon_range(gpu, oracle, eps):
    """epsilon negative (outside the gate), 0, the usual one, and 1.01 escR (beyond the gate)"""
    scene = syn.config3(n=64, size=48)[0]
    if eps in ("-0.01", "0"):                                         # some rays creep to the step cap (flagged): a tile of a 4-sphere cloud keeps that to seconds
        render_columns(gpu, oracle, syn.config3(n=4, size=8)[0], 8, 8, eps=float(eps))
        return
    ds = gpu.scene(scene)
    escR = ds.support_sphere()[3]
    ds.close()
    render_columns(gpu, oracle, scene, 48, 48, eps=1.01 * escR if eps == "beyond" else float(eps))


@pytest.mark.gpu
@pytest.mark.parametrize("lights", ["point", "two_directional"])
def test_lights(gpu, oracle, lights):
    """a point light's shadow rays have |dir| = 1 / distance: no members; two directional lights: a wave's shadow rays of two directions"""
    L = [syn.SdfLight.point((3.0, 4.0, -6.0), (0.0, 20.0, 30.0))] if lights == "point" else \
        [syn.SdfLight.directional((-0.5, -1.0, 1.0), (0.5, 0.5, 0.5)), syn.SdfLight.directional((0.6, -1.0, -0.3), (0.4, 0.3, 0.2))]
    C, R = children(128)
    st = render_columns(gpu, oracle, scene_of(C, R, 0.25, L), 64, 64)
    assert st["bundle_only"]["sdf_evals"] < st["cert_off"]["sdf_evals"]


@pytest.mark.gpu
def test_views(gpu, oracle):
    """3 cameras at 32^2: 16 tiles per view, and the wave that crosses from one view into the next holds rays of two cameras"""
    scene = syn.config3(n=128, size=32)[0]
    cams = [syn.default_camera(), look((7.0, 3.0, -7.0), (0.0, 0.0, 0.0)), look((4.6, 0.4, -9.0), (4.2, 0.1, 9.0))]
    os_ = oracle.Oracle().scene(scene)
    per = [os_.render(EPS, LEN, 32, 32, c.as_array(), nthreads=16) for c in cams]
    want = np.stack([w for w, _ in per])
    ocnt = {k: sum(c[k] for _, c in per) for k in FRAME_COUNTERS}
    ds = gpu.scene(scene)
    try:
        for refill in (64, 1):                                       # refill_min 1: lanes of a wave take rays of the next view as they fall idle
            st = run_columns(gpu, lambda: ds.render_views(EPS, LEN, ft.ImageSize(32, 32), cams), want, ocnt, FRAME_COUNTERS, extra={"refill_min": refill})
    finally:
        ds.close()
    assert st["bundle_only"]["sdf_evals"] < st["cert_off"]["sdf_evals"]


AIMED = (0, 27, 40, 63)


def hand_made_waves():
    """ray buffers of whole waves (64 consecutive rays each) for C3's 256 children"""
    C, R = children(256)
    Cd, Rd = C.astype(np.float64), R.astype(np.float64)
    rs = np.random.default_rng(23)
    reach = np.linalg.norm(Cd, axis=1) + Rd
    far = int(np.argmax(reach))                                       # the child that sticks out most: nothing else reaches beyond its tip
    outward = unit(Cd[far])
    side = unit(np.cross(outward, [0.3, 1.0, 0.2]))
    waves = []
    # 63 rays that pass the cloud by, 0.6 above that tip (inside the support sphere: they march), and 1 aimed at the child, in lanes that are / are not the axis
    for pos in AIMED:
        o = outward * (reach[far] + 0.6) - side * 9.0 + rs.normal(size=(64, 3)) * 0.01
        d = np.tile(side, (64, 1))
        d[pos] = unit(Cd[far] - o[pos])
        waves.append(np.concatenate([o, d], axis=1))
    # rays on both sides of one small child, the axis (lane 27's ray) passing beside it
    tip = Cd[far] + outward * Rd[far]
    o = tip + outward * 0.6 - side * 8.0 + np.outer(np.linspace(-1.2, 1.2, 64) + 0.31, outward)
    waves.append(np.concatenate([o, np.tile(side, (64, 1))], axis=1))
    # tangent to single children within +- 2 margins (0.048), parallel, one wave per child
    for i in np.argsort(reach)[-3:]:                                  # the three children that reach out most, grazed on their outer side
        u = unit(Cd[i]); v = unit(np.cross(u, rs.normal(size=3)))
        closest = Cd[i] + np.outer(Rd[i] + 0.01 + rs.uniform(-2.0, 2.0, 64) * 0.048, u)
        waves.append(np.concatenate([closest - v * 9.0, np.tile(v, (64, 1))], axis=1))
    # 64 rays of unrelated directions: W is huge, the bundle simply fails
    d = unit(rs.normal(size=(64, 3)))
    waves.append(np.concatenate([rs.normal(size=(64, 3)) * 3.0 - d * 8.0, d], axis=1))
    od = np.concatenate(waves)
    return np.concatenate([od, np.full((len(od), 1), LEN), np.full((len(od), 1), EPS)], axis=1).astype(np.float32)


@pytest.mark.gpu
def test_hand_made_waves(gpu, oracle):
    scene = syn.config3(n=256, size=16)[0]
    rays = hand_made_waves()
    assert len(rays) % 64 == 0
    with np.errstate(all="ignore"):
        want, ocnt = oracle.Oracle().scene(scene).trace_rays(rays)
    rec, _ = oracle.Oracle().scene(scene).object_try_trace(rays)
    hit = rec[:, 14].view(np.int32) != 0
    for w, pos in enumerate(AIMED):                                   # the aimed ray hits, its 63 companions miss
        assert hit[64 * w + pos] and hit[64 * w:64 * w + 64].sum() == 1, (w, pos, hit[64 * w:64 * w + 64].sum())
    assert 0 < hit[256:320].sum() < 64 and 0 < hit[320:512].sum() < 192, (hit[256:320].sum(), hit[320:512].sum())
    ds = gpu.scene(scene)
    try:
        st = run_columns(gpu, lambda: ds.trace_rays(rays), want, ocnt, RAY_COUNTERS)
    finally:
        ds.close()
    assert st["bundle_only"]["sdf_evals"] < st["cert_off"]["sdf_evals"]


@pytest.mark.gpu
def test_shade_and_visibility_forms(gpu, oracle):
    """C3's hit records of a 48^2 frame under other lights: colours (against the oracle) and masks equal with the bundle on and off"""
    scene = syn.config3(n=256, size=48)[0]
    cam = syn.default_camera().as_array()
    rays = np.ascontiguousarray(np.stack([oracle.pixel_ray(cam, 48, 48, x, y, EPS, LEN) for x in range(48) for y in range(48)]))
    lights = (ft.SdfLight.directional((0.6, -1.0, -0.3), (0.9, 0.8, 0.7)), ft.SdfLight.directional((0.0, 1.0, 0.2), (0.3, 0.3, 0.3)))
    bg = (0.02, 0.03, 0.05)
    rec, _ = oracle.Oracle().scene(scene).object_try_trace(rays)
    want, ocnt = oracle.Oracle().scene(ft.SdfScene(scene.Object, bg, lights)).trace_rays(rays)
    relit = gpu.scene(scene).relight(bg, lights)
    masks = {}

    def both():
        rgb, st = relit.shade_hits(rec)
        masks[gpu.get_option("cert_policy"), gpu.get_option("cert"), gpu.get_option("escape")], _ = relit.light_visibility(rec)
        return rgb, st
    try:
        st = run_columns(gpu, both, want, ocnt, ("rays_shadow", "hits_shadow", "flags"))
    finally:
        relit.close()
    assert len(masks) == len(COLS)
    ref = masks.pop((BUNDLE_ONLY, 0, 1))
    assert 0 < np.count_nonzero(ref) < ref.size
    for key, m in masks.items():
        assert np.array_equal(m, ref), key
    assert st["bundle_only"]["sdf_evals"] < st["cert_off"]["sdf_evals"]


@pytest.mark.gpu
def test_extension_ambient_occlusion(gpu, oracle):
    st = render_columns(gpu, oracle, syn.config3(n=128, size=48)[0], 48, 48, ao_samples=4, ao_radius=0.5)
    assert st["bundle_only"]["sdf_evals"] < st["cert_off"]["sdf_evals"]


@pytest.mark.gpu
def test_extension_glass(gpu, oracle):
    """4 glass blobs, 3 bounces: paths inside a body march on -Distance and are no members"""
    rng = syn.Rng(31)
    kids = [syn.SdfForm.Primitive.sphere(rng.pointInBall(2.0), rng.range(0.6, 0.9)) for _ in range(4)]
    obj = syn.SdfObject.create(syn.SdfMaterial.createGlass((0.95, 0.9, 0.8), 1.45, 0.03), syn.SdfForm.unionSmooth(0.25, kids))
    scene = syn.SdfScene(obj, syn.BACKGROUND, syn.program_lights())
    st = render_columns(gpu, oracle, scene, 48, 48, counters=FRAME_COUNTERS + ("rays_ext",), max_bounces=3)
    assert st["bundle_only"]["rays_ext"] > 48 * 48 // 20
    assert st["bundle_only"]["sdf_evals"] < st["cert_off"]["sdf_evals"]


BUNDLE_ALONE = 255 | (255 << 8) | (16 << 16) | (6 << 24)          # the shipped bundle schedule (bits 30-31 = 0), per-lane never


def tile_over_margin(ds, cam, size):
    """capi.cpp launchTrace: the side of an 8x8 pixel tile at the far side of the support sphere, over certM"""
    ca, sup = cam.as_array().astype(np.float64), ds.support_sphere()
    n = lambda v: float(np.sqrt((v * v).sum()))
    return 8.0 * max(n(ca[6:9]), n(ca[9:12])) / size * (n(ca[0:3] - np.array(sup[:3])) + sup[3]) / n(ca[3:6]) / ds.miss_certificate()["margin"]


@pytest.mark.gpu
@pytest.mark.parametrize("tiles", ["narrow", "wide"])
def test_word_0_by_tile_width(gpu, oracle, tiles):
    """Word 0 is the shipped bundle schedule with the per-lane schedule 0 / 6 / 16 / every 6, except on a camera frame whose tiles are at most certM
    wide at the far side of the support sphere: there it is the bundle alone.  96^2 frames on either side of that criterion — a 0.06-degree lens on the
    cloud's rim (0.85 of the margin) and the Program.fs camera (28 times the margin): the frame equals the oracle's under word 0 and under both
    explicit words, and word 0 counts the evaluations of the explicit word it stands for.  An explicit word is taken as it stands on either side."""
    scene = syn.config3(n=128, size=96)[0]
    cam = syn.default_camera()
    if tiles == "narrow":
        cam = ft.Camera.lookAt(Position=(0.0, 0.0, -10.0), LookAt=(2.0, 2.0, 0.0), Up=(0.0, 1.0, 0.0), Lens=ft.Lens.create(0.06))
    ds = gpu.scene(scene)
    ratio = tile_over_margin(ds, cam, 96)
    ds.close()
    assert (0.5 < ratio <= 1.0) if tiles == "narrow" else ratio > 2.0, ratio
    cols = {"word0": {"cert": 1, "cert_policy": 0}, "both": {"cert": 1, "cert_policy": SHIPPED_LANES}, "alone": {"cert": 1, "cert_policy": BUNDLE_ALONE},
            "cert_off": {"cert": 0, "cert_policy": 0}}
    st = render_columns(gpu, oracle, scene, 96, 96, cols=cols, cam=cam)
    ev = {k: v["sdf_evals"] for k, v in st.items()}
    print(tiles, round(ratio, 3), ev)
    assert ev["both"] != ev["alone"], ev                              # the two schedules can be told apart on this frame
    assert ev["word0"] == (ev["alone"] if tiles == "narrow" else ev["both"]), ev
    assert ev["word0"] < ev["cert_off"], ev
