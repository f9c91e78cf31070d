"""Scenes, waves and lane masks for tests/test_gpu_cull_pass.py, and a numpy float32 restatement of the culling pass's rule (kernels.hip
ft_cull_children) that chooses the waves: it says, with room to spare, which children a wave's pass will drop, so that the clusters can be put
where the pass has something to do.  What the device then did is asserted on the device's answer, never on this prediction."""
import numpy as np

import fraytracer_amd as ft
from fraytracer_amd import SdfForm, SdfMaterial, SdfObject, SdfScene
from fraytracer_amd import synthetic as syn

import wave_restatement as wr

F = np.float32
CULL_MIN, CULL_MAX = 32, 256                       # kernels.hip FT_CULL_MIN, ft_kernels.h FT_CULL_MAX
FAST_P_MAX = 20000.0                               # kernels.hip FT_FAST_P_MAX
PITCH = 2.0 * 10.0 * np.tan(np.radians(30.0)) / 3072      # a pixel of a 3072-wide frame, 60 degrees across, at the benchmark camera's distance of 10
SPARE = 1.5                                        # log2 to spare in a predicted decision: v_sqrt_f32 and v_exp_f32 are within an ulp or two of numpy's, and
                                                   # a prefix sum that differs in its last bits can move its exponent by one

ALL = (1 << 64) - 1
MASKS = {"all lanes": ALL, "lane 0 idle": ALL & ~1, "lane 63 only": 1 << 63, "one middle lane": 1 << 29,
         "alternating lanes": int("01" * 32, 2), "upper 32 lanes": ALL & ~((1 << 32) - 1)}


def lanes_of(mask):
    return np.array([(mask >> l) & 1 for l in range(64)], bool)


# ---- scenes: name -> (scene description, what the accumulator holds in front of the run at the points P (float64), or None) -------------------

def seg_dist(P, a, b):
    ab = b - a
    t = np.clip(((P - a) @ ab) / (ab @ ab), 0.0, 1.0)
    return np.linalg.norm(P - (a + t[:, None] * ab), axis=1)


CAPSULE = ((-1.0, 0.0, 0.0), (1.0, 0.5, 0.0), 0.3)
TORUS = ((0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 1.0, 0.2)


def accumulator_behind_capsule_and_torus(P, si):
    """exp(si d) of the capsule and of the torus that stand in front of the run in `run behind other kinds`, in float64"""
    a, b, r = (np.array(v, np.float64) for v in CAPSULE)
    d_cap = seg_dist(P, a, b) - r
    c, n = np.array(TORUS[0], np.float64), np.array(TORUS[1], np.float64)
    q = P - c
    h = q @ n
    radial = np.sqrt(np.maximum((q * q).sum(axis=1) - h * h, 0.0))
    d_tor = np.sqrt((radial - TORUS[2]) ** 2 + h * h) - TORUS[3]
    return np.exp(si * d_cap) + np.exp(si * d_tor)


def general_scene(form):
    mat = SdfMaterial.createSolid((0.2, 0.8, 0.5))
    return SdfScene(SdfObject.create(mat, form), syn.BACKGROUND, syn.program_lights())


def scenes():
    out = {}
    for strength in (0.25, 0.1):
        for n in (32, 33, 64, 65, 130, 256, 257):
            out[f"config3 n={n} strength={strength}"] = (syn.config3(n=n, size=64, strength=strength)[0], None)
    P = SdfForm.Primitive
    rng = syn.Rng(61)
    balls = lambda n, spread=3.0: [P.sphere(rng.pointInBall(spread), rng.range(0.15, 0.5)) for _ in range(n)]
    out["run behind other kinds"] = (general_scene(SdfForm.unionSmooth(0.25, [P.capsule(*CAPSULE), P.torus(*TORUS)] + balls(90))),
                                     accumulator_behind_capsule_and_torus)
    out["run under an intersect"] = (general_scene(SdfForm.intersect([SdfForm.unionSmooth(0.25, balls(120)), P.sphere((0.0, 0.0, 0.0), 2.6)])), None)
    return out


NO_SITE = "config3 n=31"


def scene_without_a_site():
    return syn.config3(n=31, size=64)[0]


# ---- the rule, restated -----------------------------------------------------------------------------------------------------------------------

def restated_pass(rec, si, pts, active):
    """One wave's pass in numpy float32, operation by operation as kernels.hip states it.  -> None where fast_point_ok fails, else (drop, keep): per
    looked-at child, True where the decision holds with SPARE to spare (a child in neither is too close to call here)."""
    p = np.asarray(pts, F)
    act = np.flatnonzero(active)
    with np.errstate(all="ignore"):
        m = np.abs(p[act]).max(axis=1)
        if np.isnan(p[act]).any() or not (m < F(FAST_P_MAX)).all():
            return None
        sq = lambda d: ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F)
        q00 = p[act[0]]
        far2 = np.where(active, sq(p - q00), F(0.0)).astype(F)
        q01 = p[np.flatnonzero(active & (far2 == far2.max()))[0]]
        q0 = (F(0.5) * (q00 + q01)).astype(F)
        rho2 = np.where(active, sq(p - q0), F(0.0)).astype(F).max()
        rho = F(np.sqrt(rho2) * F(1.001) + F(1e-6))
        c = np.asarray(rec[:CULL_MAX], F)
        n = len(c)
        dq = np.sqrt(sq(c[:, :3] - q0)).astype(F)
        dc = (dq - c[:, 3]).astype(F)
        slack = F(F(0.01) + rho)
        dlo, dhi = (dc - slack).astype(F), (dc + slack).astype(F)
        low = np.exp2(np.maximum((F(si) * dhi * F(1.44269504) - F(0.02)).astype(F), F(-200.0))).astype(F)
        padded = np.zeros(-(-n // 64) * 64, F)
        padded[:n] = low
        slow = np.zeros_like(padded)
        carry = F(0.0)
        for k, chunk in enumerate(padded.reshape(-1, 64)):
            _, excl, total = wr.wave_scan(chunk)
            slow[64 * k:64 * k + 64] = ((carry + excl) * F(0.99609375)).astype(F)
            carry = F(carry + total)
        slow = slow[:n]
        x = np.clip((F(si) * dlo * F(1.44269504)).astype(F), F(-1000.0), F(1000.0))
        normal = (slow >= F(2.0 ** -126)) & np.isfinite(slow)
        expo = np.frexp(np.where(normal, slow, F(1.0)))[1] - 1
        drop = normal & (x + F(0.02) + F(SPARE) <= expo - 24)
        keep = ~normal & (slow == 0) | normal & (x + F(0.02) - F(SPARE) > expo - 24)
    return drop, keep


# ---- waves ------------------------------------------------------------------------------------------------------------------------------------

def tile(centre, direction, pitch, rng):
    """64 points as a wave of the trace kernel holds them: an 8 x 8 tile of rays, `pitch` apart, at slightly different depths along `direction`"""
    d = direction / np.linalg.norm(direction)
    u = np.cross(d, (0.0, 1.0, 0.0) if abs(d[1]) < 0.9 else (1.0, 0.0, 0.0))
    u /= np.linalg.norm(u)
    v = np.cross(d, u)
    i, j = np.divmod(np.arange(64), 8)
    return (centre + ((i - 3.5) * pitch)[:, None] * u + ((j - 3.5) * pitch)[:, None] * v + (rng.uniform(-2.0, 2.0, 64) * pitch)[:, None] * d).astype(F)


def predicted_drops(rec, si, pts, later_only):
    """the smallest number, over MASKS, of children the restated pass surely drops (later_only: in a pass after the first)"""
    worst = None
    for mask in MASKS.values():
        r = restated_pass(rec, si, pts, lanes_of(mask))
        k = int(r[0][64:].sum() if later_only else r[0].sum())
        worst = k if worst is None else min(worst, k)
    return worst


def waves_for(rec, si, seed):
    """-> (points (W, 64, 3) float32, kinds: one name per wave, extras: per wave the child whose centre one of its points is, or -1, and that lane)"""
    rng = np.random.default_rng(seed)
    n = len(rec)
    centres = rec[:, :3].astype(np.float64)
    middle, reach = centres.mean(axis=0), np.linalg.norm(centres - centres.mean(axis=0), axis=1).max()
    pts, kinds, on_centre = [], [], []

    def add(kind, p, child=-1, lane=-1):
        pts.append(np.asarray(p, F)); kinds.append(kind); on_centre.append((child, lane))

    # tight clusters near the rim: of many candidates, the three the restated rule drops most children for under every mask
    cands = []
    for _ in range(96):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        t = tile(middle + d * reach * rng.uniform(0.85, 1.25), -d, PITCH, rng)
        cands.append((predicted_drops(rec, si, t, later_only=n >= 130), len(cands), t))
    cands.sort(key=lambda c: (-c[0], c[1]))
    for score, _, t in cands[:3]:
        add("tight", t)
    # clusters a few radii wide, inside the blob
    for _ in range(2):
        add("wide", middle + rng.normal(size=(64, 3)) * 0.8 + rng.normal(size=3) * 0.3 * reach)
    # around one child's centre, one point exactly on it: the first child, the last one the pass looks at, one in between
    for child, lane in ((0, 63), (min(n, CULL_MAX) - 1, 0), (min(n, CULL_MAX) // 2, 40)):
        p = (centres[child] + rng.normal(size=(64, 3)) * 0.05).astype(F)
        p[lane] = rec[child, :3]
        add("on a centre", p, child, lane)
    # one point far outside the scene: fast_point_ok fails wherever its lane evaluates
    for lane, far in ((0, (3.0e4, 0.0, 0.0)), (63, (0.0, -1.0e30, 0.0)), (29, (0.0, 0.0, np.inf))):
        p = cands[0][2].copy()
        p[lane] = far
        add("one point outside", p, -1, lane)
    # every lane at the same point (the ball's radius is its floor of 1e-6)
    add("one point 64 times", np.repeat(cands[1][2][17][None, :], 64, axis=0))
    return np.array(pts, F), kinds, on_centre, [c[0] for c in cands[:3]]
