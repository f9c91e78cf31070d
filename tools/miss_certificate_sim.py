#!/usr/bin/env python3
"""CPU model of the miss certificate on the C3 frame (kernels.hip ft_miss_certificate; DESIGN.md section 4 "Miss certificate"), in the spirit of
esc_sim.py / lazy_sim.py: float64 marches of random 8x8 tiles of the 4096^2 frame with the escape shortcut, the certificate's first-success step per
ray, and per-wave rounds (a wave lasts as long as its longest lane) for fixed trigger schedules, a certificate round priced at TC evaluation rounds.
Usage: python tools/miss_certificate_sim.py [N=128: N*N pixels] [margin=0.048: scene.cpp certM of C3] [TC=0.8]"""
import os
import sys
import numpy as np
# load Rng without importing the package (no GPU library needed)
src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'fraytracer_amd', 'synthetic.py')).read()
F = np.float32
ns = {'np': np, 'F': F}
start = src.index('class Rng:'); end = src.index('\ndef ', start)
exec(src[start:end], ns)
rng = ns['Rng'](3)
C = []; R = []
for _ in range(256):
    c = rng.pointInBall(4.0); r = rng.range(0.1, 0.5); C.append(c); R.append(r)
C = np.array(C, np.float64); R = np.array(R, np.float64)
k = 4.0  # 1/strength
def sdf(P):
    d = np.sqrt(((P[:, None, :] - C[None]) ** 2).sum(-1)) - R[None]
    m = d.min(1)
    return m - np.log(np.exp(-k * (d - m[:, None])).sum(1)) / k
N = int(sys.argv[1]) if len(sys.argv) > 1 else 128
eps = 0.01
nps = np.sin(30.0)  # near-plane scale of the model's camera
pos = np.array([0, 0, -10.0]); fwd = np.array([0, 0, 1.0]); up = np.array([0, 1.0, 0])
right = np.cross(up, fwd); right /= np.linalg.norm(right)
upS = np.cross(fwd, right) * nps; rS = right * nps
T = N * N // 64
rs = np.random.default_rng(1)
tx = rs.integers(0, 512, T); ty = rs.integers(0, 512, T)
lx, ly = np.meshgrid(np.arange(8), np.arange(8), indexing='ij')
xs = ((tx[:, None] * 8 + lx.ravel()[None]) / 4096.0).ravel(); ys = ((ty[:, None] * 8 + ly.ravel()[None]) / 4096.0).ravel()
D = fwd[None] + (xs.ravel() - 0.5)[:, None] * rS[None] + (ys.ravel() - 0.5)[:, None] * upS[None]
supR = 4.0 + 0.5 + 0.25 * np.log(256) + 0.05
def march(O, Dir, L, maxsteps=2000):
    O = O.copy(); L = L.copy(); n = len(O)
    alive = np.ones(n, bool); hit = np.zeros(n, bool); steps = np.zeros(n, int)
    for _ in range(maxsteps):
        idx = np.where(alive)[0]
        if len(idx) == 0: break
        # escape: outside support sphere and heading away / passing by (approx: closest approach of remaining ray > supR)
        o = O[idx]; dd = Dir[idx]
        t = np.clip(-(o * dd).sum(1) / (dd * dd).sum(1), 0, None)
        closest = np.linalg.norm(o + t[:, None] * dd, axis=1)
        esc = (np.linalg.norm(o, axis=1) > supR) & (closest > supR)
        alive[idx[esc]] = False
        idx = idx[~esc]
        if len(idx) == 0: break
        Lz = L[idx] <= 0
        alive[idx[Lz]] = False; idx = idx[~Lz]
        d = sdf(O[idx]); steps[idx] += 1
        h = d < eps
        hit[idx[h]] = True; alive[idx[h]] = False
        mv = idx[~h]
        O[mv] += Dir[mv] * d[~h][:, None]; L[mv] -= d[~h]
    return hit, steps, O
hit, st, P = march(np.repeat(pos[None], N * N, 0), D, np.full(N * N, 30.0))
print('pixels', N * N, 'hits', hit.sum(), 'primary march evals/pixel', st.mean())
Ph = P[hit]
e2 = eps * 0.125
base = sdf(Ph)
nrm = np.stack([sdf(Ph + [e2, 0, 0]) - base, sdf(Ph + [0, e2, 0]) - base, sdf(Ph + [0, 0, e2]) - base], 1)
nrm /= np.linalg.norm(nrm, axis=1)[:, None]
ldir = -np.array([-0.5, -1.0, 1.0]); ldir /= np.linalg.norm(ldir)
cos = nrm @ ldir
lit_side = cos > 0
print('hits facing light (shadow rays)', lit_side.sum(), 'normal evals/pixel', 4 * hit.sum() / N / N)
# shadow ray: origin = hit point moved by -eps along primary dir (Ray.move -eps)
Dh = D[hit] / 1.0
So = Ph[lit_side] - eps * Dh[lit_side]
Sd = np.repeat(ldir[None], len(So), 0)
sh, sst, _ = march(So, Sd, np.full(len(So), 1000.0))
print('shadow rays', len(So), 'occluded', sh.sum(), 'shadow evals/pixel', sst.sum() / N / N,
      'evals occluded', sst[sh].sum() / N / N, 'evals lit', sst[~sh].sum() / N / N)
tot = st.sum() + 4 * hit.sum() + sst.sum()
print('total evals/pixel', tot / N / N)
MARGIN = float(sys.argv[2]) if len(sys.argv) > 2 else 0.048
def miss_proof_steps(O, Dir, L, M=MARGIN):
    """march like march(); at each step also evaluate the exact-miss proof for the rest of the ray (segment [0, L] from current point):
       F_lo = -ln(sum exp(-k * dmin_i))/k with dmin_i = dist(segment, c_i) - r_i.  returns steps and first step index where proof holds (or -1)"""
    O = O.copy(); L = L.copy(); n = len(O)
    alive = np.ones(n, bool); hit = np.zeros(n, bool); steps = np.zeros(n, int); first = np.full(n, -1)
    for _ in range(2000):
        idx = np.where(alive)[0]
        if len(idx) == 0: break
        o = O[idx]; dd = Dir[idx]
        t = np.clip(-(o * dd).sum(1) / (dd * dd).sum(1), 0, None)
        closest = np.linalg.norm(o + t[:, None] * dd, axis=1)
        esc = (np.linalg.norm(o, axis=1) > supR) & (closest > supR)
        alive[idx[esc]] = False; idx = idx[~esc]
        if len(idx) == 0: break
        Lz = L[idx] <= 0; alive[idx[Lz]] = False; idx = idx[~Lz]
        o = O[idx]; dd = Dir[idx]
        rel = C[None] - o[:, None]
        s = np.clip((rel * dd[:, None]).sum(-1) / (dd * dd).sum(1)[:, None], 0, np.minimum(L[idx], 40.0)[:, None])
        dmin = np.linalg.norm(rel - s[..., None] * dd[:, None], axis=-1) - R[None]
        m = dmin.min(1)
        Flo = m - np.log(np.exp(-k * (dmin - m[:, None])).sum(1)) / k
        pr = (Flo > eps + M) & (first[idx] < 0)
        first[idx[pr]] = steps[idx[pr]]
        d = sdf(o); steps[idx] += 1
        h = d < eps
        hit[idx[h]] = True; alive[idx[h]] = False
        mv = idx[~h]
        O[mv] += Dir[mv] * d[~h][:, None]; L[mv] -= d[~h]
    return hit, steps, first
for name, (O0, D0, L0) in {'primary': (np.repeat(pos[None], N * N, 0), D, np.full(N * N, 30.0)),
                           'shadow': (So, Sd, np.full(len(So), 1000.0))}.items():
    h2, s2, f2 = miss_proof_steps(O0, D0, L0)
    assert not (h2 & (f2 >= 0)).any(), 'false miss proof'
    miss = ~h2
    saved = np.where(f2 >= 0, s2 - f2, 0)
    print(f'{name}: rays {len(h2)} misses {miss.sum()} evals of misses/pixel {s2[miss].sum() / N / N:.3f}; proof ever holds on {(f2 >= 0).sum()} rays; '
          f'ideal saved/pixel {saved.sum() / N / N:.3f} = {saved.sum() / tot:.1%} of all; first-proof step median {np.median(f2[f2 >= 0]) if (f2 >= 0).any() else -1}')
    for pol in (0, 1, 2, 3, 4, 6):
        ok = (f2 >= 0) & (f2 <= pol)
        sv = np.where(ok, s2 - pol, 0).clip(0)
        print(f'   test once at step {pol}: proved {ok.sum()} saved/pixel {sv.sum() / N / N:.3f} ({sv.sum() / tot:.1%}); tests cost {(s2 > pol).sum() / tot:.1%}')

# per-tile (8x8 = one wave) rounds: a wave runs until its longest lane ends (ignores the latency mode's discount)
hp, sp, fp = miss_proof_steps(np.repeat(pos[None], N * N, 0), D, np.full(N * N, 30.0))
hs, ss, fs = miss_proof_steps(So, Sd, np.full(len(So), 1000.0))
lane_base = sp + 4 * hp
shadow_full = np.zeros(N * N, int); shadow_full[np.where(hit)[0][lit_side]] = ss
shadow_first = np.full(N * N, -1); shadow_first[np.where(hit)[0][lit_side]] = fs
def tiles(cost):
    t = cost.reshape(-1, 64)
    return t.max(1).sum(), t.sum()
b_rounds, b_lane = tiles(lane_base + shadow_full)
print('baseline: wave rounds', b_rounds, 'lane evals', b_lane, 'utilisation', b_lane / (64 * b_rounds))
TC = float(sys.argv[3]) if len(sys.argv) > 3 else 0.8  # a certificate round against an evaluation round (20 against 25 VALU per child)
for pp, ps in ((0, None), (None, 4), (0, 4), (0, 3), (0, 6), (None, 6), (0, 8)):
    cost = np.zeros(N * N)
    prim = sp.astype(float).copy()
    if pp is not None:
        ok = (fp >= 0) & (fp <= pp) & (sp > pp)
        prim = np.where(ok, pp, prim) + np.where(sp > pp, TC, 0)
    sh = shadow_full.astype(float).copy()
    if ps is not None:
        ok = (shadow_first >= 0) & (shadow_first <= ps) & (shadow_full > ps)
        sh = np.where(ok, ps, sh) + np.where(shadow_full > ps, TC, 0)
    r, l = tiles(prim + 4 * hp + sh)
    print(f'policy primary@{pp} shadow@{ps}: wave rounds {r:.0f} ({r / b_rounds - 1:+.1%})')
