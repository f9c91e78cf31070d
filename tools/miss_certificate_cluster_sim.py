#!/usr/bin/env python3
"""CPU model of a clustered miss certificate on the C3 frame, priced in VALU per wave (go/no-go for DESIGN.md section 4 "Miss certificate").
float64 marches of random 8x8 tiles of the 4096^2 frame (the tile model of miss_certificate_sim.py), then a lock-step replay of each tile as one wave:
before every evaluation round the lanes that are due try the certificate once enough of them are, and a wave lasts as long as its longest lane.
Priced per wave: an evaluation round E VALU; a certificate term (a child or a cluster bound) 20 VALU.
  flat:      all n children in evaluation order, leaving once every testing lane's partial sum has reached the threshold (checked every 8 children).
  clustered: pass 1 sums the K cluster bounds n_c 2^(A (dist(S, C) - R)); a lane whose sum is below thr succeeds.  Each lane marks the clusters whose
             bound is >= f thr / K; pass 2 visits the clusters some open lane marked and adds their members' exact terms (the lane's total is the sum
             of its unmarked bounds plus the exact terms of its marked clusters), leaving once every open lane's exact terms alone have reached thr.
Usage: python tools/miss_certificate_cluster_sim.py [N=64: N*N pixels] [margin=0.0476: scene.cpp certM of C3] [E=4300: VALU per evaluation round]"""
import os
import sys
import numpy as np
src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'fraytracer_amd', 'synthetic.py')).read()
F = np.float32
ns = {'np': np, 'F': F}
start = src.index('class Rng:'); end = src.index('\ndef ', start)
exec(src[start:end], ns)
rng = ns['Rng'](3)
C32 = []; R32 = []
for _ in range(256):
    C32.append(rng.pointInBall(4.0)); R32.append(rng.range(0.1, 0.5))
C = np.array(C32, np.float64); R = np.array(R32, np.float64)
k = 4.0  # 1/strength
N = int(sys.argv[1]) if len(sys.argv) > 1 else 64
MARGIN = float(sys.argv[2]) if len(sys.argv) > 2 else 0.0476
E = float(sys.argv[3]) if len(sys.argv) > 3 else 4300.0
TERM = 20.0
eps = 0.01
thr = np.exp(-k * (eps + MARGIN))
supR = 4.0 + 0.5 + 0.25 * np.log(256) + 0.05


def sdf(P):
    d = np.sqrt(((P[:, None, :] - C[None]) ** 2).sum(-1)) - R[None]
    m = d.min(1)
    return m - np.log(np.exp(-k * (d - m[:, None])).sum(1)) / k


def clusters(leaf):
    """recursive median split on the longest axis of the centres' box, leaves of at most `leaf` children; centre = the box's mid-point (float32),
    radius = max |c_i - C| + r_i in double"""
    out = []

    def rec(idx):
        if len(idx) <= leaf:
            lo = C32a[idx].min(0); hi = C32a[idx].max(0)
            cc = ((lo.astype(np.float64) + hi) * 0.5).astype(np.float32).astype(np.float64)
            rr = (np.linalg.norm(C[idx] - cc, axis=1) + R[idx]).max() * (1 + 1e-6)
            out.append((idx, cc, rr)); return
        ext = C32a[idx].max(0) - C32a[idx].min(0); ax = int(np.argmax(ext))
        o = idx[np.argsort(C32a[idx, ax], kind='stable')]
        h = len(o) // 2
        rec(o[:h]); rec(o[h:])
    rec(np.arange(len(C)))
    return out


C32a = np.array(C32, np.float32)
camera = np.array([0, 0, -10.0]); fwd = np.array([0, 0, 1.0]); up = np.array([0, 1.0, 0])
right = np.cross(up, fwd); right /= np.linalg.norm(right)
nps = np.sin(30.0)
upS = np.cross(fwd, right) * nps; rS = right * nps
T = N * N // 64
rs = np.random.default_rng(1)
tx = rs.integers(0, 512, T); ty = rs.integers(0, 512, T)
lx, ly = np.meshgrid(np.arange(8), np.arange(8), indexing='ij')
xs = ((tx[:, None] * 8 + lx.ravel()[None]) / 4096.0).ravel(); ys = ((ty[:, None] * 8 + ly.ravel()[None]) / 4096.0).ravel()
D = fwd[None] + (xs - 0.5)[:, None] * rS[None] + (ys - 0.5)[:, None] * upS[None]


def march(O, Dir, L):
    """-> hit, per-ray list of (point, remaining Length) before each evaluation"""
    O = O.copy(); L = L.copy(); n = len(O)
    alive = np.ones(n, bool); hit = np.zeros(n, bool); trail = [[] for _ in range(n)]
    for _ in range(2000):
        idx = np.where(alive)[0]
        if len(idx) == 0: break
        o = O[idx]; dd = Dir[idx]
        t = np.clip(-(o * dd).sum(1) / (dd * dd).sum(1), 0, None)
        esc = (np.linalg.norm(o, axis=1) > supR) & (np.linalg.norm(o + t[:, None] * dd, axis=1) > supR)
        alive[idx[esc]] = False; idx = idx[~esc]
        Lz = L[idx] <= 0; alive[idx[Lz]] = False; idx = idx[~Lz]
        if len(idx) == 0: break
        for j in idx: trail[j].append((O[j].copy(), L[j]))
        d = sdf(O[idx])
        h = d < eps
        hit[idx[h]] = True; alive[idx[h]] = False
        mv = idx[~h]
        O[mv] += Dir[mv] * d[~h][:, None]; L[mv] -= d[~h]
    return hit, trail, O


hitP, trailP, P = march(np.repeat(camera[None], N * N, 0), D, np.full(N * N, 30.0))
Ph = P[hitP]
e2 = eps * 0.125
base = sdf(Ph)
nrm = np.stack([sdf(Ph + [e2, 0, 0]) - base, sdf(Ph + [0, e2, 0]) - base, sdf(Ph + [0, 0, e2]) - base], 1)
nrm /= np.linalg.norm(nrm, axis=1)[:, None]
ldir = -np.array([-0.5, -1.0, 1.0]); ldir /= np.linalg.norm(ldir)
lit = (nrm @ ldir) > 0
So = Ph[lit] - eps * D[hitP][lit]
hitS, trailS, _ = march(So, np.repeat(ldir[None], len(So), 0), np.full(len(So), 1000.0))
shadowOf = np.full(N * N, -1); shadowOf[np.where(hitP)[0][lit]] = np.arange(len(So))


def terms(pts, dirs, Ls, cc, rr):
    """exact terms exp(-k (dist(S, c) - r)) of the clipped rest-of-line segments S (rows) against spheres (cc, rr); inf where no segment"""
    b = (pts * dirs).sum(1); dd = (dirs * dirs).sum(1); ww = (pts * pts).sum(1)
    disc = b * b - dd * (ww - supR * supR)
    sq = np.sqrt(np.maximum(disc, 0))
    t0 = np.maximum((-b - sq) / dd, 0); t1 = np.minimum((sq - b) / dd, Ls)
    ok = (disc > 0) & (t1 > t0)
    p0 = pts + dirs * t0[:, None]; sv = dirs * (t1 - t0)[:, None]
    rel = cc[None] - p0[:, None]
    t = np.clip((rel * sv[:, None]).sum(-1) / np.maximum((sv * sv).sum(1), 1e-30)[:, None], 0, 1)
    dist = np.linalg.norm(rel - t[..., None] * sv[:, None], axis=-1) - rr[None]
    return np.where(ok[:, None], np.exp(-k * dist), 0.0)


def cert_flat(pts, dirs, Ls):
    """-> success per lane, VALU"""
    tt = terms(pts, dirs, Ls, C, R)
    cs = np.cumsum(tt, 1)
    tot = cs[:, -1]
    # groups of 8: the wave leaves after group g once every lane's partial sum >= thr
    part = cs[:, 7::8]
    failed_all = (part >= thr).all(0)
    g = int(np.argmax(failed_all)) + 1 if failed_all.any() else len(C) // 8
    return tot < thr, TERM * 8 * g + 60


def make_cert_cluster(cl, f):
    K = len(cl)
    cc = np.array([c[1] for c in cl]); rr = np.array([c[2] for c in cl]); nc = np.array([len(c[0]) for c in cl], float)
    order = np.concatenate([c[0] for c in cl])
    starts = np.concatenate([[0], np.cumsum(nc)]).astype(int)

    def cert(pts, dirs, Ls):
        bnd = terms(pts, dirs, Ls, cc, rr) * nc[None]
        s1 = bnd.sum(1)
        ok = s1 < thr
        cost = TERM * K + 60 + 4 * K
        open_ = ~ok
        if not open_.any(): return ok, cost
        mark = bnd >= f * thr / K
        small = np.where(mark, 0.0, bnd).sum(1)
        ex = terms(pts, dirs, Ls, C[order], R[order])
        exact = np.zeros(len(pts))
        for c in range(K):
            if not (mark[:, c] & open_).any(): continue
            cost += TERM * nc[c] + 10
            exact += np.where(mark[:, c], ex[:, starts[c]:starts[c + 1]].sum(1), 0.0)
            if (exact[open_] >= thr).all(): break
        ok = ok | (open_ & (small + exact < thr))
        return ok, cost
    return cert


# per-lane timelines: primary steps, 4 normal evaluations, shadow steps
lanes = []
for i in range(N * N):
    sh = trailS[shadowOf[i]] if shadowOf[i] >= 0 else []
    lanes.append((trailP[i], hitP[i], sh))
dirP = D; dirS = ldir


def replay(cert, prim, shad, minDue, repeat):
    """lock-step waves; -> evaluation rounds, certificate VALU, evaluations, total VALU"""
    rounds = 0; cv = 0.0; evals = 0
    for t in range(T):
        ph = np.zeros(64, int); stp = np.zeros(64, int); due = np.zeros(64)
        L = [lanes[t * 64 + j] for j in range(64)]
        for j in range(64): ph[j] = 0 if len(L[j][0]) else (1 if L[j][1] else 3); due[j] = prim
        nrmLeft = np.full(64, 4)
        while True:
            for j in range(64):                                  # phase changes
                while True:
                    if ph[j] == 0 and stp[j] >= len(L[j][0]):
                        ph[j] = 1 if L[j][1] else 3; stp[j] = 0
                    elif ph[j] == 1 and nrmLeft[j] == 0:
                        ph[j] = 2 if len(L[j][2]) else 3; stp[j] = 0; due[j] = shad
                    elif ph[j] == 2 and stp[j] >= len(L[j][2]):
                        ph[j] = 3
                    else: break
            if (ph == 3).all(): break
            dl = [j for j in range(64) if ph[j] in (0, 2) and stp[j] >= due[j]]
            if cert is not None and len(dl) >= minDue:
                pts = np.array([(L[j][0] if ph[j] == 0 else L[j][2])[stp[j]][0] for j in dl])
                Ls = np.array([(L[j][0] if ph[j] == 0 else L[j][2])[stp[j]][1] for j in dl])
                dirs = np.array([dirP[t * 64 + j] if ph[j] == 0 else dirS for j in dl])
                ok, c = cert(pts, dirs, Ls)
                cv += c
                for j, o in zip(dl, ok):
                    if o: ph[j] = 3                              # a proven primary is a miss (no shadow ray); a proven shadow ray ends the lane
                    else: due[j] = stp[j] + repeat if repeat else 1 << 30
                if (ph == 3).all(): break
            act = ph != 3
            rounds += 1; evals += int(act.sum())
            stp[(ph == 0) | (ph == 2)] += 1; nrmLeft[ph == 1] -= 1
    return rounds, cv, evals, rounds * E + cv


if __name__ == '__main__':
    print(f'N={N} tiles={T} thr={thr:.4f} E={E:.0f} VALU/round, {TERM:.0f} VALU/term')
    r0 = replay(None, 0, 0, 64, 0)
    print(f'no certificate: rounds {r0[0]} evals {r0[2]} VALU {r0[3] / 1e6:.2f} M')
    fl = replay(cert_flat, 1, 6, 16, 0)
    print(f'shipped flat (1, 6, 16, once): rounds {fl[0]} evals {fl[2]} cert VALU {fl[1] / 1e6:.2f} M total {fl[3] / 1e6:.2f} M ({fl[3] / r0[3] - 1:+.1%} vs none)')
    for name, cfg in (('flat', None), ('leaf16', 16), ('leaf8', 8)):
        for f in ((1.0,) if cfg is None else (1.0, 0.5)):
            cert = cert_flat if cfg is None else make_cert_cluster(clusters(cfg), f)
            for prim, shad, mn, rep in ((1, 6, 16, 0), (0, 4, 16, 4), (0, 4, 8, 4), (0, 2, 16, 2), (0, 4, 16, 8), (1, 4, 16, 4), (0, 6, 16, 6)):
                r = replay(cert, prim, shad, mn, rep)
                print(f'{name:6s} f={f:.2f} prim@{prim} shadow@{shad} due>={mn:2d} repeat {rep}: rounds {r[0]} evals {r[2]} cert VALU {r[1] / 1e6:.2f} M '
                      f'total {r[3] / 1e6:.2f} M ({r[3] / fl[3] - 1:+.1%} vs shipped)', flush=True)
