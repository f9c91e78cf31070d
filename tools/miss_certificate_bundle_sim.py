#!/usr/bin/env python3
"""CPU model of the bundle certificate on the C3 frame (kernels.hip ft_bundle_certificate), priced in VALU per wave like miss_certificate_cluster_sim.py,
whose tiles, marches and per-lane certificate it reuses.  Before an evaluation round — every `period`-th of the wave — the wave tries ONE certificate
for all its primary rays, then one for all its shadow rays of at least `shadowFrom` steps, at their true (misaligned) steps: the kernel's bound with its
own paddings (axis line, width W = max (a_l + b_l t1_l), axis interval I), for either axis choice: "lane" (the first member at or after lane 27, else the
first) or "mean" (the members' mean origin and direction).  "ideal" is the bound the issue's first model assumed: per child the minimum over the
members of the per-lane dmin, less a pad.  A bundle try is priced at B VALU whatever its outcome; an evaluation round at E, or, with `latency`, at
E * 1.34 * rays / 64 once at most 32 rays are left (the latency mode's measured price per ray).  The per-lane certificate is the shipped clustered one.
Usage: python tools/miss_certificate_bundle_sim.py [N=64: N*N pixels] [margin=0.0476] [E=4300]      (B = 200 and 300 are both printed)"""
import os
import sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import miss_certificate_cluster_sim as m

C, R, k, thr, T, E, lanes, D, dirS, supR = m.C, m.R, m.k, m.thr, m.T, m.E, m.lanes, m.dirP, m.dirS, m.supR


def segments(pts, dirs, Ls):
    b = (pts * dirs).sum(1); dd = (dirs * dirs).sum(1); ww = (pts * pts).sum(1)
    disc = b * b - dd * (ww - supR * supR)
    sq = np.sqrt(np.maximum(disc, 0))
    t0 = np.maximum((-b - sq) / dd, 0); t1 = np.minimum((sq - b) / dd, Ls)
    return (disc > 0) & (t1 > t0), t0, t1


def seg_dist(a, b):
    ab = b - a
    t = np.clip(((C - a) @ ab) / max(ab @ ab, 1e-30), 0.0, 1.0)
    return np.linalg.norm(C - (a + t[:, None] * ab), axis=1)


def bundle(idx, pts, dirs, Ls, axis, pad):
    """-> members (indices into idx) the bundle ends, possibly none"""
    ok, t0, t1 = segments(pts, dirs, Ls)
    mem = np.where(ok)[0]
    if len(mem) == 0:
        return mem
    if axis == 'ideal':
        dmin = np.min([seg_dist(pts[j] + dirs[j] * t0[j], pts[j] + dirs[j] * t1[j]) for j in mem], axis=0) - R - pad
        return mem if np.exp(-k * dmin).sum() < thr else mem[:0]
    if axis == 'lane':
        at = [j for j in mem if idx[j] >= 27]
        a = at[0] if at else mem[0]
        oc, dc = pts[a], dirs[a]
    else:
        oc, dc = pts[mem].mean(0), dirs[mem].mean(0)
    g = pts[mem] - oc
    s = (g @ dc) / (dc @ dc)
    al = np.linalg.norm(g - s[:, None] * dc, axis=1); bl = np.linalg.norm(dirs[mem] - dc, axis=1)
    W = (al + bl * t1[mem]).max() * 1.001 + 1e-6 + 4e-6 * supR
    lo, hi = (s + t0[mem]).min() - 4e-6 * supR, (s + t1[mem]).max() + 4e-6 * supR
    total = np.exp(-k * (seg_dist(oc + lo * dc, oc + hi * dc) - W - R)).sum()
    return mem if total < thr else mem[:0]


def replay(cert, prim, shad, minDue, repeat, axis=None, period=1, minMem=1, shadowFrom=0, B=200.0, pad=0.0, latency=False, per_tile=None):
    """lock-step waves; -> evaluation rounds, priced evaluation VALU, certificate VALU, bundle tries, bundles that held; per_tile: a list that receives
    every tile's rounds"""
    rounds = 0; ev = 0.0; cv = 0.0; tries = 0; held = 0
    for t in range(T):
        ph = np.zeros(64, int); stp = np.zeros(64, int); due = np.zeros(64)
        L = [lanes[t * 64 + j] for j in range(64)]
        for j in range(64): ph[j] = 0 if len(L[j][0]) else (1 if L[j][1] else 3); due[j] = prim
        nrmLeft = np.full(64, 4)
        wave = 0; before = rounds
        while True:
            for j in range(64):
                while True:
                    if ph[j] == 0 and stp[j] >= len(L[j][0]):
                        ph[j] = 1 if L[j][1] else 3; stp[j] = 0
                    elif ph[j] == 1 and nrmLeft[j] == 0:
                        ph[j] = 2 if len(L[j][2]) else 3; stp[j] = 0; due[j] = shad
                    elif ph[j] == 2 and stp[j] >= len(L[j][2]):
                        ph[j] = 3
                    else: break
            if (ph == 3).all(): break

            def state(js):
                pts = np.array([(L[j][0] if ph[j] == 0 else L[j][2])[stp[j]][0] for j in js])
                Ls = np.array([(L[j][0] if ph[j] == 0 else L[j][2])[stp[j]][1] for j in js])
                dirs = np.array([D[t * 64 + j] if ph[j] == 0 else dirS for j in js])
                return pts, dirs, Ls
            if axis is not None and wave % period == 0:
                for cls in (0, 2):
                    js = [j for j in range(64) if ph[j] == cls and (cls == 0 or stp[j] >= shadowFrom)]
                    if len(js) < max(minMem, 1): continue
                    tries += 1; cv += B
                    got = bundle(js, *state(js), axis, pad)
                    if len(got): held += 1
                    for i in got: ph[js[i]] = 3
                if (ph == 3).all(): break
            dl = [j for j in range(64) if ph[j] in (0, 2) and stp[j] >= due[j]]
            if cert is not None and len(dl) >= minDue:
                ok, c = cert(*state(dl))
                cv += c
                for j, o in zip(dl, ok):
                    if o: ph[j] = 3
                    else: due[j] = stp[j] + repeat if repeat else 1 << 30
                if (ph == 3).all(): break
            act = int((ph != 3).sum())
            rounds += 1; wave += 1
            ev += E * min(1.0, 1.34 * act / 64.0) if latency and act <= 32 else E
            stp[(ph == 0) | (ph == 2)] += 1; nrmLeft[ph == 1] -= 1
        if per_tile is not None: per_tile.append(rounds - before)
    return rounds, ev, cv, tries, held


if __name__ == '__main__':
    lane_cert = m.make_cert_cluster(m.clusters(16), 0.5)
    NEVER = 1 << 30
    for latency in (False, True):
        print(f'N={m.N} tiles={T} thr={thr:.4f} E={E:.0f} VALU/round' + (', rounds of <= 32 rays at the latency mode\'s price' if latency else ''))
        r0 = replay(None, 0, 0, 64, 0, latency=latency)
        print(f'no certificate: rounds {r0[0]} VALU {(r0[1] + r0[2]) / 1e6:.2f} M')
        sh = replay(lane_cert, 0, 6, 16, 6, latency=latency)
        base = sh[1] + sh[2]
        print(f'shipped per-lane schedule (0 / +6, shadow 6 / +6, 16 lanes): rounds {sh[0]} VALU {base / 1e6:.2f} M ({base / (r0[1] + r0[2]) - 1:+.1%} vs none)')
        rows = [('ideal pad 0', dict(axis='ideal', period=2, shadowFrom=2), None), ('ideal pad 0.03', dict(axis='ideal', period=2, shadowFrom=2, pad=0.03), None)]
        for axis in ('lane', 'mean'):
            rows += [(f'{axis} axis, bundle only, every round', dict(axis=axis, period=1), None),
                     (f'{axis} axis, bundle only, every 2nd round, shadow from 2', dict(axis=axis, period=2, shadowFrom=2), None),
                     (f'{axis} axis, bundle only, every 3rd round, shadow from 2', dict(axis=axis, period=3, shadowFrom=2), None)]
        rows += [('lane axis, every 2nd, shadow from 3', dict(axis='lane', period=2, shadowFrom=3), None),
                 ('lane axis, every 2nd, shadow from 4', dict(axis='lane', period=2, shadowFrom=4), None),
                 ('lane axis, every 2nd, shadow from 2, >= 16 members', dict(axis='lane', period=2, shadowFrom=2, minMem=16), None),
                 ('lane axis, every 2nd, shadow from 2 + shipped per-lane', dict(axis='lane', period=2, shadowFrom=2), (0, 6, 16, 6)),
                 ('lane axis, every round + shipped per-lane', dict(axis='lane', period=1), (0, 6, 16, 6)),
                 ('lane axis, every 2nd, shadow from 2 + sparse per-lane (0 / +12, shadow 12 / +12)', dict(axis='lane', period=2, shadowFrom=2), (0, 12, 16, 12))]
        for name, kw, lanes_pol in rows:
            pol = lanes_pol or (NEVER, NEVER, 64, 0)
            r = replay(lane_cert if lanes_pol else None, *pol, B=0.0, latency=latency, **kw)
            out = [f'{(r[1] + r[2] + B * r[3]) / 1e6:.2f} M ({(r[1] + r[2] + B * r[3]) / base - 1:+.1%})' for B in (200.0, 300.0)]
            print(f'{name}: rounds {r[0]} bundle tries {r[3]} held {r[4]} VALU at B = 200 / 300: {out[0]} / {out[1]} vs shipped', flush=True)
