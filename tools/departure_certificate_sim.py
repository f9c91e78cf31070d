#!/usr/bin/env python3
"""CPU model of the departure certificate on the C3 frame (FT_OPT_DEPART; kernels.hip ft_miss_certificate with a tilted margin, scene.cpp "Departure
certificate"), on the float64 tiles and marches of miss_certificate_cluster_sim.py.  A lit shadow ray is certified where, child by child at the clamped
closest approach t_c of its line,  sum_i exp(-k (d_i(t_c) - slope t_c)) < exp(-k (eps + base + slope t0)),  slope = depE / eps.  Reported:
  * the share of the lit shadow rays certified at birth (their first evaluation comes from the cache: birth is step 1) and by step, against the flat
    certificate's first step;
  * the evaluation rounds of the lock-step tiles under candidate schedules of the per-lane tries (first try at birth, again `repeat` steps after a
    failure, a wave tries once `lanes` of its rays are due), every ray also ending where its own flat certificate first holds (the ideal the bundle
    certificate approaches), and the rounds net of the tries priced at TRY VALU against E per round.  TRY is the measured cost of a try round of the
    cluster certificate on this frame, 1 440 VALU (profiles/departure_certificate_pmc.txt: the build's VALU instructions per launch less its rounds at
    the parent's VALU per round, over the tries this model counts for the shipped schedule); 1 000 and 2 000 are printed beside it.
No certified ray's float64 march may hit: asserted for every try the model makes.
Usage: python tools/departure_certificate_sim.py [N=96: N*N pixels] [margin=0.0476] [E=4300] [depE=1.63e-5] [depB=4.4e-4] [depK=15.8] [TRY=1440]"""
import os
import sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) < 2:
    sys.argv.append('96')
import miss_certificate_cluster_sim as m

C, R, k, eps, T, E, dirS = m.C, m.R, m.k, m.eps, m.T, m.E, m.ldir
depE = float(sys.argv[4]) if len(sys.argv) > 4 else 1.63e-5
depB = float(sys.argv[5]) if len(sys.argv) > 5 else 4.4e-4
depK = float(sys.argv[6]) if len(sys.argv) > 6 else 15.8
TRY = float(sys.argv[7]) if len(sys.argv) > 7 else 1440.0
slope = depE / eps
base = 2.0 * depE + depB + depK * slope * slope
clipR = m.supR + 0.05 * m.supR                                         # the support sphere grown by depCap


def tilted(o, d, L):
    """does the tilted certificate hold for the line o + t d, 0 <= t <= L"""
    b = o @ d; dd = d @ d; ww = o @ o
    disc = b * b - dd * (ww - clipR * clipR)
    if disc <= 0.0:
        return True                                                    # the line misses the clip ball: nothing to sum
    sq = np.sqrt(disc)
    t0 = max((-b - sq) / dd, 0.0); t1 = min((sq - b) / dd, L)
    if t1 <= t0:
        return True
    tc = np.clip(((C - o) @ d) / dd, t0, t1)
    dist = np.linalg.norm(C - (o + tc[:, None] * d), axis=1) - R
    return np.exp(-k * (dist - slope * (tc - t0))).sum() < np.exp(-k * (eps + base + slope * t0))


def first_flat(trail, d):
    """the first step of a missing march from which the flat miss certificate of its own line holds (ideal: tried every step)"""
    if not trail:
        return 0
    pts = np.array([p for p, _ in trail]); Ls = np.array([l for _, l in trail])
    s = m.terms(pts, np.repeat(d[None], len(pts), 0), Ls, C, R).sum(1)
    ok = np.where(s < m.thr)[0]
    return int(ok[0]) if len(ok) else len(trail)


if __name__ == '__main__':
    nS = len(m.hitS)
    lit = np.where(~m.hitS)[0]
    print(f'N={m.N} tiles={T} shadow rays {nS}, lit {len(lit)} ({len(lit) / nS:.1%}); margin m(t) = {base:.3g} + {slope:.3g} t (depE {depE:.3g}, depB {depB:.3g}, depK {depK:.3g}), eps {eps}; flat margin {m.MARGIN}')
    memo = {}

    def holds(s, step):
        key = (s, step)
        if key not in memo:
            tr = m.trailS[s]
            o, L = tr[min(step, len(tr) - 1)]
            memo[key] = bool(tilted(o, dirS, L))
            assert not (memo[key] and m.hitS[s]), 'a certified ray marches to a hit'
        return memo[key]

    firstT = np.array([next((st for st in range(1, len(m.trailS[s]) + 1) if st >= len(m.trailS[s]) or holds(s, st)), len(m.trailS[s])) for s in lit])
    firstF = np.array([first_flat(m.trailS[s], dirS) for s in lit])
    for s in np.where(m.hitS)[0]:                                       # occluded rays: tried at every step they take, never certified
        for st in range(1, len(m.trailS[s])):
            holds(s, st)
    by = ', '.join(f'step {q}: {np.mean(firstT <= q):.1%}' for q in (1, 2, 3, 4, 6, 8))
    print(f'lit shadow rays certified by the tilted margin at birth (step 1) and by {by}; first step: tilted mean {firstT.mean():.2f}, flat mean {firstF.mean():.2f}')
    flatOf = dict(zip(lit.tolist(), firstF.tolist()))

    def tile_rounds(t, sched):
        """lock-step rounds of tile t and the tries made; sched = None (no per-lane tries) or (repeat, lanes)"""
        end = np.zeros(64, int); birth = np.full(64, -1); sOf = np.full(64, -1)
        for j in range(64):
            r = t * 64 + j
            if m.hitP[r]:
                n = len(m.trailP[r]) + 4
                s = m.shadowOf[r]
                if s >= 0:
                    birth[j] = n; sOf[j] = s
                    n += max((len(m.trailS[s]) if m.hitS[s] else flatOf[s]) - 1, 0)
            else:
                key = ('p', r)
                if key not in memo: memo[key] = first_flat(m.trailP[r], m.D[r])
                n = memo[key]
            end[j] = n
        tries = 0
        if sched is not None:
            repeat, lanes = sched
            certAt = np.where(birth >= 0, 1, 1 << 30)                   # in steps of the shadow ray; born with one step taken
            w, last = 0, int(end.max())
            while w < last:
                steps = 1 + w - birth
                due = [j for j in range(64) if birth[j] >= 0 and birth[j] <= w < end[j] and steps[j] >= certAt[j]]
                if len(due) >= lanes:
                    tries += 1
                    for j in due:
                        if holds(sOf[j], int(steps[j])): end[j] = w
                        else: certAt[j] = steps[j] + repeat if repeat else 1 << 30
                    last = int(end.max())
                w += 1
        return int(end.max()), tries

    r0 = sum(tile_rounds(t, None)[0] for t in range(T))
    print(f'rounds with ideal flat per-lane certificates and no tilted try: {r0}')
    rows = []
    for name, sched in (('birth only, 1 lane', (0, 1)), ('birth + 2 steps later, 1 lane', (2, 1)), ('birth + repeat 2, 8 lanes', (2, 8)), ('birth + repeat 2, 16 lanes', (2, 16)),
                        ('birth + repeat 3, 16 lanes', (3, 16)), ('birth only, 8 lanes', (0, 8)), ('birth only, 16 lanes', (0, 16)), ('every step, 1 lane', (1, 1))):
        rounds = tries = 0
        for t in range(T):
            a, b = tile_rounds(t, sched); rounds += a; tries += b
        nets = ', '.join(f'at {p} {(rounds + tries * p / E) / r0 - 1:+.2%}' for p in (1000, 2000))
        rows.append(((rounds + tries * TRY / E) / r0 - 1, name))
        print(f'{name}: rounds {rounds} ({rounds / r0 - 1:+.2%}), tries {tries}, net at the measured {TRY:.0f} VALU a try {rows[-1][0]:+.2%} ({nets}; a round: {E:.0f} VALU)', flush=True)
    rows.sort()
    print('best at the measured price: ' + '; '.join(f'{n} {v:+.2%}' for v, n in rows[:3]))
